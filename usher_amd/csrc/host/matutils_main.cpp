// matutils_main.cpp -- `matutils-amd`: the matUtils subcommands this project runs on the GPU.
//
//   matutils-amd uncertainty -i tree.pb -s samples.txt [-e epps.tsv] [-o placements.tsv] [-T n] [--device k]
//
// uncertainty_main / findEPPs_wrapper (uncertainty.cpp:279-339, 541-560): load the MAT, uncondense its leaves, read the sample
// names, and for every sample report its equally parsimonious placements and neighborhood size (-e) and the candidate parents
// (-o), in the reference's file formats.  The per-sample searches run on the device as one batch (ugp_uncertainty).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "mat.hpp"
#include "usher_amd.h"

namespace {

void usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd uncertainty -i tree.pb -s samples.txt [-e epps.tsv] [-o placements.tsv] [-T n] [--device k]\n"
            "  -i, --input-mat          input mutation-annotated tree [REQUIRED]\n"
            "  -s, --samples            text file of sample names to calculate uncertainty for\n"
            "  -e, --find-epps          tsv of equally parsimonious placements and neighborhood sizes\n"
            "  -o, --record-placements  two-column tsv of potential parents for each sample\n"
            "  -T, --threads            accepted for compatibility (the searches run on the device)\n"
            "      --device             HIP device ordinal [0]\n"
            "  (-d / --dropout-mutations is not supported)\n");
}

int uncertainty(int argc, char **argv) {
    std::string mat, samples, fepps, flocs;
    int device = 0;
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); return false; }
            dst = argv[++i];
            return true;
        };
        std::string tmp;
        if (a == "-i" || a == "--input-mat") { if (!val(mat)) return 1; }
        else if (a == "-s" || a == "--samples") { if (!val(samples)) return 1; }
        else if (a == "-e" || a == "--find-epps") { if (!val(fepps)) return 1; }
        else if (a == "-o" || a == "--record-placements") { if (!val(flocs)) return 1; }
        else if (a == "-T" || a == "--threads") { if (!val(tmp)) return 1; }
        else if (a == "--device") { if (!val(tmp)) return 1; device = atoi(tmp.c_str()); }
        else if (a == "-d" || a == "--dropout-mutations") {
            fprintf(stderr, "ERROR: -d/--dropout-mutations is not supported by matutils-amd (use the reference matUtils)\n");
            return 1;
        }
        else if (a == "-h" || a == "--help") { usage(stdout); return 0; }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); usage(stderr); return 1; }
    }
    if (mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); usage(stderr); return 1; }
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    if (!T.condensed_nodes.empty()) T.uncondense_leaves();
    if (samples.empty()) return 0;   // uncertainty_main computes nothing without -s (:550-553)
    fprintf(stderr, "Calculating placement uncertainty\n");
    const auto t0 = std::chrono::steady_clock::now();

    std::vector<uh::Node *> chosen;
    {
        std::ifstream in(samples);
        if (!in) { fprintf(stderr, "ERROR: could not open the indicated sample file\n"); return 1; }
        std::string line;
        while (std::getline(in, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            uh::Node *n = T.get_node(line);
            if (!n) {
                fprintf(stderr, "ERROR: Sample missing in input MAT!\n");
                fprintf(stderr, "%s\n", line.c_str());
                return 1;
            }
            chosen.push_back(n);
        }
    }
    fprintf(stderr, "Processing %ld samples\n", (long)chosen.size());

    // the tree as breadth-first arrays (the C ABI's numbering)
    const std::vector<uh::Node *> bfs = T.bfs();
    const uint64_t N = bfs.size();
    for (uint64_t j = 0; j < N; j++) { bfs[j]->flat_index = (uint32_t)j; bfs[j]->flat_epoch = 0; }
    std::vector<uint32_t> parent(N);
    std::vector<uint64_t> mut_off(N + 1, 0);
    std::vector<int32_t> pos;
    std::vector<uint8_t> ref, par, nuc;
    for (uint64_t j = 0; j < N; j++) {
        const uh::Node *n = bfs[j];
        parent[j] = n->parent ? n->parent->flat_index : UINT32_MAX;
        for (const auto &m : n->mutations) {
            pos.push_back(m.position); ref.push_back((uint8_t)m.ref_nuc); par.push_back((uint8_t)m.par_nuc); nuc.push_back((uint8_t)m.mut_nuc);
        }
        mut_off[j + 1] = pos.size();
    }
    const ugp_tree_desc desc{N, parent.data(), mut_off.data(), pos.data(), ref.data(), par.data(), nuc.data()};
    std::vector<uint32_t> nodes(chosen.size());
    for (size_t i = 0; i < chosen.size(); i++) nodes[i] = chosen[i]->flat_index;

    ugp_mat *h = nullptr;
    int rc = ugp_mat_create(&desc, device, &h);
    if (rc == UGP_OK) rc = ugp_uncertainty_attach(h, &desc);
    std::vector<uint32_t> dfs2bfs(N);
    if (rc == UGP_OK) rc = ugp_node_order(h, UGP_ORDER_DFS, dfs2bfs.data());
    const size_t n = nodes.size();
    std::vector<uint32_t> epps(n), nsize(n), tcount(n);
    uint32_t cap = 64;
    std::vector<uint32_t> ties;
    if (rc == UGP_OK) {
        ties.resize(n * cap);
        rc = ugp_uncertainty(h, nodes.data(), n, cap, epps.data(), nsize.data(), ties.data(), tcount.data());
    }
    // samples whose tie set did not fit: asked again with room for all of them
    std::vector<std::vector<uint32_t>> long_ties(n);
    if (rc == UGP_OK) {
        std::vector<uint32_t> again;
        uint32_t big = 0;
        for (size_t i = 0; i < n; i++) if (tcount[i] > cap) { again.push_back(nodes[i]); big = std::max(big, tcount[i]); }
        if (!again.empty()) {
            std::vector<uint32_t> e2(again.size()), s2(again.size()), c2(again.size()), t2((size_t)again.size() * big);
            rc = ugp_uncertainty(h, again.data(), again.size(), big, e2.data(), s2.data(), t2.data(), c2.data());
            for (size_t i = 0, k = 0; rc == UGP_OK && i < n; i++)
                if (tcount[i] > cap) { long_ties[i].assign(t2.begin() + k * big, t2.begin() + k * big + c2[k]); k++; }
        }
    }
    if (rc != UGP_OK) {
        fprintf(stderr, "ERROR: %s\n", ugp_last_error());
        if (h) ugp_mat_destroy(h);
        return 1;
    }
    ugp_mat_destroy(h);

    std::string eo = "sample\tequally_parsimonious_placements\tneighborhood_size\n", lo = "placement\tsample\n";
    for (size_t i = 0; i < n; i++) {
        const std::string &id = chosen[i]->id;
        eo += id + "\t" + std::to_string(epps[i]) + "\t" + std::to_string(nsize[i]) + "\n";
        lo += id + "\t" + id + "\n";
        if (epps[i] > 1) {
            const uint32_t *t = tcount[i] > cap ? long_ties[i].data() : &ties[i * cap];
            for (uint32_t k = 0; k < tcount[i]; k++) lo += bfs[dfs2bfs[t[k]]]->id + "\t" + id + "\n";
        } else if (epps[i] == 1) {
            lo += (chosen[i]->parent ? chosen[i]->parent->id : std::string()) + "\t" + id + "\n";   // the original parent (:245-252)
        }
    }
    if (!fepps.empty()) {
        std::ofstream f(fepps, std::ios::binary);
        f << eo;
        if (!f) { fprintf(stderr, "ERROR: could not write %s\n", fepps.c_str()); return 1; }
    }
    if (!flocs.empty()) {
        std::ofstream f(flocs, std::ios::binary);
        f << lo;
        if (!f) { fprintf(stderr, "ERROR: could not write %s\n", flocs.c_str()); return 1; }
    }
    const long ms = (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "Completed in %ld msec \n\n", ms);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) { usage(argc < 2 ? stderr : stdout); return argc < 2 ? 1 : 0; }
    if (!strcmp(argv[1], "uncertainty")) return uncertainty(argc - 2, argv + 2);
    fprintf(stderr, "ERROR: unsupported matUtils subcommand '%s' (matutils-amd runs: uncertainty)\n", argv[1]);
    return 1;
}
