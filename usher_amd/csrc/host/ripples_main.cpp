// ripples_main.cpp -- `ripples-amd`: RIPPLES' recombination search (ripples/main.cpp) with the per-branch search on the device.
//
//   ripples-amd -i tree.pb [-l 3] [-r 1000] [-R 10000000] [-d .] [-s samples.txt] [-p 3] [-n 10] [-T n] [-S s -E e] [--device k]
//
// Host side, as the reference does it: load and uncondense the MAT (:186-191), the branch list (:196-251: every non-root node
// with >= l mutations and >= n leaves, or the root paths of the names in -s), std::sort then std::shuffle with
// std::default_random_engine(0), the [S, E) slice (:291-298), the interval refinement of every event (:608-666),
// combine_intervals (:133-164) and both output files.  The search itself (:300-606) is ugp_ripples, in batches of branches.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <unordered_set>
#include <vector>

#include "mat.hpp"
#include "usher_amd.h"

namespace {

void usage(FILE *f) {
    fprintf(f,
            "Usage: ripples-amd -i tree.pb [options]\n"
            "  -i, --input-mat              input mutation-annotated tree [REQUIRED]\n"
            "  -l, --branch-length          minimum length of the branch to consider for recombination events [3]\n"
            "  -r, --min-coordinate-range   minimum range of the genomic coordinates of the mutations on the recombinant branch [1000]\n"
            "  -R, --max-coordinate-range   maximum range of the genomic coordinates of the mutations on the recombinant branch [10000000]\n"
            "  -d, --outdir                 output directory [.]\n"
            "  -s, --samples-filename       restrict the search to the ancestors of the samples in this file\n"
            "  -p, --parsimony-improvement  minimum improvement in parsimony score of the recombinant sequence [3]\n"
            "  -n, --num-descendants        minimum number of leaves of a considered branch [10]\n"
            "  -T, --threads                accepted for compatibility (the search runs on the device)\n"
            "  -S, --start-index            start index [-1]\n"
            "  -E, --end-index              end index [-1]\n"
            "      --device                 HIP device ordinal [0]\n"
            "  -h, --help                   print this message\n");
}

struct Row { int pos; int8_t ref, nuc; };

// Pruned_Sample (main.cpp:68-90) of n's root path: the lowest occurrence of a position wins, reversions drop out; by position.
std::vector<Row> pruned(const uh::Tree &T, uh::Node *n) {
    std::vector<Row> rows;
    std::unordered_set<int> seen;
    for (uh::Node *v : T.rsearch(n, true))
        for (const auto &m : v->mutations) {
            if (m.ref_nuc != m.mut_nuc && !seen.count(m.position)) {
                auto it = std::lower_bound(rows.begin(), rows.end(), m.position, [](const Row &r, int p) { return r.pos < p; });
                rows.insert(it, Row{m.position, m.ref_nuc, m.mut_nuc});
            }
            seen.insert(m.position);
        }
    return rows;
}

struct RNode { std::string name; int node_parsimony, parsimony; char is_sibling; };
struct Interval {
    RNode d, a;
    int sl, sh, el, eh;
    bool operator<(const Interval &o) const { return el < o.el; }
};
struct CompFirst {
    bool operator()(const Interval &x, const Interval &y) const { return x.sl < y.sl; }
};

// combine_intervals (main.cpp:133-164), with the same std::sort calls
std::vector<Interval> combine(std::vector<Interval> pairs) {
    std::sort(pairs.begin(), pairs.end());
    for (size_t i = 0; i < pairs.size(); i++)
        for (size_t j = i + 1; j < pairs.size(); j++)
            if (pairs[i].d.name == pairs[j].d.name && pairs[i].a.name == pairs[j].a.name && pairs[i].sl == pairs[j].sl &&
                pairs[i].sh == pairs[j].sh && pairs[i].eh == pairs[j].el &&
                pairs[i].d.parsimony + pairs[i].a.parsimony == pairs[j].d.parsimony + pairs[j].a.parsimony) {
                pairs[i].eh = pairs[j].eh;
                pairs.erase(pairs.begin() + j);
                j--;
            }
    std::sort(pairs.begin(), pairs.end(), CompFirst());
    for (size_t i = 0; i < pairs.size(); i++)
        for (size_t j = i + 1; j < pairs.size(); j++)
            if (pairs[i].d.name == pairs[j].d.name && pairs[i].a.name == pairs[j].a.name && pairs[i].el == pairs[j].el &&
                pairs[i].eh == pairs[j].eh && pairs[i].sh == pairs[j].sl &&
                pairs[i].d.parsimony + pairs[i].a.parsimony == pairs[j].d.parsimony + pairs[j].a.parsimony) {
                pairs[i].sh = pairs[j].sh;
                pairs.erase(pairs.begin() + j);
                j--;
            }
    return pairs;
}

bool has_pos(const std::vector<Row> &rows, int p) {
    for (const Row &r : rows) if (r.pos == p) return true;
    return false;
}

}  // namespace

int main(int argc, char **argv) {
    std::string mat, outdir = ".", samples;
    long l = 3, r = 1000, R = 10000000, p = 3, nd = 10, S = -1, E = -1;
    int device = 0;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        std::string v;
        auto val = [&]() -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); usage(stderr); return false; }
            v = argv[++i];
            return true;
        };
        auto num = [&](long &dst) -> bool {
            if (!val()) return false;
            char *end = nullptr;
            dst = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end) { fprintf(stderr, "ERROR: bad value '%s' for %s\n", v.c_str(), a.c_str()); usage(stderr); return false; }
            return true;
        };
        if (a == "-h" || a == "--help") { usage(stdout); return 0; }
        else if (a == "-i" || a == "--input-mat") { if (!val()) return 1; mat = v; }
        else if (a == "-d" || a == "--outdir") { if (!val()) return 1; outdir = v; }
        else if (a == "-s" || a == "--samples-filename") { if (!val()) return 1; samples = v; }
        else if (a == "-l" || a == "--branch-length") { if (!num(l)) return 1; }
        else if (a == "-r" || a == "--min-coordinate-range") { if (!num(r)) return 1; }
        else if (a == "-R" || a == "--max-coordinate-range") { if (!num(R)) return 1; }
        else if (a == "-p" || a == "--parsimony-improvement") { if (!num(p)) return 1; }
        else if (a == "-n" || a == "--num-descendants") { if (!num(nd)) return 1; }
        else if (a == "-S" || a == "--start-index") { if (!num(S)) return 1; }
        else if (a == "-E" || a == "--end-index") { if (!num(E)) return 1; }
        else if (a == "-T" || a == "--threads") { if (!val()) return 1; }
        else if (a == "--device") { if (!val()) return 1; device = atoi(v.c_str()); }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); usage(stderr); return 1; }
    }
    if (mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); usage(stderr); return 1; }
    if (l < 1 || p < 0 || nd < 0) { fprintf(stderr, "ERROR: ripples-amd needs -l >= 1, -p >= 0 and -n >= 0\n"); return 1; }

    fprintf(stderr, "Loading input MAT file %s.\n", mat.c_str());
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    T.uncondense_leaves();
    const uh::TreeArrays A(T);   // the tree as breadth-first arrays (the C ABI's numbering)
    const std::vector<uh::Node *> &bfs = A.bfs;
    const uint64_t N = bfs.size();

    // the branches to consider (:196-251)
    std::unordered_set<std::string> chosen;
    if (!samples.empty()) {
        std::ifstream in(samples);
        if (!in) { fprintf(stderr, "ERROR: Could not open the samples file: %s!\n", samples.c_str()); return 1; }
        fprintf(stderr, "Reading samples from the file %s.\n", samples.c_str());
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::vector<std::string> words;
            std::string w;
            while (ss >> w) words.push_back(w);
            if (words.size() != 1) { fprintf(stderr, "ERROR: Incorrect format for samples file: %s!\n", samples.c_str()); return 1; }
            uh::Node *n = T.get_node(words[0]);
            if (!n) { fprintf(stderr, "ERROR: Node id %s not found!\n", words[0].c_str()); return 1; }
            for (uh::Node *anc : T.rsearch(n, true)) chosen.insert(anc->id);
        }
    } else {
        std::vector<size_t> nleaves(N, 0);   // get_num_leaves: true leaves
        for (uint64_t j = N; j-- > 0;) {
            if (bfs[j]->is_leaf()) nleaves[j] = 1;
            if (j) nleaves[bfs[j]->parent->flat_index] += nleaves[j];
        }
        for (uint64_t j = 1; j < N; j++)
            if (bfs[j]->mutations.size() >= (size_t)l && nleaves[j] >= (size_t)nd) chosen.insert(bfs[j]->id);
    }
    std::vector<std::string> names(chosen.begin(), chosen.end());
    std::sort(names.begin(), names.end());
    std::shuffle(names.begin(), names.end(), std::default_random_engine(0));
    fprintf(stderr, "Found %zu long branches\n", names.size());

    mkdir(outdir.c_str(), 0777);   // boost::filesystem::create_directory: one level, an existing directory is fine
    const std::string desc_fn = outdir + "/descendants.tsv", recomb_fn = outdir + "/recombination.tsv";
    FILE *desc_file = fopen(desc_fn.c_str(), "w");
    FILE *recomb_file = fopen(recomb_fn.c_str(), "w");
    if (!desc_file || !recomb_file) { fprintf(stderr, "ERROR: could not create the output files in %s\n", outdir.c_str()); return 1; }
    fprintf(desc_file, "#node_id\tdescendants\n");
    fprintf(recomb_file,
            "#recomb_node_id\tbreakpoint-1_interval\tbreakpoint-2_interval\tdonor_node_id\tdonor_is_sibling\tdonor_parsimony\tacceptor_node_id"
            "\tacceptor_is_sibling\tacceptor_parsimony\toriginal_parsimony\tmin_starting_parsimony\trecomb_parsimony\n");

    size_t s = 0, e = names.size();
    if (S >= 0 && E >= 0) {
        s = (size_t)S;
        if (E <= (long)e) e = (size_t)E;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<uint32_t> rank = A.name_rank();
    const ugp_tree_desc tdesc = A.desc();
    ugp_mat *h = nullptr;
    int rc = s < e ? ugp_mat_create(&tdesc, device, &h) : UGP_OK;
    if (rc == UGP_OK && h) rc = ugp_ripples_attach(h, &tdesc, rank.data());
    const ugp_ripples_opts o{(uint32_t)l, (int32_t)r, (int32_t)R, (int32_t)p, (uint32_t)nd};
    const size_t kBatch = 256;
    size_t num_done = 0;
    std::vector<ugp_ripples_event> ev(4096);
    for (size_t b0 = s; rc == UGP_OK && b0 < e; b0 += kBatch) {
        const size_t b1 = std::min(e, b0 + kBatch);
        std::vector<uint32_t> br;
        for (size_t x = b0; x < b1; x++) br.push_back(T.get_node(names[x])->flat_index);
        uint64_t n_out = 0;
        rc = ugp_ripples(h, &o, br.data(), br.size(), ev.data(), ev.size(), &n_out);
        if (rc == UGP_OK && n_out > ev.size()) {
            ev.resize(n_out);
            rc = ugp_ripples(h, &o, br.data(), br.size(), ev.data(), ev.size(), &n_out);
        }
        if (rc != UGP_OK) break;
        size_t x = 0;
        for (size_t bi = 0; bi < br.size(); bi++) {
            uh::Node *nid = bfs[br[bi]];
            fprintf(stderr, "At node id: %s\n", nid->id.c_str());
            const int orig = (int)nid->mutations.size();
            const std::vector<Row> ps = pruned(T, nid);
            std::vector<Interval> valid;
            for (; x < n_out && ev[x].branch == bi; x++) {
                const ugp_ripples_event &q = ev[x];
                int sh = ps[q.i].pos, sl = q.i >= 1 ? ps[q.i - 1].pos : 0, el = q.j >= 1 ? ps[q.j - 1].pos : 0, eh = 1000000000;
                // the refinement against the donor's own root path (:608-666)
                const std::vector<Row> dn = pruned(T, bfs[q.donor]);
                for (const Row &m : dn) {
                    if (m.pos > sl && m.pos <= sh && !has_pos(ps, m.pos)) sl = m.pos;
                    if (m.pos > el && m.pos <= eh && !has_pos(ps, m.pos)) eh = m.pos;
                }
                for (const Row &m : ps) {
                    if (m.pos > sl && m.pos <= sh && !has_pos(dn, m.pos)) sl = m.pos;
                    if (m.pos > el && m.pos <= eh && !has_pos(dn, m.pos)) eh = m.pos;
                }
                valid.push_back(Interval{RNode{bfs[q.donor]->id, q.donor_score, (int)q.donor_count, q.donor_sibling ? 'y' : 'n'},
                                         RNode{bfs[q.acceptor]->id, q.acceptor_score, (int)q.acceptor_count, q.acceptor_sibling ? 'y' : 'n'},
                                         sl, sh, el, eh});
            }
            const bool has_recomb = !valid.empty();
            for (const Interval &pr : combine(valid)) {
                const std::string ehs = pr.eh == 1000000000 ? "GENOME_SIZE" : std::to_string(pr.eh);
                fprintf(recomb_file, "%s\t(%i,%i)\t(%i,%s)\t%s\t%c\t%i\t%s\t%c\t%i\t%i\t%i\t%i\n", nid->id.c_str(), pr.sl, pr.sh, pr.el, ehs.c_str(),
                        pr.d.name.c_str(), pr.d.is_sibling, pr.d.node_parsimony, pr.a.name.c_str(), pr.a.is_sibling, pr.a.node_parsimony, orig,
                        std::min({orig, pr.d.node_parsimony, pr.a.node_parsimony}), pr.d.parsimony + pr.a.parsimony);
            }
            if (has_recomb) {
                fprintf(desc_file, "%s\t", nid->id.c_str());
                for (uh::Node *lf : T.leaves(nid)) fprintf(desc_file, "%s,", lf->id.c_str());
                fprintf(desc_file, "\n");
                fprintf(stderr, "Done %zu/%zu branches [RECOMBINATION FOUND!]\n\n", ++num_done, names.size());
            } else {
                fprintf(stderr, "Done %zu/%zu branches\n\n", ++num_done, names.size());
            }
        }
    }
    if (h) ugp_mat_destroy(h);
    fclose(desc_file);
    fclose(recomb_file);
    if (rc != UGP_OK) { fprintf(stderr, "ERROR: %s\n", ugp_last_error()); return 1; }
    const long ms = (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "Completed in %ld msec \n\n", ms);
    return 0;
}
