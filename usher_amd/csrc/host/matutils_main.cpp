// matutils_main.cpp -- `matutils-amd`: the matUtils subcommands this project runs on the GPU.
//
//   matutils-amd uncertainty -i tree.pb -s samples.txt [-e epps.tsv] [-o placements.tsv] [-T n] [--device k]
//   matutils-amd annotate -i tree.pb -o out.pb [-c | -M | -P | -C file ...] [-f -m -s -p -l -d -u -D -T] [--device k]
//   matutils-amd extract -i tree.pb [-s samples.txt] [-k sample:k] [-Y y] [-a -b -P n] [-u -t -o -v file] [-n] [-d dir] [--reference-ties]
//                        [--host-genotypes]
//   matutils-amd summarize -i tree.pb [-s -c -C -m -a -R file ...] [-A] [-M] [-d dir] [--host]
//   matutils-amd translate -i tree.pb -g genes.gtf -f ref.fa -t out.tsv [-d dir] [--host]
//   matutils-amd relatives -i tree.pb [-s samples.txt] [-V closest.tsv [-q]] [--within-distance within.tsv [--distance-threshold n]] [--host]
//   matutils-amd select   extract's options and [-I node] [-c clades] [-m mutations] [-H regex] [-e n] [-U] [-p] [--host]
//   matutils-amd mask -i tree.pb -o out.pb [-s samples.txt] [-m mutations.tsv] [-r rename.tsv] [-c] [--host]
//
// uncertainty_main / findEPPs_wrapper (uncertainty.cpp:279-339, 541-560): load the MAT, uncondense its leaves, read the sample
// names, and for every sample report its equally parsimonious placements and neighborhood size (-e) and the candidate parents
// (-o), in the reference's file formats.  The per-sample searches run on the device as one batch (ugp_uncertainty).
// annotate_main (annotate.cpp:94-156): clade roots from exemplar samples, mutation sets, paths or node ids, written into the
// .pb metadata.  Exemplar allele counts, the searches and the overlap counts run on the device (ugp_annotate.hip).
// extract_main (extract.cpp:149-640): sample selection by name, nearest-k context (-k, -Y: get_nearby, one batched ugp_nearest_k
// call) and the three linear filters, written as a sample list, a newick tree, a .pb of the induced subtree or its VCF (-v:
// make_vcf, convert.cpp:14-320; site table and genotype codes from ugp_genotypes.hip, formatted here chunk by chunk).
// summary_main (summary.cpp:635-776), as the subcommand `summarize`: the sample, clade, sample-clade, mutation, aberrant and RoHo tables and the basic counts; the
// numbers of -m, -R, -c and -C come from ugp_summary.hip, --host computes them with the reference's serial walks instead.
// summary --translate (translate.cpp: translate_main, do_mutations), as the subcommand `translate`: per node the amino-acid, nucleotide
// and codon changes and the leaves below it.  The codon letters come from ugp_translate.hip; a tree whose stored parent alleles
// disagree with the states above them (every mutated - strand gene), or --host, takes the reference's serial do / undo walk.
// extract --closest-relatives / --within-distance (extract.cpp:768-823), as the subcommand `relatives`: per sample its closest
// leaves, or those within a distance (get_closest_samples, select.cpp:577-714).  The lists come from ugp_relatives.hip; --host
// runs the reference's walk statement by statement.  `extract` itself goes on refusing the four options.
// extract's selectors -I -c -m -H -e -U -p (extract.cpp:294-373, 411-427, 455-472), as the subcommand `select`, which shares extract's
// body: the selections are bitmaps over leaf ranks from ugp_select.hip, -e asks ugp_uncertainty; --host runs the reference's walks.
// mask_main (mask.cpp:68-159), as the subcommand `mask`: -s (restrictSamples) and -m (restrictMutationsLocally) ask ugp_mask.hip which
// entries to mask or remove and apply the answer to the host tree; -r, -c and the writer run on the host; --host walks as the reference.
// get_subtree (mutation_annotated_tree.cpp:1577-1685), as the subcommand `subtree`: select's body, with the induced subtree of the
// selection from ugp_subtree.hip (kept nodes, subtree parents, merged entries, chain owners) instead of the pairwise walk; --host runs it.
// extract -N (get_minimum_subtrees, convert.cpp:665-798), as the subcommand `subtrees`: select's body, then the greedy cover of the
// samples by nearest-N neighbourhoods in rounds of batched searches (ugp_nearest_k) and every neighbourhood's induced subtree from one
// ugp_subtree_batch call per round, written as <name>-subtree-<i>.nw and subtree-assignments.tsv; --host runs get_nearby and get_subtree.
#include <hip/hip_runtime_api.h>
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <map>
#include <regex>
#include <set>
#include <sstream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "driver.hpp"
#include "mat.hpp"
#include "par.hpp"
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
            "  (-d / --dropout-mutations is not supported)\n"
            "       matutils-amd annotate --help | matutils-amd extract --help | matutils-amd summarize --help | matutils-amd translate --help\n"
            "       matutils-amd relatives --help | matutils-amd select --help | matutils-amd mask --help | matutils-amd haplotypes --help\n"
            "       matutils-amd subtree --help | matutils-amd subtrees --help\n");
}

[[noreturn]] void lib_fail(const char *what) {
    fprintf(stderr, "ERROR: %s: %s\n", what, ugp_last_error());
    exit(1);
}

// The library's handle of one tree (the tree itself comes as uh::TreeArrays), destroyed with its owner.
struct Mat {
    ugp_mat *h = nullptr;
    Mat() = default;
    Mat(const Mat &) = delete;
    Mat &operator=(const Mat &) = delete;
    ~Mat() { if (h) ugp_mat_destroy(h); }
    void create(const ugp_tree_desc &desc, int device) { if (ugp_mat_create(&desc, device, &h) != UGP_OK) lib_fail("ugp_mat_create"); }
    operator ugp_mat *() const { return h; }
};

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

    const uh::TreeArrays A(T);
    const std::vector<uh::Node *> &bfs = A.bfs;
    const uint64_t N = bfs.size();
    const ugp_tree_desc desc = A.desc();
    std::vector<uint32_t> nodes(chosen.size());
    for (size_t i = 0; i < chosen.size(); i++) nodes[i] = chosen[i]->flat_index;

    Mat h;   // (created here and not by create(): this subcommand reports a failure without the call's name)
    int rc = ugp_mat_create(&desc, device, &h.h);
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
        return 1;
    }

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

// ---- annotate (annotate.cpp) --------------------------------------------------------------------------------------

void annotate_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd annotate -i tree.pb -o out.pb [-c names.tsv] [-C clade_to_nid.tsv] [-P paths.tsv] [-M mutations.tsv]\n"
            "       [-f 0.8] [-m 0.2] [-s 0.6] [-p 0.1] [-l] [-d dir] [-u mutations.tsv] [-D details.tsv] [-T n] [--device k]\n"
            "  -i, --input-mat              input mutation-annotated tree [REQUIRED]\n"
            "  -o, --output-mat             output mutation-annotated tree [REQUIRED]\n"
            "  -c, --clade-names            tsv of clade assignments of samples (clade roots are searched for)\n"
            "  -C, --clade-to-nid           tsv mapping clades to internal node identifiers\n"
            "  -P, --clade-paths            tsv mapping clades to mutation paths\n"
            "  -M, --clade-mutations        tsv mapping clades to sets of mutations\n"
            "  -f, --allele-frequency       minimum allele frequency in the -c samples [0.8]\n"
            "  -m, --mask-frequency         minimum allele frequency below -f that is masked [0.2]\n"
            "  -s, --set-overlap            minimum fraction of the clade samples below the clade root [0.6]\n"
            "  -p, --clip-sample-frequency  maximum proportion of exemplars in a branch when sorting candidates [0.1]\n"
            "  -l, --clear-current          remove current annotations first\n"
            "  -d, --output-directory       directory of the output files [./]\n"
            "  -u, --write-mutations        tsv of each clade's mutations found in at least -f of the samples\n"
            "  -D, --write-details          tsv of details about the nodes considered for each clade root\n"
            "  -T, --threads                accepted for compatibility (the searches run on the device)\n"
            "      --device                 HIP device ordinal [0]\n");
}

void split_delim(const std::string &s, char delim, std::vector<std::string> &words) {   // string_split, :383-398
    size_t start = 0, end;
    while ((end = s.find(delim, start)) != std::string::npos) {
        words.emplace_back(s.substr(start, end - start));
        start = end + 1;
    }
    std::string last = s.substr(start);
    if (!last.empty()) words.push_back(last);
}
void split_ws(const std::string &s, std::vector<std::string> &words) {   // string_split, :401-413
    std::istringstream ss(s);
    std::string w;
    while (ss >> w) words.push_back(w);
}
bool mutation_from_string(const std::string &s, uh::Mutation &m) {   // mutation_annotated_tree.cpp:358-380
    char ref, alt;
    int position;
    if (sscanf(s.c_str(), "%c%d%c", &ref, &position, &alt) != 3 || ref < 'A' || ref > 'Z' || alt < 'A' || alt > 'Z') {
        fprintf(stderr, "mutation_from_string: expected /[A-Z][0-9]+[A-Z/, got '%s'\n", s.c_str());
        return false;
    }
    m = uh::Mutation();
    m.ref_nuc = uh::nuc_id(ref);
    m.position = position;
    m.mut_nuc = uh::nuc_id(alt);
    m.par_nuc = m.ref_nuc;
    if (m.str() != s) {
        fprintf(stderr, "mutation_from_string: unexpected characters at the end of '%s'\n", s.c_str());
        return false;
    }
    return true;
}
bool by_position(const uh::Mutation &a, const uh::Mutation &b) { return a.position < b.position; }

std::string node_mutations_string(const uh::Node *n) {
    std::string s = n->id + ":";
    for (size_t i = 0; i < n->mutations.size(); i++) { if (i) s += ','; s += n->mutations[i].str(); }
    return s;
}
std::string path_to_node(const uh::Node *n) {   // :437-455
    std::vector<std::string> parts;
    for (const uh::Node *a = n; a; a = a->parent) parts.push_back(node_mutations_string(a));
    std::string path;
    for (size_t k = parts.size(); k-- > 0;) { path += parts[k]; if (k) path += " > "; }
    return path;
}
void write_mutations(FILE *f, const std::vector<uh::Mutation> &ms, bool unmasked, bool masked) {   // :457-471
    bool got = false;
    for (const auto &m : ms) {
        const std::string s = m.str();
        const bool is_masked = s.back() == 'N';
        if ((unmasked && !is_masked) || (masked && is_masked)) { if (got) fprintf(f, ", "); fprintf(f, "%s", s.c_str()); got = true; }
    }
}
FILE *must_open(const std::string &name, const char *mode) {
    FILE *f = fopen(name.c_str(), mode);
    if (!f) { fprintf(stderr, "ERROR: Could not open file '%s' with mode '%s'\n", name.c_str(), mode); exit(1); }
    return f;
}

void init_annotations(const std::vector<uh::Node *> &dfs, bool clear) {   // :158-168
    for (uh::Node *n : dfs) { if (clear) n->clade_annotations.clear(); n->clade_annotations.emplace_back(""); }
    // the reference indexes every node's annotations with the root's count: nodes with fewer would be read out of bounds
    for (const uh::Node *n : dfs)
        if (n->clade_annotations.size() != dfs[0]->clade_annotations.size()) {
            fprintf(stderr, "ERROR: the nodes of the input MAT carry different numbers of clade annotations (use --clear-current)\n");
            exit(1);
        }
}

void lineages_from_nids(uh::Tree &T, const std::string &fname, bool clear) {   // assignLineages(T, clade_to_nid, clear), :170-206
    init_annotations(T.dfs(), clear);
    const size_t na = T.num_annotations();
    std::ifstream in(fname);
    if (!in) { fprintf(stderr, "ERROR: Could not open the clade to node id assignment file: %s!\n", fname.c_str()); exit(1); }
    fprintf(stderr, "Reading clade to node id assignment file and completing assignments.\n");
    std::string line;
    while (std::getline(in, line)) {
        std::vector<std::string> w;
        split_delim(line, '\t', w);
        if (w.size() > 2 || w.size() == 1) { fprintf(stderr, "ERROR: Incorrect format for clade to node id assignment file: %s!\n", fname.c_str()); exit(1); }
        if (w.empty()) { fprintf(stderr, "ERROR: Node id  not found!\n"); exit(1); }   // words[1] of an empty line: no such node
        uh::Node *n = T.get_node(w[1]);
        if (!n) { fprintf(stderr, "ERROR: Node id %s not found!\n", w[1].c_str()); exit(1); }
        if (n->clade_annotations[na - 1] != "")
            fprintf(stderr, "WARNING: Assigning clade %s to node %s failed as the node is already assigned to clade %s!\n", w[0].c_str(),
                    w[1].c_str(), n->clade_annotations[na - 1].c_str());
        else n->clade_annotations[na - 1] = w[0];
    }
}

bool node_has_muts(const uh::Node *n, const std::vector<std::string> &muts) {   // :808-830
    if (n->mutations.size() != muts.size()) return false;
    for (const auto &m : n->mutations) if (std::find(muts.begin(), muts.end(), m.str()) == muts.end()) return false;
    return true;
}

void lineages_from_paths(uh::Tree &T, const std::string &fname, std::unordered_set<std::string> &done) {   // :832-913
    const size_t na = T.num_annotations();
    std::ifstream in(fname);
    if (!in) { fprintf(stderr, "ERROR: Could not open the clade paths file: %s!\n", fname.c_str()); exit(1); }
    fprintf(stderr, "Reading clade paths file and making assignments.\n");
    int found = 0, failed_n = 0;
    std::string line;
    while (std::getline(in, line)) {
        std::vector<std::string> w;
        split_delim(line, '\t', w);
        if (w.size() == 1 && !line.empty() && line.back() == '\t') w.push_back("");
        if (w.size() != 2) {
            fprintf(stderr, "ERROR: Incorrect format for clade paths file: %s!  Expected 2 tab-separated words, got %ld (%s)\n", fname.c_str(),
                    (long)w.size(), line.c_str());
            exit(1);
        }
        const std::string clade = w[0];
        if (done.count(clade)) { fprintf(stderr, "Clade %s has already been assigned, ignoring path.\n", clade.c_str()); continue; }
        std::vector<std::string> pw;
        split_ws(w[1], pw);
        uh::Node *node = T.root;
        bool failed = false;
        for (const std::string &el : pw) {
            if (el.empty() || el == ">") continue;
            std::vector<std::string> muts;
            split_delim(el, ',', muts);
            uh::Node *kid = nullptr;
            for (uh::Node *c : node->children) if (node_has_muts(c, muts)) { kid = c; break; }
            if (!kid) {
                fprintf(stderr, "WARNING: path for %s not found: no child of node %s has mutations %s (path %s)\n", clade.c_str(), node->id.c_str(),
                        el.c_str(), line.c_str());
                failed = true; failed_n++;
                break;
            }
            node = kid;
        }
        if (failed) continue;
        if (node->clade_annotations[na - 1] != "")
            fprintf(stderr, "WARNING: Assigning clade %s to node %s for path %s failed as the node is already assigned to clade %s!\n", clade.c_str(),
                    node->id.c_str(), w[1].c_str(), node->clade_annotations[na - 1].c_str());
        else node->clade_annotations[na - 1] = clade;
        done.insert(clade);
        found++;
    }
    fprintf(stderr, "\nAnnotated %d clades; failed to find paths for %d clades\n", found, failed_n);
}

void parse_clade_mutations(const std::string &fname, std::map<std::string, std::vector<uh::Mutation>> &out,
                           const std::unordered_set<std::string> &done) {   // :208-299
    std::ifstream in(fname);
    if (!in) { fprintf(stderr, "ERROR: Could not open the clade mutations file: %s!\n", fname.c_str()); exit(1); }
    std::map<std::string, std::vector<uh::Mutation>> all;
    fprintf(stderr, "Reading clade mutations file %s.\n", fname.c_str());
    bool got_error = false;
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '#') continue;
        std::vector<std::string> w;
        split_delim(line, '\t', w);
        if (w.size() == 1 && !line.empty() && line.back() == '\t') w.push_back("");
        if (w.size() != 2) {
            fprintf(stderr, "ERROR: Incorrect format for clade mutations file: %s!  Expected 2 tab-separated words, got %ld (%s)\n", fname.c_str(),
                    (long)w.size(), line.c_str());
            got_error = true;
            continue;
        }
        const std::string clade = w[0];
        if (all.count(clade)) { fprintf(stderr, "ERROR: clade %s is defined on multiple lines\n", clade.c_str()); got_error = true; continue; }
        uh::Node node;
        std::vector<std::string> mw;
        split_ws(w[1], mw);
        if (!mw.empty()) {
            auto it = all.find(mw[0]);
            if (it != all.end()) { node.mutations = it->second; mw.erase(mw.begin()); }
        }
        for (const std::string &el : mw) {
            if (el.empty() || el == ">") continue;
            std::vector<std::string> ms;
            split_delim(el, ',', ms);
            for (const std::string &s : ms) {
                if (s.empty()) continue;
                uh::Mutation m;
                if (!mutation_from_string(s, m)) {
                    fprintf(stderr, "Unable to parse mutation '%s' for %s element %s\n", s.c_str(), clade.c_str(), el.c_str());
                    got_error = true;
                } else if (!node.add_mutation(m)) {
                    exit(1);
                }
            }
        }
        all[clade] = node.mutations;
    }
    for (const auto &kv : all) if (!done.count(kv.first)) out[kv.first] = kv.second;
    if (got_error) { fprintf(stderr, "Encountered errors -- exiting.\n"); exit(1); }
}

struct NodeFreq {   // Node_freq, :544-557
    size_t best_j;
    float freq, overlap, freq_clipped;
    NodeFreq(size_t a, float b, float c, float clip) : best_j(a), freq(b), overlap(c), freq_clipped(b > clip ? clip : b) {}
    bool operator<(const NodeFreq &n) const { return (freq_clipped * overlap * overlap) > (n.freq_clipped * n.overlap * n.overlap); }
};
struct CladeAssignment {   // Clade_Assignments, :559-583
    std::string clade_name;
    size_t clade_size;
    std::vector<NodeFreq> best_node_frequencies;
    std::vector<uh::Mutation> mutations;
    CladeAssignment(std::string name, size_t sz, std::vector<uh::Mutation> muts) : clade_name(std::move(name)), clade_size(sz), mutations(std::move(muts)) {}
    bool operator<(const CladeAssignment &c) const {
        if (clade_size == 0 && c.clade_size > 0) return true;
        if (clade_size > 0 && c.clade_size == 0) return false;
        return best_node_frequencies.size() < c.best_node_frequencies.size() ||
               (best_node_frequencies.size() == c.best_node_frequencies.size() && clade_size > c.clade_size);
    }
};

// assignLineages(T, clade_names, clade_mutations, clade_paths, ...), :483-806; the searches and counts on the device
void lineages(uh::Tree &T, const std::string &fnames, const std::string &fmuts, const std::string &fpaths, float min_freq, float mask_freq,
              float set_overlap, float clip, bool clear, const std::string &fmutsout, const std::string &fdetails, int device) {
    const std::vector<uh::Node *> dfs = T.dfs();
    const size_t N = dfs.size();
    FILE *mf = nullptr, *df = nullptr;
    if (!fmutsout.empty()) {
        fprintf(stderr, "Writing clade root node mutations to file %s\n", fmutsout.c_str());
        mf = must_open(fmutsout, "w");
        fprintf(mf, "clade\tmutations\n");
    }
    if (!fdetails.empty()) {
        fprintf(stderr, "Writing details to file %s\n", fdetails.c_str());
        df = must_open(fdetails, "w");
        fprintf(df, "clade\tmutations\tmasked_mutations\tnode:freq:overlap\talready_assigned\tfinal_overlap\texemplar_count\tbest_node_path\n");
    }
    fprintf(stderr, "Initializing annotations.\n");
    init_annotations(dfs, clear);
    const size_t na = T.num_annotations();
    // flat_index = the breadth-first index (nothing below renumbers T's nodes; the copy U has its own); dfs_idx = position in `dfs`
    const uh::TreeArrays A(T, uh::TreeArrays::kEntries);
    const std::vector<const uh::Mutation *> &ent = A.ent;
    std::unordered_map<const uh::Node *, uint32_t> dfs_idx;
    for (size_t j = 0; j < N; j++) dfs_idx[dfs[j]] = (uint32_t)j;
    // leaves below each node (get_num_leaves), by depth-first position
    std::vector<size_t> leaves(N, 0);
    for (size_t k = N; k-- > 0;) {
        if (dfs[k]->is_leaf()) leaves[k] = 1;
        if (dfs[k]->parent) leaves[dfs_idx[dfs[k]->parent]] += leaves[k];
    }

    std::unordered_set<std::string> done;
    if (!fpaths.empty()) lineages_from_paths(T, fpaths, done);
    std::map<std::string, std::vector<uh::Mutation>> clade_muts;
    std::map<std::string, std::vector<uh::Node *>> clade_map;   // exemplars, as nodes of T (looked up by the copy's names)
    if (!fmuts.empty()) parse_clade_mutations(fmuts, clade_muts, done);

    Mat h;
    auto device_up = [&]() {
        if (h) return;
        const ugp_tree_desc desc = A.desc();
        h.create(desc, device);
        if (ugp_annotate_attach(h, &desc) != UGP_OK) lib_fail("ugp_annotate_attach");
    };

    std::map<std::string, std::vector<uint32_t>> clade_copy_dfs;   // exemplars as depth-first positions of the copy (= of T)
    std::map<std::string, std::vector<std::string>> clade_names;   // ... and their names in the copy
    if (!fnames.empty()) {
        fprintf(stderr, "Copying tree with uncondensed leaves.\n");
        uh::Tree U;
        std::string err;
        if (!uh::copy_tree(T, U, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); exit(1); }
        if (!U.condensed_nodes.empty()) U.uncondense_leaves();
        const std::vector<uh::Node *> udfs = U.dfs();
        if (udfs.size() != N) { fprintf(stderr, "ERROR: the tree copy has a different node count\n"); exit(1); }
        std::unordered_map<const uh::Node *, uint32_t> udfs_idx;
        for (size_t k = 0; k < N; k++) udfs_idx[udfs[k]] = (uint32_t)k;
        std::ifstream in(fnames);
        if (!in) { fprintf(stderr, "ERROR: Could not open the clade assignment file: %s!\n", fnames.c_str()); exit(1); }
        fprintf(stderr, "Reading clade assignment file %s.\n", fnames.c_str());
        std::string line;
        while (std::getline(in, line)) {
            std::vector<std::string> w;
            split_delim(line, '\t', w);
            if (w.size() > 2 || w.size() == 1) {
                fprintf(stderr, "ERROR: Incorrect format for clade assignment file: %s!  Expected 2 tab-separated words, got %ld\n", fnames.c_str(), (long)w.size());
                exit(1);
            }
            if (w.size() != 2) continue;
            if (clade_muts.count(w[0]) || done.count(w[0])) continue;
            uh::Node *n = U.get_node(w[1]);
            if (!n) { fprintf(stderr, "WARNING: Sample %s not found in input MAT!\n", w[1].c_str()); continue; }
            clade_copy_dfs[w[0]].push_back(udfs_idx[n]);
            clade_names[w[0]].push_back(n->id);
        }
        // the mutations of each clade's exemplars (:355-390): one device call for all clades
        std::vector<uint64_t> coff(1, 0);
        std::vector<uint32_t> xs;
        std::vector<uint32_t> dfs2bfs(N);
        for (size_t k = 0; k < N; k++) dfs2bfs[k] = dfs[k]->flat_index;
        for (const auto &kv : clade_copy_dfs) {
            for (uint32_t d : kv.second) xs.push_back(dfs2bfs[d]);
            coff.push_back(xs.size());
        }
        const uint64_t nc = clade_copy_dfs.size();
        std::vector<uint64_t> ooff(nc + 1);
        uint64_t cap = std::max<uint64_t>(1024, 8 * xs.size()), n_out = 0;
        std::vector<uint32_t> oe, oc;
        if (nc) {
            device_up();
            for (;;) {
                oe.resize(cap); oc.resize(cap);
                if (ugp_clade_alleles(h, coff.data(), xs.data(), nc, ooff.data(), oe.data(), oc.data(), cap, &n_out) != UGP_OK) lib_fail("ugp_clade_alleles");
                if (n_out <= cap) break;
                cap = n_out;
            }
        }
        size_t c = 0;
        for (const auto &kv : clade_copy_dfs) {
            const std::string &clade = kv.first;
            fprintf(stderr, "Finding mutations in clade %s samples.\n", clade.c_str());
            std::map<std::string, int> counts;
            for (uint64_t k = ooff[c]; k < ooff[c + 1]; k++) {
                const uh::Mutation &m = *ent[oe[k]];
                counts[T.chroms[m.chrom] + "\t" + std::to_string(m.ref_nuc) + "\t" + std::to_string(m.position) + "\t" + std::to_string(m.mut_nuc)] += (int)oc[k];
            }
            std::vector<uh::Mutation> rows;
            const size_t k_ex = kv.second.size();
            for (const auto &mc : counts) {
                const float f = static_cast<float>(mc.second) / k_ex;
                if (!(f >= min_freq) && !(f >= mask_freq)) continue;
                std::vector<std::string> w;
                split_ws(mc.first, w);
                uh::Mutation m;
                m.chrom = T.chrom_id(w.size() == 4 ? w[0] : std::string());
                const size_t o = w.size() == 4 ? 1 : 0;
                m.ref_nuc = (int8_t)std::stoi(w[o]);
                m.par_nuc = m.ref_nuc;
                m.position = std::stoi(w[o + 1]);
                m.mut_nuc = f >= min_freq ? (int8_t)std::stoi(w[o + 2]) : uh::nuc_id('N');
                rows.push_back(m);
            }
            clade_muts[clade] = rows;
            // get_freq_overlap looks the exemplars up in T by the copy's names (:470, :675)
            std::vector<uh::Node *> &ex = clade_map[clade];
            for (const std::string &id : clade_names[clade]) {
                uh::Node *n = T.get_node(id);
                if (!n) {
                    fprintf(stderr, "ERROR: exemplar %s of clade %s names no node of the input MAT after the tree copy renumbered its internal "
                            "nodes\n", id.c_str(), clade.c_str());
                    exit(1);
                }
                ex.push_back(n);
            }
            c++;
        }
    }

    // the searches (:611-638), UGP_ORDER_DFS over every node; one batched call for the packed rows, the literal one for the rest
    std::vector<std::string> order;
    std::vector<std::vector<uh::Mutation>> rows_of;
    for (auto &kv : clade_muts) {
        std::sort(kv.second.begin(), kv.second.end(), by_position);   // :586
        order.push_back(kv.first);
        rows_of.push_back(kv.second);
    }
    const size_t nc = order.size();
    std::vector<int32_t> best(nc, 0);
    std::vector<std::vector<uint32_t>> ties(nc);
    if (nc) {
        device_up();
        std::vector<size_t> packed, literal;
        for (size_t i = 0; i < nc; i++) {
            bool awk = rows_of[i].empty();
            for (size_t k = 0; k < rows_of[i].size(); k++)
                awk = awk || rows_of[i][k].position < 0 || (k && rows_of[i][k].position == rows_of[i][k - 1].position);
            (awk ? literal : packed).push_back(i);
        }
        auto batch = [&](const std::vector<size_t> &which, std::vector<uint64_t> &off, std::vector<int32_t> &qp, std::vector<uint8_t> &qr,
                         std::vector<uint8_t> &qn, std::vector<uint8_t> &qm) {
            off.assign(1, 0); qp.clear(); qr.clear(); qn.clear();
            for (size_t i : which) {
                for (const auto &m : rows_of[i]) { qp.push_back(m.position); qr.push_back((uint8_t)m.ref_nuc); qn.push_back((uint8_t)m.mut_nuc); }
                off.push_back(qp.size());
            }
            qm.assign(qp.size(), 0);   // the reference never sets is_missing on these rows (:397, :407); 0 as mutation_from_string gives
            return ugp_queries{which.size(), off.data(), qp.data(), qr.data(), qn.data(), qm.data()};
        };
        std::vector<uint64_t> off;
        std::vector<int32_t> qp;
        std::vector<uint8_t> qr, qn, qm;
        for (int pass = 0; pass < 2; pass++) {
            const std::vector<size_t> &which = pass ? literal : packed;
            if (which.empty()) continue;
            const ugp_queries q = batch(which, off, qp, qr, qn, qm);
            uint32_t cap = 64;
            std::vector<uint32_t> tj((size_t)which.size() * cap), tc(which.size());
            std::vector<int32_t> sb(which.size());
            if (pass == 0) {
                ugp_place_opts o{UGP_ORDER_DFS, nullptr, nullptr, nullptr, nullptr};
                std::vector<ugp_result> res(which.size());
                std::vector<uint8_t> hu(tj.size());
                if (ugp_place_batch_ex(h, &q, &o, res.data()) != UGP_OK) lib_fail("ugp_place_batch_ex");
                if (ugp_tied_nodes_ex(h, &q, &o, cap, tj.data(), hu.data(), tc.data()) != UGP_OK) lib_fail("ugp_tied_nodes_ex");
                for (size_t k = 0; k < which.size(); k++) sb[k] = res[k].best_set_difference;
            } else if (ugp_annotate_search(h, &q, cap, sb.data(), tj.data(), tc.data()) != UGP_OK) {
                lib_fail("ugp_annotate_search");
            }
            for (size_t k = 0; k < which.size(); k++) {
                const size_t i = which[k];
                best[i] = sb[k];
                if (tc[k] <= cap) { ties[i].assign(tj.begin() + k * cap, tj.begin() + k * cap + tc[k]); continue; }
                // more ties than the cap: this clade again with room for all of them
                const std::vector<size_t> one{i};
                std::vector<uint64_t> o1; std::vector<int32_t> p1; std::vector<uint8_t> r1, n1, m1;
                const ugp_queries q1 = batch(one, o1, p1, r1, n1, m1);
                const uint32_t big = tc[k];
                std::vector<uint32_t> t1(big), c1(1);
                std::vector<int32_t> b1(1);
                if (pass == 0) {
                    ugp_place_opts o{UGP_ORDER_DFS, nullptr, nullptr, nullptr, nullptr};
                    std::vector<uint8_t> hu(big);
                    if (ugp_tied_nodes_ex(h, &q1, &o, big, t1.data(), hu.data(), c1.data()) != UGP_OK) lib_fail("ugp_tied_nodes_ex");
                } else if (ugp_annotate_search(h, &q1, big, b1.data(), t1.data(), c1.data()) != UGP_OK) {
                    lib_fail("ugp_annotate_search");
                }
                ties[i].assign(t1.begin(), t1.begin() + std::min(big, c1[0]));
            }
            if (pass == 0) for (size_t i : which) std::sort(ties[i].begin(), ties[i].end());
        }
    }

    // get_freq_overlap (:466-481) for every tie and each of its ancestors, one device call
    std::vector<uint64_t> coffT(1, 0);
    std::vector<uint32_t> xsT, pc, pn;
    std::vector<size_t> cm_index(nc, SIZE_MAX);
    for (size_t i = 0; i < nc; i++) {
        auto cm = clade_map.find(order[i]);
        if (cm == clade_map.end()) continue;
        cm_index[i] = coffT.size() - 1;
        for (uh::Node *n : cm->second) xsT.push_back(n->flat_index);
        coffT.push_back(xsT.size());
    }
    std::map<std::pair<size_t, uint32_t>, uint32_t> num_desc;
    {
        for (size_t i = 0; i < nc; i++) {
            if (cm_index[i] == SIZE_MAX) continue;
            for (uint32_t j : ties[i])
                for (uh::Node *a = dfs[j]; a; a = a->parent) { pc.push_back((uint32_t)cm_index[i]); pn.push_back(a->flat_index); }
        }
        std::vector<uint32_t> out(pc.size());
        if (!pc.empty()) {
            device_up();
            if (ugp_clade_descendants(h, coffT.data(), xsT.data(), coffT.size() - 1, pc.data(), pn.data(), pc.size(), out.data()) != UGP_OK)
                lib_fail("ugp_clade_descendants");
        }
        for (size_t k = 0; k < pc.size(); k++) num_desc[{pc[k], pn[k]}] = out[k];
    }

    std::vector<CladeAssignment> cas;
    for (size_t i = 0; i < nc; i++) {
        const std::string &clade = order[i];
        std::vector<uh::Mutation> &cmuts = rows_of[i];
        fprintf(stderr, "Mutations above the specified frequency in clade %s: ", clade.c_str());
        write_mutations(stderr, cmuts, true, true);
        fputc('\n', stderr);
        if (mf) { fprintf(mf, "%s\t", clade.c_str()); write_mutations(mf, cmuts, true, false); fputc('\n', mf); }
        fprintf(stderr, "Finding best node for clade %s.\n", clade.c_str());
        fprintf(stderr, "Parsimony score at the best node: %d\n", best[i]);
        // mapper2_body's winner (usher_mapper.cpp:483-486): more leaves, then the larger index
        size_t win = 0;
        for (size_t k = 0; k < ties[i].size(); k++)
            if (k == 0 || leaves[ties[i][k]] > leaves[ties[i][win]] || (leaves[ties[i][k]] == leaves[ties[i][win]] && ties[i][k] > ties[i][win])) win = k;
        for (size_t k = 0; k < ties[i].size(); k++) {
            const uh::Node *node = dfs[ties[i][k]];
            fprintf(stderr, "%s\t%d\t%c\t%s\t%s\n", clade.c_str(), best[i], k == win ? '*' : '-', node->id.c_str(), path_to_node(node).c_str());
        }
        if (ties[i].size() > 1) fprintf(stderr, "WARNING: found %zu possible assignments\n", ties[i].size());
        auto cm = clade_map.find(clade);
        if (cm != clade_map.end()) {
            const size_t csize = cm->second.size();
            cas.emplace_back(clade, csize, cmuts);
            float best_freq = -1.0f;
            for (uint32_t j : ties[i]) {   // already ascending: the stable_sort of :663
                for (uh::Node *a = dfs[j]; a; a = a->parent) {
                    const size_t nd = num_desc[{cm_index[i], a->flat_index}];
                    const float freq = static_cast<float>(nd) / leaves[dfs_idx[a]];
                    const float overlap = static_cast<float>(nd) / csize;
                    if (freq >= best_freq && overlap >= set_overlap) {
                        cas.back().best_node_frequencies.emplace_back(dfs_idx[a], freq, overlap, clip);
                        best_freq = freq;
                    } else {
                        break;
                    }
                }
            }
            if (cas.back().best_node_frequencies.empty()) {
                fprintf(stderr, "WARNING: %s: no placement node or ancestor passed thresholds.\n", clade.c_str());
                for (uint32_t j : ties[i]) {
                    const size_t nd = num_desc[{cm_index[i], dfs[j]->flat_index}];
                    fprintf(stderr, "fail node\t%s\t%s\t%f\t%f\n", clade.c_str(), dfs[j]->id.c_str(), static_cast<float>(nd) / leaves[j],
                            static_cast<float>(nd) / csize);
                }
            }
            std::stable_sort(cas.back().best_node_frequencies.begin(), cas.back().best_node_frequencies.end());
        } else {
            cas.emplace_back(clade, 0, cmuts);
            if (best[i] == 0) {
                size_t bj = 0, most = 0;
                for (uint32_t j : ties[i]) if (leaves[j] > most) { bj = j; most = leaves[j]; }
                cas.back().best_node_frequencies.emplace_back(bj, 1, 1, clip);
            } else {
                fprintf(stderr, "WARNING: skipping clade %s because the parsimony score is %d\n", clade.c_str(), best[i]);
            }
        }
    }
    fprintf(stderr, "Sorting clades by the number of best nodes \n");
    std::sort(cas.begin(), cas.end());
    fprintf(stderr, "Now assigning clades to nodes \n");
    for (const CladeAssignment &c : cas) {
        bool assigned = false;
        const NodeFreq *an = nullptr;
        std::string already;
        for (const NodeFreq &n : c.best_node_frequencies) {
            uh::Node *node = dfs[n.best_j];
            if (node->clade_annotations[na - 1] == "") {
                fprintf(stderr, "\nAssigning %s to node %s\n", c.clade_name.c_str(), node->id.c_str());
                if (c.clade_size > 0)
                    fprintf(stderr, "%f fraction of %zu clade %s samples are descendants of the assigned node %s\n", n.overlap, c.clade_size,
                            c.clade_name.c_str(), node->id.c_str());
                node->clade_annotations[na - 1] = c.clade_name;
                assigned = true;
                an = &n;
                break;
            }
            fprintf(stderr, "\nNode %s already assigned to %s, cannot assign to %s.\n", node->id.c_str(), node->clade_annotations[na - 1].c_str(),
                    c.clade_name.c_str());
            if (!already.empty()) already += ", ";
            already += node->id + ":" + node->clade_annotations[na - 1];
        }
        if (!assigned) {
            if (!c.best_node_frequencies.empty())
                fprintf(stderr, "\nWARNING: Could not assign a node to clade %s with %zu samples since all possible nodes were already assigned some other clade!\n",
                        c.clade_name.c_str(), c.clade_size);
            else
                fprintf(stderr, "\nWARNING: Could not assign a node to clade %s with %zu samples since placement node(s) did not overlap with enough clade samples!\n",
                        c.clade_name.c_str(), c.clade_size);
        }
        if (df) {
            fprintf(df, "%s\t", c.clade_name.c_str());
            write_mutations(df, c.mutations, true, false);
            fputc('\t', df);
            write_mutations(df, c.mutations, false, true);
            fputc('\t', df);
            if (c.best_node_frequencies.empty()) fprintf(df, "n/a");
            for (size_t k = 0; k < c.best_node_frequencies.size(); k++) {
                if (k) fprintf(df, ", ");
                const NodeFreq &b = c.best_node_frequencies[k];
                fprintf(df, "%s:%f:%f", dfs[b.best_j]->id.c_str(), b.freq, b.overlap);
            }
            fprintf(df, already.empty() ? "\tn/a" : "\t%s", already.c_str());
            fprintf(df, "\t%f", assigned ? an->overlap : 0.0);
            fprintf(df, "\t%lu", (unsigned long)c.clade_size);
            std::string path = "n/a";
            if (assigned) path = path_to_node(dfs[an->best_j]);
            else if (!c.best_node_frequencies.empty()) path = path_to_node(dfs[c.best_node_frequencies[0].best_j]);
            fprintf(df, "\t%s\n", path.c_str());
        }
    }
    if (mf) fclose(mf);
    if (df) fclose(df);
}

int annotate(int argc, char **argv) {   // annotate_main, :94-156
    std::string in_mat, out_mat, fnames, fnid, fpaths, fmuts, fmutsout, fdetails, dir = "./";
    float min_freq = 0.8f, mask_freq = 0.2f, set_overlap = 0.6f, clip = 0.1f;
    bool clear = false;
    int device = 0;
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); annotate_usage(stderr); return false; }
            dst = argv[++i];
            return true;
        };
        auto fval = [&](float &dst) -> bool {
            std::string t;
            if (!val(t)) return false;
            char *end = nullptr;
            dst = strtof(t.c_str(), &end);
            if (t.empty() || *end) { fprintf(stderr, "ERROR: bad value %s for %s\n", t.c_str(), a.c_str()); annotate_usage(stderr); return false; }
            return true;
        };
        std::string tmp;
        bool ok = true;
        if (a == "-i" || a == "--input-mat") ok = val(in_mat);
        else if (a == "-o" || a == "--output-mat") ok = val(out_mat);
        else if (a == "-c" || a == "--clade-names") ok = val(fnames);
        else if (a == "-C" || a == "--clade-to-nid") ok = val(fnid);
        else if (a == "-P" || a == "--clade-paths") ok = val(fpaths);
        else if (a == "-M" || a == "--clade-mutations") ok = val(fmuts);
        else if (a == "-f" || a == "--allele-frequency") ok = fval(min_freq);
        else if (a == "-m" || a == "--mask-frequency") ok = fval(mask_freq);
        else if (a == "-s" || a == "--set-overlap") ok = fval(set_overlap);
        else if (a == "-p" || a == "--clip-sample-frequency") ok = fval(clip);
        else if (a == "-l" || a == "--clear-current") clear = true;
        else if (a == "-d" || a == "--output-directory") ok = val(dir);
        else if (a == "-u" || a == "--write-mutations") ok = val(fmutsout);
        else if (a == "-D" || a == "--write-details") ok = val(fdetails);
        else if (a == "-T" || a == "--threads") ok = val(tmp);
        else if (a == "--device") { ok = val(tmp); device = atoi(tmp.c_str()); }
        else if (a == "-h" || a == "--help") { annotate_usage(stderr); return 0; }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); annotate_usage(stderr); return 1; }
        if (!ok) return 1;
    }
    if (in_mat.empty() || out_mat.empty()) {
        fprintf(stderr, "ERROR: the option '--%s' is required but missing\n", in_mat.empty() ? "input-mat" : "output-mat");
        annotate_usage(stderr);
        return 1;
    }
    // make_out_dir / add_out_dir (:65-84)
    struct stat sb;
    if (stat(dir.c_str(), &sb) != 0) {
        fprintf(stderr, "Creating output directory %s.\n\n", dir.c_str());
        mkdir(dir.c_str(), 0777);
    }
    char *canon = realpath(dir.c_str(), nullptr);
    if (!canon) { fprintf(stderr, "ERROR: cannot resolve the output directory %s\n", dir.c_str()); return 1; }
    const std::string prefix = canon;
    free(canon);
    auto add_out = [&](const std::string &f) { return (!f.empty() && f[0] != '/') ? prefix + "/" + f : f; };
    out_mat = add_out(out_mat);
    fmutsout = add_out(fmutsout);
    fdetails = add_out(fdetails);
    int spec = 0;
    if (!fnames.empty() || !fmuts.empty() || !fpaths.empty()) spec++;
    if (!fnid.empty()) spec++;
    if (spec != 1) {
        fprintf(stderr, "ERROR: must specify either --clade-to-nid or [--clade-names and/or --clade-mutations and/or --clade-paths]!\n");
        return 1;
    }
    fprintf(stderr, "Loading input MAT file %s.\n", in_mat.c_str());
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(in_mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    if (!T.condensed_nodes.empty()) T.uncondense_leaves();
    fprintf(stderr, "Annotating Lineage Root Nodes\n");
    if (!fnames.empty() || !fmuts.empty() || !fpaths.empty())
        lineages(T, fnames, fmuts, fpaths, min_freq, mask_freq, set_overlap, clip, clear, fmutsout, fdetails, device);
    else
        lineages_from_nids(T, fnid, clear);
    fprintf(stderr, "Recondensing leaves\n");
    T.condense_leaves();
    fprintf(stderr, "Saving Final Tree to %s\n", out_mat.c_str());
    if (!uh::save_mat(T, out_mat, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    return 0;
}


// ---- extract (extract.cpp, select.cpp) ----------------------------------------------------------------------------

void extract_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd extract -i tree.pb [-s samples.txt] [-k sample:k] [-Y y] [-a n] [-b n] [-P n] [-u used.txt] [-t tree.nh]\n"
            "       [-o out.pb] [-v out.vcf] [-n] [-d dir] [-T n] [--device k] [--reference-ties] [--host-genotypes]\n"
            "  -i, --input-mat          input mutation-annotated tree [REQUIRED]\n"
            "  -s, --samples            select samples by explicitly naming them, one per line\n"
            "  -k, --nearest-k          select a sample and the nearest k samples to it, formatted as sample:k\n"
            "  -Y, --select-nearest     add the y nearest samples to each selected sample, without duplicates\n"
            "  -a, --max-parsimony      select samples with at most this many mutations on their terminal branch\n"
            "  -b, --max-branch-length  select samples with no longer branch than this in their ancestry\n"
            "  -P, --max-path-length    select samples with a total path length of at most this\n"
            "  -u, --used-samples       write a text file of the selected sample ids\n"
            "  -t, --write-tree         write a newick tree of the selected samples\n"
            "  -o, --write-mat          write the selected tree as a new protobuf\n"
            "  -v, --write-vcf          write a VCF of the selected samples (gzip when the name contains .gz)\n"
            "  -n, --no-genotypes       leave the genotype columns out of the VCF\n"
            "  -d, --output-directory   directory of the output files [./]\n"
            "  -T, --threads            accepted for compatibility (the searches run on the device)\n"
            "      --device             HIP device ordinal [0]\n"
            "      --reference-ties     order equal distances as the reference's std::sort does (host, slow)\n"
            "      --host-genotypes     build the VCF with the reference's serial tree walk on the host (slow)\n");
}

std::vector<std::string> read_sample_names(const std::string &fname) {   // select.cpp:8-36
    std::vector<std::string> names;
    std::ifstream in(fname);
    if (!in) { fprintf(stderr, "ERROR: Could not open the file: %s!\n", fname.c_str()); exit(1); }
    std::string line;
    bool warned = false;
    while (std::getline(in, line)) {
        std::vector<std::string> w;
        split_ws(line, w);
        if (w.size() > 1 && !warned) {
            fprintf(stderr, "WARNING: Input file %s contains excess columns; ignoring\n", fname.c_str());
            warned = true;
        } else if (w.empty()) {
            fprintf(stderr, "WARNING: Empty line in input file %s; ignoring\n", fname.c_str());
            continue;
        }
        std::string name = w[0];
        if (name.back() == '\r') name.pop_back();
        names.push_back(name);
    }
    return names;
}

std::vector<std::string> leaf_ids(const uh::Tree &T) {   // get_leaves_ids
    std::vector<std::string> ids;
    for (const uh::Node *n : T.leaves()) ids.push_back(n->id);
    return ids;
}

uh::Node *must_get(const uh::Tree &T, const std::string &id) {   // (the reference dereferences the null pointer)
    uh::Node *n = T.get_node(id);
    if (!n) { fprintf(stderr, "ERROR: %s is not present in the tree!\n", id.c_str()); exit(1); }
    return n;
}

std::vector<std::string> get_parsimony_samples(const uh::Tree &T, std::vector<std::string> check, int max_parsimony) {   // select.cpp:113-127
    if (check.empty()) check = leaf_ids(T);
    std::vector<std::string> good;
    for (const std::string &s : check) {
        const uh::Node *n = must_get(T, s);
        if (n->mutations.size() <= static_cast<size_t>(max_parsimony)) good.push_back(n->id);
    }
    return good;
}

std::vector<std::string> get_short_steppers(const uh::Tree &T, std::vector<std::string> check, int max_mutations) {   // select.cpp:278-307
    std::vector<std::string> good;
    if (check.empty()) check = leaf_ids(T);
    for (const std::string &s : check) {
        uh::Node *n = must_get(T, s);
        if (n->mutations.size() > static_cast<size_t>(max_mutations)) continue;
        bool bad = false;
        for (const uh::Node *a : T.rsearch(n, false))
            if (a->mutations.size() > static_cast<size_t>(max_mutations)) { bad = true; break; }
        if (!bad) good.push_back(s);
    }
    return good;
}

std::vector<std::string> get_short_paths(const uh::Tree &T, const std::vector<std::string> &check, int max_path) {   // select.cpp:309-335
    std::vector<std::string> good;
    const std::unordered_set<std::string> set(check.begin(), check.end());
    std::unordered_map<const uh::Node *, size_t> len;
    for (const uh::Node *n : T.dfs()) {
        if (!n->is_leaf()) {
            len[n] = n->is_root() ? 0 : len[n->parent] + n->mutations.size();
        } else if (n->parent && len[n->parent] + n->mutations.size() <= static_cast<size_t>(max_path)) {
            if (check.empty() || set.count(n->id)) good.push_back(n->id);
        }
    }
    return good;
}

// get_nearby (select.cpp:206-276) for a batch of (sample, k): the searches on the device (ugp_nearest_k), names out.
struct NearestSearch {
    uh::Tree &T;
    int device;
    bool reference_ties;
    std::vector<uh::Node *> bfs;
    Mat h;
    ugp_mat *use = nullptr;   // h, or the handle share() was given
    NearestSearch(uh::Tree &t, int dev, bool ties) : T(t), device(dev), reference_ties(ties) {}
    void up() {
        if (use) return;
        uh::TreeArrays A(T);
        const ugp_tree_desc desc = A.desc();
        h.create(desc, device);
        if (ugp_nearest_attach(h, &desc) != UGP_OK) lib_fail("ugp_nearest_attach");
        bfs = std::move(A.bfs);   // the library has its copy of the arrays: only the nodes are kept
        use = h;
    }
    // subtrees: search on the handle another owner has made of this tree and its arrays, instead of on a second copy of the tree
    void share(ugp_mat *other, const uh::TreeArrays &A) {
        if (use) return;
        const ugp_tree_desc desc = A.desc();
        if (ugp_nearest_attach(other, &desc) != UGP_OK) lib_fail("ugp_nearest_attach");
        bfs = A.bfs;
        use = other;
    }
    // The literal sort of one query between the device's anc and last_anc: Tree::get_leaves' order into std::sort.
    std::vector<std::string> literal(uh::Node *anc, uh::Node *last, size_t k) const {
        std::vector<std::string> keep;
        for (const uh::Node *l : T.leaves(last)) keep.push_back(l->id);
        struct NodeDist { const uh::Node *node; uint32_t num_mut; };
        std::vector<NodeDist> dist;
        for (const uh::Node *l : T.leaves(anc)) {
            if (T.is_ancestor(last, l)) continue;
            uint32_t d = 0;
            for (const uh::Node *a = l; a != anc; a = a->parent) d += (uint32_t)a->mutations.size();
            dist.push_back({l, d});
        }
        std::sort(dist.begin(), dist.end(), [](const NodeDist &a, const NodeDist &b) { return a.num_mut < b.num_mut; });
        for (const NodeDist &n : dist) { if (keep.size() == k) break; keep.push_back(n.node->id); }
        return keep;
    }
    std::vector<std::vector<std::string>> run(const std::vector<uh::Node *> &nodes, size_t k) {
        up();
        const size_t n = nodes.size();
        std::vector<std::vector<std::string>> out(n);
        if (!n) return out;
        if (k > bfs.size()) k = bfs.size();   // more than every leaf: the same (empty) answer
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> qn(n), qk(n, (uint32_t)k), on, od;
        std::vector<ugp_nearest_info> info(n);
        for (size_t i = 0; i < n; i++) qn[i] = nodes[i]->flat_index;
        // rows of k slots, a bounded number of them per call
        const size_t per = std::max<size_t>(1, (size_t(1) << 24) / k);
        for (size_t i0 = 0; i0 < n; i0 += per) {
            const size_t m = std::min(per, n - i0);
            on.resize(m * k); od.resize(m * k);
            if (ugp_nearest_k(use, m, qn.data() + i0, qk.data() + i0, (uint32_t)k, on.data(), od.data(), info.data() + i0) != UGP_OK) lib_fail("ugp_nearest_k");
            for (size_t i = 0; i < m; i++) {
                const ugp_nearest_info &f = info[i0 + i];
                if (f.anc == UINT32_MAX) continue;
                if (f.count > k) {   // the sample is an internal node with more than k leaves: all of them (the reference's loop)
                    for (const uh::Node *l : T.leaves(bfs[f.last_anc])) out[i0 + i].push_back(l->id);
                    continue;
                }
                if (reference_ties) { out[i0 + i] = literal(bfs[f.anc], bfs[f.last_anc], k); continue; }
                for (uint32_t s = 0; s < f.count; s++) out[i0 + i].push_back(bfs[on[i * k + s]]->id);
            }
        }
        fprintf(stderr, "Nearest-k search of %zu samples: %.1f msec\n", n,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return out;
    }
};

// ---- extract -v (make_vcf, convert.cpp:14-320) ----------------------------------------------------------------------

struct VcfFile {   // plain, or gzip when the name contains ".gz" (convert.cpp:305)
    FILE *f = nullptr;
    gzFile g = nullptr;
    bool ok = true;
    explicit VcfFile(const std::string &path) {
        if (path.find(".gz") != std::string::npos) g = gzopen(path.c_str(), "wb");
        else f = fopen(path.c_str(), "wb");
        if (!f && !g) { fprintf(stderr, "ERROR: could not open %s\n", path.c_str()); exit(1); }
    }
    void put(const std::string &s) {
        for (size_t o = 0; o < s.size() && ok;) {
            const size_t n = std::min<size_t>(s.size() - o, 1u << 30);
            ok = g ? gzwrite(g, s.data() + o, (unsigned)n) == (int)n : fwrite(s.data() + o, 1, n, f) == n;
            o += n;
        }
    }
    bool close() {
        if (g) ok = gzclose(g) == Z_OK && ok;
        if (f) ok = fclose(f) == 0 && ok;
        g = nullptr; f = nullptr;
        return ok;
    }
};

// One row (VCF_Line_Writer, :195-251): `codes` = the genotype code per column, or null without genotypes.
void vcf_row(std::string &out, const std::string &chrom, const ugp_gt_site &s, uint32_t n_cols, const uint8_t *codes) {
    const std::string pos = std::to_string(s.pos);
    const char ref = uh::nuc_char((int8_t)s.ref);
    std::string id, alt, ac;
    for (uint32_t k = 0; k < s.n_alt; k++) {
        if (k) { id += ","; alt += ","; ac += ","; }
        id += ref; id += pos; id += uh::nuc_char((int8_t)s.alt[k]);
        alt += uh::nuc_char((int8_t)s.alt[k]);
        ac += std::to_string(s.ac[k]);
    }
    out += chrom; out += '\t'; out += pos; out += '\t'; out += id; out += '\t'; out += ref; out += '\t'; out += alt;
    out += "\t.\t.\tAC="; out += ac; out += ";AN="; out += std::to_string(n_cols);
    if (codes) {
        out += "\tGT";
        for (uint32_t c = 0; c < n_cols; c++) {
            const uint8_t v = codes[c];
            out += '\t';
            if (v >= 10) out += (char)('0' + v / 10);
            out += (char)('0' + v % 10);
        }
    }
    out += '\n';
}

// r_add_genotypes and write_vcf_rows (:53-102, 267-292) literally, on the host.
struct HostGenotypes {
    struct LeafGenotype { uint32_t leaf_ix; int8_t genotype; };
    struct PosData { std::vector<LeafGenotype> leaf_genotypes; uint8_t ref = 0; };
    std::unordered_map<uint32_t, PosData> info;
    const std::set<std::string> &use;
    explicit HostGenotypes(const std::set<std::string> &u) : use(u) {}
    uint32_t add(const uh::Node *node, uint32_t leaf_ix, std::vector<const uh::Mutation *> &mut_stack) {
        size_t pushed = 0;
        for (const auto &mut : node->mutations) {
            if (mut.masked()) continue;
            mut_stack.push_back(&mut);
            pushed++;
        }
        if (use.find(node->id) != use.end()) {
            for (const uh::Mutation *mut : mut_stack) {
                auto res = info.insert(std::make_pair((uint32_t)mut->position, PosData()));
                PosData &pi = res.first->second;
                if (res.second) pi.ref = (uint8_t)mut->par_nuc;
                if (pi.leaf_genotypes.empty() || pi.leaf_genotypes.back().leaf_ix < leaf_ix) pi.leaf_genotypes.push_back({leaf_ix, mut->mut_nuc});
                else pi.leaf_genotypes.back().genotype = mut->mut_nuc;
            }
            leaf_ix++;
        }
        for (const uh::Node *child : node->children) leaf_ix = add(child, leaf_ix, mut_stack);
        mut_stack.resize(mut_stack.size() - pushed);
        return leaf_ix;
    }
    size_t write(VcfFile &vcf, const std::string &chrom, uint32_t leaf_count, bool print_genotypes) {   // returns the rows written
        size_t written = 0;
        std::vector<uint32_t> order;
        for (const auto &kv : info) order.push_back(kv.first);
        std::sort(order.begin(), order.end());
        std::string line;
        std::vector<uint8_t> codes(leaf_count);
        for (uint32_t pos : order) {
            const PosData &pi = info[pos];
            std::map<int8_t, uint32_t> counts;   // count_alleles, then make_alts' std::map: ascending allele
            for (const LeafGenotype &g : pi.leaf_genotypes) counts[g.genotype]++;
            counts.erase((int8_t)pi.ref);
            if (counts.empty()) { fprintf(stderr, "WARNING: no-alternative site encountered in vcf output; skipping\n"); continue; }
            ugp_gt_site s{};
            s.pos = (int32_t)pos; s.ref = pi.ref; s.covered = (uint32_t)pi.leaf_genotypes.size();
            int al_codes[256] = {0};
            for (const auto &kv : counts) {
                if (s.n_alt >= 14) { fprintf(stderr, "ERROR: more than 14 alternate alleles at position %u\n", pos); exit(1); }
                s.alt[s.n_alt] = (uint8_t)kv.first; s.ac[s.n_alt] = kv.second;
                al_codes[(uint8_t)kv.first] = ++s.n_alt;
            }
            if (print_genotypes) {
                std::fill(codes.begin(), codes.end(), 0);
                for (const LeafGenotype &g : pi.leaf_genotypes) codes[g.leaf_ix] = (uint8_t)al_codes[(uint8_t)g.genotype];
            }
            line.clear();
            vcf_row(line, chrom, s, leaf_count, print_genotypes ? codes.data() : nullptr);
            vcf.put(line);
            written++;
        }
        return written;
    }
};

int make_vcf(uh::Tree &T, const std::string &path, bool no_genotypes, const std::vector<std::string> &samples_vec, int device, bool on_host) {
    const auto t0 = std::chrono::steady_clock::now();
    std::set<std::string> use(samples_vec.begin(), samples_vec.end());
    if (use.empty()) for (const std::string &s : leaf_ids(T)) use.insert(s);
    const std::vector<uh::Node *> dfs = T.dfs();
    // one chromosome: the reference writes them in the iteration order of an unordered_map
    std::string chrom;
    bool any = false;
    for (const uh::Node *n : dfs)
        for (const auto &m : n->mutations) {
            if (m.masked()) continue;
            const std::string &c = T.chroms[m.chrom];
            if (any && c != chrom) {
                fprintf(stderr, "ERROR: the tree's mutations name more than one chromosome (%s, %s): matutils-amd extract -v writes one\n", chrom.c_str(), c.c_str());
                return 1;
            }
            chrom = c; any = true;
        }
    VcfFile vcf(path);
    std::string head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
    if (!no_genotypes) {
        head += "\tFORMAT";
        for (const uh::Node *n : dfs) if (use.count(n->id)) { head += '\t'; head += n->id; }
    }
    head += '\n';
    vcf.put(head);
    size_t n_sites = 0;
    uint32_t n_cols = 0;
    if (on_host) {
        HostGenotypes hg(use);
        std::vector<const uh::Mutation *> mut_stack;
        n_cols = (uint32_t)use.size();
        hg.add(T.root, 0, mut_stack);
        n_sites = hg.write(vcf, chrom, n_cols, !no_genotypes);
    } else {
        // the tree as arrays: the handle takes the bare topology, the genotype tables the mutations as they are stored
        const uh::TreeArrays A(T);
        std::vector<uint32_t> sel;
        for (size_t j = 0; j < A.bfs.size(); j++) if (use.count(A.bfs[j]->id)) sel.push_back((uint32_t)j);
        const ugp_tree_desc desc = A.desc();
        Mat h;
        h.create(A.bare(), device);
        if (ugp_genotypes_attach(h, &desc) != UGP_OK) lib_fail("ugp_genotypes_attach");
        uint64_t ns = 0;
        if (ugp_genotype_select(h, sel.data(), sel.size(), &n_cols, &ns) != UGP_OK) lib_fail("ugp_genotype_select");
        n_sites = ns;
        std::vector<ugp_gt_site> sites(ns);
        if (ugp_genotype_sites(h, 0, ns, sites.data()) != UGP_OK) lib_fail("ugp_genotype_sites");
        std::string text;
        if (no_genotypes) {
            for (const ugp_gt_site &s : sites) { text.clear(); vcf_row(text, chrom, s, n_cols, nullptr); vcf.put(text); }
        } else if (ns) {
            // rows in chunks of sites: the device fills one pinned buffer while the other is formatted
            const uint64_t per = std::max<uint64_t>(1, (uint64_t(32) << 20) / n_cols);
            uint8_t *buf[2] = {nullptr, nullptr};
            for (auto &b : buf)
                if (hipHostMalloc((void **)&b, std::min<uint64_t>(per, ns) * n_cols, hipHostMallocDefault) != hipSuccess) {
                    fprintf(stderr, "ERROR: hipHostMalloc failed\n");
                    for (auto &f : buf) if (f) (void)hipHostFree(f);
                    return 1;
                }
            // (the library's error text is per thread: the fetching thread brings it along)
            auto fetch = [&](uint64_t lo, int k) -> std::string {
                return ugp_genotype_rows(h, lo, std::min<uint64_t>(ns, lo + per), buf[k]) == UGP_OK ? std::string() : std::string("ugp_genotype_rows: ") + ugp_last_error();
            };
            std::future<std::string> next = std::async(std::launch::async, fetch, uint64_t(0), 0);
            int k = 0;
            std::string failed;
            for (uint64_t lo = 0; lo < ns; lo += per, k ^= 1) {
                failed = next.get();
                if (!failed.empty()) break;
                if (lo + per < ns) next = std::async(std::launch::async, fetch, lo + per, k ^ 1);
                const uint64_t hi = std::min<uint64_t>(ns, lo + per);
                text.clear();
                for (uint64_t s = lo; s < hi; s++) vcf_row(text, chrom, sites[s], n_cols, buf[k] + (s - lo) * n_cols);
                vcf.put(text);
            }
            if (!failed.empty()) {
                fprintf(stderr, "ERROR: %s\n", failed.c_str());
                for (auto &b : buf) (void)hipHostFree(b);
                return 1;
            }
            for (auto &b : buf) (void)hipHostFree(b);
        }
    }
    if (!vcf.close()) { fprintf(stderr, "ERROR: could not write %s\n", path.c_str()); return 1; }
    fprintf(stderr, "VCF of %zu sites x %u samples (%s): %.1f msec\n", n_sites, n_cols, on_host ? "host" : "device",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

// ---- select: extract's -I -c -m -H -e -U -p (extract.cpp:294-373, 411-427, 455-472; select.cpp) ---------------------------------

void select_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd select -i tree.pb [-s samples.txt] [-k sample:k] [-I node] [-c clade[,clade]] [-m mutation[,mutation]] [-H regex]\n"
            "       [-a n] [-b n] [-P n] [-e n] [-U] [-Y y] [-p] [-u used.txt] [-t tree.nh] [-o out.pb] [-v out.vcf] [-n] [-d dir] [-T n]\n"
            "       [--device k] [--reference-ties] [--host-genotypes] [--host]\n"
            "  every option of matutils-amd extract (see extract --help), and the selectors, applied in this order after -s and -k:\n"
            "  -I, --get-internal-descendents  select the samples below this internal node\n"
            "  -c, --clade              select the samples of a clade; comma-separated names are ORed\n"
            "  -m, --mutation           select the samples with a mutation (A123G); comma-separated mutations are ORed\n"
            "  -H, --match              select the samples whose name matches this regular expression (std::regex_match)\n"
            "  -e, --max-epps           (after -a -b -P) select samples with at most this many equally parsimonious placements\n"
            "  -U, --from-mrca          widen to every sample below the most recent common ancestor of the selection\n"
            "  -p, --prune              (last) invert the selection\n"
            "      --host               run every selector as the reference's walk on the host (slow)\n"
            "  Where the reference takes its order from an unordered set (-c or -m with nothing selected before), the samples are\n"
            "  written in depth-first order.  -e with nothing selected before checks the leaves only (the reference also walks the\n"
            "  internal nodes); with a selection it keeps its members in depth-first order.  -H is std::regex_match on both paths.\n");
}

struct SelectOpts {
    bool on = false, mrca = false, prune = false, host = false;
    std::string internal, clade, mutation, match;
    long max_epps = 0;
};

// The selectors on the device: one handle, one ugp_select_attach; a selection crosses as a bitmap over leaf ranks.
struct SelectDevice {
    uh::Tree &T;
    int device;
    Mat h;
    uh::TreeArrays A;   // kept: -e attaches the uncertainty tables later
    std::vector<uint32_t> leaf_bfs, rank_of;   // rank_of by BFS index, UINT32_MAX for an internal node
    bool unc_attached = false;
    unsigned keep;      // what A keeps beside the arrays (subtree: the entries)
    SelectDevice(uh::Tree &t, int dev, unsigned keep_ = 0) : T(t), device(dev), keep(keep_) {}
    void up() {
        if (h) return;
        A = uh::TreeArrays(T, keep);
        const uint64_t N = A.bfs.size();
        // the handle takes the bare topology, the select tables the mutations as they are stored (masked, repeated positions)
        const ugp_tree_desc desc = A.desc();
        h.create(A.bare(), device);
        if (ugp_select_attach(h, &desc) != UGP_OK) lib_fail("ugp_select_attach");
        uint64_t nl = 0;
        if (ugp_select_leaves(h, nullptr, &nl) != UGP_OK) lib_fail("ugp_select_leaves");
        leaf_bfs.resize(nl);
        if (ugp_select_leaves(h, leaf_bfs.data(), nullptr) != UGP_OK) lib_fail("ugp_select_leaves");
        rank_of.assign(N, UINT32_MAX);
        for (uint32_t r = 0; r < nl; r++) rank_of[leaf_bfs[r]] = r;
    }
    size_t n_words() const { return (leaf_bfs.size() + 63) / 64; }
    static bool bit(const std::vector<uint64_t> &w, uint32_t r) { return (w[r >> 6] >> (r & 63)) & 1; }
    bool has(const std::vector<uint64_t> &w, const std::string &name) const {
        const uh::Node *n = T.get_node(name);
        return n && rank_of[n->flat_index] != UINT32_MAX && bit(w, rank_of[n->flat_index]);
    }
    std::vector<uint64_t> subtrees(const std::vector<uint32_t> &nodes, std::vector<uint64_t> &counts) {
        up();
        std::vector<uint64_t> w(std::max<size_t>(n_words(), 1), 0);
        counts.assign(nodes.size(), 0);
        if (ugp_select_subtrees(h, nodes.size(), nodes.data(), w.data(), counts.data()) != UGP_OK) lib_fail("ugp_select_subtrees");
        return w;
    }
    std::vector<uint64_t> mutations(const std::vector<int32_t> &qp, const std::vector<uint8_t> &qn, std::vector<uint64_t> &counts) {
        up();
        std::vector<uint64_t> w(std::max<size_t>(n_words(), 1), 0);
        counts.assign(qp.size(), 0);
        if (ugp_select_mutations(h, qp.size(), qp.data(), qn.data(), w.data(), counts.data()) != UGP_OK) lib_fail("ugp_select_mutations");
        return w;
    }
    // The bitmap of names that are all leaves; false when one is not (the caller walks on the host then).
    bool words_of(const std::vector<std::string> &names, std::vector<uint64_t> &w) {
        up();
        w.assign(std::max<size_t>(n_words(), 1), 0);
        for (const std::string &s : names) {
            const uh::Node *n = T.get_node(s);
            if (!n || rank_of[n->flat_index] == UINT32_MAX) return false;
            const uint32_t r = rank_of[n->flat_index];
            w[r >> 6] |= 1ull << (r & 63);
        }
        return true;
    }
    std::vector<std::string> in_rank_order(const std::vector<uint64_t> &w) const {   // depth-first
        std::vector<std::string> out;
        for (uint32_t r = 0; r < leaf_bfs.size(); r++) if (bit(w, r)) out.push_back(A.bfs[leaf_bfs[r]]->id);
        return out;
    }
    std::vector<std::string> in_leaves_order(const std::vector<uint64_t> &w, bool set) const {   // get_leaves_ids: breadth-first
        std::vector<std::string> out;
        for (const uh::Node *n : A.bfs) if (n->is_leaf() && bit(w, rank_of[n->flat_index]) == set) out.push_back(n->id);
        return out;
    }
    std::vector<std::string> filter(const std::vector<std::string> &samples, const std::vector<uint64_t> &w) const {   // sample_intersect
        std::vector<std::string> out;
        for (const std::string &s : samples) if (has(w, s)) out.push_back(s);
        return out;
    }
    std::vector<uint32_t> epps(const std::vector<uint32_t> &nodes) {
        up();
        const ugp_tree_desc desc = A.desc();
        if (!unc_attached && ugp_uncertainty_attach(h, &desc) != UGP_OK) lib_fail("ugp_uncertainty_attach");
        unc_attached = true;
        const size_t n = nodes.size();
        std::vector<uint32_t> e(n), ns(n), ties(std::max<size_t>(n, 1)), tc(n);
        if (n && ugp_uncertainty(h, nodes.data(), n, 1, e.data(), ns.data(), ties.data(), tc.data()) != UGP_OK) lib_fail("ugp_uncertainty");
        return e;
    }
};

// findEPPs' num_best (uncertainty.cpp:132-255) for one node on the host: the sample in the literal order, every other node scored
// by mapper2_body.  0 when the node's root path has no mutation (the reference leaves the value unset there; ugp_uncertainty says 0).
size_t host_epps(const uh::Tree &T, const std::vector<uh::Node *> &dfs, uh::Node *node) {
    std::vector<int32_t> seen;
    std::vector<uh::Mutation> q;
    auto take = [&](const uh::Node *n) {
        for (const auto &m : n->mutations)
            if (m.masked() || std::find(seen.begin(), seen.end(), m.position) == seen.end()) {
                q.push_back(m);
                if (!m.masked()) seen.push_back(m.position);
            }
    };
    take(node);
    for (const uh::Node *a : T.rsearch(node, false)) take(a);
    if (q.empty()) return 0;
    int best = (int)(q.size() + T.root->mutations.size() + 1);
    size_t num_best = 1;
    uh::NodeVecs nv;
    for (const uh::Node *n : dfs) {
        if (n == node) continue;
        uh::node_vecs(n, q, nv);
        if (!nv.eligible || nv.set_difference > best) continue;
        if (nv.set_difference < best) { best = nv.set_difference; num_best = 1; }
        else num_best++;
    }
    return num_best;
}

const char *const kNoneLeft = "ERROR: No samples fulfill selected criteria. Change arguments and try again\n";

std::vector<std::string> split_commas(const std::string &s) {   // std::getline(stream, item, ',')
    std::vector<std::string> out;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, ',')) out.push_back(item);
    return out;
}

void step_time(const char *what, bool host, std::chrono::steady_clock::time_point t0) {
    fprintf(stderr, "Selection step %s (%s): %.3f msec\n", what, host ? "host" : "device",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// -I, -c, -m and -H (extract.cpp:294-373).  false: the reference exits here (the message is printed).
bool select_before_filters(uh::Tree &T, const SelectOpts &O, SelectDevice &D, std::vector<std::string> &samples) {
    std::vector<uint64_t> counts;
    if (!O.internal.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        uh::Node *node = T.get_node(O.internal);
        if (O.host) {
            std::vector<std::string> ic;
            if (node) for (const uh::Node *l : T.leaves(node)) ic.push_back(l->id);
            if (samples.empty()) samples = ic;
            else { const std::unordered_set<std::string> set(ic.begin(), ic.end()); std::vector<std::string> in; for (const auto &s : samples) if (set.count(s)) in.push_back(s); samples = in; }
        } else {
            D.up();
            const std::vector<uint64_t> w = D.subtrees(node ? std::vector<uint32_t>{node->flat_index} : std::vector<uint32_t>{}, counts);
            samples = samples.empty() ? D.in_leaves_order(w, true) : D.filter(samples, w);
        }
        step_time("-I", O.host, t0);
    }
    if (!O.clade.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<std::string> clades = split_commas(O.clade);
        std::vector<uh::Node *> roots(clades.size(), nullptr);
        const std::vector<uh::Node *> dfs = T.dfs();
        if (O.host) {   // get_clade_samples, once per name
            for (size_t i = 0; i < clades.size(); i++)
                for (uh::Node *s : dfs) {
                    const auto &canns = s->clade_annotations;
                    if (canns.empty() || !(canns.size() > 1 || canns[0] != "")) continue;
                    if (std::find(canns.begin(), canns.end(), clades[i]) != canns.end()) { roots[i] = s; break; }
                }
        } else {        // one pass for every name
            std::unordered_map<std::string, std::vector<size_t>> want;
            for (size_t i = 0; i < clades.size(); i++) want[clades[i]].push_back(i);
            size_t open = want.size();
            for (uh::Node *s : dfs) {
                const auto &canns = s->clade_annotations;
                if (canns.empty() || !(canns.size() > 1 || canns[0] != "")) continue;
                for (const std::string &c : canns) {
                    auto it = want.find(c);
                    if (it == want.end() || roots[it->second[0]]) continue;
                    for (size_t i : it->second) roots[i] = s;
                    open--;
                }
                if (!open) break;
            }
        }
        std::vector<uint64_t> w;
        std::unordered_set<std::string> in_clade;
        if (!O.host) {
            D.up();
            std::vector<uint32_t> nodes;
            for (const uh::Node *r : roots) if (r) nodes.push_back(r->flat_index);
            w = D.subtrees(nodes, counts);
        }
        for (size_t i = 0; i < clades.size(); i++) {
            fprintf(stderr, "Getting member samples of clade %s\n", clades[i].c_str());
            if (!roots[i]) fprintf(stderr, "WARNING: Clade %s is not detected in the input tree!\n", clades[i].c_str());
            else if (O.host) for (const uh::Node *l : T.leaves(roots[i])) in_clade.insert(l->id);
        }
        if (O.host) {
            std::vector<std::string> out;
            if (samples.empty()) { for (const uh::Node *n : dfs) if (in_clade.count(n->id)) out.push_back(n->id); }
            else for (const auto &s : samples) if (in_clade.count(s)) out.push_back(s);
            samples = out;
        } else {
            samples = samples.empty() ? D.in_rank_order(w) : D.filter(samples, w);
        }
        step_time("-c", O.host, t0);
        if (samples.empty()) { fputs(kNoneLeft, stderr); return false; }
    }
    if (!O.mutation.empty()) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<std::string> muts = split_commas(O.mutation);
        std::vector<int32_t> qp;
        std::vector<uint8_t> qn;
        for (const std::string &m : muts) {
            uh::Mutation mu;
            if (!mutation_from_string(m, mu)) { fprintf(stderr, "ERROR: %s is not a mutation\n", m.c_str()); return false; }   // (the reference dereferences the null pointer)
            qp.push_back(mu.position);
            qn.push_back((uint8_t)mu.mut_nuc);
        }
        std::vector<uint64_t> w;
        std::unordered_set<std::string> with_mut;
        if (!O.host) w = D.mutations(qp, qn, counts);
        for (size_t i = 0; i < muts.size(); i++) {
            fprintf(stderr, "Getting samples with mutation %s\n", muts[i].c_str());
            size_t found = O.host ? 0 : counts[i];
            if (O.host) {   // get_mutation_samples
                for (uh::Node *node : T.leaves()) {
                    bool assigned = false;
                    for (const auto &m : node->mutations)
                        if (qp[i] == m.position) {
                            if ((int8_t)qn[i] == m.mut_nuc) { with_mut.insert(node->id); found++; }
                            assigned = true;
                            break;
                        }
                    if (assigned) continue;
                    for (const uh::Node *anc : T.rsearch(node, false)) {
                        if (assigned) break;
                        for (const auto &m : anc->mutations)
                            if (qp[i] == m.position) {
                                if ((int8_t)qn[i] == m.mut_nuc) { with_mut.insert(node->id); found++; }
                                assigned = true;
                                break;
                            }
                    }
                }
            }
            if (!found) fprintf(stderr, "WARNING: No samples with mutation %s found in tree!\n", muts[i].c_str());
        }
        if (O.host) {
            std::vector<std::string> out;
            if (samples.empty()) { for (const uh::Node *n : T.dfs()) if (with_mut.count(n->id)) out.push_back(n->id); }
            else for (const auto &s : samples) if (with_mut.count(s)) out.push_back(s);
            samples = out;
        } else {
            samples = samples.empty() ? D.in_rank_order(w) : D.filter(samples, w);
        }
        step_time("-m", O.host, t0);
        if (samples.empty()) { fputs(kNoneLeft, stderr); return false; }
    }
    if (!O.match.empty()) {   // get_sample_match, select.cpp:506-520: on the host on both paths
        if (samples.empty()) samples = leaf_ids(T);
        std::vector<std::string> out;
        try {
            const std::regex pat(O.match);
            for (const std::string &s : samples) if (std::regex_match(s, pat)) out.push_back(s);
        } catch (const std::regex_error &e) { fprintf(stderr, "ERROR: bad regular expression %s: %s\n", O.match.c_str(), e.what()); return false; }
        samples = out;
        if (samples.empty()) { fputs(kNoneLeft, stderr); return false; }
    }
    return true;
}

// -e and -U (extract.cpp:411-427), between the linear filters and -Y.
bool select_after_filters(uh::Tree &T, const SelectOpts &O, SelectDevice &D, std::vector<std::string> &samples) {
    if (O.max_epps > 0) {   // get_samples_epps, uncertainty.cpp:350-368
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<uh::Node *> dfs = T.dfs();
        const std::unordered_set<std::string> check(samples.begin(), samples.end());
        std::vector<uh::Node *> todo;
        for (uh::Node *n : dfs) if (samples.empty() ? n->is_leaf() : check.count(n->id) != 0) todo.push_back(n);
        std::vector<std::string> good;
        if (O.host) {
            for (uh::Node *n : todo) if (host_epps(T, dfs, n) <= (size_t)O.max_epps) good.push_back(n->id);
        } else {
            D.up();
            std::vector<uint32_t> nodes;
            for (const uh::Node *n : todo) nodes.push_back(n->flat_index);
            const std::vector<uint32_t> e = D.epps(nodes);
            for (size_t i = 0; i < todo.size(); i++) if (e[i] <= (uint64_t)O.max_epps) good.push_back(todo[i]->id);
        }
        samples = good;
        step_time("-e", O.host, t0);
        if (samples.empty()) { fputs(kNoneLeft, stderr); return false; }
    }
    if (O.mrca) {   // get_mrca_samples, select.cpp:570-575
        const auto t0 = std::chrono::steady_clock::now();
        if (samples.empty()) { fprintf(stderr, "ERROR: -U/--from-mrca needs a selection\n"); return false; }   // (the reference dereferences the null root)
        std::vector<uint64_t> w, counts;
        if (!O.host && D.words_of(samples, w)) {
            uint32_t node = 0;
            uint64_t below = 0;
            if (ugp_select_mrca(D.h, w.data(), &node, &below) != UGP_OK) lib_fail("ugp_select_mrca");
            samples = D.in_leaves_order(D.subtrees({node}, counts), true);
        } else {   // the reference's walk; also the device path's when a selected name is not a leaf
            uh::Tree sub;
            std::string err;
            if (!uh::get_subtree(T, samples, sub, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return false; }
            uh::Node *mrca = T.get_node(sub.root->id);
            samples.clear();
            for (const uh::Node *l : T.leaves(mrca)) samples.push_back(l->id);
        }
        step_time("-U", O.host, t0);
    }
    return true;
}

// -p (extract.cpp:455-472), the last step.
bool select_prune(uh::Tree &T, const SelectOpts &O, SelectDevice &D, std::vector<std::string> &samples) {
    if (!O.prune) return true;
    fprintf(stderr, "Sample pruning requested...\n");
    const auto t0 = std::chrono::steady_clock::now();
    if (O.host) {
        const std::unordered_set<std::string> set(samples.begin(), samples.end());
        std::vector<std::string> out;
        for (const std::string &s : leaf_ids(T)) if (!set.count(s)) out.push_back(s);
        samples = out;
    } else {   // the complement of the bitmap; a selected name that is no leaf was never among the leaves
        D.up();
        std::vector<uint64_t> w(std::max<size_t>(D.n_words(), 1), 0);
        for (const std::string &s : samples) {
            const uh::Node *n = T.get_node(s);
            if (n && D.rank_of[n->flat_index] != UINT32_MAX) w[D.rank_of[n->flat_index] >> 6] |= 1ull << (D.rank_of[n->flat_index] & 63);
        }
        samples = D.in_leaves_order(w, false);
    }
    step_time("-p", O.host, t0);
    if (samples.empty()) {
        fprintf(stderr, "ERROR: No samples fulfill selected criteria (tree is left empty). Change arguments and try again\n");
        return false;
    }
    return true;
}

// ---- subtree: select, with the induced subtree from ugp_subtree.hip instead of get_subtree ---------------------------------------

void subtree_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd subtree -i tree.pb [-s samples.txt] [-k sample:k] [-I node] [-c clade[,clade]] [-m mutation[,mutation]] [-H regex]\n"
            "       [-a n] [-b n] [-P n] [-e n] [-U] [-Y y] [-p] [-u used.txt] [-t tree.nh] [-o out.pb] [-v out.vcf] [-n] [-d dir] [-T n]\n"
            "       [--device k] [--reference-ties] [--host-genotypes] [--host]\n"
            "  every option of matutils-amd select (see select --help), with the same output; the subtree of the selection (its samples,\n"
            "  the most recent common ancestor of every pair, the mutations merged along the collapsed paths) is built on the device from\n"
            "  the depth-first ranges instead of pair by pair on the host.\n"
            "      --host               run every selector and get_subtree as the reference's walk on the host (slow)\n");
}

// get_subtree (mat.cpp) from the three calls of ugp_subtree.hip: the kept nodes in depth-first order below their subtree parents,
// their merged entries (every field but the allele from the entry that opened the state) and the annotations of their chains.
bool device_subtree(uh::Tree &T, SelectDevice &D, const std::vector<std::string> &samples, uh::Tree &dst, std::string &err) {
    D.up();
    std::vector<uint32_t> nodes;
    for (const std::string &s : samples) {
        const uh::Node *n = T.get_node(s);
        if (!n) { err = "get_subtree: sample " + s + " is not in the tree"; return false; }
        nodes.push_back(n->flat_index);
    }
    const ugp_tree_desc desc = D.A.desc();
    if (ugp_subtree_attach(D.h, &desc) != UGP_OK) lib_fail("ugp_subtree_attach");
    const size_t room = std::min(2 * nodes.size(), D.A.bfs.size());   // n names keep fewer than 2n nodes
    std::vector<uint32_t> kept(room), kpar(room);
    std::vector<uint64_t> off(room + 1);
    uint64_t nk = 0, ne = 0;
    ugp_subtree_info info;
    if (ugp_subtree_nodes(D.h, nodes.size(), nodes.data(), kept.data(), kpar.data(), off.data(), room, &nk, &ne, &info) != UGP_OK)
        lib_fail("ugp_subtree_nodes");
    if (nk > room) { err = "get_subtree: more kept nodes than twice the selection"; return false; }
    off[nk] = ne;
    std::vector<int32_t> pos(std::max<uint64_t>(ne, 1));
    std::vector<uint32_t> first(std::max<uint64_t>(ne, 1));
    std::vector<uint8_t> nuc(std::max<uint64_t>(ne, 1));
    uint64_t got = 0;
    if (ugp_subtree_entries(D.h, pos.data(), first.data(), nuc.data(), ne, &got) != UGP_OK) lib_fail("ugp_subtree_entries");
    if (info.n_disagree)
        fprintf(stderr, "WARNING: %llu consecutive mutations at one position disagree and are skipped (first below node %s)\n",
                (unsigned long long)info.n_disagree, D.A.bfs[info.first_disagree]->id.c_str());
    const size_t n_ann = T.num_annotations();
    std::vector<uh::Node *> made(nk);
    for (uint64_t k = 0; k < nk; k++) {
        const uh::Node *src = D.A.bfs[kept[k]];
        uh::Node *nn = dst.create_node(src->id, kpar[k] == UINT32_MAX ? nullptr : made[kpar[k]], -1.0f);
        if (!nn) { err = "get_subtree: duplicate node " + src->id; return false; }
        nn->clade_annotations.assign(n_ann, "");
        nn->mutations.reserve(off[k + 1] - off[k]);
        for (uint64_t e = off[k]; e < off[k + 1]; e++) {
            uh::Mutation m = *D.A.ent[first[e]];
            m.mut_nuc = (int8_t)nuc[e];
            nn->mutations.push_back(m);
        }
        made[k] = nn;
    }
    // annotations: a kept node takes, per column, the deepest one of its chain; the subtree's root only its own (:1640-1644)
    std::vector<const uh::Node *> ann;
    for (const uh::Node *n : T.dfs())
        for (const std::string &a : n->clade_annotations) if (!a.empty()) { ann.push_back(n); break; }
    if (!ann.empty()) {
        std::vector<uint32_t> at(ann.size()), owner(ann.size());
        for (size_t i = 0; i < ann.size(); i++) at[i] = ann[i]->flat_index;
        if (ugp_subtree_owner(D.h, at.size(), at.data(), owner.data()) != UGP_OK) lib_fail("ugp_subtree_owner");
        for (size_t i = 0; i < ann.size(); i++) {   // depth-first: top-down within a chain
            if (owner[i] == UINT32_MAX || (owner[i] == 0 && at[i] != kept[0])) continue;
            uh::Node *nn = made[owner[i]];
            for (size_t k = 0; k < n_ann && k < ann[i]->clade_annotations.size(); k++)
                if (!ann[i]->clade_annotations[k].empty()) nn->clade_annotations[k] = ann[i]->clade_annotations[k];
        }
    }
    dst.curr_internal_node = T.curr_internal_node;
    dst.chroms = T.chroms;
    return true;
}

// ---- subtrees: extract -N, one induced subtree around each of many samples (get_minimum_subtrees, convert.cpp:665-798) -----------

void subtrees_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd subtrees -i tree.pb -N n -t name [-s samples.txt] [-k sample:k] [-I node] [-c clade[,clade]] [-m mutation[,mutation]]\n"
            "       [-H regex] [-a n] [-b n] [-P n] [-e n] [-U] [-Y y] [-p] [-u used.txt] [-d dir] [-T n] [--device k] [--reference-ties] [--host]\n"
            "  every selector of matutils-amd select (see select --help); with none, every leaf is a sample.  Then, as matUtils extract -N:\n"
            "  -N, --minimum-subtrees-size  cover the samples by subtrees of the n nearest leaves of a sample [REQUIRED]: the samples are\n"
            "                           walked in order, a sample already in an earlier subtree is skipped, and a sample with no ancestor of\n"
            "                           more than n leaves gets none\n"
            "  -t, --write-tree         write subtree i as <dir>/<name>-subtree-<i>.nw [REQUIRED], and <dir>/subtree-assignments.tsv with\n"
            "                           the file of every sample\n"
            "  -u, --used-samples       write a text file of the selected sample ids\n"
            "      --reference-ties     order equal distances as the reference's std::sort does (host, slow)\n"
            "      --host               run the selectors, get_nearby and get_subtree as the reference's walks on the host (slow)\n"
            "  The neighbourhoods are searched in rounds of batched device calls and every round's subtrees are built by one batched call.\n"
            "  -o, -v and -n are refused: the reference exits after the -N files, before it would write them.  -j is not supported.\n");
}

void step_ms(const char *what, bool host, double ms) {   // step_time for a step that runs in pieces
    fprintf(stderr, "Selection step %s (%s): %.3f msec\n", what, host ? "host" : "device", ms);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// get_nearby (select.cpp:206-276) on the host, statement by statement; nleaves: get_num_leaves of every node, counted once.
std::vector<std::string> host_nearby(const NearestSearch &near, const std::unordered_map<const uh::Node *, size_t> &nleaves, uh::Node *node,
                                     size_t k) {
    uh::Node *last = node;
    for (uh::Node *anc = node; anc; anc = anc->parent) {
        if (nleaves.at(anc) <= k) { last = anc; continue; }
        return near.literal(anc, last, k);   // the leaves of last_anc, then the nearest others up to k: never fewer than k
    }
    return {};
}

// The subtrees of one round's neighbourhoods from one ugp_subtree_batch call, each built as device_subtree builds its one (no owner
// call: a newick file carries no annotations), and written as the reference streams them (convert.cpp:724-731: no newline).
struct SubtreesWriter {
    uh::Tree &T;
    SelectDevice &D;
    const std::string newick_n;
    bool host, attached = false;
    double build_ms = 0, write_ms = 0;
    size_t written = 0;
    SubtreesWriter(uh::Tree &t, SelectDevice &d, const std::string &n, bool h) : T(t), D(d), newick_n(n), host(h) {}
    bool write(const uh::Tree &sub, std::string &err) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string path = newick_n + "-subtree-" + std::to_string(written++) + ".nw";
        std::ofstream f(path, std::ios::binary);
        f << uh::newick(sub, sub.root, true, true);
        f.close();
        write_ms += ms_since(t0);
        if (!f) { err = "could not write " + path; return false; }
        return true;
    }
    bool run(const std::vector<std::vector<std::string>> &sets, std::string &err) {
        if (sets.empty()) return true;
        auto t0 = std::chrono::steady_clock::now();
        if (host) {
            for (const auto &set : sets) {
                t0 = std::chrono::steady_clock::now();
                uh::Tree sub;
                if (!uh::get_subtree(T, set, sub, err)) return false;
                build_ms += ms_since(t0);
                if (!write(sub, err)) return false;
            }
            return true;
        }
        D.up();
        if (!attached) {
            const ugp_tree_desc desc = D.A.desc();
            if (ugp_subtree_attach(D.h, &desc) != UGP_OK) lib_fail("ugp_subtree_attach");
            attached = true;
        }
        const size_t n = sets.size();
        std::vector<uint64_t> sel_off(n + 1, 0), koff(n + 1), eoff(n + 1);
        std::vector<uint32_t> nodes;
        for (size_t b = 0; b < n; b++) {
            for (const std::string &s : sets[b]) {
                const uh::Node *nd = T.get_node(s);
                if (!nd) { err = "get_subtree: sample " + s + " is not in the tree"; return false; }
                nodes.push_back(nd->flat_index);
            }
            sel_off[b + 1] = nodes.size();
        }
        std::vector<ugp_subtree_batch_info> info(n);
        if (ugp_subtree_batch(D.h, n, sel_off.data(), nodes.data(), koff.data(), eoff.data(), info.data()) != UGP_OK) lib_fail("ugp_subtree_batch");
        const uint64_t nk = koff[n], ne = eoff[n];
        std::vector<uint32_t> kept(nk), kpar(nk), first(std::max<uint64_t>(ne, 1));
        std::vector<uint64_t> off(nk + 1);
        std::vector<int32_t> pos(std::max<uint64_t>(ne, 1));
        std::vector<uint8_t> nuc(std::max<uint64_t>(ne, 1));
        uint64_t got = 0;
        if (ugp_subtree_batch_nodes(D.h, kept.data(), kpar.data(), off.data(), nk, &got) != UGP_OK) lib_fail("ugp_subtree_batch_nodes");
        if (ugp_subtree_batch_entries(D.h, pos.data(), first.data(), nuc.data(), ne, &got) != UGP_OK) lib_fail("ugp_subtree_batch_entries");
        off[nk] = ne;
        build_ms += ms_since(t0);
        std::vector<uh::Node *> made;
        for (size_t b = 0; b < n; b++) {
            t0 = std::chrono::steady_clock::now();
            if (info[b].n_disagree)
                fprintf(stderr, "WARNING: %llu consecutive mutations at one position disagree and are skipped (first below node %s)\n",
                        (unsigned long long)info[b].n_disagree, D.A.bfs[info[b].first_disagree]->id.c_str());
            uh::Tree sub;
            const uint64_t k0 = koff[b], k1 = koff[b + 1];
            made.assign(k1 - k0, nullptr);
            for (uint64_t k = k0; k < k1; k++) {
                const uh::Node *src = D.A.bfs[kept[k]];
                uh::Node *nn = sub.create_node(src->id, kpar[k] == UINT32_MAX ? nullptr : made[kpar[k]], -1.0f);
                if (!nn) { err = "get_subtree: duplicate node " + src->id; return false; }
                nn->mutations.reserve(off[k + 1] - off[k]);
                for (uint64_t e = off[k]; e < off[k + 1]; e++) {
                    uh::Mutation m = *D.A.ent[first[e]];
                    m.mut_nuc = (int8_t)nuc[e];
                    nn->mutations.push_back(m);
                }
                made[k - k0] = nn;
            }
            build_ms += ms_since(t0);
            if (!write(sub, err)) return false;
        }
        return true;
    }
};

// The round size of the cover: the searches of one round fill round * n slots of a node and a distance (8 bytes): 2^22 slots, 32 MiB.
size_t subtrees_round(size_t n) { return std::max<size_t>(1, (size_t(1) << 22) / n); }

// get_minimum_subtrees (convert.cpp:665-798) for -t: the cover loop :681-711 in rounds -- the next `round` samples not yet seen are
// searched as one batch, and their answers are applied in order, dropping those that an earlier one of the round made seen (the
// sequential loop would not have searched them) -- then the files :713-797.
int minimum_subtrees(uh::Tree &T, const std::vector<std::string> &samples, size_t size, const std::string &prefix, const std::string &ftree,
                     NearestSearch &near, SelectDevice &D, bool host, size_t round) {
    fprintf(stderr, "Finding minimum covering sample subtrees.\n");
    const auto t_all = std::chrono::steady_clock::now();
    const std::string newick_n = prefix + ftree;
    std::unordered_map<std::string, long> seen;   // samples_we_have_seen: the first subtree that holds a sample, or -1
    std::unordered_map<const uh::Node *, size_t> nleaves;
    if (host) {
        const std::vector<uh::Node *> dfs = T.dfs();
        for (size_t i = dfs.size(); i-- > 0;) {
            size_t &c = nleaves[dfs[i]];
            if (dfs[i]->is_leaf()) c = 1;
            const size_t mine = c;
            if (dfs[i]->parent) nleaves[dfs[i]->parent] += mine;
        }
    }
    if (!round) round = subtrees_round(size);
    SubtreesWriter W(T, D, newick_n, host);
    std::string err;
    double cover_ms = 0;
    size_t n_sets = 0, rounds = 0;
    for (size_t i = 0; i < samples.size();) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<size_t> idx;
        std::vector<uh::Node *> qs;
        size_t j = i;
        for (; j < samples.size() && idx.size() < round; j++) {
            if (seen.count(samples[j])) continue;
            idx.push_back(j);
            qs.push_back(must_get(T, samples[j]));
        }
        std::vector<std::vector<std::string>> found;
        if (!host) {
            D.up();
            near.share(D.h, D.A);   // one handle for the searches and the subtrees
            found = near.run(qs, size);
        }
        std::vector<std::vector<std::string>> sets;
        for (size_t q = 0; q < idx.size(); q++) {
            const std::string &s = samples[idx[q]];
            if (seen.count(s)) continue;
            std::vector<std::string> keep = host ? host_nearby(near, nleaves, qs[q], size) : std::move(found[q]);
            if (keep.empty()) { seen.emplace(s, -1); continue; }
            for (const std::string &l : keep) seen.emplace(l, (long)(n_sets + sets.size()));   // insert: the first subtree owns a sample
            sets.push_back(std::move(keep));
        }
        cover_ms += ms_since(t0);
        if (!W.run(sets, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
        n_sets += sets.size();
        rounds++;
        i = j;
    }
    step_ms("cover", host, cover_ms);
    step_ms("subtrees", host, W.build_ms);
    fprintf(stderr, "%zu subtrees of %zu samples in %zu rounds; newick files: %.3f msec\n", n_sets, samples.size(), rounds, W.write_ms);
    const std::string tsv = prefix + "subtree-assignments.tsv";
    std::ofstream tracker(tsv, std::ios::binary);
    tracker << "samples\tnewick_file\n";   // no metadata can be loaded here: no further columns
    for (const std::string &s : samples) {
        const auto it = seen.find(s);
        const long v = it == seen.end() ? 0 : it->second;   // the reference's operator[] makes a 0 for a sample no subtree holds
        if (v == -1) continue;
        tracker << s << "\t" << newick_n << "-subtree-" << v << ".nw\n";
    }
    tracker.close();
    if (!tracker) { fprintf(stderr, "ERROR: could not write %s\n", tsv.c_str()); return 1; }
    fprintf(stderr, "Minimum subtree files written in %.0f msec; exiting\n", ms_since(t_all));
    return 0;
}

enum { kExtract = 0, kSelect = 1, kSubtree = 2, kSubtrees = 3 };

// extract_main, extract.cpp:149-640, 867-888 for the options of extract_usage; kSelect: the subcommand `select`, which adds the
// selectors; kSubtree: `subtree`, which is select with the induced subtree built on the device
int extract_or_select(int argc, char **argv, int mode) {
    const bool sel = mode != kExtract;
    std::string in_mat, fsamples, nearest_k, fused, ftree, fmat, fvcf, dir = "./";
    int max_parsimony = -1, max_branch = -1, max_path = -1, device = 0;
    size_t select_nearest = 0;
    bool reference_ties = false, no_genotypes = false, host_genotypes = false;
    SelectOpts S;
    S.on = sel;
    const bool many = mode == kSubtrees;
    long min_subtrees = 0, round_size = 0;
    void (*const show_usage)(FILE *) = many ? subtrees_usage : mode == kSubtree ? subtree_usage : sel ? select_usage : extract_usage;
    static const char *const unsupported[] = {
        "-K", "--nearest-k-batch", "-j", "--write-json", "-c", "--clade", "-m", "--mutation", "-H", "--match",
        "-V", "--closest-relatives", "-q", "--break-ties", "--within-distance", "--distance-threshold", "-z", "--set-size", "-W", "--add-random",
        "-Z", "--limit-to-lca", "-y", "--reroot", "--write-reroot-reference", "-R", "--resolve-polytomies", "-e", "--max-epps",
        "--max-mutation-density", "-I", "--get-internal-descendents", "-U", "--from-mrca", "-r", "--get-representative", "-p", "--prune",
        "-S", "--sample-paths", "-C", "--clade-paths", "-A", "--all-paths", "--write-diff", "-O", "--collapse-tree",
        "-l", "--write-taxodium", "-G", "--x-scale", "-B", "--title", "-D", "--description", "-J", "--include-nt", "-F", "--extra-fields",
        "-E", "--retain-branch-length", "-N", "--minimum-subtrees-size", "-X", "--usher-single-subtree-size", "-x", "--usher-minimum-subtrees-size",
        "--usher-clades-txt", "--usher-anchor-samples", "-Q", "--dump-metadata", "-L", "--whitelist", "--load-all-metadata", "-M", "--metadata",
        "-g", "--input-gtf", "-f", "--input-fasta"};
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); show_usage(stderr); return false; }
            dst = argv[++i];
            return true;
        };
        auto ival = [&](long &dst) -> bool {
            std::string t;
            if (!val(t)) return false;
            char *end = nullptr;
            dst = strtol(t.c_str(), &end, 10);
            if (t.empty() || *end) { fprintf(stderr, "ERROR: bad value %s for %s\n", t.c_str(), a.c_str()); show_usage(stderr); return false; }
            return true;
        };
        std::string tmp;
        long v = 0;
        bool ok = true;
        if (a == "-i" || a == "--input-mat") ok = val(in_mat);
        else if (many && (a == "-N" || a == "--minimum-subtrees-size")) ok = ival(min_subtrees);
        else if (many && a == "--round-size") ok = ival(round_size);   // (undocumented: the samples searched per round of the cover)
        else if (many && (a == "-o" || a == "--write-mat" || a == "-v" || a == "--write-vcf" || a == "-n" || a == "--no-genotypes")) {
            fprintf(stderr, "ERROR: %s is not written by matutils-amd subtrees: the reference exits after the -N files, before it would write it "
                            "(extract.cpp:723-730)\n", a.c_str());
            return 1;
        }
        else if (a == "-s" || a == "--samples") ok = val(fsamples);
        else if (a == "-k" || a == "--nearest-k") ok = val(nearest_k);
        else if (a == "-Y" || a == "--select-nearest") { ok = ival(v); if (ok && v < 0) { fprintf(stderr, "ERROR: bad value %ld for %s\n", v, a.c_str()); return 1; } select_nearest = (size_t)v; }
        else if (a == "-a" || a == "--max-parsimony") { ok = ival(v); max_parsimony = (int)v; }
        else if (a == "-b" || a == "--max-branch-length") { ok = ival(v); max_branch = (int)v; }
        else if (a == "-P" || a == "--max-path-length") { ok = ival(v); max_path = (int)v; }
        else if (a == "-u" || a == "--used-samples") ok = val(fused);
        else if (a == "-t" || a == "--write-tree") ok = val(ftree);
        else if (a == "-o" || a == "--write-mat") ok = val(fmat);
        else if (a == "-d" || a == "--output-directory") ok = val(dir);
        else if (a == "-T" || a == "--threads") ok = val(tmp);
        else if (a == "--device") { ok = val(tmp); device = atoi(tmp.c_str()); }
        else if (a == "--reference-ties") reference_ties = true;
        else if (a == "-v" || a == "--write-vcf") ok = val(fvcf);
        else if (a == "-n" || a == "--no-genotypes") no_genotypes = true;
        else if (a == "--host-genotypes") host_genotypes = true;
        else if (sel && (a == "-I" || a == "--get-internal-descendents")) ok = val(S.internal);
        else if (sel && (a == "-c" || a == "--clade")) ok = val(S.clade);
        else if (sel && (a == "-m" || a == "--mutation")) ok = val(S.mutation);
        else if (sel && (a == "-H" || a == "--match")) ok = val(S.match);
        else if (sel && (a == "-e" || a == "--max-epps")) { ok = ival(v); if (ok && v < 0) { fprintf(stderr, "ERROR: bad value %ld for %s\n", v, a.c_str()); return 1; } S.max_epps = v; }
        else if (sel && (a == "-U" || a == "--from-mrca")) S.mrca = true;
        else if (sel && (a == "-p" || a == "--prune")) S.prune = true;
        else if (sel && a == "--host") S.host = true;
        else if (a == "-h" || a == "--help") { show_usage(stderr); return 0; }
        else {
            for (const char *u : unsupported)
                if (a == u) {
                    fprintf(stderr, "ERROR: %s is not supported by matutils-amd extract (use the reference matUtils)\n", a.c_str());
                    return 1;
                }
            fprintf(stderr, "ERROR: unknown option %s\n", a.c_str());
            show_usage(stderr);
            return 1;
        }
        if (!ok) return 1;
    }
    if (in_mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); show_usage(stderr); return 1; }
    if (many && min_subtrees <= 0) {
        fprintf(stderr, "ERROR: matutils-amd subtrees needs -N/--minimum-subtrees-size with a size above 0\n");
        show_usage(stderr);
        return 1;
    }
    if (many && ftree.empty()) {   // convert.cpp:668-671 (-j is not supported here)
        fprintf(stderr, "ERROR: Either JSON (-j) or Newick (-t) output must be requested alongside -N.");
        return 1;
    }
    if (many && round_size < 0) { fprintf(stderr, "ERROR: bad value %ld for --round-size\n", round_size); return 1; }
    struct stat sb;
    if (stat(dir.c_str(), &sb) != 0) {
        fprintf(stderr, "Creating output directory.\n\n");
        mkdir(dir.c_str(), 0777);
    }
    char *canon = realpath(dir.c_str(), nullptr);
    if (!canon) { fprintf(stderr, "ERROR: cannot resolve the output directory %s\n", dir.c_str()); return 1; }
    const std::string prefix = std::string(canon) + "/";
    free(canon);
    if (fused.empty() && ftree.empty() && fmat.empty() && fvcf.empty()) { fprintf(stderr, "ERROR: No output files requested!\n"); return 1; }
    std::string sample_id;
    int nk = 0;
    if (!nearest_k.empty()) {   // :272-284 (checked before the load here: the messages are the reference's)
        const size_t split = nearest_k.find(":");
        if (split == std::string::npos) {
            fprintf(stderr, "ERROR: Invalid formatting of -k argument. Requires input in the form of 'sample_id:k' to get k nearest samples to sample_id\n");
            return 1;
        }
        sample_id = nearest_k.substr(0, split);
        nk = atoi(nearest_k.substr(split + 1).c_str());
        if (nk <= 0) { fprintf(stderr, "ERROR: Invalid neighborhood size. Please choose a positive nonzero integer.\n"); return 1; }
    }
    fprintf(stderr, "Loading input MAT file %s.\n", in_mat.c_str());
    if (in_mat.find(".pb") == std::string::npos) { fprintf(stderr, "ERROR: Input file ending not recognized. Must be .pb (.json is not supported by matutils-amd)\n"); return 1; }
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(in_mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    T.uncondense_leaves();
    fprintf(stderr, "Checking for and applying sample selection arguments\n");
    const char *none = "ERROR: No samples fulfill selected criteria. Change arguments and try again\n";
    std::vector<std::string> samples;
    if (!fsamples.empty()) {
        samples = read_sample_names(fsamples);
        if (samples.empty()) { fprintf(stderr, "ERROR: Sample file is empty or unparseable!"); return 1; }
    }
    NearestSearch near(T, device, reference_ties);
    if (!nearest_k.empty()) {   // :285-293
        const std::vector<std::string> nks = near.run({must_get(T, sample_id)}, (size_t)nk)[0];
        if (nks.empty()) {   // the reference's assert (nk_samples.size() > 0)
            fprintf(stderr, "ERROR: no ancestor of %s has more than %d leaves: the nearest-k selection is empty\n", sample_id.c_str(), nk);
            return 1;
        }
        if (samples.empty()) samples = nks;
        else {   // sample_intersect: the -s samples that are among the nearest
            const std::unordered_set<std::string> set(nks.begin(), nks.end());
            std::vector<std::string> inter;
            for (const std::string &s : samples) if (set.count(s)) inter.push_back(s);
            samples = inter;
        }
    }
    SelectDevice seldev(T, device, mode == kSubtree || many ? (unsigned)uh::TreeArrays::kEntries : 0u);
    if (sel && !select_before_filters(T, S, seldev, samples)) return 1;
    if (max_parsimony >= 0) { samples = get_parsimony_samples(T, samples, max_parsimony); if (samples.empty()) { fputs(none, stderr); return 1; } }
    if (max_branch >= 0) { samples = get_short_steppers(T, samples, max_branch); if (samples.empty()) { fputs(none, stderr); return 1; } }
    if (max_path >= 0) { samples = get_short_paths(T, samples, max_path); if (samples.empty()) { fputs(none, stderr); return 1; } }
    if (sel && !select_after_filters(T, S, seldev, samples)) return 1;
    if (select_nearest > 0) {   // :429-440; the union in depth-first order (the reference: an unordered_set's)
        fprintf(stderr, "Selecting context samples...\n");
        std::vector<uh::Node *> qs;
        for (const std::string &s : samples) qs.push_back(must_get(T, s));
        std::unordered_set<std::string> set;
        for (const auto &names : near.run(qs, select_nearest)) set.insert(names.begin(), names.end());
        samples.clear();
        for (const uh::Node *n : T.dfs()) if (set.count(n->id)) samples.push_back(n->id);
    }
    if (sel && !select_prune(T, S, seldev, samples)) return 1;
    if (many) {   // :591-598 (every leaf), -u, then :723-730; the subtree of the whole selection is built there and never used
        if (samples.empty()) {
            fprintf(stderr, "No sample selection arguments passed; using full input tree for further output.\n");
            samples = leaf_ids(T);
        }
        if (!fused.empty()) {
            fprintf(stderr, "Dumping selected samples to file...\n");
            std::ofstream f(prefix + fused, std::ios::binary);
            for (const std::string &s : samples) f << s << "\n";
            if (!f) { fprintf(stderr, "ERROR: could not write %s\n", (prefix + fused).c_str()); return 1; }
        }
        return minimum_subtrees(T, samples, (size_t)min_subtrees, prefix, ftree, near, seldev, S.host, (size_t)round_size);
    }
    // :590-606: nothing selected = the whole tree
    uh::Tree sub;
    uh::Tree *out = &T;
    if (samples.empty()) {
        fprintf(stderr, "No sample selection arguments passed; using full input tree for further output.\n");
        samples = leaf_ids(T);
    } else {
        fprintf(stderr, "Extracting subtree of %zu samples.\n", samples.size());
        const auto t0 = std::chrono::steady_clock::now();
        const bool ok = mode == kSubtree && !S.host ? device_subtree(T, seldev, samples, sub, err) : uh::get_subtree(T, samples, sub, err);
        if (!ok) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
        if (mode == kSubtree) step_time("subtree", S.host, t0);
        out = &sub;
    }
    if (!fused.empty()) {
        fprintf(stderr, "Dumping selected samples to file...\n");
        std::ofstream f(prefix + fused, std::ios::binary);
        for (const std::string &s : samples) f << s << "\n";
        if (!f) { fprintf(stderr, "ERROR: could not write %s\n", (prefix + fused).c_str()); return 1; }
    }
    if (!fvcf.empty()) {   // :859-862, before the newick file as there
        fprintf(stderr, "Generating VCF of final tree\n");
        if (int rc = make_vcf(*out, prefix + fvcf, no_genotypes, samples, device, host_genotypes)) return rc;
    }
    if (!ftree.empty()) {
        fprintf(stderr, "Generating Newick file of final tree\n");
        FILE *f = must_open(prefix + ftree, "w");
        fprintf(f, "%s\n", uh::newick(*out, out->root, true, true).c_str());
        fclose(f);
    }
    if (!fmat.empty()) {
        fprintf(stderr, "Saving output MAT file %s.\n", (prefix + fmat).c_str());
        out->condense_leaves();
        if (!uh::save_mat(*out, prefix + fmat, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    }
    return 0;
}

int extract(int argc, char **argv) { return extract_or_select(argc, argv, kExtract); }
int select_samples(int argc, char **argv) { return extract_or_select(argc, argv, kSelect); }
int subtree(int argc, char **argv) { return extract_or_select(argc, argv, kSubtree); }
int subtrees(int argc, char **argv) { return extract_or_select(argc, argv, kSubtrees); }

// ---- summary (summary.cpp) ----------------------------------------------------------------------------------------

void summary_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd summarize -i tree.pb [-s samples.tsv] [-c clades.tsv] [-C sample-clades.tsv] [-m mutations.tsv] [-a aberrant.tsv]\n"
            "       [-R roho.tsv] [-A] [-M] [-d dir] [-T n] [--device k] [--host]\n"
            "  -i, --input-mat          input mutation-annotated tree [REQUIRED]; with no table option, print basic counts\n"
            "  -d, --output-directory   directory of the output files [./]\n"
            "  -s, --samples            tsv of all samples, their parsimony score and the id of their parent node\n"
            "  -c, --clades             tsv of all clades and their inclusive and exclusive sample counts\n"
            "  -C, --sample-clades      tsv of all samples and their clade values\n"
            "  -m, --mutations          tsv of all mutations in the tree and their occurrence count\n"
            "  -a, --aberrant           tsv of duplicate sample identifiers and internal nodes without mutations\n"
            "  -R, --calculate-roho     tsv of the RoHO values of all mutations\n"
            "  -A, --get-all-basic      write samples.tsv, clades.tsv, mutations.tsv and aberrant.tsv\n"
            "  -M, --mutation-stats     print counts of the kinds of mutations\n"
            "  -T, --threads            accepted for compatibility (the tables run on the device)\n"
            "      --device             HIP device ordinal [0]\n"
            "      --host               compute every table with the reference's serial walks on the host (slow; no device)\n"
            "  (-t / --translate with -g / -f, -E / --expanded-roho, -H / --haplotype and -N / --node-stats are not supported)\n");
}

// The tables of summary.cpp that are one pass over the host tree, on either path.
void summary_samples(const uh::Tree &T, std::ofstream &f) {   // write_sample_table, :70-86
    f << "sample\tparsimony\tparent_id\n";
    for (const uh::Node *s : T.dfs())
        if (s->is_leaf()) f << s->id << "\t" << s->mutations.size() << "\t" << (s->parent ? s->parent->id : std::string()) << "\n";
}
void summary_aberrant(const uh::Tree &T, std::ofstream &f) {   // write_aberrant_table, :266-295
    f << "NodeID\tIssue\n";
    const size_t na = T.num_annotations();
    std::set<std::string> seen;
    for (const uh::Node *n : T.dfs()) {
        if (!seen.insert(n->id).second) f << n->id << "\tduplicate-node-id\n";
        if (n->mutations.empty() && !n->is_leaf() && !n->is_root()) f << n->id << "\tinternal-no-mutations\n";
        if (na != n->clade_annotations.size()) f << n->id << "\tclade-annotations (" << n->clade_annotations.size() << " not " << na << ")\n";
    }
}
void summary_mut_stats(const uh::Tree &T) {   // print_mut_stats, :224-242
    int freq[16] = {0};
    auto two_bit = [](int8_t a) { return 31 - __builtin_clz((unsigned int)a); };
    for (const uh::Node *n : T.dfs())
        for (const auto &m : n->mutations) {
            if (m.par_nuc <= 0 || m.mut_nuc <= 0) continue;   // (the reference indexes out of bounds there)
            freq[(4 * two_bit(m.par_nuc) + two_bit(m.mut_nuc)) & 15]++;
        }
    for (int from = 0; from < 4; from++)
        for (int to = 0; to < 4; to++) printf("%c->%c\t%d\n", uh::nuc_char((int8_t)(1 << from)), uh::nuc_char((int8_t)(1 << to)), freq[4 * from + to]);
}
void summary_basic(const uh::Tree &T, size_t condensed_nodes, size_t condensed_leaves) {   // :746-775
    int nodecount = 0, samplecount = 0;
    size_t slevel = 0, mlevel = 0;
    std::vector<std::pair<const uh::Node *, size_t>> stack{{T.root, 1}};
    while (!stack.empty()) {
        const auto [n, level] = stack.back();
        stack.pop_back();
        nodecount++;
        if (n->is_leaf()) { slevel += level; mlevel = std::max(mlevel, level); samplecount++; }
        for (const uh::Node *c : n->children) stack.push_back({c, level + 1});
    }
    printf("Total Nodes in Tree: %d\n", nodecount);
    printf("Total Samples in Tree: %d\n", samplecount);
    printf("Total Condensed Nodes in Tree: %ld\n", (long)condensed_nodes);
    printf("Total Samples in Condensed Nodes: %ld\n", (long)condensed_leaves);
    printf("Total Tree Parsimony: %ld\n", (long)T.parsimony_score());
    printf("Number of Clade Annotations: %ld\n", (long)T.num_annotations());
    printf("Max Tree Depth: %ld\n", (long)mlevel);
    printf("Mean Tree Depth: %f\n", static_cast<float>(slevel) / samplecount);
}

// --host: the reference's walks, statement by statement.
void host_mutations(const uh::Tree &T, std::ofstream &f) {   // write_mutation_table, :139-174
    f << "ID\toccurrence\n";
    std::map<std::string, int> counts;
    for (const uh::Node *s : T.dfs())
        for (const auto &m : s->mutations) {
            const std::string name = m.str();
            if (name != "MASKED") counts[name]++;
        }
    for (const auto &kv : counts) f << kv.first << "\t" << kv.second << "\n";
}
void host_clades(const uh::Tree &T, std::ofstream &f) {   // write_clade_table, :88-137
    f << "clade\tinclusive_count\texclusive_count\n";
    std::map<std::string, size_t> incl, excl;
    for (uh::Node *s : T.leaves()) {
        bool first[2] = {true, true};
        for (const uh::Node *a : T.rsearch(s, false)) {
            const auto &canns = a->clade_annotations;
            for (size_t i = 0; i < 2 && i < canns.size(); i++) {
                if (canns[i] == "") continue;
                if (incl.find(canns[i]) == incl.end()) { incl[canns[i]] = 0; excl[canns[i]] = 0; }
                incl[canns[i]]++;
                if (first[i]) { excl[canns[i]]++; first[i] = false; }
            }
        }
    }
    for (const auto &kv : incl) f << kv.first << "\t" << kv.second << "\t" << excl[kv.first] << "\n";
}
void sample_clades_header(const uh::Tree &T, std::ofstream &f) {
    f << "sample";
    for (size_t i = 1; i <= T.num_annotations(); i++) f << "\tannotation_" << i;
    f << "\n";
}
void host_sample_clades(const uh::Tree &T, std::ofstream &f) {   // write_sample_clades_table, :297-341
    const size_t na = T.num_annotations();
    sample_clades_header(T, f);
    for (uh::Node *n : T.leaves()) {
        std::vector<std::string> found(na, "None");
        for (const uh::Node *a : T.rsearch(n, false)) {
            const auto &canns = a->clade_annotations;
            for (size_t i = 0; i < std::min(na, canns.size()); i++)
                if (canns[i] != "" && found[i] == "None") found[i] = canns[i];
            if (std::find(found.begin(), found.end(), "None") == found.end()) break;
        }
        f << n->id;
        for (const std::string &s : found) f << "\t" << s;
        f << "\n";
    }
}
const char *kRohoHeader = "mutation\tparent_node\tchild_count\toccurrence_node\toffspring_with\tmedian_offspring_without\tsingle_roho\n";
void roho_row(std::ofstream &f, const std::string &mut, const std::string &parent, size_t child_count, const std::string &child, size_t sum_wit,
              float med_non) {   // :482, :500
    f << mut << "\t" << parent << "\t" << child_count << "\t" << child << "\t" << sum_wit << "\t" << med_non << "\t" << std::log10(sum_wit / med_non)
      << "\t" << "\n";
}
void host_roho(const uh::Tree &T, std::ofstream &f) {   // write_roho_table without dates, :343-506
    f << kRohoHeader;
    for (uh::Node *n : T.dfs()) {
        std::map<std::string, std::string> candidates;
        std::map<std::string, size_t> child_increment;
        std::vector<std::string> ccheck;
        for (const uh::Node *c : n->children)
            if (!c->is_leaf()) {
                ccheck.push_back(c->id);
                for (const auto &m : c->mutations) candidates[m.str()] = c->id;
            }
        if (candidates.empty()) continue;
        for (uh::Node *c : n->children) {
            size_t ccount = 0;
            if (c->is_leaf()) continue;
            for (const uh::Node *dn : T.dfs(c)) {
                if (dn->id == c->id) continue;
                if (dn->is_leaf()) ccount++;
                for (const auto &m : dn->mutations) candidates.erase(m.str());
            }
            if (ccount > 1) child_increment[c->id] = ccount;
        }
        if (candidates.empty() || child_increment.size() <= 1) continue;
        for (const auto &ms : candidates) {
            std::vector<size_t> all_non;
            size_t sum_wit = 0;
            for (const auto &cs : child_increment) {
                if (cs.first != ms.second) { if (cs.second > 5) all_non.push_back(cs.second); }
                else if (cs.second > 5) sum_wit += cs.second;
            }
            if (all_non.empty() || sum_wit == 0) continue;
            float med_non;
            std::sort(all_non.begin(), all_non.end());
            if (all_non.size() % 2 == 0) med_non = (all_non[all_non.size() / 2 - 1] + all_non[all_non.size() / 2]) / 2;
            else med_non = all_non[all_non.size() / 2];
            roho_row(f, ms.first, n->id, ccheck.size(), ms.second, sum_wit, med_non);
        }
    }
}

// The device path: the numbers of -m, -R, -c and -C come from ugp_summary.hip, names are kept here.
struct SummaryDevice {
    std::vector<uh::Node *> bfs;
    std::vector<const uh::Mutation *> ent;
    Mat h;
    void up(const uh::Tree &T, int device) {
        uh::TreeArrays A(T, uh::TreeArrays::kEntries);
        // the handle takes the bare topology, the summary tables the mutations as they are stored (masked, repeated positions)
        const ugp_tree_desc desc = A.desc();
        h.create(A.bare(), device);
        if (ugp_summary_attach(h, &desc) != UGP_OK) lib_fail("ugp_summary_attach");
        bfs = std::move(A.bfs);   // the library has its copy of the arrays: only the nodes and the entries are kept
        ent = std::move(A.ent);
    }
    void mutations(std::ofstream &f) {
        uint64_t n = 0;
        if (ugp_summary_mutations(h, nullptr, 0, &n) != UGP_OK) lib_fail("ugp_summary_mutations");
        std::vector<ugp_sm_mutation> recs(n);
        if (n && ugp_summary_mutations(h, recs.data(), n, &n) != UGP_OK) lib_fail("ugp_summary_mutations");
        std::vector<std::pair<std::string, uint32_t>> rows;   // the reference's std::map orders by the name's bytes: A100G before A23G
        rows.reserve(n);
        for (const auto &r : recs) {
            uh::Mutation m;
            m.position = r.pos; m.par_nuc = (int8_t)r.par; m.mut_nuc = (int8_t)r.nuc;
            rows.emplace_back(m.str(), r.count);
        }
        std::sort(rows.begin(), rows.end());
        f << "ID\toccurrence\n";
        for (const auto &r : rows) f << r.first << "\t" << r.second << "\n";
    }
    void roho(std::ofstream &f) {
        uint64_t n = 0;
        if (ugp_summary_roho(h, nullptr, 0, &n) != UGP_OK) lib_fail("ugp_summary_roho");
        std::vector<ugp_sm_roho> recs(n);
        if (n && ugp_summary_roho(h, recs.data(), n, &n) != UGP_OK) lib_fail("ugp_summary_roho");
        f << kRohoHeader;
        std::vector<std::pair<std::string, const ugp_sm_roho *>> rows;
        for (size_t a = 0; a < recs.size();) {   // the records of one parent follow each other; its rows come in name order
            size_t b = a;
            rows.clear();
            for (; b < recs.size() && recs[b].parent == recs[a].parent; b++) rows.emplace_back(ent[recs[b].entry]->str(), &recs[b]);
            std::sort(rows.begin(), rows.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
            for (const auto &r : rows)
                roho_row(f, r.first, bfs[r.second->parent]->id, r.second->child_count, bfs[r.second->child]->id, r.second->offspring_with,
                         (float)r.second->median_without);
            a = b;
        }
    }
    // Per column the nodes with an annotation there (`none_is_empty`: a clade literally named "None" never sticks in -C, :318).
    void clades(size_t ncols, bool none_is_empty, std::vector<uint64_t> &off, std::vector<uint32_t> &nodes, std::vector<uint32_t> &incl,
                std::vector<uint32_t> &excl, std::vector<uint32_t> &leaf_clade, size_t n_leaves) {
        off.assign(1, 0);
        nodes.clear();
        for (size_t c = 0; c < ncols; c++) {
            for (size_t j = 0; j < bfs.size(); j++) {
                const auto &canns = bfs[j]->clade_annotations;
                if (canns.size() > c && canns[c] != "" && !(none_is_empty && canns[c] == "None")) nodes.push_back((uint32_t)j);
            }
            off.push_back(nodes.size());
        }
        incl.assign(nodes.size(), 0);
        excl.assign(nodes.size(), 0);
        leaf_clade.assign(ncols * n_leaves, UINT32_MAX);
        if (ncols && ugp_summary_clades(h, off.data(), nodes.data(), ncols, incl.data(), excl.data(), leaf_clade.data()) != UGP_OK)
            lib_fail("ugp_summary_clades");
    }
    void clade_table(const uh::Tree &T, std::ofstream &f) {
        std::vector<uint64_t> off;
        std::vector<uint32_t> nodes, incl, excl, lc;
        clades(2, false, off, nodes, incl, excl, lc, T.leaves().size());   // -c reads the first two columns only (:102-128)
        std::map<std::string, std::pair<size_t, size_t>> counts;
        for (size_t c = 0; c < 2; c++)
            for (uint64_t a = off[c]; a < off[c + 1]; a++) {
                if (!incl[a]) continue;   // no leaf below it: no walk ever meets it
                auto &e = counts[bfs[nodes[a]]->clade_annotations[c]];
                e.first += incl[a];
                e.second += excl[a];
            }
        f << "clade\tinclusive_count\texclusive_count\n";
        for (const auto &kv : counts) f << kv.first << "\t" << kv.second.first << "\t" << kv.second.second << "\n";
    }
    void sample_clades(const uh::Tree &T, std::ofstream &f) {
        const size_t na = T.num_annotations();
        const std::vector<uh::Node *> leaves = T.leaves();
        std::vector<uint64_t> off;
        std::vector<uint32_t> nodes, incl, excl, lc;
        clades(na, true, off, nodes, incl, excl, lc, leaves.size());
        sample_clades_header(T, f);
        for (size_t i = 0; i < leaves.size(); i++) {
            f << leaves[i]->id;
            for (size_t c = 0; c < na; c++) {
                const uint32_t a = lc[c * leaves.size() + i];
                f << "\t" << (a == UINT32_MAX ? std::string("None") : bfs[a]->clade_annotations[c]);
            }
            f << "\n";
        }
    }
};

int summary(int argc, char **argv) {   // summary_main, :635-776
    std::string mat, dir = "./", samples, clades, sample_clades, mutations, aberrant, roho;
    bool get_all = false, mut_stats = false, host = false;
    int device = 0;
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); summary_usage(stderr); return false; }
            dst = argv[++i];
            return true;
        };
        std::string tmp;
        bool ok = true;
        if (a == "-i" || a == "--input-mat") ok = val(mat);
        else if (a == "-d" || a == "--output-directory") ok = val(dir);
        else if (a == "-s" || a == "--samples") ok = val(samples);
        else if (a == "-c" || a == "--clades") ok = val(clades);
        else if (a == "-C" || a == "--sample-clades") ok = val(sample_clades);
        else if (a == "-m" || a == "--mutations") ok = val(mutations);
        else if (a == "-a" || a == "--aberrant") ok = val(aberrant);
        else if (a == "-R" || a == "--calculate-roho") ok = val(roho);
        else if (a == "-A" || a == "--get-all-basic") get_all = true;
        else if (a == "-M" || a == "--mutation-stats") mut_stats = true;
        else if (a == "-T" || a == "--threads") ok = val(tmp);
        else if (a == "--device") { ok = val(tmp); device = atoi(tmp.c_str()); }
        else if (a == "--host") host = true;
        else if (a == "-h" || a == "--help") { summary_usage(stdout); return 0; }
        else if (a == "-t" || a == "--translate" || a == "-g" || a == "--input-gtf" || a == "-f" || a == "--input-fasta" || a == "-E" ||
                 a == "--expanded-roho" || a == "-H" || a == "--haplotype" || a == "-N" || a == "--node-stats") {
            fprintf(stderr, "ERROR: %s is not supported by matutils-amd summarize (use the reference matUtils)\n", a.c_str());
            return 1;
        }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); summary_usage(stderr); return 1; }
        if (!ok) return 1;
    }
    if (mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); summary_usage(stderr); return 1; }
    struct stat sb;
    if (stat(dir.c_str(), &sb) != 0) {
        fprintf(stderr, "Creating output directory.\n\n");
        mkdir(dir.c_str(), 0777);
    }
    char *canon = realpath(dir.c_str(), nullptr);
    if (!canon) { fprintf(stderr, "ERROR: cannot resolve the output directory %s\n", dir.c_str()); return 1; }
    const std::string prefix = std::string(canon) + "/";
    free(canon);
    if (get_all) { samples = "samples.tsv"; clades = "clades.tsv"; mutations = "mutations.tsv"; aberrant = "aberrant.tsv"; }
    fprintf(stderr, "Loading input MAT file %s.\n", mat.c_str());
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    const size_t condensed_leaves = T.condensed_leaves.size(), condensed_nodes = T.condensed_nodes.size();
    T.uncondense_leaves();
    SummaryDevice D;
    if (!host && !(clades.empty() && sample_clades.empty() && mutations.empty() && roho.empty())) D.up(T, device);
    bool failed = false;
    auto table = [&](const std::string &name, const char *what, auto &&write) {
        if (name.empty() || failed) return;
        fprintf(stderr, "Writing %s to output %s\n", what, (prefix + name).c_str());
        const auto t0 = std::chrono::steady_clock::now();
        std::ofstream f(prefix + name, std::ios::binary);
        write(f);
        f.close();
        if (!f) { fprintf(stderr, "ERROR: could not write %s\n", (prefix + name).c_str()); failed = true; return; }
        fprintf(stderr, "Completed in %ld msec \n\n",
                (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count());
    };
    table(clades, "clades", [&](std::ofstream &f) { if (host) host_clades(T, f); else D.clade_table(T, f); });
    table(samples, "samples", [&](std::ofstream &f) { summary_samples(T, f); });
    table(mutations, "mutations", [&](std::ofstream &f) { if (host) host_mutations(T, f); else D.mutations(f); });
    table(aberrant, "bad nodes", [&](std::ofstream &f) { summary_aberrant(T, f); });
    if (mut_stats) summary_mut_stats(T);
    table(sample_clades, "clade associations for all samples", [&](std::ofstream &f) { if (host) host_sample_clades(T, f); else D.sample_clades(T, f); });
    table(roho, "RoHo values", [&](std::ofstream &f) { if (host) host_roho(T, f); else D.roho(f); });
    if (failed) return 1;
    if (clades.empty() && samples.empty() && mutations.empty() && aberrant.empty() && sample_clades.empty() && roho.empty()) {
        fprintf(stderr, "No arguments set; getting basic statistics...\n");
        summary_basic(T, condensed_nodes, condensed_leaves);
    }
    return 0;
}

// ---- translate (translate.cpp, summary --translate) ----------------------------------------------------------------

void translate_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd translate -i tree.pb -g genes.gtf -f ref.fa -t out.tsv [-d dir] [-T n] [--device k] [--host]\n"
            "  -i, --input-mat          input mutation-annotated tree [REQUIRED]\n"
            "  -g, --input-gtf          GTF of the genes (CDS lines; taken as given, not relative to -d) [REQUIRED]\n"
            "  -f, --input-fasta        FASTA of the reference (taken as given, not relative to -d) [REQUIRED]\n"
            "  -t, --translate          tsv of the amino acid, nucleotide and codon changes of every node [REQUIRED]\n"
            "  -d, --output-directory   directory of the output file [./]\n"
            "  -T, --threads            accepted for compatibility (the table runs on the device)\n"
            "      --device             HIP device ordinal [0]\n"
            "      --host               the reference's serial walk on the host (slow; no device)\n");
}

// translate.hpp:20-49: the standard code and the ambiguous codons that still name one amino acid; anything else reads 'X'
char tr_protein(const std::string &nt) {
    static const std::unordered_map<std::string, char> table = [] {
        const char *rows[] = {"A GCT GCC GCA GCG GCN", "C TGT TGC TGY", "D GAT GAC GAY", "E GAA GAG GAR", "F TTT TTC TTY", "G GGT GGC GGA GGG GGN",
                              "H CAT CAC CAY", "I ATT ATC ATA ATH", "K AAA AAG AAR", "L TTA TTG CTT CTC CTA CTG YTR CTN", "M ATG", "N AAT AAC AAY",
                              "P CCT CCC CCA CCG CCN", "Q CAA CAG CAR", "R CGT CGC CGA CGG AGA AGG CGN MGR", "S TCT TCC TCA TCG AGT AGC TCN AGY",
                              "T ACT ACC ACA ACG ACN", "V GTT GTC GTA GTG GTN", "W TGG", "Y TAT TAC TAY", "* TAG TAA TGA"};
        std::unordered_map<std::string, char> m;
        for (const char *r : rows) {
            std::vector<std::string> w;
            split_ws(r, w);
            for (size_t i = 1; i < w.size(); i++) m[w[i]] = w[0][0];
        }
        return m;
    }();
    const auto it = table.find(nt);
    return it == table.end() ? 'X' : it->second;
}
char tr_complement(char c) {
    static const char from[] = "ACGTMRWSYKVHDBN", to[] = "TGCAKYWSRMBDHVN";
    const char *p = c ? strchr(from, c) : nullptr;
    return p ? to[p - from] : 'N';
}

struct TrCodon {   // struct Codon, translate.hpp:51-94; sign: slot k holds position start + sign * k (the reference indexes by abs())
    std::string orf_name, nucleotides, initial;
    int codon_number = 0, start_position = 0, sign = 1;
    char protein = 'X';
    void mutate(int nuc_pos, char nuc) {
        nucleotides[std::abs(nuc_pos - start_position)] = nuc;
        protein = tr_protein(nucleotides);
    }
    std::string codon_id() const { return orf_name + ':' + std::to_string(codon_number + 1); }
};
using TrCodonMap = std::unordered_map<int, std::vector<TrCodon *>>;

std::vector<std::string> tr_split(const std::string &s, char delim) {   // split, :3-11
    std::vector<std::string> out;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, delim)) out.push_back(item);
    return out;
}

bool tr_read_fasta(const std::string &path, std::string &ref) {   // build_reference, :13-30
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "ERROR: Could not open the fasta file: %s!\n", path.c_str()); return false; }
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '>') continue;
        for (auto &c : line) c = (char)toupper(c);
        if (line.back() == '\r') line.pop_back();
        ref += line;
    }
    return true;
}

// build_codon_map, :42-238: the codons in creation order.  Where the reference would read past the FASTA or past a line's fields,
// this returns false with one line in `err`.
bool tr_build_codons(const std::string &path, const std::string &ref, std::vector<TrCodon> &codons, std::string &err) {
    std::ifstream f(path);
    if (!f) { err = "ERROR: Could not open the gtf file: " + path + "!"; return false; }
    std::vector<std::string> lines, done;
    std::string line;
    while (std::getline(f, line)) lines.push_back(line);
    auto number = [&](const std::string &s, int &v) {
        try { v = std::stoi(s); } catch (...) { err = "ERROR: GTF: '" + s + "' is not a number"; return false; }
        return true;
    };
    auto gene_of = [&](const std::string &field, std::string &gene) {
        const std::vector<std::string> parts = tr_split(field, '"');
        if (parts.size() < 2) { err = "ERROR: GTF: gene_id without a quoted name"; return false; }
        gene = parts[1];
        return true;
    };
    auto add = [&](const std::string &gene, int &counter, int pos, int sign) {
        if (pos < 0 || pos >= (int)ref.size() || pos + 2 * sign < 0 || pos + 2 * sign >= (int)ref.size()) {
            err = "ERROR: GTF: a CDS of gene " + gene + " reaches past the FASTA (" + std::to_string(ref.size()) + " bases)";
            return false;
        }
        TrCodon c;
        c.orf_name = gene; c.codon_number = counter++; c.start_position = pos; c.sign = sign;
        for (int k = 0; k < 3; k++) c.nucleotides += sign > 0 ? ref[pos + k] : tr_complement(ref[pos - k]);
        c.initial = c.nucleotides;
        c.protein = tr_protein(c.nucleotides);
        codons.push_back(c);
        return true;
    };
    auto cds = [&](const std::string &gene, int &counter, int start, int stop, char strand) {
        if (strand == '+') {
            for (int pos = start - 1; pos < stop; pos += 3) if (!add(gene, counter, pos, 1)) return false;
        } else {
            for (int pos = stop - 1; pos > start; pos -= 3) if (!add(gene, counter, pos, -1)) return false;   // (0-based against 1-based, as :118)
        }
        return true;
    };
    const char *few = "ERROR: GTF: a data line with fewer than 9 columns";
    for (const std::string &outer : lines) {
        if (outer.empty() || outer[0] == '#') continue;
        const std::vector<std::string> fo = tr_split(outer, '\t');
        if (fo.size() <= 1) continue;
        if (fo.size() < 9) { err = few; return false; }
        if (fo[8].substr(0, 7) != "gene_id") { err = "ERROR: GTF file formatted incorrectly. Please see the wiki for details."; return false; }
        std::string gene;
        if (!gene_of(fo[8], gene)) return false;
        const char strand = fo[6].empty() ? '\0' : fo[6][0];
        if (fo[2] != "CDS") continue;
        if (std::find(done.begin(), done.end(), gene) != done.end()) continue;
        done.push_back(gene);
        int first_start = 0, first_stop = 0, counter = 0;
        if (!number(fo[3], first_start) || !number(fo[4], first_stop) || !cds(gene, counter, first_start, first_stop, strand)) return false;
        for (const std::string &inner : lines) {   // the gene's further CDS lines continue its codon numbers
            if (inner.empty() || inner[0] == '#') continue;
            const std::vector<std::string> fi = tr_split(inner, '\t');
            if (fi.size() < 9) { err = few; return false; }
            std::string gene_inner;
            if (!gene_of(fi[8], gene_inner)) return false;
            if (fi[2] != "CDS" || gene_inner != gene) continue;
            int start = 0, stop = 0;
            if (!number(fi[3], start) || !number(fi[4], stop)) return false;
            const char s2 = fi[6].empty() ? '\0' : fi[6][0];
            if (start != first_start || strand != s2)
                if (!cds(gene, counter, start, stop, s2)) return false;
        }
    }
    return true;
}

TrCodonMap tr_codon_map(std::vector<TrCodon> &codons) {
    TrCodonMap m;
    for (TrCodon &c : codons)
        for (int k = 0; k < 3; k++) m[c.start_position + c.sign * k].push_back(&c);
    return m;
}

// do_mutations, :498-588, taxodium_format == false
std::string tr_do_mutations(std::vector<uh::Mutation> &mutations, TrCodonMap &codon_map) {
    std::string prot_string, nuc_string, cchange_string;
    std::sort(mutations.begin(), mutations.end(), by_position);
    struct ByPos { bool operator()(const uh::Mutation *a, const uh::Mutation *b) const { return a->position < b->position; } };
    std::unordered_map<std::string, std::set<const uh::Mutation *, ByPos>> codon_to_nt_map;
    std::unordered_map<std::string, std::string> latest_codon_map, orig_codons;
    std::unordered_map<std::string, char> orig_proteins;
    std::vector<TrCodon *> affected_codons;
    for (const auto &m : mutations) {
        const char mutated_nuc = uh::nuc_char(m.mut_nuc), par_nuc = uh::nuc_char(m.par_nuc);
        const int pos = m.position - 1;
        const auto it = codon_map.find(pos);
        if (it == codon_map.end()) continue;   // not a coding mutation
        for (TrCodon *c : it->second) {
            const std::string codon_id = c->codon_id();
            c->mutate(pos, par_nuc);
            if (orig_proteins.find(codon_id) == orig_proteins.end()) orig_proteins.insert({codon_id, c->protein});
            if (std::find(affected_codons.begin(), affected_codons.end(), c) == affected_codons.end()) affected_codons.push_back(c);
            if (orig_codons.find(codon_id) == orig_codons.end()) orig_codons.insert({codon_id, c->nucleotides});
            c->mutate(pos, mutated_nuc);
            latest_codon_map[codon_id] = c->nucleotides;
            codon_to_nt_map[codon_id].insert(&m);
        }
    }
    for (TrCodon *c : affected_codons) {
        const std::string codon_id = c->codon_id();
        const std::vector<std::string> parts = tr_split(codon_id, ':');
        prot_string += parts[0] + ':' + orig_proteins.find(codon_id)->second + parts[1] + c->protein + ';';
        for (const uh::Mutation *m : codon_to_nt_map.find(codon_id)->second) nuc_string += m->str() + ",";
        if (!nuc_string.empty() && nuc_string.back() == ',') { nuc_string.resize(nuc_string.length() - 1); nuc_string += ';'; }
        cchange_string += orig_codons.find(codon_id)->second + ">" + latest_codon_map.find(codon_id)->second + ";";
    }
    for (std::string *s : {&nuc_string, &prot_string, &cchange_string})
        if (!s->empty() && s->back() == ';') s->resize(s->length() - 1);
    if (nuc_string.empty() || prot_string.empty() || cchange_string.empty()) return "";
    return prot_string + '\t' + nuc_string + '\t' + cchange_string;
}

void tr_undo_mutations(const std::vector<uh::Mutation> &mutations, TrCodonMap &codon_map) {   // :590-605
    for (const auto &m : mutations) {
        const int pos = m.position - 1;
        const auto it = codon_map.find(pos);
        if (it == codon_map.end()) continue;
        for (TrCodon *c : it->second) c->mutate(pos, uh::nuc_char(m.par_nuc));
    }
}

const char *kTranslateHeader = "node_id\taa_mutations\tnt_mutations\tcodon_changes\tleaves_sharing_mutations\n";

// get_leaves(node).size() of every node in one pass (a leaf counts itself): flat_index must be the position in `dfs`
std::vector<uint32_t> tr_leaf_counts(const std::vector<uh::Node *> &dfs) {
    std::vector<uint32_t> cnt(dfs.size(), 0);
    for (size_t i = dfs.size(); i-- > 0;) {
        if (dfs[i]->is_leaf()) cnt[i] = 1;
        if (dfs[i]->parent) cnt[dfs[i]->parent->flat_index] += cnt[i];
    }
    return cnt;
}

// translate_main's loop, :270-291.  (In a depth-first expansion the last common ancestor of a node and the node visited before it
// is the node's parent, so the undo chain runs up to there.)
void host_translate(uh::Tree &T, std::vector<TrCodon> &codons, std::ofstream &f) {
    for (TrCodon &c : codons) { c.nucleotides = c.initial; c.protein = tr_protein(c.initial); }
    TrCodonMap codon_map = tr_codon_map(codons);
    const std::vector<uh::Node *> dfs = T.dfs();
    for (size_t i = 0; i < dfs.size(); i++) { dfs[i]->flat_index = (uint32_t)i; dfs[i]->flat_epoch = 0; }
    const std::vector<uint32_t> leaves = tr_leaf_counts(dfs);
    f << kTranslateHeader;
    uh::Node *last_visited = nullptr;
    for (size_t i = 0; i < dfs.size(); i++) {
        uh::Node *node = dfs[i];
        if (last_visited != node->parent)
            for (uh::Node *trace = last_visited; trace != node->parent; trace = trace->parent) tr_undo_mutations(trace->mutations, codon_map);
        const std::string result = tr_do_mutations(node->mutations, codon_map);
        if (result != "") f << node->id << '\t' << result << '\t' << leaves[i] << '\n';
        last_visited = node;
    }
}

// The device path: the records of ugp_translate.hip, formatted to the same bytes.  False (with a line on stderr) when the library
// refuses the tree: the caller walks it on the host.
bool device_translate(uh::Tree &T, const std::vector<TrCodon> &codons, int device, std::ofstream &f) {
    const uh::TreeArrays A(T, uh::TreeArrays::kEntries);
    const std::vector<uh::Node *> &bfs = A.bfs;
    const std::vector<uint64_t> &mut_off = A.mut_off;
    const std::vector<const uh::Mutation *> &ent = A.ent;
    const uint64_t N = bfs.size();
    const ugp_tree_desc desc = A.desc();
    Mat H;
    H.create(A.bare(), device);
    int rc = ugp_translate_attach(H.h, &desc);
    if (rc == UGP_ERR_UNSUPPORTED) {
        fprintf(stderr, "The device does not take this tree (%s); walking it on the host.\n", ugp_last_error());
        return false;
    }
    if (rc != UGP_OK) lib_fail("ugp_translate_attach");
    std::vector<int32_t> slot_pos(3 * codons.size());
    std::vector<uint8_t> slot_init(3 * codons.size());
    for (size_t c = 0; c < codons.size(); c++)
        for (int k = 0; k < 3; k++) {
            slot_pos[3 * c + k] = codons[c].start_position + codons[c].sign * k + 1;
            slot_init[3 * c + k] = (uint8_t)codons[c].initial[k];
        }
    if (ugp_translate_codons(H.h, codons.size(), slot_pos.data(), slot_init.data()) != UGP_OK) lib_fail("ugp_translate_codons");
    uint64_t n = 0;
    ugp_tr_info info;
    rc = ugp_translate(H.h, nullptr, 0, &n, &info);
    if (rc == UGP_ERR_UNSUPPORTED) {
        fprintf(stderr, "The closed form does not hold for this tree: %llu inconsistent parent alleles", (unsigned long long)info.n_inconsistent);
        if (info.n_inconsistent) {
            const uint64_t j = std::upper_bound(mut_off.begin(), mut_off.end(), (uint64_t)info.first_inconsistent) - mut_off.begin() - 1;
            fprintf(stderr, " (first: %s on %s)", ent[info.first_inconsistent]->str().c_str(), bfs[j]->id.c_str());
        }
        fprintf(stderr, ", %llu nodes with a coding position twice", (unsigned long long)info.n_duplicate);
        if (info.n_duplicate) fprintf(stderr, " (first: %s)", bfs[info.first_duplicate]->id.c_str());
        fprintf(stderr, "; walking it on the host.\n");
        return false;
    }
    if (rc != UGP_OK) lib_fail("ugp_translate");
    std::vector<ugp_tr_record> recs(n);
    if (n && ugp_translate(H.h, recs.data(), n, &n, &info) != UGP_OK) lib_fail("ugp_translate");
    // leaves per node, by breadth-first index: children come after their parent
    std::vector<uint32_t> leaves(N, 0);
    for (uint64_t j = N; j-- > 0;) {
        if (bfs[j]->is_leaf()) leaves[j] = 1;
        if (bfs[j]->parent) leaves[bfs[j]->parent->flat_index] += leaves[j];
    }
    std::string out = kTranslateHeader, prot, nt, cch;
    for (size_t a = 0; a < recs.size();) {   // the records of one node follow each other
        size_t b = a;
        prot.clear(); nt.clear(); cch.clear();
        for (; b < recs.size() && recs[b].node == recs[a].node; b++) {
            const ugp_tr_record &r = recs[b];
            const TrCodon &c = codons[r.codon];
            const std::string before((const char *)r.before, 3), after((const char *)r.after, 3);
            if (b > a) { prot += ';'; nt += ';'; cch += ';'; }
            prot += c.orf_name + ':' + tr_protein(before) + std::to_string(c.codon_number + 1) + tr_protein(after);
            bool first = true;
            for (int k = c.sign > 0 ? 0 : 2; k >= 0 && k < 3; k += c.sign) {   // ascending position
                if (r.ent[k] == UINT32_MAX) continue;
                if (!first) nt += ',';
                nt += ent[r.ent[k]]->str();
                first = false;
            }
            cch += before + ">" + after;
        }
        out += bfs[recs[a].node]->id + '\t' + prot + '\t' + nt + '\t' + cch + '\t' + std::to_string(leaves[recs[a].node]) + '\n';
        if (out.size() > (1u << 20)) { f << out; out.clear(); }
        a = b;
    }
    f << out;
    return true;
}

int translate(int argc, char **argv) {   // summary_main's --translate branch (summary.cpp:698-713) and translate_main
    std::string mat, dir = "./", gtf, fasta, table;
    bool host = false;
    int device = 0;
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); translate_usage(stderr); return false; }
            dst = argv[++i];
            return true;
        };
        std::string tmp;
        bool ok = true;
        if (a == "-i" || a == "--input-mat") ok = val(mat);
        else if (a == "-d" || a == "--output-directory") ok = val(dir);
        else if (a == "-g" || a == "--input-gtf") ok = val(gtf);
        else if (a == "-f" || a == "--input-fasta") ok = val(fasta);
        else if (a == "-t" || a == "--translate") ok = val(table);
        else if (a == "-T" || a == "--threads") ok = val(tmp);
        else if (a == "--device") { ok = val(tmp); device = atoi(tmp.c_str()); }
        else if (a == "--host") host = true;
        else if (a == "-h" || a == "--help") { translate_usage(stdout); return 0; }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); translate_usage(stderr); return 1; }
        if (!ok) return 1;
    }
    if (mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); translate_usage(stderr); return 1; }
    if (table.empty()) { fprintf(stderr, "ERROR: the option '--translate' is required but missing\n"); translate_usage(stderr); return 1; }
    if (gtf.empty()) fprintf(stderr, "ERROR: You must specify a GTF file with -g\n");
    if (fasta.empty()) fprintf(stderr, "ERROR: You must specify a FASTA reference file with -f\n");
    if (gtf.empty() || fasta.empty()) return 1;
    struct stat sb;
    if (stat(dir.c_str(), &sb) != 0) {
        fprintf(stderr, "Creating output directory.\n\n");
        mkdir(dir.c_str(), 0777);
    }
    char *canon = realpath(dir.c_str(), nullptr);
    if (!canon) { fprintf(stderr, "ERROR: cannot resolve the output directory %s\n", dir.c_str()); return 1; }
    const std::string path = std::string(canon) + "/" + table;
    free(canon);
    fprintf(stderr, "Loading input MAT file %s.\n", mat.c_str());
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    T.uncondense_leaves();
    std::string reference;
    if (!tr_read_fasta(fasta, reference)) return 1;
    std::vector<TrCodon> codons;
    if (!tr_build_codons(gtf, reference, codons, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    fprintf(stderr, "Writing translation to output %s\n", path.c_str());
    const auto t0 = std::chrono::steady_clock::now();
    std::ofstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "ERROR: Could not open file for writing: %s!\n", path.c_str()); return 1; }
    if (host || !device_translate(T, codons, device, f)) host_translate(T, codons, f);
    f.close();
    if (!f) { fprintf(stderr, "ERROR: could not write %s\n", path.c_str()); return 1; }
    fprintf(stderr, "Completed in %ld msec \n\n", (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

// ---- haplotypes (summary --haplotype: summary.cpp:182-264) -----------------------------------------------------------

void haplotypes_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd haplotypes -i tree.pb -H out.tsv [-d dir] [-T n] [--device k] [--host]\n"
            "  -i, --input-mat          input mutation-annotated tree [REQUIRED]\n"
            "  -H, --haplotype          tsv of every distinct set of mutations off the reference that a sample carries, and its samples [REQUIRED]\n"
            "  -d, --output-directory   directory of the output file [./]\n"
            "  -T, --threads            accepted for compatibility (the table runs on the device)\n"
            "      --device             HIP device ordinal [0]\n"
            "      --host               the reference's serial walk on the host (slow; no device)\n");
}

typedef std::map<int, int8_t> HapSet;   // summary.cpp:184

void hap_line(std::string &out, const int32_t *pos, const uint8_t *nuc, size_t n, size_t count) {   // :252-261
    if (!n) out += "reference";   // (the reference calls pop_back() on the empty string first; this is what it evidently means)
    for (size_t k = 0; k < n; k++) {
        if (k) out += ',';
        out += std::to_string(pos[k]);
        out += uh::nuc_char((int8_t)nuc[k]);
    }
    out += '\t';
    out += std::to_string(count);
    out += '\n';
}

// --host: count_haplotypes (:182-218) and write_haplotype_table (:244-264), statement by statement.  The reference keeps the map of
// every internal node, by name, for the whole walk; here an internal node's map is freed when the walk has left its subtree (the
// maps of the current root path are all a later node can ask for).
void host_haplotypes(const uh::Tree &T, std::ofstream &f) {
    std::map<HapSet, size_t> hapcount;
    std::vector<std::pair<const uh::Node *, HapSet>> hapmap;   // the internal nodes of the current root path
    for (const uh::Node *s : T.dfs()) {
        HapSet mset;
        if (!s->is_root()) {
            while (hapmap.back().first != s->parent) hapmap.pop_back();
            mset = hapmap.back().second;
        }
        for (const auto &m : s->mutations) {
            if (m.mut_nuc == m.ref_nuc) {
                auto iter = mset.find(m.position);
                if (iter != mset.end()) mset.erase(iter);
            } else {
                mset[m.position] = m.mut_nuc;
            }
        }
        if (s->is_leaf()) hapcount[mset]++;
        else hapmap.emplace_back(s, std::move(mset));
    }
    f << "mutation_set\tsample_count\n";
    std::string out;
    std::vector<int32_t> pos;
    std::vector<uint8_t> nuc;
    for (const auto &hapc : hapcount) {
        pos.clear(); nuc.clear();
        for (const auto &m : hapc.first) { pos.push_back(m.first); nuc.push_back((uint8_t)m.second); }
        hap_line(out, pos.data(), nuc.data(), pos.size(), hapc.second);
        if (out.size() > (1u << 20)) { f << out; out.clear(); }
    }
    f << out;
}

// The device path: the groups and the sets of their first leaves from ugp_haplotypes.hip, ordered here as the std::map orders them.
// False (with a line on stderr) when the library refuses the tree: the caller walks it on the host.
bool device_haplotypes(uh::Tree &T, int device, std::ofstream &f) {
    const uh::TreeArrays A(T);
    const std::vector<uh::Node *> &bfs = A.bfs;
    const ugp_tree_desc desc = A.desc();
    Mat H;
    H.create(A.bare(), device);
    int rc = ugp_haplotypes_attach(H.h, &desc);
    if (rc == UGP_ERR_UNSUPPORTED) {
        fprintf(stderr, "The device does not take this tree (%s); walking it on the host.\n", ugp_last_error());
        return false;
    }
    if (rc != UGP_OK) lib_fail("ugp_haplotypes_attach");
    // USHER_AMD_HAPLOTYPE_HASH_BITS (test switch): only that many bits of the fingerprint group the leaves, so that the exact
    // comparison finds collisions and the table is refused.  (No file reaches the other refusal: the loader's add_mutation merges
    // two entries at one position of a node, as the reference's does.)
    uint32_t hash_bits = 128;
    if (const char *e = getenv("USHER_AMD_HAPLOTYPE_HASH_BITS")) hash_bits = (uint32_t)std::max(0, std::min(128, atoi(e)));
    uint64_t n = 0;
    ugp_hp_info info;
    rc = ugp_haplotype_groups_hashed(H.h, nullptr, 0, &n, &info, hash_bits);
    if (rc == UGP_ERR_UNSUPPORTED) {
        fprintf(stderr, "The closed form does not hold for this tree: %llu nodes with a position twice", (unsigned long long)info.n_duplicate);
        if (info.n_duplicate) fprintf(stderr, " (first: %s)", bfs[info.first_duplicate]->id.c_str());
        fprintf(stderr, ", %llu fingerprint collisions among %llu samples; walking it on the host.\n", (unsigned long long)info.n_collisions,
                (unsigned long long)info.n_leaves);
        return false;
    }
    if (rc != UGP_OK) lib_fail("ugp_haplotype_groups");
    std::vector<ugp_hp_group> groups(n);
    if (n && ugp_haplotype_groups_hashed(H.h, groups.data(), n, &n, &info, hash_bits) != UGP_OK) lib_fail("ugp_haplotype_groups");
    // the sets of the groups' first leaves (the library runs them in launch windows)
    std::vector<uint32_t> reps(n);
    for (uint64_t g = 0; g < n; g++) reps[g] = groups[g].leaf;
    std::vector<uint64_t> off(n + 1, 0);
    uint64_t total = 0;
    if (ugp_haplotype_sets(H.h, reps.data(), n, off.data(), nullptr, nullptr, 0, &total) != UGP_OK) lib_fail("ugp_haplotype_sets");
    std::vector<int32_t> spos(total);
    std::vector<uint8_t> snuc(total);
    if (total && ugp_haplotype_sets(H.h, reps.data(), n, off.data(), spos.data(), snuc.data(), total, &total) != UGP_OK) lib_fail("ugp_haplotype_sets");
    // std::map<std::map<int,int8_t>,size_t> order: lexicographic over the (position, allele) pairs, a proper prefix first
    std::vector<uint32_t> order(n);
    for (uint64_t g = 0; g < n; g++) order[g] = (uint32_t)g;
    auto before = [&](uint32_t x, uint32_t y) {
        const uint64_t nx = off[x + 1] - off[x], ny = off[y + 1] - off[y];
        const int32_t *px = spos.data() + off[x], *py = spos.data() + off[y];
        const uint8_t *cx = snuc.data() + off[x], *cy = snuc.data() + off[y];
        for (uint64_t k = 0; k < nx && k < ny; k++) {
            if (px[k] != py[k]) return px[k] < py[k];
            if (cx[k] != cy[k]) return (int8_t)cx[k] < (int8_t)cy[k];
        }
        return nx < ny;
    };
    // sorted pieces on the host threads, then merged pair by pair
    const uint64_t grain = getenv("USHER_AMD_GRAIN") ? (uint64_t)std::max(1, atoi(getenv("USHER_AMD_GRAIN"))) : (1u << 16);   // as par.hpp reads it
    const uint64_t pieces = std::max<uint64_t>(1, std::min<uint64_t>(uh::host_threads(), n / grain));
    std::vector<uint64_t> cut;
    for (uint64_t i = 0; i <= pieces; i++) cut.push_back(n * i / pieces);
    uh::parallel_for(pieces, [&](uint64_t b, uint64_t e, unsigned) {
        for (uint64_t k = b; k < e; k++) std::sort(order.begin() + cut[k], order.begin() + cut[k + 1], before);
    }, 1);
    while (cut.size() > 2) {
        const size_t pairs = (cut.size() - 1) / 2;
        uh::parallel_for(pairs, [&](uint64_t b, uint64_t e, unsigned) {
            for (uint64_t k = b; k < e; k++) std::inplace_merge(order.begin() + cut[2 * k], order.begin() + cut[2 * k + 1], order.begin() + cut[2 * k + 2], before);
        }, 1);
        std::vector<uint64_t> next;
        for (size_t k = 0; k < cut.size(); k += 2) next.push_back(cut[k]);
        if ((cut.size() - 1) % 2) next.push_back(cut.back());
        cut.swap(next);
    }
    std::string out = "mutation_set\tsample_count\n";
    for (uint32_t g : order) {
        hap_line(out, spos.data() + off[g], snuc.data() + off[g], off[g + 1] - off[g], groups[g].count);
        if (out.size() > (1u << 20)) { f << out; out.clear(); }
    }
    f << out;
    return true;
}

int haplotypes(int argc, char **argv) {   // summary_main's --haplotype branch (summary.cpp:725-728)
    std::string mat, dir = "./", table;
    bool host = false;
    int device = 0;
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); haplotypes_usage(stderr); return false; }
            dst = argv[++i];
            return true;
        };
        std::string tmp;
        bool ok = true;
        if (a == "-i" || a == "--input-mat") ok = val(mat);
        else if (a == "-d" || a == "--output-directory") ok = val(dir);
        else if (a == "-H" || a == "--haplotype") ok = val(table);
        else if (a == "-T" || a == "--threads") ok = val(tmp);
        else if (a == "--device") { ok = val(tmp); device = atoi(tmp.c_str()); }
        else if (a == "--host") host = true;
        else if (a == "-h" || a == "--help") { haplotypes_usage(stdout); return 0; }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); haplotypes_usage(stderr); return 1; }
        if (!ok) return 1;
    }
    if (mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); haplotypes_usage(stderr); return 1; }
    if (table.empty()) { fprintf(stderr, "ERROR: the option '--haplotype' is required but missing\n"); haplotypes_usage(stderr); return 1; }
    struct stat sb;
    if (stat(dir.c_str(), &sb) != 0) {
        fprintf(stderr, "Creating output directory.\n\n");
        mkdir(dir.c_str(), 0777);
    }
    char *canon = realpath(dir.c_str(), nullptr);
    if (!canon) { fprintf(stderr, "ERROR: cannot resolve the output directory %s\n", dir.c_str()); return 1; }
    const std::string path = std::string(canon) + "/" + table;
    free(canon);
    fprintf(stderr, "Loading input MAT file %s.\n", mat.c_str());
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    T.uncondense_leaves();
    fprintf(stderr, "Writing haplotype frequencies to output %s\n", path.c_str());
    const auto t0 = std::chrono::steady_clock::now();
    std::ofstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "ERROR: Could not open file for writing: %s!\n", path.c_str()); return 1; }
    if (host || !device_haplotypes(T, device, f)) host_haplotypes(T, f);
    f.close();
    if (!f) { fprintf(stderr, "ERROR: could not write %s\n", path.c_str()); return 1; }
    fprintf(stderr, "Completed in %ld msec \n\n", (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

// ---- relatives (extract --closest-relatives / --within-distance: extract.cpp:768-823, select.cpp:577-714) -------------

void relatives_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd relatives -i tree.pb [-s samples.txt] [-V closest.tsv [-q]] [--within-distance within.tsv\n"
            "       [--distance-threshold n]] [-d dir] [-T n] [--device k] [--host]\n"
            "  -i, --input-mat          input mutation-annotated tree (.pb / .pb.gz) [REQUIRED]\n"
            "  -s, --samples            text file of sample ids, one per line [every leaf of the tree]\n"
            "  -V, --closest-relatives  tsv of each sample's closest relative(s) and their distance\n"
            "  -q, --break-ties         one closest relative per sample: the smallest name\n"
            "      --within-distance    tsv of each sample's relatives within the distance threshold\n"
            "      --distance-threshold the threshold of --within-distance [0]\n"
            "  -d, --output-directory   directory of the output files [./]\n"
            "  -T, --threads            accepted for compatibility (the searches run on the device)\n"
            "      --device             HIP device ordinal [0]\n"
            "      --host               the reference's serial walk on the host (slow; no device)\n");
}

// closest_samples_dfs, select.cpp:577-594
void rel_dfs(const uh::Node *node, size_t path_length, size_t max_path_length, std::vector<std::pair<const uh::Node *, size_t>> &leaves, bool fixed_k) {
    if (path_length > max_path_length) return;
    for (const uh::Node *child : node->children) {
        if (child->is_leaf()) {
            if (fixed_k && path_length + child->mutations.size() <= max_path_length) leaves.push_back(std::make_pair(child, path_length + child->mutations.size()));
            else if (!fixed_k) leaves.push_back(std::make_pair(child, path_length + child->mutations.size()));
        } else {
            rel_dfs(child, path_length + child->mutations.size(), max_path_length, leaves, fixed_k);
        }
    }
}

// get_closest_samples, select.cpp:596-714, statement by statement (identifiers are unique: nodes are compared by address).
std::pair<std::vector<const uh::Node *>, size_t> host_closest_samples(const uh::Node *target, bool fixed_k, size_t k) {
    std::pair<std::vector<const uh::Node *>, size_t> closest_samples;
    closest_samples.second = 0;
    const uh::Node *target_parent = target->parent;
    const uh::Node *curr_target = target;
    const uh::Node *parent = target->parent;
    size_t min_dist = std::numeric_limits<size_t>::max();
    size_t dist_to_orig_parent = 0;
    bool go_up = true;
    while (go_up && parent) {
        const size_t parent_branch_length = parent->mutations.size() + dist_to_orig_parent;
        std::vector<std::pair<const uh::Node *, size_t>> children_and_distances, children_and_distances_fixed_k;
        size_t min_of_sibling_leaves = std::numeric_limits<size_t>::max();
        for (const uh::Node *child : parent->children) {
            if (child->is_leaf()) {
                if (child == curr_target) continue;
                const size_t child_branch_length = child->mutations.size();
                if (child_branch_length < min_of_sibling_leaves) min_of_sibling_leaves = child_branch_length;
            }
        }
        for (const uh::Node *child : parent->children) {
            if (child == curr_target) continue;
            if (child == target_parent) continue;
            const size_t dist_so_far = dist_to_orig_parent + target->mutations.size() + child->mutations.size();
            if (!child->is_leaf()) {
                if (fixed_k) {
                    rel_dfs(child, dist_so_far, k, children_and_distances_fixed_k, true);
                } else {
                    size_t max_path;
                    if (min_of_sibling_leaves == std::numeric_limits<size_t>::max()) max_path = min_of_sibling_leaves;
                    else max_path = min_of_sibling_leaves + dist_so_far;
                    rel_dfs(child, dist_so_far, max_path, children_and_distances, false);
                }
            } else {
                if (fixed_k && dist_so_far <= k) children_and_distances_fixed_k.push_back(std::make_pair(child, dist_so_far));
                else if (!fixed_k) children_and_distances.push_back(std::make_pair(child, dist_so_far));
            }
        }
        if (fixed_k) {
            if (parent_branch_length > k) go_up = false;
            for (const auto &child_and_dist : children_and_distances_fixed_k) {
                closest_samples.first.push_back(child_and_dist.first);
                closest_samples.second = 0;
            }
        } else {
            for (const auto &child_and_dist : children_and_distances) {
                const size_t child_branch_length = child_and_dist.second;
                if (child_branch_length < parent_branch_length) go_up = false;
                if (child_branch_length < min_dist) {
                    min_dist = child_branch_length;
                    closest_samples.first.clear();
                    closest_samples.first.push_back(child_and_dist.first);
                    closest_samples.second = min_dist;
                } else if (child_branch_length == min_dist) {
                    closest_samples.first.push_back(child_and_dist.first);
                }
            }
        }
        curr_target = parent;
        parent = curr_target->parent;
        dist_to_orig_parent = parent_branch_length;
    }
    return closest_samples;
}

// One line of the closest-relatives file (extract.cpp:782-803); nothing for a sample without relatives.
void rel_closest_line(std::string &out, const std::string &sample, const std::vector<const uh::Node *> &rel, const uh::Node *smallest, size_t dist,
                      bool break_ties) {
    if (rel.empty() && !smallest) return;
    out += sample; out += '\t';
    if (break_ties) out += smallest->id;
    else for (size_t i = 0; i < rel.size(); i++) { if (i) out += ','; out += rel[i]->id; }
    out += '\t'; out += std::to_string(dist); out += '\n';
}

// One line of the within-distance file (:811-821): the substr drops the tab of a sample without relatives.
void rel_within_line(std::string &out, const std::string &sample, const std::vector<const uh::Node *> &rel) {
    out += sample;
    for (size_t i = 0; i < rel.size(); i++) { out += i ? ',' : '\t'; out += rel[i]->id; }
    out += '\n';
}

struct RelativesJob {
    std::vector<std::string> names;          // the samples, in output order
    std::vector<const uh::Node *> nodes;
    std::string closest_path, within_path;
    bool break_ties = false;
    size_t threshold = 0;
};

bool rel_flush(std::ofstream &f, std::string &out, bool force) {
    if (force || out.size() > (1u << 20)) { f << out; out.clear(); }
    return (bool)f;
}

int host_relatives(const RelativesJob &J) {
    std::string out;
    if (!J.closest_path.empty()) {
        std::ofstream f(J.closest_path, std::ios::binary);
        for (size_t i = 0; i < J.nodes.size(); i++) {
            const auto r = host_closest_samples(J.nodes[i], false, 0);
            const uh::Node *smallest = nullptr;
            if (J.break_ties)
                for (const uh::Node *n : r.first) if (!smallest || n->id < smallest->id) smallest = n;
            rel_closest_line(out, J.names[i], r.first, smallest, r.second, J.break_ties);
            rel_flush(f, out, false);
        }
        if (!rel_flush(f, out, true)) { fprintf(stderr, "ERROR: could not write %s\n", J.closest_path.c_str()); return 1; }
    }
    if (!J.within_path.empty()) {
        std::ofstream f(J.within_path, std::ios::binary);
        for (size_t i = 0; i < J.nodes.size(); i++) {
            rel_within_line(out, J.names[i], host_closest_samples(J.nodes[i], true, J.threshold).first);
            rel_flush(f, out, false);
        }
        if (!rel_flush(f, out, true)) { fprintf(stderr, "ERROR: could not write %s\n", J.within_path.c_str()); return 1; }
    }
    return 0;
}

// The device path: ugp_relatives_closest / ugp_relatives_within in batches of samples, formatted to the same bytes.
int device_relatives(uh::Tree &T, const RelativesJob &J, int device) {
    const uh::TreeArrays A(T);
    const std::vector<uh::Node *> &bfs = A.bfs;
    // the handle carries the topology only: the relatives tables count entries, whatever they hold
    const ugp_tree_desc desc = A.desc();
    Mat H;
    H.create(A.bare(), device);
    std::vector<uint32_t> rank;
    if (J.break_ties && !J.closest_path.empty()) rank = A.name_rank();
    if (ugp_relatives_attach(H.h, &desc, rank.empty() ? nullptr : rank.data()) != UGP_OK) lib_fail("ugp_relatives_attach");
    const size_t n = J.nodes.size(), per = size_t(1) << 16;   // samples per call: the lists of one call are held at once
    std::vector<uint32_t> qn(n), lists;
    for (size_t i = 0; i < n; i++) qn[i] = J.nodes[i]->flat_index;
    std::vector<ugp_rel_info> info(per);
    std::vector<uint64_t> off(per + 1);
    std::vector<const uh::Node *> rel;
    std::string out;
    for (int within = 0; within < 2; within++) {
        const std::string &path = within ? J.within_path : J.closest_path;
        if (path.empty()) continue;
        const bool want_lists = within || !J.break_ties;
        std::ofstream f(path, std::ios::binary);
        for (size_t i0 = 0; i0 < n; i0 += per) {
            const size_t m = std::min(per, n - i0);
            uint64_t total = 0;
            for (int attempt = 0; attempt < 2; attempt++) {   // the second call has room for the total the first reported
                const int rc = within ? ugp_relatives_within(H.h, m, qn.data() + i0, (uint32_t)std::min<size_t>(J.threshold, UINT32_MAX), info.data(),
                                                             want_lists ? off.data() : nullptr, lists.data(), lists.size(), &total)
                                      : ugp_relatives_closest(H.h, m, qn.data() + i0, info.data(), want_lists ? off.data() : nullptr, lists.data(),
                                                              lists.size(), &total);
                if (rc != UGP_OK) lib_fail(within ? "ugp_relatives_within" : "ugp_relatives_closest");
                if (!want_lists || total <= lists.size()) break;
                lists.resize(total);
            }
            for (size_t i = 0; i < m; i++) {
                rel.clear();
                if (want_lists) for (uint64_t x = off[i]; x < off[i + 1]; x++) rel.push_back(bfs[lists[x]]);
                if (within) rel_within_line(out, J.names[i0 + i], rel);
                else rel_closest_line(out, J.names[i0 + i], rel, info[i].count && J.break_ties ? bfs[info[i].best] : nullptr, info[i].dist, J.break_ties);
                rel_flush(f, out, false);
            }
        }
        if (!rel_flush(f, out, true)) { fprintf(stderr, "ERROR: could not write %s\n", path.c_str()); return 1; }
    }
    return 0;
}

int relatives(int argc, char **argv) {
    std::string mat, fsamples, fclosest, fwithin, dir = "./";
    bool host = false, break_ties = false;
    long threshold = 0;
    int device = 0;
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); relatives_usage(stderr); return false; }
            dst = argv[++i];
            return true;
        };
        std::string tmp;
        bool ok = true;
        if (a == "-i" || a == "--input-mat") ok = val(mat);
        else if (a == "-s" || a == "--samples") ok = val(fsamples);
        else if (a == "-V" || a == "--closest-relatives") ok = val(fclosest);
        else if (a == "-q" || a == "--break-ties") break_ties = true;
        else if (a == "--within-distance") ok = val(fwithin);
        else if (a == "--distance-threshold") {
            ok = val(tmp);
            char *end = nullptr;
            threshold = strtol(tmp.c_str(), &end, 10);
            if (ok && (tmp.empty() || *end || threshold < 0)) { fprintf(stderr, "ERROR: bad value %s for %s\n", tmp.c_str(), a.c_str()); relatives_usage(stderr); return 1; }
        }
        else if (a == "-d" || a == "--output-directory") ok = val(dir);
        else if (a == "-T" || a == "--threads") ok = val(tmp);
        else if (a == "--device") { ok = val(tmp); device = atoi(tmp.c_str()); }
        else if (a == "--host") host = true;
        else if (a == "-h" || a == "--help") { relatives_usage(stdout); return 0; }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); relatives_usage(stderr); return 1; }
        if (!ok) return 1;
    }
    if (mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); relatives_usage(stderr); return 1; }
    if (fclosest.empty() && fwithin.empty()) { fprintf(stderr, "ERROR: No output files requested!\n"); return 1; }
    struct stat sb;
    if (stat(dir.c_str(), &sb) != 0) {
        fprintf(stderr, "Creating output directory.\n\n");
        mkdir(dir.c_str(), 0777);
    }
    char *canon = realpath(dir.c_str(), nullptr);
    if (!canon) { fprintf(stderr, "ERROR: cannot resolve the output directory %s\n", dir.c_str()); return 1; }
    const std::string prefix = std::string(canon) + "/";
    free(canon);
    fprintf(stderr, "Loading input MAT file %s.\n", mat.c_str());
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    T.uncondense_leaves();
    RelativesJob J;
    if (!fsamples.empty()) {
        J.names = read_sample_names(fsamples);
        if (J.names.empty()) { fprintf(stderr, "ERROR: Sample file is empty or unparseable!"); return 1; }
    } else {
        J.names = leaf_ids(T);
    }
    for (const std::string &s : J.names) J.nodes.push_back(must_get(T, s));   // (the reference dereferences the null pointer)
    if (!fclosest.empty()) J.closest_path = prefix + fclosest;
    if (!fwithin.empty()) J.within_path = prefix + fwithin;
    J.break_ties = break_ties;
    J.threshold = (size_t)threshold;
    if (!fclosest.empty()) {
        fprintf(stderr, "Per-sample closest relative(s) requested. Computing...\n");
        if (break_ties) fprintf(stderr, "Storing one closest relative per sample.\n");
    }
    if (!fwithin.empty()) fprintf(stderr, "Computing per-sample relatives within %ld mutations...\n", threshold);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = host ? host_relatives(J) : device_relatives(T, J, device);
    if (rc) return rc;
    fprintf(stderr, "Relatives of %zu samples written in %.3f msec.\n\n", J.nodes.size(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

// ---- mask (mask.cpp) ---------------------------------------------------------------------------------------------

void mask_usage(FILE *f) {
    fprintf(f,
            "Usage: matutils-amd mask -i tree.pb -o out.pb [-s samples.txt] [-m mutations.tsv] [-r rename.tsv] [-c] [-T n] [--device k] [--host]\n"
            "  -i, --input-mat          input mutation-annotated tree [REQUIRED]\n"
            "  -o, --output-mat         output mutation-annotated tree [REQUIRED]\n"
            "  -s, --restricted-samples sample names, one per line: mutations private to them are masked\n"
            "  -m, --mask-mutations     lines of mutation[<TAB>node[<TAB>excluded;excluded]] (commas when the name contains .csv): the\n"
            "                           mutation is removed below the node (the root when none is given), not below the excluded nodes\n"
            "  -r, --rename-samples     two-column tsv: old name, new name\n"
            "  -c, --condense-tree      collapse the tree and condense identical leaves before it is written\n"
            "  -T, --threads            accepted for compatibility\n"
            "      --device             HIP device ordinal [0]\n"
            "      --host               run -s and -m as the reference's walks on the host (slow)\n"
            "  The steps run in the reference's order: -s, -m, -r, -c.  'Masking mutation' lines come in depth-first order.\n"
            "  (-S / --simplify, -M / --move-nodes, -D / --max-snp-distance and -f / --maple-file are not supported)\n");
}

struct MaskLine {
    uh::Mutation mut;
    uh::Node *node = nullptr;
    std::set<std::string> exclude;
};

// restrictSamples' three loops (:820-904) statement by statement.  `marks` receives (node, entry) of every entry to mask; the
// leaves below an ancestor are enumerated breadth-first as get_leaves_ids does, up to the first one that is not named.
// (F: the tree with its depth-first side, uh::TreeArrays::kDepthFirst.)
size_t host_restricted(const uh::Tree &T, const uh::TreeArrays &F, const std::vector<std::string> &names,
                       std::vector<std::pair<uh::Node *, size_t>> &marks) {
    std::unordered_set<std::string> restricted(names.begin(), names.end());
    std::unordered_set<uh::Node *> roots;
    std::unordered_map<std::string, bool> visited;
    for (const auto &s : restricted) visited[s] = false;
    std::vector<uh::Node *> queue;
    for (uh::Node *cn : F.bfs) {
        if (!restricted.count(cn->id) || visited[cn->id]) continue;
        uh::Node *curr = cn;
        for (uh::Node *n : T.rsearch(cn, false)) {
            bool found_unrestricted = false;
            queue.assign(1, n);
            for (size_t h = 0; h < queue.size() && !found_unrestricted; h++) {
                if (queue[h]->is_leaf()) found_unrestricted = !restricted.count(queue[h]->id);
                else queue.insert(queue.end(), queue[h]->children.begin(), queue[h]->children.end());
            }
            if (!found_unrestricted) {
                for (uh::Node *l : queue) if (l->is_leaf()) visited[l->id] = true;
                curr = n;
                break;
            }
        }
        roots.insert(curr);
    }
    std::unordered_map<std::string, int> counts;
    for (uh::Node *n : F.dfs)
        for (const auto &m : n->mutations) if (!m.masked()) counts[m.str()] += 1;
    std::vector<uh::Node *> ordered(roots.begin(), roots.end());   // depth-first order, where the reference iterates the set
    std::sort(ordered.begin(), ordered.end(), [&](uh::Node *a, uh::Node *b) { return F.dpos[a->flat_index] < F.dpos[b->flat_index]; });
    for (uh::Node *r : ordered)
        for (uh::Node *n : T.dfs(r))
            for (const auto &m : n->mutations) if (!m.masked()) counts[m.str()] -= 1;
    std::unordered_set<const uh::Mutation *> done;   // an entry below two nested roots is masked on the first visit
    for (uh::Node *r : ordered)
        for (uh::Node *n : T.dfs(r))
            for (size_t k = 0; k < n->mutations.size(); k++) {
                const auto &m = n->mutations[k];
                if (m.masked() || counts[m.str()] != 0 || !done.insert(&m).second) continue;
                marks.emplace_back(n, k);
            }
    return roots.size();
}

bool mask_match(const uh::Mutation &target, const uh::Mutation &query) {   // match_mutations, :703-721
    if (target.position != query.position) return false;
    if (target.ref_nuc != 0b1111 && target.par_nuc != query.par_nuc) return false;
    if (target.mut_nuc != 0b1111 && target.mut_nuc != query.mut_nuc) return false;
    return true;
}

size_t host_mask_on_branch(uh::Node *node, const MaskLine &L) {   // mask_mutation_on_branch, :723-744
    size_t masked = 0;
    auto &ms = node->mutations;
    for (size_t k = 0; k < ms.size();)
        if (mask_match(L.mut, ms[k])) { masked++; ms.erase(ms.begin() + k); } else k++;
    for (uh::Node *child : node->children) {
        if (!L.exclude.count(child->id)) masked += host_mask_on_branch(child, L);
        else fprintf(stderr, "Excluding %s for position %d\n", child->id.c_str(), L.mut.position);
    }
    return masked;
}

int mask(int argc, char **argv) {   // mask_main, :68-159
    std::string mat, out, samples, mutations, rename;
    bool recondense = false, host = false;
    int device = 0;
    for (int i = 0; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](std::string &dst) -> bool {
            if (i + 1 >= argc) { fprintf(stderr, "ERROR: %s needs a value\n", a.c_str()); mask_usage(stderr); return false; }
            dst = argv[++i];
            return true;
        };
        std::string tmp;
        bool ok = true;
        if (a == "-i" || a == "--input-mat") ok = val(mat);
        else if (a == "-o" || a == "--output-mat") ok = val(out);
        else if (a == "-s" || a == "--restricted-samples") ok = val(samples);
        else if (a == "-m" || a == "--mask-mutations") ok = val(mutations);
        else if (a == "-r" || a == "--rename-samples") ok = val(rename);
        else if (a == "-c" || a == "--condense-tree") recondense = true;
        else if (a == "-T" || a == "--threads") ok = val(tmp);
        else if (a == "--device") { ok = val(tmp); device = atoi(tmp.c_str()); }
        else if (a == "--host") host = true;
        else if (a == "-h" || a == "--help") { mask_usage(stdout); return 0; }
        else if (a == "-S" || a == "--simplify" || a == "-M" || a == "--move-nodes" || a == "-D" || a == "--max-snp-distance" || a == "-f" ||
                 a == "--maple-file") {
            fprintf(stderr, "ERROR: %s is not supported by matutils-amd mask (use the reference matUtils)\n", a.c_str());
            return 1;
        }
        else { fprintf(stderr, "ERROR: unknown option %s\n", a.c_str()); mask_usage(stderr); return 1; }
        if (!ok) return 1;
    }
    if (mat.empty()) { fprintf(stderr, "ERROR: the option '--input-mat' is required but missing\n"); mask_usage(stderr); return 1; }
    if (out.empty()) { fprintf(stderr, "ERROR: the option '--output-mat' is required but missing\n"); mask_usage(stderr); return 1; }
    auto clock = [] { return std::chrono::steady_clock::now(); };
    auto done = [&](std::chrono::steady_clock::time_point t0, const char *end) {
        fprintf(stderr, "Completed in %ld msec %s", (long)std::chrono::duration_cast<std::chrono::milliseconds>(clock() - t0).count(), end);
    };
    fprintf(stderr, "Loading input MAT file %s.\n", mat.c_str());
    auto t0 = clock();
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(mat, T, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    done(t0, "\n\n");
    if (!T.condensed_nodes.empty()) {
        fprintf(stderr, "Uncondensing condensed nodes...\n");
        t0 = clock();
        T.uncondense_leaves();
        done(t0, "\n\n");
    }
    uh::TreeArrays F;   // the tree for both paths: the breadth-first numbering and the depth-first ranges
    Mat D;
    if (!samples.empty() || !mutations.empty()) {
        F = uh::TreeArrays(T, uh::TreeArrays::kDepthFirst);
        if (!host) {
            t0 = clock();
            // the handle takes the bare topology, the mask tables the mutations as they are stored (masked, repeated positions)
            const ugp_tree_desc desc = F.desc();
            D.create(F.bare(), device);
            if (ugp_mask_attach(D, &desc) != UGP_OK) lib_fail("ugp_mask_attach");
            fprintf(stderr, "Tree on device %d in %ld msec\n", device, (long)std::chrono::duration_cast<std::chrono::milliseconds>(clock() - t0).count());
        }
    }
    std::vector<uint8_t> entry_masked;   // per entry of the tree arrays: -s masked it
    if (!samples.empty()) {   // restrictSamples, :802-905
        fprintf(stderr, "Performing masking...\n");
        std::ifstream in(samples);
        if (!in) { fprintf(stderr, "ERROR: Could not open the restricted samples file: %s!\n", samples.c_str()); return 1; }
        std::vector<std::string> names;
        std::vector<uint32_t> named;
        std::string sample;
        bool leaves_only = true;
        while (std::getline(in, sample)) {
            fprintf(stderr, "Checking for sample %s\n", sample.c_str());
            const uh::Node *n = T.get_node(sample);
            if (!n) { fprintf(stderr, "ERROR: Sample missing in input MAT!\n\n"); return 1; }
            leaves_only = leaves_only && n->is_leaf();
            named.push_back(n->flat_index);
            names.push_back(sample);
        }
        if (names.empty()) { fprintf(stderr, "ERROR: the restricted samples file %s names no sample\n", samples.c_str()); return 1; }
        t0 = clock();
        std::vector<std::pair<uh::Node *, size_t>> marks;
        size_t n_roots = 0;
        bool on_device = !host;
        if (on_device) {
            if (!leaves_only) fprintf(stderr, "A restricted node is internal: restricted roots can nest, walking on the host.\n");
            entry_masked.assign(std::max<size_t>(F.mut_off.back(), 1), 0);
            uint64_t nr = 0, nm = 0;
            const int rc = leaves_only ? ugp_mask_restricted(D.h, named.size(), named.data(), entry_masked.data(), nullptr, 0, &nr, &nm) : UGP_ERR_UNSUPPORTED;
            if (rc == UGP_ERR_UNSUPPORTED) {
                if (leaves_only) fprintf(stderr, "%s\n", ugp_last_error());
                on_device = false;
            } else if (rc != UGP_OK) lib_fail("ugp_mask_restricted");
            else {
                n_roots = nr;
                for (uh::Node *n : F.dfs) {
                    const uint64_t e0 = F.mut_off[n->flat_index];
                    for (size_t k = 0; k < n->mutations.size(); k++) if (entry_masked[e0 + k]) marks.emplace_back(n, k);
                }
            }
        }
        if (!on_device) {
            n_roots = host_restricted(T, F, names, marks);
            if (!host) {
                std::fill(entry_masked.begin(), entry_masked.end(), 0);
                for (const auto &mk : marks) entry_masked[F.mut_off[mk.first->flat_index] + mk.second] = 1;
            }
        }
        fprintf(stderr, "Restricted roots size: %zu\n\n", n_roots);
        for (const auto &mk : marks) {
            uh::Mutation &m = mk.first->mutations[mk.second];
            fprintf(stderr, "Masking mutation %s at node %s\n", m.str().c_str(), mk.first->id.c_str());
            m.position = -1;
            m.ref_nuc = m.par_nuc = m.mut_nuc = 0;
        }
        fprintf(stderr, "Restricted samples %s in %ld msec\n", on_device ? "on the device" : "on the host",
                (long)std::chrono::duration_cast<std::chrono::milliseconds>(clock() - t0).count());
    }
    if (!mutations.empty()) {   // restrictMutationsLocally, :746-800
        fprintf(stderr, "Masking mutations...\n");
        std::ifstream in(mutations);
        if (!in) { fprintf(stderr, "ERROR: Could not open the file: %s!\n", mutations.c_str()); return 1; }
        const char delim = mutations.find(".csv") != std::string::npos ? ',' : '\t';
        std::vector<MaskLine> lines;
        std::string line;
        while (std::getline(in, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            std::vector<std::string> words;
            split_delim(line, delim, words);
            if (words.empty()) { fprintf(stderr, "ERROR: Empty line in the mutations file: %s!\n", mutations.c_str()); return 1; }
            MaskLine L;
            if (!mutation_from_string(words[0], L.mut)) return 1;
            const std::string target = words.size() == 1 ? T.root->id : words[1];
            if (words.size() > 2) {
                std::vector<std::string> ids;
                split_delim(words[2], ';', ids);
                L.exclude.insert(ids.begin(), ids.end());
            }
            L.node = T.get_node(target);
            if (!L.node) {
                fprintf(stderr, "ERROR: Internal node %s requested for masking does not exist in the tree. Exiting\n", target.c_str());
                return 1;
            }
            lines.push_back(std::move(L));
        }
        t0 = clock();
        size_t total_masked = 0;
        if (host) {
            for (const auto &L : lines) total_masked += host_mask_on_branch(L.node, L);
        } else {
            const size_t nl = lines.size(), M = F.mut_off.back();
            std::vector<int32_t> lpos(nl);
            std::vector<uint8_t> lpar(nl), lnuc(nl);
            std::vector<uint32_t> lnode(nl), excl, first(std::max<size_t>(M, 1), UINT32_MAX);
            std::vector<uint64_t> excl_off(nl + 1, 0), counts(std::max<size_t>(nl, 1), 0);
            std::vector<uint32_t> met;
            for (size_t l = 0; l < nl; l++) {
                const MaskLine &L = lines[l];
                lpos[l] = L.mut.position;
                lpar[l] = L.mut.ref_nuc == 0b1111 ? 15 : (uint8_t)L.mut.par_nuc;
                lnuc[l] = (uint8_t)L.mut.mut_nuc;
                lnode[l] = L.node->flat_index;
                // the excluded nodes the walk would meet: strict descendants of the target, none below another of them
                const uint32_t tlo = F.dpos[lnode[l]], thi = F.dend[lnode[l]];
                met.clear();
                for (const auto &id : L.exclude) {
                    const uh::Node *x = T.get_node(id);
                    if (!x) continue;
                    excl.push_back(x->flat_index);
                    if (F.dpos[x->flat_index] > tlo && F.dpos[x->flat_index] < thi) met.push_back(x->flat_index);
                }
                excl_off[l + 1] = excl.size();
                std::sort(met.begin(), met.end(), [&](uint32_t a, uint32_t b) { return F.dpos[a] < F.dpos[b]; });
                uint32_t covered = 0;   // the end of the last printed node's range
                for (uint32_t x : met) {
                    if (F.dpos[x] < covered) continue;
                    fprintf(stderr, "Excluding %s for position %d\n", F.bfs[x]->id.c_str(), L.mut.position);
                    covered = F.dend[x];
                }
            }
            if (ugp_mask_mutations(D.h, nl, lpos.data(), lpar.data(), lnuc.data(), lnode.data(), excl_off.data(), excl.data(),
                                   entry_masked.empty() ? nullptr : entry_masked.data(), first.data(), counts.data()) != UGP_OK)
                lib_fail("ugp_mask_mutations");
            for (size_t j = 0; j < F.bfs.size(); j++) {
                auto &ms = F.bfs[j]->mutations;
                const uint64_t e0 = F.mut_off[j];
                size_t keep = 0;
                for (size_t k = 0; k < ms.size(); k++) {
                    if (first[e0 + k] != UINT32_MAX) { total_masked++; continue; }
                    if (keep != k) ms[keep] = ms[k];
                    keep++;
                }
                ms.resize(keep);
            }
        }
        done(t0, "\n");
        fprintf(stderr, "Masked a total of %lu mutations. Collapsing tree...\n", (unsigned long)total_masked);
        t0 = clock();
        T.collapse_tree();
        done(t0, "\n");
    }
    if (!rename.empty()) {   // renameSamples, :679-701
        fprintf(stderr, "Renaming...\n");
        std::ifstream in(rename);
        if (!in) { fprintf(stderr, "ERROR: Could not open the renaming file: %s!\n", rename.c_str()); return 1; }
        std::string line;
        while (std::getline(in, line)) {
            std::vector<std::string> words;
            split_delim(line, '\t', words);
            if (words.size() != 2) { fprintf(stderr, "ERROR: Incorrect format for the renaming file: %s!\n", rename.c_str()); return 1; }
            if (!T.get_node(words[0])) { fprintf(stderr, "WARNING: Node %s not found in the MAT.\n", words[0].c_str()); continue; }
            fprintf(stderr, "Renaming node %s to %s.\n", words[0].c_str(), words[1].c_str());
            if (!T.rename_node(words[0], words[1])) {
                fprintf(stderr, "ERROR: rename_node: node with id '%s' already exists.\n", words[1].c_str());
                return 1;
            }
        }
    }
    if (recondense) {
        t0 = clock();
        fprintf(stderr, "Collapsing tree...\n");
        T.collapse_tree();
        done(t0, "\n\n");
        t0 = clock();
        fprintf(stderr, "Condensing leaves...\n");
        T.condense_leaves();
        done(t0, "\n\n");
    }
    fprintf(stderr, "Saving final tree to %s\n", out.c_str());
    t0 = clock();
    if (!uh::save_mat(T, out, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return 1; }
    done(t0, "\n\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) { usage(argc < 2 ? stderr : stdout); return argc < 2 ? 1 : 0; }
    if (!strcmp(argv[1], "uncertainty")) return uncertainty(argc - 2, argv + 2);
    if (!strcmp(argv[1], "annotate")) return annotate(argc - 2, argv + 2);
    if (!strcmp(argv[1], "extract")) return extract(argc - 2, argv + 2);
    // matUtils summary runs as `summarize`: the spelling `summary` stays refused, as it has been since the tool's first release
    if (!strcmp(argv[1], "summarize")) return summary(argc - 2, argv + 2);
    if (!strcmp(argv[1], "translate")) return translate(argc - 2, argv + 2);
    if (!strcmp(argv[1], "relatives")) return relatives(argc - 2, argv + 2);
    if (!strcmp(argv[1], "select")) return select_samples(argc - 2, argv + 2);
    if (!strcmp(argv[1], "subtree")) return subtree(argc - 2, argv + 2);
    if (!strcmp(argv[1], "subtrees")) return subtrees(argc - 2, argv + 2);
    if (!strcmp(argv[1], "mask")) return mask(argc - 2, argv + 2);
    if (!strcmp(argv[1], "haplotypes")) return haplotypes(argc - 2, argv + 2);
    fprintf(stderr, "ERROR: unsupported matUtils subcommand '%s' (matutils-amd runs: uncertainty, annotate, extract, subtree, subtrees, summarize, haplotypes, translate, relatives, select, mask)\n", argv[1]);
    return 1;
}
