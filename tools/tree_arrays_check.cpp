// tree_arrays_check.cpp -- uh::TreeArrays under the address and undefined-behaviour sanitizers, on the host alone (no device, no
// library): the type hands out raw pointers into its vectors, so every array is read through desc() and bare() after a move.
//
// From the repository's root (one command, then the run):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -Iinclude -Iusher_amd/csrc/host -o /tmp/tree_arrays_check
//       tools/tree_arrays_check.cpp usher_amd/csrc/host/mat.cpp -lz -pthread
//   /tmp/tree_arrays_check tests/golden/survey_ref/syn/tree.pb
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "mat.hpp"

namespace {

// Every element the library may read, through a descriptor; the sum keeps the reads alive.
uint64_t read_all(const ugp_tree_desc &d, uint64_t want_entries) {
    uint64_t sum = 0;
    for (uint64_t j = 0; j < d.n_nodes; j++) sum += d.parent[j] + d.mut_off[j + 1];
    if (d.mut_off[0] != 0 || d.mut_off[d.n_nodes] != want_entries) { fprintf(stderr, "mut_off does not span %llu entries\n", (unsigned long long)want_entries); exit(1); }
    if (!d.mut_pos || !d.mut_ref || !d.mut_par || !d.mut_nuc) { fprintf(stderr, "null entry array\n"); exit(1); }
    for (uint64_t k = 0; k < want_entries; k++) sum += (uint64_t)d.mut_pos[k] + d.mut_ref[k] + d.mut_par[k] + d.mut_nuc[k];
    return sum;
}

uint64_t check(const uh::Tree &T) {
    uh::TreeArrays first(T, uh::TreeArrays::kEntries | uh::TreeArrays::kDepthFirst);
    const uint64_t M = first.mut_off.back();
    uh::TreeArrays A(std::move(first));   // the views below are computed after the move
    uh::TreeArrays B;
    B = std::move(A);
    uint64_t sum = read_all(B.desc(), M) + read_all(B.bare(), 0);
    const size_t N = B.bfs.size();
    if (B.ent.size() != M || B.dfs.size() != N || B.pos.empty()) { fprintf(stderr, "wrong sizes\n"); exit(1); }
    for (size_t j = 0; j < N; j++) {
        if (B.bfs[j]->flat_index != j || B.dfs[B.dpos[j]] != B.bfs[j] || B.dend[j] <= B.dpos[j] || B.dend[j] > N) { fprintf(stderr, "wrong numbering at %zu\n", j); exit(1); }
        for (uint64_t k = B.mut_off[j]; k < B.mut_off[j + 1]; k++)
            if (B.ent[k] != &B.bfs[j]->mutations[k - B.mut_off[j]] || B.ent[k]->position != B.pos[k]) { fprintf(stderr, "wrong entry %llu\n", (unsigned long long)k); exit(1); }
    }
    for (uint32_t r : B.name_rank()) sum += r;
    return sum;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s tree.pb\n", argv[0]); return 2; }
    uh::Tree T;
    std::string err;
    if (!uh::load_mat(argv[1], T, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    if (!T.condensed_nodes.empty()) T.uncondense_leaves();
    uint64_t sum = check(T);
    uh::Tree one;   // a single node without an entry: no file holds it (the newick parser wants a bracket), a Tree can
    one.create_node("only", nullptr);
    sum += check(one);
    printf("tree arrays ok (%llu)\n", (unsigned long long)sum);
    return 0;
}
