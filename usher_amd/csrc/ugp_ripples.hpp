// ugp_ripples.hpp -- RIPPLES' recombination search (ripples/main.cpp:300-680) on the device: for each long branch, pass 1
// (mapper2_body over every node with enough descendants), the unmatched-mutation counts of every candidate donor / acceptor
// for every breakpoint pair, and the selected (donor, acceptor) of each pair.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct RipState;

// Host tables of `tree` (BFS order) and the name ranks, uploaded to `device`; bfs2dfs = the handle's preorder position of each
// node.  *out is replaced.
int rip_attach(const ugp_tree_desc *tree, const uint32_t *name_rank, const std::vector<uint32_t> &bfs2dfs, int device, RipState **out);
void rip_free(RipState *s);
// branches: BFS indices.  Outputs as ugp_ripples documents them.
int rip_run(RipState *s, const ugp_ripples_opts *opts, const uint32_t *branches, uint64_t n, ugp_ripples_event *out, uint64_t cap,
            uint64_t *n_out);

}  // namespace ugp
