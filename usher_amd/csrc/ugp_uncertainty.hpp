// ugp_uncertainty.hpp -- matUtils uncertainty (uncertainty.cpp:132-339) on the device: equally parsimonious placements and
// neighborhood size of nodes already in the tree, with the sample built in the reference's literal (unsorted) row order.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct UncState;

// A state on `device` that reads the handle's depth-first tables *tables (ugp_dense.hpp; built from `tree` in the expansion
// `dfs2bfs` (+ inverse) when there are none yet).  *out is replaced.
int unc_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, UncState **out);
void unc_free(UncState *s);
// nodes: BFS indices.  Outputs as ugp_uncertainty documents them.
int unc_run(UncState *s, const uint32_t *nodes, uint64_t n, uint32_t cap, uint32_t *epps, uint32_t *nsize, uint32_t *tie_dfs, uint32_t *tie_count);

}  // namespace ugp
