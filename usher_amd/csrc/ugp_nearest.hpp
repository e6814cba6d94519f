// ugp_nearest.hpp -- matUtils extract's "k nearest samples" (get_nearby, select.cpp:206-276) for a batch of queries on the
// device: a segmented "k smallest keys over a depth-first range" on the depth-first tables of ugp_dense.hpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct NearState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet) and adds
// the leaf prefix table and the depth-first -> breadth-first map.  `dfs2bfs` must outlive the state.  *out is replaced.
int nk_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, NearState **out);
void nk_free(NearState *s);
// Outputs as ugp_nearest_k documents them; chunk_queries = 0: the default workspace chunk.
int nk_run(NearState *s, uint64_t n_queries, const uint32_t *nodes, const uint32_t *k, uint32_t out_stride, uint32_t *out_nodes,
           uint32_t *out_dist, ugp_nearest_info *info, uint32_t chunk_queries);

}  // namespace ugp
