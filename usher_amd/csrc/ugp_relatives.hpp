// ugp_relatives.hpp -- matUtils extract's per-sample relatives (get_closest_samples, select.cpp:577-714) for a batch of samples on
// the device: a short climb and a few range queries per sample on the depth-first tables of ugp_dense.hpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct RelState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet; tables built
// from other mutation arrays are UGP_ERR_INVALID) and adds the leaf tables, the range minima and the (cum, leaf) order.
// name_rank [n] by BFS index is a permutation, or null.  `dfs2bfs` must outlive the state.  *out is replaced.
int rel_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               const uint32_t *name_rank, DfsTables **tables, RelState **out);
void rel_free(RelState *s);
// Outputs as ugp_relatives_closest / ugp_relatives_within document them; chunk_samples = 0: the default workspace chunk.
// kernel_ms (bench hook) non-null: nothing but *n_out is written, the lists stay on the device, and kernel_ms[0] / [1] receive
// the device time of the counting pass with its prefix sum and of the fill pass.
int rel_run(RelState *s, bool within, uint64_t n, const uint32_t *nodes, uint32_t threshold, ugp_rel_info *info, uint64_t *out_off,
            uint32_t *out_nodes, uint64_t cap, uint64_t *n_out, uint32_t chunk_samples, double *kernel_ms);

}  // namespace ugp
