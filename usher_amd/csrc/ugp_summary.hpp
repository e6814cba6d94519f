// ugp_summary.hpp -- matUtils summary (matUtils/summary.cpp) on the device: the mutation table (-m), the RoHo records (-R) and the
// clade counts (-c / -C), over the depth-first tables of ugp_dense.hpp and an occurrence list of the tree's mutation entries.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct SmState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet) and adds the
// occurrence list, the strict-descendant leaf counts and the per-parent sorted leaf counts.  `dfs2bfs` must outlive the state.
// *out is replaced.  Tables that an earlier attach of the handle built from other mutation arrays are UGP_ERR_INVALID.
int sm_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, SmState **out);
void sm_free(SmState *s);
// As ugp_summary_mutations_chunked / _roho_chunked / _clades document them.
int sm_mutations(SmState *s, ugp_sm_mutation *out, uint64_t cap, uint64_t *n_out, uint64_t chunk_items);
int sm_roho(SmState *s, ugp_sm_roho *out, uint64_t cap, uint64_t *n_out, uint64_t chunk_items);
int sm_clades(SmState *s, const uint64_t *col_off, const uint32_t *nodes, uint64_t n_cols, uint32_t *incl, uint32_t *excl, uint32_t *leaf_clade);
// Bench hook: the device time of the occurrence-list sort alone and of the RoHo kernel alone (no compaction, no copy), mean of `reps`.
int sm_time(SmState *s, uint32_t reps, double *sort_ms, double *roho_ms);

}  // namespace ugp
