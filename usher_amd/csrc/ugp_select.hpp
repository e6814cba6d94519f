// ugp_select.hpp -- matUtils extract's sample selectors (get_mutation_samples, get_leaves_ids, get_mrca_samples, select.cpp) on the
// device: bitmaps over leaf ranks from the per-position owner lists and the leaf ranges of the depth-first tables of ugp_dense.hpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct SelState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet; tables built
// from other mutation arrays are UGP_ERR_INVALID) and adds the leaf-rank tables and, unless translate made them, the owners' nodes.
// `dfs2bfs` must outlive the state.  *out is replaced.
int sel_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, SelState **out);
void sel_free(SelState *s);
// As ugp_select_leaves / _mutations_chunked / _subtrees_chunked / _mrca / _time document them; a chunk of 0 is the default.
int sel_leaves(SelState *s, uint32_t *bfs_by_rank, uint64_t *n_leaves);
int sel_mutations(SelState *s, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc, uint64_t *words, uint64_t *counts, uint32_t chunk);
int sel_subtrees(SelState *s, uint64_t n, const uint32_t *nodes, uint64_t *words, uint64_t *counts, uint32_t chunk);
int sel_mrca(SelState *s, const uint64_t *words, uint32_t *node, uint64_t *n_below);
int sel_time(SelState *s, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc, uint32_t reps, double *ms);

}  // namespace ugp
