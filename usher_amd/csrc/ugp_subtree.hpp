// ugp_subtree.hpp -- the subtree induced by a selection (mutation_annotated_tree.cpp: get_subtree :1577-1685) on the device, in closed
// form over the depth-first tables of ugp_dense.hpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct SubState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet; tables built
// from other mutation arrays are UGP_ERR_INVALID) and adds the stored parent allele and allele of every entry (an allele above 15:
// UGP_ERR_UNSUPPORTED).  `dfs2bfs` must outlive the state.  *out is replaced.
int sub_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, SubState **out);
void sub_free(SubState *s);
// As ugp_subtree_nodes_chunked / _entries / _owner / _time document them; a chunk of 0 is the default.
int sub_nodes(SubState *s, uint64_t n, const uint32_t *nodes_bfs, uint32_t *kept_bfs, uint32_t *kept_parent, uint64_t *ent_off, uint64_t cap,
              uint64_t *n_kept, uint64_t *n_entries, ugp_subtree_info *info, uint64_t chunk);
int sub_entries(SubState *s, int32_t *pos, uint32_t *first_entry, uint8_t *nuc, uint64_t cap, uint64_t *n_out);
int sub_owner(SubState *s, uint64_t n, const uint32_t *nodes_bfs, uint32_t *owner);
int sub_time(SubState *s, uint64_t n, const uint32_t *nodes_bfs, uint32_t reps, double *nodes_ms, double *merge_ms);
// ugp_subtree_batch.hip: as ugp_subtree_batch_chunked / _nodes / _entries / _time document them; 0 is either default.
int sub_batch(SubState *s, uint64_t n_sel, const uint64_t *sel_off, const uint32_t *nodes_bfs, uint64_t *kept_off, uint64_t *entry_off,
              ugp_subtree_batch_info *info, uint64_t group_positions, uint64_t chunk_items);
int sub_batch_nodes(SubState *s, uint32_t *kept_bfs, uint32_t *kept_parent, uint64_t *ent_off, uint64_t cap, uint64_t *n_out);
int sub_batch_entries(SubState *s, int32_t *pos, uint32_t *first_entry, uint8_t *nuc, uint64_t cap, uint64_t *n_out);
int sub_batch_time(SubState *s, uint64_t n_sel, const uint64_t *sel_off, const uint32_t *nodes_bfs, uint32_t reps, double *nodes_ms,
                   double *merge_ms);

}  // namespace ugp
