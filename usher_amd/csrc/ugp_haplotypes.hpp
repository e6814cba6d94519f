// ugp_haplotypes.hpp -- matUtils summary --haplotype (matUtils/summary.cpp: count_haplotypes, write_haplotype_table) on the device:
// the distinct haplotypes of the leaves and their counts, over the depth-first tables of ugp_dense.hpp and their per-position
// owner lists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct HpState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet) and adds the
// owners' nodes by position (tr_owner_nodes) and the leaves in depth-first order.  `dfs2bfs` must outlive the state.  *out is
// replaced.  Tables that an earlier attach of the handle built from other mutation arrays are UGP_ERR_INVALID.
int hp_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, HpState **out);
void hp_free(HpState *s);
// As ugp_haplotype_groups_hashed / ugp_haplotype_sets_chunked / ugp_haplotype_time document them.
int hp_groups(HpState *s, ugp_hp_group *out, uint64_t cap, uint64_t *n_out, ugp_hp_info *info, uint32_t hash_bits);
int hp_sets(HpState *s, const uint32_t *leaves, uint64_t n, uint64_t *off, int32_t *pos, uint8_t *nuc, uint64_t cap, uint64_t *n_out,
            uint64_t chunk_leaves);
int hp_time(HpState *s, uint32_t reps, double *scan_ms, double *sort_ms, double *verify_ms);

}  // namespace ugp
