// ugp_mask.hpp -- matUtils mask (matUtils/mask.cpp: restrictSamples :802-905, restrictMutationsLocally :703-800) on the device: both
// in closed form over the depth-first tables of ugp_dense.hpp and the leaf-rank ranges ugp_select.hip also builds.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct MskState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet; tables built
// from other mutation arrays are UGP_ERR_INVALID) and adds the leaf-rank ranges, "has a leaf child" and the stored parent allele and
// allele of every entry (an allele above 15: UGP_ERR_UNSUPPORTED).  `dfs2bfs` must outlive the state.  *out is replaced.
int msk_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, MskState **out);
void msk_free(MskState *s);
// As ugp_mask_restricted / _mutations_chunked / _time document them; a chunk of 0 is the default.
int msk_restricted(MskState *s, uint64_t n, const uint32_t *leaves_bfs, uint8_t *entry_masked, uint32_t *roots_bfs, uint64_t roots_cap,
                   uint64_t *n_roots, uint64_t *n_masked);
int msk_mutations(MskState *s, uint64_t n_lines, const int32_t *pos, const uint8_t *par, const uint8_t *nuc, const uint32_t *node_bfs,
                  const uint64_t *excl_off, const uint32_t *excl_bfs, const uint8_t *skip, uint32_t *first_line, uint64_t *counts,
                  uint32_t chunk);
int msk_time(MskState *s, uint64_t n, const uint32_t *leaves_bfs, uint64_t n_lines, const int32_t *pos, const uint8_t *par,
             const uint8_t *nuc, const uint32_t *node_bfs, const uint64_t *excl_off, const uint32_t *excl_bfs, uint32_t reps,
             double *restricted_ms, double *mutations_ms);

}  // namespace ugp
