// ugp_genotypes.hpp -- matUtils extract -v (make_vcf / r_add_genotypes, matUtils/convert.cpp:14-320) on the device: the site
// table and the genotype codes of a selection of nodes, over the depth-first tables of ugp_dense.hpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct GtState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet) and adds,
// per owner, its node, the owner above it, its allele and its stored parent allele.  `dfs2bfs` must outlive the state.  *out is
// replaced.  Tables that an earlier attach of the handle built from other mutation arrays are UGP_ERR_INVALID.
int gt_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, GtState **out);
void gt_free(GtState *s);
// As ugp_genotype_select / _columns / _sites / _rows_chunked document them.
int gt_select(GtState *s, const uint32_t *nodes, uint64_t n, uint32_t *n_cols, uint64_t *n_sites);
int gt_columns(GtState *s, uint32_t *nodes);
int gt_sites(GtState *s, uint64_t lo, uint64_t hi, ugp_gt_site *out);
int gt_rows(GtState *s, uint64_t lo, uint64_t hi, uint8_t *codes, uint64_t chunk_cells);
// Bench hook: the device time of the row kernel alone over sites [lo, hi) (no copy to the host), mean of `reps` runs.
int gt_rows_time(GtState *s, uint64_t lo, uint64_t hi, uint32_t reps, double *ms);

}  // namespace ugp
