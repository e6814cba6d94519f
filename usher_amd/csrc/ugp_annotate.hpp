// ugp_annotate.hpp -- matUtils annotate (annotate.cpp:301-419, 466-481, 611-638) on the device: clade allele counts from
// exemplar samples, descendant counts of candidate nodes, and the literal search for clade rows the packed search refuses.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct AnnState;

// A state on `device` that reads the handle's depth-first tables *tables (ugp_dense.hpp; built from `tree` in the expansion
// `dfs2bfs` (+ inverse) when there are none yet).  *out is replaced.
int ann_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, AnnState **out);
void ann_free(AnnState *s);
// Outputs as ugp_clade_alleles / ugp_clade_descendants / ugp_annotate_search document them.
int ann_alleles(AnnState *s, const uint64_t *clade_off, const uint32_t *nodes, uint64_t n_clades, uint64_t *out_off, uint32_t *out_ent,
                uint32_t *out_cnt, uint64_t cap, uint64_t *n_out);
int ann_descendants(AnnState *s, const uint64_t *clade_off, const uint32_t *nodes, uint64_t n_clades, const uint32_t *pair_clade,
                    const uint32_t *pair_node, uint64_t n_pairs, uint32_t *out);
int ann_search(AnnState *s, const ugp_queries *q, uint32_t cap, int32_t *best, uint32_t *tie_dfs, uint32_t *tie_count);

}  // namespace ugp
