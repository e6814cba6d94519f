// ugp_vectors.hpp -- node_excess_mutations and node_imputed_mutations of mapper2_body (usher_mapper.cpp:167-504 with compute_vecs) for
// (sample, node) pairs on the device, in closed form over the per-position owner lists of the depth-first tables of ugp_dense.hpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct VecState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet; tables built
// from other mutation arrays are UGP_ERR_INVALID) and adds the stored parent alleles and, unless translate or select made them, the
// owners' nodes.  *out is replaced.
int vec_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, VecState **out);
void vec_free(VecState *s);
// UGP_OK when `s` is attached and every pair names a sample of q and a node of the tree; `who` names the call in the error.
int vec_check(VecState *s, const char *who, const ugp_queries *q, uint64_t n_pairs, const uint32_t *sample, const uint32_t *node);
// As ugp_vectors_chunked documents it, after vec_check; the rows of q are on the device already (d_pos .. d_missing, checked, null
// without rows).  kernel_ms != null (the bench hook): the two passes alone into kernel_ms[0..1], nothing is copied back.
int vec_run(VecState *s, const ugp_queries *q, const int32_t *d_pos, const uint8_t *d_ref, const uint8_t *d_nuc, const uint8_t *d_missing,
            uint64_t n_pairs, const uint32_t *sample, const uint32_t *node, ugp_vec_info *info, uint64_t *ex_off, ugp_vec_entry *excess,
            uint64_t ex_cap, uint64_t *n_excess, uint64_t *im_off, ugp_vec_entry *imputed, uint64_t im_cap, uint64_t *n_imputed,
            uint32_t chunk_pairs, double *kernel_ms);

}  // namespace ugp
