// ugp_translate.hpp -- matUtils summary --translate (matUtils/translate.cpp) on the device: per node the codons its mutations touch and
// their letters before and after, over the depth-first tables of ugp_dense.hpp and their per-position owner lists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "usher_amd.h"

namespace ugp {

struct DfsTables;
struct TrState;

// A state on `device` that reads the handle's depth-first tables *tables (built from `tree` when there are none yet) and adds the
// owners' nodes by position and the stored parent alleles.  `dfs2bfs` must outlive the state.  *out is replaced.  Tables that an
// earlier attach of the handle built from other mutation arrays are UGP_ERR_INVALID.
int tr_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, TrState **out);
void tr_free(TrState *s);
// The owners' nodes by list slot (tables->onode), made once per tables whoever asks first: translate and select both search them.
int tr_owner_nodes(DfsTables *tables, hipStream_t stream);
// As ugp_translate_codons / ugp_translate_chunked / ugp_translate_time document them.
int tr_codons(TrState *s, uint64_t n_codons, const int32_t *slot_pos, const uint8_t *slot_init);
int tr_run(TrState *s, ugp_tr_record *out, uint64_t cap, uint64_t *n_out, ugp_tr_info *info, uint64_t chunk_items);
int tr_time(TrState *s, uint32_t reps, double *ms);

}  // namespace ugp
