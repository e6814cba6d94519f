// ugp_select.hip -- matUtils extract's sample selectors on the device (select.cpp: get_mutation_samples :67-111, get_leaves_ids as
// get_clade_samples and -I use it, get_mrca_samples :570-575).
//
// A selection is a bitmap over LEAF RANKS: leaf r is the r-th leaf in depth-first order, bit r & 63 of word r >> 6.  With lbefore[i]
// the leaves in front of depth-first position i, the leaves below node v are the ranks [lbefore[v], lbefore[dend[v]]).
//   k_sel_mutations   one lane per leaf, the queries of a batch in a loop inside the lane: the last owner of the position at or
//                     before the leaf in depth-first order (a binary search over the owners' nodes, ugp_translate.hip's onode), then
//                     up the owners above (mlink) until one's subtree holds the leaf -- allele_above of ugp_translate.hip with the
//                     leaf itself included.  The leaf is selected when that owner's allele is the query's; none: not selected.
//                     A wave's answers are one ballot: lane 0 ORs it into the wave's word and adds its popcount to counts[q].
//   k_sel_ranges      one lane per leaf against sorted disjoint rank ranges (the union of the subtrees asked for).
//   k_sel_minmax      the first and last set rank of a bitmap;  k_sel_climb: from the first leaf up until dend passes the last.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_select.hpp"
#include "ugp_translate.hpp"

namespace ugp {
namespace {

constexpr uint32_t kDefaultQueries = 1024;       // mutation queries staged per launch
constexpr uint32_t kDefaultRanges = 1u << 20;    // rank ranges staged per launch
typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "bitmap words and counts are 64-bit");

__global__ void __launch_bounds__(kBlock) k_sel_mutations(DfsView t, const uint32_t *onode, const uint32_t *leaf_dfs, uint32_t nleaf,
                                                          const int32_t *qpos, const uint8_t *qnuc, uint32_t nq, u64 *words, u64 *counts) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    const bool live = r < nleaf;
    const uint32_t v = live ? leaf_dfs[r] : 0u;
    const bool first = (threadIdx.x & 63u) == 0;
    u64 acc = 0;
    for (uint32_t q = 0; q < nq; q++) {
        const int32_t p = qpos[q];
        bool sel = false;
        if (live && (uint32_t)p < t.tp) {   // p < 0 and p >= tp: nobody, and poff is not touched
            const uint32_t lo = t.poff[p], x = lower_bound_u32(onode, lo, t.poff[p + 1], v + 1);
            uint32_t cur = x > lo ? t.pent[x - 1] : kNil;
            while (cur != kNil && v >= t.dend[t.mnode[cur]]) cur = t.mlink[cur];
            sel = cur != kNil && b_nuc(t.mbits[cur]) == (uint32_t)qnuc[q];
        }
        const u64 votes = __ballot(sel);
        if (votes) {
            acc |= votes;
            if (first) atomicAdd(&counts[q], (u64)__popcll(votes));
        }
    }
    if (first && live && acc) words[r >> 6] |= acc;   // the wave owns its word
}

// Ranges [lo[k], hi[k]), k < nr, sorted and disjoint: leaf r is selected when one holds it.
__global__ void __launch_bounds__(kBlock) k_sel_ranges(uint32_t nleaf, const uint32_t *lo, const uint32_t *hi, uint32_t nr, u64 *words) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    bool sel = false;
    if (r < nleaf) {
        const uint32_t x = lower_bound_u32(lo, 0, nr, r + 1);   // ranges that start at or before r
        sel = x > 0 && r < hi[x - 1];
    }
    const u64 votes = __ballot(sel);
    if ((threadIdx.x & 63u) == 0 && votes) words[r >> 6] |= votes;
}

// mm[0] = min, mm[1] = max over the set ranks below nleaf (kNil, 0 when there are none).
__global__ void __launch_bounds__(kBlock) k_sel_minmax(uint32_t nleaf, uint32_t nwords, const u64 *words, uint32_t *mm) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t mn = kNil, mx = 0;
    if (i < nwords) {
        u64 w = words[i];
        const uint32_t tail = nleaf - i * 64u;   // ranks of this word that exist
        if (tail < 64u) w &= (1ull << tail) - 1ull;
        if (w) {
            mn = i * 64u + (uint32_t)__ffsll((long long)w) - 1u;
            mx = i * 64u + 63u - (uint32_t)__clzll((long long)w);
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
    }
    if ((threadIdx.x & 63u) == 0 && mn != kNil) {
        atomicMin(&mm[0], mn);
        atomicMax(&mm[1], mx);
    }
}

// One lane: out[0] = the deepest node (depth-first position) whose subtree holds leaves mm[0] and mm[1], out[1], out[2] its rank range.
__global__ void __launch_bounds__(kBlock) k_sel_climb(DfsView t, const uint32_t *leaf_dfs, const uint32_t *lbefore, const uint32_t *mm, uint32_t *out) {
    if (blockIdx.x || threadIdx.x) return;
    if (mm[0] == kNil) { out[0] = kNil; out[1] = out[2] = 0; return; }
    uint32_t v = leaf_dfs[mm[0]];
    const uint32_t last = leaf_dfs[mm[1]];
    while (v != 0 && t.dend[v] <= last) v = t.dpar[v];
    out[0] = v;
    out[1] = lbefore[v];
    out[2] = lbefore[t.dend[v]];
}

}  // namespace

struct SelState : QueryBase {
    uint32_t nleaf = 0, nwords = 0;
    std::vector<uint32_t> h_lbefore, h_dend, h_bfs_by_rank;   // [n + 1], [n], [nleaf]
    DBuf<uint32_t> leaf_dfs, lbefore;
    // per call
    DBuf<int32_t> qpos;
    DBuf<uint8_t> qnuc;
    DBuf<uint32_t> rlo, rhi, mm;
    DBuf<u64> words, counts;
};

void sel_free(SelState *s) { query_free(s); }

int sel_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, SelState **out) {
    return query_attach("ugp_select_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out, NoCheck(), [&](SelState *S) {
        LeafRanks R;
        leaf_ranks(tree, dfs2bfs, bfs2dfs, &R);
        const std::vector<uint32_t> &leaf_dfs = R.leaf_dfs;
        S->h_lbefore = std::move(R.lbefore);
        S->h_dend = std::move(R.dend);
        for (uint32_t i : leaf_dfs) S->h_bfs_by_rank.push_back(dfs2bfs[i]);
        S->nleaf = (uint32_t)leaf_dfs.size();
        S->nwords = (S->nleaf + 63u) / 64u;
        const StreamDrain drain{S->stream};   // leaf_dfs
        hipError_t err = S->leaf_dfs.upload(leaf_dfs, S->stream);
        if (err == hipSuccess) err = S->lbefore.upload(S->h_lbefore, S->stream);
        if (err == hipSuccess) err = S->words.alloc(S->nwords);
        if (err == hipSuccess) err = S->mm.alloc(5);
        if (err == hipSuccess) err = hipStreamSynchronize(S->stream);   // leaf_dfs is read until here
        if (int rc = hip_rc("ugp_select_attach", err)) return rc;
        return tr_owner_nodes(*tables, S->stream);
    });
}

static int sel_ready(SelState *S, const char *who) { return query_ready(S, who, "select"); }

int sel_leaves(SelState *S, uint32_t *bfs_by_rank, uint64_t *n_leaves) {
    if (int rc = sel_ready(S, "ugp_select_leaves")) return rc;
    if (!bfs_by_rank && !n_leaves) return set_error(UGP_ERR_INVALID, "null argument");
    if (n_leaves) *n_leaves = S->nleaf;
    if (bfs_by_rank) std::copy(S->h_bfs_by_rank.begin(), S->h_bfs_by_rank.end(), bfs_by_rank);
    return UGP_OK;
}

// The queries to the device (qpos, qnuc); the host arrays are read until the stream is synchronised.
static int sel_stage(SelState *S, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc) {
    UGP_HIP_TRY(S->counts.alloc(n_mut));
    UGP_HIP_TRY(S->qpos.upload(pos, n_mut, S->stream));
    UGP_HIP_TRY(S->qnuc.upload(nuc, n_mut, S->stream));
    return UGP_OK;
}

// The staged queries batch by batch, ORed into S->words (cleared first) with their counts in S->counts (cleared first, [n_mut]).
static int sel_mutation_batches(SelState *S, uint64_t n_mut, uint32_t chunk) {
    hipStream_t st = S->stream;
    UGP_HIP_TRY(hipMemsetAsync(S->words.p, 0, std::max<size_t>(S->nwords, 1) * sizeof(u64), st));
    UGP_HIP_TRY(hipMemsetAsync(S->counts.p, 0, std::max<size_t>(n_mut, 1) * sizeof(u64), st));
    if (!S->nleaf) return UGP_OK;
    const DfsView t = S->T->view();
    for (uint64_t q0 = 0; q0 < n_mut; q0 += chunk) {
        const uint32_t nq = (uint32_t)std::min<uint64_t>(chunk, n_mut - q0);
        k_sel_mutations<<<blocks_for(S->nleaf), kBlock, 0, st>>>(t, S->T->onode.p, S->leaf_dfs.p, S->nleaf, S->qpos.p + q0, S->qnuc.p + q0, nq,
                                                                 S->words.p, S->counts.p + q0);
        UGP_HIP_TRY(hipGetLastError());
    }
    return UGP_OK;
}

int sel_mutations(SelState *S, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc, uint64_t *words, uint64_t *counts, uint32_t chunk) {
    if (int rc = sel_ready(S, "ugp_select_mutations")) return rc;
    if (!words || (n_mut && (!pos || !nuc || !counts))) return set_error(UGP_ERR_INVALID, "null argument");
    if (n_mut >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "more than 2^31 mutation queries");
    UGP_HIP_TRY(hipSetDevice(S->device));
    int rc = sel_stage(S, n_mut, pos, nuc);
    if (!rc) rc = sel_mutation_batches(S, n_mut, chunk ? chunk : kDefaultQueries);
    if (rc) { (void)hipStreamSynchronize(S->stream); return rc; }
    if (S->nwords) UGP_HIP_TRY(hipMemcpyAsync(words, S->words.p, S->nwords * sizeof(u64), hipMemcpyDeviceToHost, S->stream));
    if (n_mut) UGP_HIP_TRY(hipMemcpyAsync(counts, S->counts.p, n_mut * sizeof(u64), hipMemcpyDeviceToHost, S->stream));
    UGP_HIP_TRY(hipStreamSynchronize(S->stream));   // pos and nuc are read until here
    return UGP_OK;
}

int sel_subtrees(SelState *S, uint64_t n, const uint32_t *nodes, uint64_t *words, uint64_t *counts, uint32_t chunk) {
    if (int rc = sel_ready(S, "ugp_select_subtrees")) return rc;
    if (!words || (n && (!nodes || !counts))) return set_error(UGP_ERR_INVALID, "null argument");
    const uint32_t N = S->T->n;
    for (uint64_t i = 0; i < n; i++)
        if (nodes[i] >= N) return set_error(UGP_ERR_INVALID, "ugp_select_subtrees: node " + std::to_string(i) + " is out of range");
    try {
        // the rank ranges, sorted and merged into disjoint ones
        std::vector<std::pair<uint32_t, uint32_t>> rg;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t v = S->T->bfs2dfs[nodes[i]], lo = S->h_lbefore[v], hi = S->h_lbefore[S->h_dend[v]];
            counts[i] = hi - lo;
            if (hi > lo) rg.emplace_back(lo, hi);
        }
        std::sort(rg.begin(), rg.end());
        std::vector<uint32_t> lo, hi;
        for (const auto &r : rg) {
            if (!hi.empty() && r.first <= hi.back()) hi.back() = std::max(hi.back(), r.second);
            else { lo.push_back(r.first); hi.push_back(r.second); }
        }
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        UGP_HIP_TRY(S->rlo.upload(lo, st));
        UGP_HIP_TRY(S->rhi.upload(hi, st));
        UGP_HIP_TRY(hipMemsetAsync(S->words.p, 0, std::max<size_t>(S->nwords, 1) * sizeof(u64), st));
        const uint32_t per = chunk ? chunk : kDefaultRanges;
        for (size_t k0 = 0; k0 < lo.size() && S->nleaf; k0 += per) {
            k_sel_ranges<<<blocks_for(S->nleaf), kBlock, 0, st>>>(S->nleaf, S->rlo.p + k0, S->rhi.p + k0, (uint32_t)std::min<size_t>(per, lo.size() - k0),
                                                                  S->words.p);
            UGP_HIP_TRY(hipGetLastError());
        }
        if (S->nwords) UGP_HIP_TRY(hipMemcpyAsync(words, S->words.p, S->nwords * sizeof(u64), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));   // lo and hi are read until here
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

int sel_mrca(SelState *S, const uint64_t *words, uint32_t *node, uint64_t *n_below) {
    if (int rc = sel_ready(S, "ugp_select_mrca")) return rc;
    if (!words || !node || !n_below) return set_error(UGP_ERR_INVALID, "null argument");
    UGP_HIP_TRY(hipSetDevice(S->device));
    hipStream_t st = S->stream;
    const uint32_t init[2] = {kNil, 0};
    uint32_t got[3] = {kNil, 0, 0};
    UGP_HIP_TRY(hipMemcpyAsync(S->mm.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    if (S->nwords) {
        UGP_HIP_TRY(hipMemcpyAsync(S->words.p, words, S->nwords * sizeof(u64), hipMemcpyHostToDevice, st));
        k_sel_minmax<<<blocks_for(S->nwords), kBlock, 0, st>>>(S->nleaf, S->nwords, S->words.p, S->mm.p);
        k_sel_climb<<<1, kBlock, 0, st>>>(S->T->view(), S->leaf_dfs.p, S->lbefore.p, S->mm.p, S->mm.p + 2);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(hipMemcpyAsync(got, S->mm.p + 2, sizeof(got), hipMemcpyDeviceToHost, st));
    }
    UGP_HIP_TRY(hipStreamSynchronize(st));   // init and words are read until here
    if (got[0] == kNil) return set_error(UGP_ERR_INVALID, "ugp_select_mrca: the bitmap is empty");
    *node = (*S->dfs2bfs)[got[0]];
    *n_below = got[2] - got[1];
    return UGP_OK;
}

int sel_time(SelState *S, uint64_t n_mut, const int32_t *pos, const uint8_t *nuc, uint32_t reps, double *ms) {
    if (int rc = sel_ready(S, "ugp_select_time")) return rc;
    if (!reps || !ms || (n_mut && (!pos || !nuc))) return set_error(UGP_ERR_INVALID, "null argument");
    if (n_mut >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "more than 2^31 mutation queries");
    *ms = 0;
    UGP_HIP_TRY(hipSetDevice(S->device));
    if (int rc = sel_stage(S, n_mut, pos, nuc)) { (void)hipStreamSynchronize(S->stream); return rc; }
    return timed(S->stream, "ugp_select_time", reps, ms, [&] { return sel_mutation_batches(S, n_mut, kDefaultQueries); });
}

}  // namespace ugp
