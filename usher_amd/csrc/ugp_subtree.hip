// ugp_subtree.hip -- the subtree induced by a selection S of nodes (mutation_annotated_tree.cpp: get_subtree :1577-1685, with
// Node::add_mutation :720-752), as a closed form over the depth-first tables.  Nothing climbs and no pair is visited.
//
// below(v) = the members of S at or below v.  v is KEPT when it is in S or two of its children have members.  A node with members
// that is not kept has them all below one child, and the nodes between it and that child in depth-first order have none: its
// OWNER, the kept node at the bottom of its chain, is the first kept node at or after it.
//   k_sub_mark     one lane per name: its byte of the flags over depth-first positions (the same value from every writer)
//   scan_flags     sb: the members in front of every position, so below(v) = sb[dend[v]] - sb[v]
//   k_sub_kept     one lane per node: a child with members, but fewer than its parent has below its children, marks the parent
//   scan_flags     kb: the kept nodes in front of every position: a kept node's output index, and every node's owner
//   k_sub_list     one lane per node: a kept node writes itself to the list; the top of a chain (a node with members whose parent
//                  is kept) writes its owner's subtree parent
//   k_sub_chains   one lane per kept node: the longest chain, in nodes, from the depths
//   k_sub_eflag / scan_flags   the entries on nodes with members, in depth-first order: top-down within every chain
//   k_sub_gather   one lane per entry of a window: (owner << 32 | position + 1, entry) to its slot
//   sort_pairs     stably by the key: one run per (kept node, position), top-down
//   k_sub_merge    one lane per run head of a window walks its run through add_mutation's states: nothing or one entry survives
//   scan_flags / k_sub_compact / k_sub_entoff   the survivors in key order and each kept node's first one
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_sort.hpp"
#include "ugp_subtree.hpp"
#include "ugp_subtree_state.hpp"

namespace ugp {
namespace {

constexpr uint64_t kDefaultWindow = 1ull << 26;   // items per launch of the gather and of the merge
typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "keys and counters are 64-bit");
enum : uint32_t { kDisagree = 0, kFirstDisagree = 1, kLongest = 2, kCounters = 3 };

__device__ __forceinline__ uint32_t below(const DfsView &t, const uint32_t *sb, uint32_t v) { return sb[t.dend[v]] - sb[v]; }

__global__ void __launch_bounds__(kBlock) k_sub_mark(uint32_t nn, const uint32_t *at, uint8_t *sel) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nn) sel[at[i]] = 1;
}

// kept starts as a copy of sel.
__global__ void __launch_bounds__(kBlock) k_sub_kept(DfsView t, const uint8_t *sel, const uint32_t *sb, uint8_t *kept) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c == 0 || c >= t.n) return;
    const uint32_t mine = below(t, sb, c);
    if (!mine) return;
    const uint32_t p = t.dpar[c];
    if (mine < below(t, sb, p) - sel[p]) kept[p] = 1;   // another child of p has members too
}

// kpar starts as kNil: the first kept node's chain starts at the root, which has no parent.
__global__ void __launch_bounds__(kBlock) k_sub_list(DfsView t, const uint8_t *kept, const uint32_t *sb, const uint32_t *kb, uint32_t *kdfs,
                                                     uint32_t *kpar) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= t.n || !below(t, sb, c)) return;
    if (kept[c]) kdfs[kb[c]] = c;
    if (c && kept[t.dpar[c]]) kpar[kb[c]] = kb[t.dpar[c]];
}

__global__ void __launch_bounds__(kBlock) k_sub_chains(DfsView t, uint32_t nk, const uint32_t *kdfs, const uint32_t *kpar, u64 *ctr) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    uint32_t len = 0;
    if (k < nk) len = kpar[k] == kNil ? t.depth[kdfs[k]] + 1 : t.depth[kdfs[k]] - t.depth[kdfs[kpar[k]]];
    for (int d = 32; d > 0; d >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, d, 64));
    if ((threadIdx.x & 63u) == 0 && len) atomicMax(&ctr[kLongest], (u64)len);
}

__global__ void __launch_bounds__(kBlock) k_sub_eflag(DfsView t, uint32_t m, const uint32_t *sb, uint8_t *eflag) {
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e < m) eflag[e] = below(t, sb, t.mnode[e]) ? 1 : 0;
}

// Entries [e0, e1).  The key's low word is position + 1: a masked entry (-1) sorts first, as in the node's sorted vector.
__global__ void __launch_bounds__(kBlock) k_sub_gather(DfsView t, uint32_t e0, uint32_t e1, const uint8_t *eflag, const uint32_t *eb,
                                                       const uint32_t *kb, u64 *key, uint32_t *val) {
    const uint32_t e = e0 + blockIdx.x * kBlock + threadIdx.x;
    if (e >= e1 || !eflag[e]) return;
    const uint32_t o = eb[e];
    key[o] = (u64)kb[t.mnode[e]] << 32 | (uint32_t)(t.mpos[e] + 1);
    val[o] = e;
}

// Sorted items [g0, g1).  The head of a run walks it; every item's survivor flag is written.
__global__ void __launch_bounds__(kBlock) k_sub_merge(uint32_t g0, uint32_t g1, uint32_t G, const u64 *key, const uint32_t *val,
                                                      const uint8_t *mpn, const uint32_t *morig, uint8_t *surv, uint32_t *sfirst,
                                                      uint8_t *snuc, u64 *ctr) {
    const uint32_t i = g0 + blockIdx.x * kBlock + threadIdx.x;
    if (i >= g1) return;
    const u64 k = key[i];
    if (i && key[i - 1] == k) { surv[i] = 0; return; }
    uint32_t first, sn, bad;
    const bool open = walk_run(i, G, k, key, val, mpn, &first, &sn, &bad);
    surv[i] = open ? 1 : 0;
    if (open) { sfirst[i] = morig[first]; snuc[i] = (uint8_t)sn; }
    if (bad) {
        atomicAdd(&ctr[kDisagree], (u64)bad);
        atomicMin(&ctr[kFirstDisagree], k >> 32);
    }
}

__global__ void __launch_bounds__(kBlock) k_sub_compact(uint32_t G, const u64 *key, const uint8_t *surv, const uint32_t *sv,
                                                        const uint32_t *sfirst, const uint8_t *snuc, int32_t *opos, uint32_t *ofirst,
                                                        uint8_t *onuc) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= G || !surv[i]) return;
    const uint32_t o = sv[i];
    opos[o] = (int32_t)(uint32_t)key[i] - 1;
    ofirst[o] = sfirst[i];
    onuc[o] = snuc[i];
}

// eoff[k] = the survivors of the kept nodes before k (k <= nk).
__global__ void __launch_bounds__(kBlock) k_sub_entoff(uint32_t nk, uint32_t G, const u64 *key, const uint32_t *sv, uint32_t *eoff) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k > nk) return;
    const u64 want = (u64)k << 32;
    uint32_t lo = 0, hi = G;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    eoff[k] = sv[lo];
}

__global__ void __launch_bounds__(kBlock) k_sub_owner(DfsView t, uint32_t nn, const uint32_t *at, const uint32_t *sb, const uint32_t *kb,
                                                      uint32_t *owner) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nn) owner[i] = below(t, sb, at[i]) ? kb[at[i]] : kNil;
}

}  // namespace

void sub_free(SubState *s) { query_free(s); }

int sub_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, SubState **out) {
    std::vector<uint8_t> mpn;
    return query_attach(
        "ugp_subtree_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out,
        [&](const DfsTables &T) { return stored_alleles(tree, dfs2bfs, T, "ugp_subtree_attach", &mpn); },
        [&](SubState *S) {
            const uint32_t N = S->T->n;
            const uint64_t M = S->T->m;
            hipError_t err = S->mpn.upload(mpn, S->stream);
            if (err == hipSuccess) err = S->sel.alloc(N);
            if (err == hipSuccess) err = S->kept.alloc(N);
            if (err == hipSuccess) err = S->sb.alloc((size_t)N + 1);
            if (err == hipSuccess) err = S->kb.alloc((size_t)N + 1);
            if (err == hipSuccess) err = S->eflag.alloc(M);
            if (err == hipSuccess) err = S->eb.alloc(M + 1);
            if (err == hipSuccess) err = S->ctr.alloc(kCounters);
            if (err == hipSuccess) err = hipStreamSynchronize(S->stream);   // mpn is read until here
            return hip_rc("ugp_subtree_attach", err);
        });
}

static int sub_ready(SubState *S, const char *who) { return query_ready(S, who, "subtree"); }

// The names as depth-first positions (duplicates stay: the flags take them once).
static int sub_positions(SubState *S, const char *who, uint64_t n, const uint32_t *nodes_bfs, std::vector<uint32_t> *at) {
    const uint32_t N = S->T->n;
    if (!n || !nodes_bfs) return set_error(UGP_ERR_INVALID, std::string(who) + ": no nodes given");
    if (n >= (1ull << 31)) return set_error(UGP_ERR_INVALID, std::string(who) + ": more than 2^31 nodes given");
    for (uint64_t i = 0; i < n; i++)
        if (nodes_bfs[i] >= N) return set_error(UGP_ERR_INVALID, std::string(who) + ": node " + std::to_string(i) + " is out of range");
    at->resize(n);
    for (uint64_t i = 0; i < n; i++) (*at)[i] = S->T->bfs2dfs[nodes_bfs[i]];
    return UGP_OK;
}

// The passes over the staged positions: sb, kept, kb and the entries' flags with their scan.
static int sub_node_passes(SubState *S, uint32_t nn) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const uint32_t N = t.n, M = (uint32_t)S->T->m;
    UGP_HIP_TRY(hipMemsetAsync(S->sel.p, 0, N, st));
    k_sub_mark<<<blocks_for(nn), kBlock, 0, st>>>(nn, S->at.p, S->sel.p);
    UGP_HIP_TRY(scan_flags(S->seg, N, S->sel.p, S->sb.p, st));
    UGP_HIP_TRY(hipMemcpyAsync(S->kept.p, S->sel.p, N, hipMemcpyDeviceToDevice, st));
    k_sub_kept<<<blocks_for(N), kBlock, 0, st>>>(t, S->sel.p, S->sb.p, S->kept.p);
    UGP_HIP_TRY(scan_flags(S->seg, N, S->kept.p, S->kb.p, st));
    if (M) k_sub_eflag<<<blocks_for(M), kBlock, 0, st>>>(t, M, S->sb.p, S->eflag.p);
    UGP_HIP_TRY(scan_flags(S->seg, M, S->eflag.p, S->eb.p, st));
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

// The list of the nk kept nodes with their subtree parents, and the counters.
static int sub_list_passes(SubState *S, uint32_t nk) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    UGP_HIP_TRY(hipMemsetAsync(S->ctr.p, 0, kCounters * sizeof(u64), st));
    UGP_HIP_TRY(hipMemsetAsync(S->ctr.p + kFirstDisagree, 0xff, sizeof(u64), st));
    UGP_HIP_TRY(hipMemsetAsync(S->kpar.p, 0xff, (size_t)nk * sizeof(uint32_t), st));
    k_sub_list<<<blocks_for(t.n), kBlock, 0, st>>>(t, S->kept.p, S->sb.p, S->kb.p, S->kdfs.p, S->kpar.p);
    k_sub_chains<<<blocks_for(nk), kBlock, 0, st>>>(t, nk, S->kdfs.p, S->kpar.p, S->ctr.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

// Gather, sort, merge and compact, for nk kept nodes and G gathered entries whose buffers are allocated.
static int sub_merge_passes(SubState *S, uint32_t nk, uint32_t G, uint64_t chunk) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const uint32_t M = (uint32_t)S->T->m;
    const uint64_t per = chunk ? chunk : kDefaultWindow;
    for (uint64_t e0 = 0; e0 < M; e0 += per) {
        const uint32_t e1 = (uint32_t)std::min<uint64_t>(M, e0 + per);
        k_sub_gather<<<blocks_for(e1 - e0), kBlock, 0, st>>>(t, (uint32_t)e0, e1, S->eflag.p, S->eb.p, S->kb.p, S->kin.p, S->vin.p);
    }
    if (G) UGP_HIP_TRY(sort_pairs(S->tmp, S->kin.p, S->kout.p, S->vin.p, S->vout.p, G, 32 + bits_for(nk), st));
    for (uint64_t g0 = 0; g0 < G; g0 += per) {
        const uint32_t g1 = (uint32_t)std::min<uint64_t>(G, g0 + per);
        k_sub_merge<<<blocks_for(g1 - g0), kBlock, 0, st>>>((uint32_t)g0, g1, G, S->kout.p, S->vout.p, S->mpn.p, t.morig, S->surv.p,
                                                          S->sfirst.p, S->snuc.p, S->ctr.p);
    }
    UGP_HIP_TRY(scan_flags(S->seg, G, S->surv.p, S->sv.p, st));
    if (G) k_sub_compact<<<blocks_for(G), kBlock, 0, st>>>(G, S->kout.p, S->surv.p, S->sv.p, S->sfirst.p, S->snuc.p, S->opos.p, S->ofirst.p,
                                                          S->onuc.p);
    k_sub_entoff<<<blocks_for((uint64_t)nk + 1), kBlock, 0, st>>>(nk, G, S->kout.p, S->sv.p, S->eoff.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

// Everything on the device for the names; S->nk, S->G, S->E and *distinct are known afterwards.
static int sub_run(SubState *S, const std::vector<uint32_t> &at, uint64_t chunk, uint32_t *distinct) {
    hipStream_t st = S->stream;
    const uint32_t N = S->T->n, M = (uint32_t)S->T->m, nn = (uint32_t)at.size();
    S->have = false;
    UGP_HIP_TRY(hipSetDevice(S->device));
    UGP_HIP_TRY(S->at.upload(at, st));
    if (int rc = sub_node_passes(S, nn)) { (void)hipStreamSynchronize(st); return rc; }
    uint32_t nk = 0, G = 0;
    UGP_HIP_TRY(hipMemcpyAsync(distinct, S->sb.p + N, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipMemcpyAsync(&nk, S->kb.p + N, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipMemcpyAsync(&G, S->eb.p + M, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));   // `at` is read until here
    UGP_HIP_TRY(S->kdfs.alloc(nk));
    UGP_HIP_TRY(S->kpar.alloc(nk));
    UGP_HIP_TRY(S->eoff.alloc((size_t)nk + 1));
    UGP_HIP_TRY(S->kin.alloc(G));
    UGP_HIP_TRY(S->kout.alloc(G));
    UGP_HIP_TRY(S->vin.alloc(G));
    UGP_HIP_TRY(S->vout.alloc(G));
    UGP_HIP_TRY(S->surv.alloc(G));
    UGP_HIP_TRY(S->sfirst.alloc(G));
    UGP_HIP_TRY(S->snuc.alloc(G));
    UGP_HIP_TRY(S->sv.alloc((size_t)G + 1));
    UGP_HIP_TRY(S->opos.alloc(G));     // no more survive than were gathered
    UGP_HIP_TRY(S->ofirst.alloc(G));
    UGP_HIP_TRY(S->onuc.alloc(G));
    int rc = sub_list_passes(S, nk);
    if (!rc) rc = sub_merge_passes(S, nk, G, chunk);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    uint32_t E = 0;
    UGP_HIP_TRY(hipMemcpyAsync(&E, S->sv.p + G, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));
    S->nk = nk; S->G = G; S->E = E;
    S->have = true;
    return UGP_OK;
}

int sub_nodes(SubState *S, uint64_t n, const uint32_t *nodes_bfs, uint32_t *kept_bfs, uint32_t *kept_parent, uint64_t *ent_off, uint64_t cap,
              uint64_t *n_kept, uint64_t *n_entries, ugp_subtree_info *info, uint64_t chunk) {
    if (int rc = sub_ready(S, "ugp_subtree_nodes")) return rc;
    if (!n_kept || !n_entries || (cap && (!kept_bfs || !kept_parent || !ent_off))) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        std::vector<uint32_t> at;
        if (int rc = sub_positions(S, "ugp_subtree_nodes", n, nodes_bfs, &at)) return rc;
        uint32_t distinct = 0;
        if (int rc = sub_run(S, at, chunk, &distinct)) return rc;
        hipStream_t st = S->stream;
        const size_t w = (size_t)std::min<uint64_t>(cap, S->nk);
        std::vector<uint32_t> kdfs(w), eoff(w);
        u64 ctr[kCounters] = {0, 0, 0};
        if (w) {
            UGP_HIP_TRY(hipMemcpyAsync(kdfs.data(), S->kdfs.p, w * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(kept_parent, S->kpar.p, w * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(eoff.data(), S->eoff.p, w * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        UGP_HIP_TRY(hipMemcpyAsync(ctr, S->ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, st));
        uint32_t first_dfs = 0;
        UGP_HIP_TRY(hipStreamSynchronize(st));
        const bool any = ctr[kDisagree] != 0;
        if (any) {
            UGP_HIP_TRY(hipMemcpyAsync(&first_dfs, S->kdfs.p + ctr[kFirstDisagree], sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipStreamSynchronize(st));
        }
        for (size_t k = 0; k < w; k++) { kept_bfs[k] = (*S->dfs2bfs)[kdfs[k]]; ent_off[k] = eoff[k]; }
        *n_kept = S->nk;
        *n_entries = S->E;
        if (info) *info = ugp_subtree_info{distinct, S->G, ctr[kDisagree], ctr[kLongest], any ? (*S->dfs2bfs)[first_dfs] : UINT32_MAX, 0};
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

static int sub_answered(SubState *S, const char *who) {
    if (int rc = sub_ready(S, who)) return rc;
    if (!S->have) return set_error(UGP_ERR_INVALID, std::string(who) + ": no selection: call ugp_subtree_nodes first");
    return UGP_OK;
}

int sub_entries(SubState *S, int32_t *pos, uint32_t *first_entry, uint8_t *nuc, uint64_t cap, uint64_t *n_out) {
    if (int rc = sub_answered(S, "ugp_subtree_entries")) return rc;
    if (!n_out || (cap && (!pos || !first_entry || !nuc))) return set_error(UGP_ERR_INVALID, "null argument");
    const size_t w = (size_t)std::min<uint64_t>(cap, S->E);
    if (w) {
        UGP_HIP_TRY(hipSetDevice(S->device));
        UGP_HIP_TRY(hipMemcpyAsync(pos, S->opos.p, w * sizeof(int32_t), hipMemcpyDeviceToHost, S->stream));
        UGP_HIP_TRY(hipMemcpyAsync(first_entry, S->ofirst.p, w * sizeof(uint32_t), hipMemcpyDeviceToHost, S->stream));
        UGP_HIP_TRY(hipMemcpyAsync(nuc, S->onuc.p, w, hipMemcpyDeviceToHost, S->stream));
        UGP_HIP_TRY(hipStreamSynchronize(S->stream));
    }
    *n_out = S->E;
    return UGP_OK;
}

int sub_owner(SubState *S, uint64_t n, const uint32_t *nodes_bfs, uint32_t *owner) {
    if (int rc = sub_answered(S, "ugp_subtree_owner")) return rc;
    if (!owner) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        std::vector<uint32_t> at;
        if (int rc = sub_positions(S, "ugp_subtree_owner", n, nodes_bfs, &at)) return rc;
        hipStream_t st = S->stream;
        UGP_HIP_TRY(hipSetDevice(S->device));
        UGP_HIP_TRY(S->qat.upload(at, st));
        UGP_HIP_TRY(S->qown.alloc(n));
        k_sub_owner<<<blocks_for(n), kBlock, 0, st>>>(S->T->view(), (uint32_t)n, S->qat.p, S->sb.p, S->kb.p, S->qown.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(hipMemcpyAsync(owner, S->qown.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));   // `at` is read until here
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

// ---- the passes alone ---------------------------------------------------------------------------------------------------

int sub_time(SubState *S, uint64_t n, const uint32_t *nodes_bfs, uint32_t reps, double *nodes_ms, double *merge_ms) {
    if (int rc = sub_ready(S, "ugp_subtree_time")) return rc;
    if (!reps || !nodes_ms || !merge_ms) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        std::vector<uint32_t> at;
        if (int rc = sub_positions(S, "ugp_subtree_time", n, nodes_bfs, &at)) return rc;
        uint32_t distinct = 0;
        if (int rc = sub_run(S, at, 0, &distinct)) return rc;   // stages the names and sizes the buffers
        const uint32_t nk = S->nk, G = S->G;
        if (int rc = timed(S->stream, "ugp_subtree_time", reps, nodes_ms, [&] { const int c = sub_node_passes(S, (uint32_t)n); return c ? c : sub_list_passes(S, nk); })) return rc;
        if (int rc = timed(S->stream, "ugp_subtree_time", reps, merge_ms, [&] { return sub_merge_passes(S, nk, G, 0); })) return rc;
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

}  // namespace ugp
