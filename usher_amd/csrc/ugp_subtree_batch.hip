// ugp_subtree_batch.hip -- many induced subtrees of one tree in one call (matUtils/convert.cpp: get_minimum_subtrees :665-798 calls
// get_subtree once per neighbourhood), each exactly what ugp_subtree.hip answers for its selection alone.
//
// The WINDOW of a selection is the depth-first range [lca, dend[lca]) of its lowest common ancestor: every kept node and every
// chain but the root's lies inside it.  The windows of a GROUP of selections are laid end to end, and the pass sequence of
// ugp_subtree.hip runs once over the concatenation: a concatenated position p of window w stands for the tree position
// lca[w] + p - woff[w], and below(v) is a difference of two values of one window, so the global flag scans need no reset.
//   k_sbat_lca      one lane per selection: from its smallest depth-first rank up dpar until dend covers its largest
//   k_sbat_wid      one lane per concatenated position: its window (a search in the window offsets, once; the passes read it)
//   k_sbat_mark / scan_flags / k_sbat_kept / scan_flags / k_sbat_list / k_sbat_chains   as k_sub_*, through the window
//   k_sbat_eflag / scan_flags   the entries of the windows' nodes with members, window after window
//   k_sbat_winfo    one lane per window: its members, its first kept index, its gathered entries
//   k_sbat_rootpath one lane per window: the entries above the lca, in front of everything gathered from the windows.  This is
//                   the ONE place that climbs: lca -> root, and an entry's slot is its rank on the root path (cum[u] counts the
//                   entries down to u), so the slots are top-down without a reversal.  They carry the window's first kept index.
//   k_sbat_gather   one lane per window entry: (group kept index << 32 | position + 1, entry) behind the root paths' slots
//   sort_pairs      stably: one run per (kept node, position), root path first, then top-down
//   k_sbat_merge / scan_flags / k_sbat_compact / k_sbat_entoff   as k_sub_*, with the counters of the run's window
// Groups run back to back on one stream; each group's lists are appended to the result on the host.  The host is asked twice per
// group (the sizes, the lists), never per selection.
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

constexpr uint64_t kDefaultChunk = 1ull << 26;   // items per launch of the gather and of the merge
// The default group budget.  ugp_subtree_attach allocates, for the single call, 10 bytes per depth-first position (sel, kept: 1 each;
// sb, kb: 4 each) and 5 per entry (eflag 1, eb 4).  A group needs 14 per concatenated position (the same and wid: 4) and 9 per window
// entry (the same and ewid: 4).  N / 2 positions and M / 2 entries (root paths included) make 7 N + 4.5 M <= 10 N + 5 M: a batch
// needs no more than the single call has already.  The floor keeps small trees in one group; one window larger than the budget
// runs alone and takes 14 bytes per position of its own.
constexpr uint64_t kBudgetFloor = 1ull << 16;
typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "keys and counters are 64-bit");
enum : uint32_t { kDisagree = 0, kFirstDisagree = 1, kLongest = 2, kCounters = 3 };   // per window

struct WinView {   // the windows of one group
    uint32_t nw;
    const uint32_t *lca;     // [nw]     depth-first position of the window's first node
    const uint32_t *woff;    // [nw + 1] concatenated positions in front of the window
    const uint32_t *eoffw;   // [nw + 1] window entries in front of the window's
    const uint32_t *rpoff;   // [nw + 1] root-path entries in front of the window's
};

// The last w with off[w] <= i (off[0] = 0 <= i < off[nw]).
__device__ __forceinline__ uint32_t window_of(const uint32_t *off, uint32_t nw, uint32_t i) {
    uint32_t lo = 0, hi = nw;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kBlock) k_sbat_lca(DfsView t, uint32_t ns, const uint32_t *lo, const uint32_t *hi, uint32_t *lca,
                                                     uint32_t *wlen, uint32_t *went, uint32_t *rpe) {
    const uint32_t b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= ns) return;
    uint32_t v = lo[b];
    const uint32_t last = hi[b];
    while (t.dend[v] <= last) v = t.dpar[v];   // the root's range covers every rank
    const uint32_t end = t.dend[v];
    lca[b] = v;
    wlen[b] = end - v;
    went[b] = t.moff[end] - t.moff[v];
    rpe[b] = v ? t.cum[t.dpar[v]] : 0;
}

__global__ void __launch_bounds__(kBlock) k_sbat_wid(uint32_t P, WinView W, uint32_t *wid) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p < P) wid[p] = window_of(W.woff, W.nw, p);
}

__global__ void __launch_bounds__(kBlock) k_sbat_mark(uint32_t nn, const uint32_t *cpos, uint8_t *sel) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nn) sel[cpos[i]] = 1;
}

// below() of the node at concatenated position p that stands for tree position c.
__device__ __forceinline__ uint32_t below_at(const DfsView &t, const uint32_t *sb, uint32_t p, uint32_t c) {
    return sb[p + (t.dend[c] - c)] - sb[p];
}

// kept starts as a copy of sel.  A window's first node has no parent in the window.
__global__ void __launch_bounds__(kBlock) k_sbat_kept(DfsView t, uint32_t P, WinView W, const uint32_t *wid, const uint8_t *sel,
                                                      const uint32_t *sb, uint8_t *kept) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const uint32_t w = wid[p], base = W.woff[w];
    if (p == base) return;
    const uint32_t c = W.lca[w] + (p - base);
    const uint32_t mine = below_at(t, sb, p, c);
    if (!mine) return;
    const uint32_t pc = t.dpar[c], pp = p - (c - pc);
    if (mine < below_at(t, sb, pp, pc) - sel[pp]) kept[pp] = 1;   // another child has members too
}

// kpar starts as kNil.  Kept indices count through the group; a subtree parent is an index within its window's slice.
__global__ void __launch_bounds__(kBlock) k_sbat_list(DfsView t, uint32_t P, WinView W, const uint32_t *wid, const uint8_t *kept,
                                                      const uint32_t *sb, const uint32_t *kb, uint32_t *kdfs, uint32_t *kpar,
                                                      uint32_t *kwin) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    const uint32_t w = wid[p], base = W.woff[w];
    const uint32_t c = W.lca[w] + (p - base);
    if (!below_at(t, sb, p, c)) return;
    const uint32_t k = kb[p];
    if (kept[p]) { kdfs[k] = c; kwin[k] = w; }
    if (p == base) return;
    const uint32_t pp = p - (c - t.dpar[c]);
    if (kept[pp]) kpar[k] = kb[pp] - kb[base];
}

__global__ void __launch_bounds__(kBlock) k_sbat_chains(DfsView t, uint32_t nk, const uint32_t *kdfs, const uint32_t *kpar,
                                                        const uint32_t *kwin, const uint32_t *koff, u64 *ctr) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= nk) return;
    const uint32_t w = kwin[k], par = kpar[k];
    const uint32_t len = par == kNil ? t.depth[kdfs[k]] + 1 : t.depth[kdfs[k]] - t.depth[kdfs[koff[w] + par]];
    atomicMax(&ctr[(size_t)w * kCounters + kLongest], (u64)len);
}

__global__ void __launch_bounds__(kBlock) k_sbat_eflag(DfsView t, uint32_t EW, WinView W, const uint32_t *sb, uint8_t *eflag, uint32_t *ewid) {
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= EW) return;
    const uint32_t w = window_of(W.eoffw, W.nw, q), top = W.lca[w];
    const uint32_t c = t.mnode[t.moff[top] + (q - W.eoffw[w])];
    eflag[q] = below_at(t, sb, W.woff[w] + (c - top), c) ? 1 : 0;
    ewid[q] = w;
}

// koff[w] = the kept nodes in front of window w (w <= nw), nsel / gath [nw]: the window's distinct members and gathered entries.
__global__ void __launch_bounds__(kBlock) k_sbat_winfo(uint32_t P, WinView W, const uint32_t *sb, const uint32_t *kb, const uint32_t *eb,
                                                       uint32_t *koff, uint32_t *nsel, uint32_t *gath) {
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    if (w > W.nw) return;
    koff[w] = kb[w < W.nw ? W.woff[w] : P];
    if (w == W.nw) return;
    nsel[w] = sb[W.woff[w + 1]] - sb[W.woff[w]];
    gath[w] = (eb[W.eoffw[w + 1]] - eb[W.eoffw[w]]) + (W.rpoff[w + 1] - W.rpoff[w]);
}

// One lane per window climbs from its lca's parent to the root.  The entries of u take the slots [cum[u] - its entries, cum[u]) of
// the window's root path.
__global__ void __launch_bounds__(kBlock) k_sbat_rootpath(DfsView t, WinView W, const uint32_t *koff, u64 *key, uint32_t *val) {
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    if (w >= W.nw) return;
    uint32_t u = W.lca[w];
    const u64 hi = (u64)koff[w] << 32;
    const uint32_t base = W.rpoff[w];
    while (u) {
        u = t.dpar[u];
        const uint32_t e0 = t.moff[u], e1 = t.moff[u + 1];
        const uint32_t slot = base + t.cum[u] - (e1 - e0);
        for (uint32_t e = e0; e < e1; e++) {
            key[slot + (e - e0)] = hi | (uint32_t)(t.mpos[e] + 1);
            val[slot + (e - e0)] = e;
        }
    }
}

// Window entries [q0, q1), behind the RP root-path slots.
__global__ void __launch_bounds__(kBlock) k_sbat_gather(DfsView t, uint32_t q0, uint32_t q1, uint32_t RP, WinView W, const uint8_t *eflag,
                                                        const uint32_t *eb, const uint32_t *ewid, const uint32_t *kb, u64 *key, uint32_t *val) {
    const uint32_t q = q0 + blockIdx.x * kBlock + threadIdx.x;
    if (q >= q1 || !eflag[q]) return;
    const uint32_t w = ewid[q], top = W.lca[w];
    const uint32_t e = t.moff[top] + (q - W.eoffw[w]);
    const uint32_t o = RP + eb[q];
    key[o] = (u64)kb[W.woff[w] + (t.mnode[e] - top)] << 32 | (uint32_t)(t.mpos[e] + 1);
    val[o] = e;
}

// Sorted items [g0, g1).  The head of a run walks it (k_sub_merge); the counters are those of the run's window.
__global__ void __launch_bounds__(kBlock) k_sbat_merge(uint32_t g0, uint32_t g1, uint32_t G, const u64 *key, const uint32_t *val,
                                                       const uint8_t *mpn, const uint32_t *morig, const uint32_t *kwin, uint8_t *surv,
                                                       uint32_t *sfirst, uint8_t *snuc, u64 *ctr) {
    const uint32_t i = g0 + blockIdx.x * kBlock + threadIdx.x;
    if (i >= g1) return;
    const u64 k = key[i];
    if (i && key[i - 1] == k) { surv[i] = 0; return; }
    uint32_t first, sn, bad;
    const bool open = walk_run(i, G, k, key, val, mpn, &first, &sn, &bad);
    surv[i] = open ? 1 : 0;
    if (open) { sfirst[i] = morig[first]; snuc[i] = (uint8_t)sn; }
    if (bad) {
        u64 *c = ctr + (size_t)kwin[k >> 32] * kCounters;
        atomicAdd(&c[kDisagree], (u64)bad);
        atomicMax(&c[kFirstDisagree], ~(k >> 32));   // the smallest kept index, inverted: the counters start at 0
    }
}

__global__ void __launch_bounds__(kBlock) k_sbat_compact(uint32_t G, const u64 *key, const uint8_t *surv, const uint32_t *sv,
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
__global__ void __launch_bounds__(kBlock) k_sbat_entoff(uint32_t nk, uint32_t G, const u64 *key, const uint32_t *sv, uint32_t *eoff) {
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

}  // namespace

struct BatState {
    // the batch: per selection
    DBuf<uint32_t> lo, hi, lca, wlen, went, rpe, cpos;
    // one group
    DBuf<uint32_t> offs, wid, seg, sb, kb, eb, ewid, koff, nsel, gath, kdfs, kpar, kwin, eoff, vin, vout, sv, sfirst, ofirst;
    DBuf<uint8_t> sel, kept, eflag, surv, snuc, onuc;
    DBuf<u64> kin, kout, ctr;
    DBuf<int32_t> opos;
    DBuf<unsigned char> tmp;
    // the last batch's answer
    bool have = false;
    std::vector<uint32_t> kept_bfs, kept_parent, first;
    std::vector<uint64_t> ent_off;
    std::vector<int32_t> pos;
    std::vector<uint8_t> nuc;
};

void bat_free(BatState *b) { delete b; }

namespace {

struct Group {   // one group's sizes and views
    uint32_t nw = 0, nn = 0, P = 0, EW = 0, RP = 0, nk = 0, G = 0;
    const uint32_t *cpos = nullptr;
    WinView W{};
};

int bat_node_passes(SubState *S, BatState *B, const Group &g) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    UGP_HIP_TRY(hipMemsetAsync(B->sel.p, 0, g.P, st));
    k_sbat_wid<<<blocks_for(g.P), kBlock, 0, st>>>(g.P, g.W, B->wid.p);
    k_sbat_mark<<<blocks_for(g.nn), kBlock, 0, st>>>(g.nn, g.cpos, B->sel.p);
    UGP_HIP_TRY(scan_flags(B->seg, g.P, B->sel.p, B->sb.p, st));
    UGP_HIP_TRY(hipMemcpyAsync(B->kept.p, B->sel.p, g.P, hipMemcpyDeviceToDevice, st));
    k_sbat_kept<<<blocks_for(g.P), kBlock, 0, st>>>(t, g.P, g.W, B->wid.p, B->sel.p, B->sb.p, B->kept.p);
    UGP_HIP_TRY(scan_flags(B->seg, g.P, B->kept.p, B->kb.p, st));
    if (g.EW) k_sbat_eflag<<<blocks_for(g.EW), kBlock, 0, st>>>(t, g.EW, g.W, B->sb.p, B->eflag.p, B->ewid.p);
    UGP_HIP_TRY(scan_flags(B->seg, g.EW, B->eflag.p, B->eb.p, st));
    k_sbat_winfo<<<blocks_for((uint64_t)g.nw + 1), kBlock, 0, st>>>(g.P, g.W, B->sb.p, B->kb.p, B->eb.p, B->koff.p, B->nsel.p, B->gath.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

int bat_list_passes(SubState *S, BatState *B, const Group &g) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const size_t nc = (size_t)g.nw * kCounters;
    UGP_HIP_TRY(hipMemsetAsync(B->ctr.p, 0, nc * sizeof(u64), st));
    UGP_HIP_TRY(hipMemsetAsync(B->kpar.p, 0xff, (size_t)g.nk * sizeof(uint32_t), st));
    k_sbat_list<<<blocks_for(g.P), kBlock, 0, st>>>(t, g.P, g.W, B->wid.p, B->kept.p, B->sb.p, B->kb.p, B->kdfs.p, B->kpar.p, B->kwin.p);
    k_sbat_chains<<<blocks_for(g.nk), kBlock, 0, st>>>(t, g.nk, B->kdfs.p, B->kpar.p, B->kwin.p, B->koff.p, B->ctr.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

int bat_merge_passes(SubState *S, BatState *B, const Group &g, uint64_t chunk) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const uint64_t per = chunk ? chunk : kDefaultChunk;
    const uint32_t G = g.G;
    if (g.RP) k_sbat_rootpath<<<blocks_for(g.nw), kBlock, 0, st>>>(t, g.W, B->koff.p, B->kin.p, B->vin.p);
    for (uint64_t q0 = 0; q0 < g.EW; q0 += per) {
        const uint32_t q1 = (uint32_t)std::min<uint64_t>(g.EW, q0 + per);
        k_sbat_gather<<<blocks_for(q1 - q0), kBlock, 0, st>>>(t, (uint32_t)q0, q1, g.RP, g.W, B->eflag.p, B->eb.p, B->ewid.p, B->kb.p,
                                                             B->kin.p, B->vin.p);
    }
    if (G) UGP_HIP_TRY(sort_pairs(B->tmp, B->kin.p, B->kout.p, B->vin.p, B->vout.p, G, 32 + bits_for(g.nk), st));
    for (uint64_t g0 = 0; g0 < G; g0 += per) {
        const uint32_t g1 = (uint32_t)std::min<uint64_t>(G, g0 + per);
        k_sbat_merge<<<blocks_for(g1 - g0), kBlock, 0, st>>>((uint32_t)g0, g1, G, B->kout.p, B->vout.p, S->mpn.p, t.morig, B->kwin.p,
                                                            B->surv.p, B->sfirst.p, B->snuc.p, B->ctr.p);
    }
    UGP_HIP_TRY(scan_flags(B->seg, G, B->surv.p, B->sv.p, st));
    if (G) k_sbat_compact<<<blocks_for(G), kBlock, 0, st>>>(G, B->kout.p, B->surv.p, B->sv.p, B->sfirst.p, B->snuc.p, B->opos.p, B->ofirst.p,
                                                           B->onuc.p);
    k_sbat_entoff<<<blocks_for((uint64_t)g.nk + 1), kBlock, 0, st>>>(g.nk, G, B->kout.p, B->sv.p, B->eoff.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

struct Answer {   // what a batch returns, built aside and swapped in when every group has run
    std::vector<uint64_t> kept_off, entry_off, ent_off;
    std::vector<ugp_subtree_batch_info> info;
    std::vector<uint32_t> kept_bfs, kept_parent, first;
    std::vector<int32_t> pos;
    std::vector<uint8_t> nuc;
};

struct Timing { uint32_t reps; double nodes_ms, merge_ms; };

// Every group of the batch; `tm`: time each group's passes after it has run.
int bat_run(SubState *S, const char *who, uint64_t ns, const uint64_t *sel_off, const uint32_t *nodes_bfs, uint64_t group_positions,
            uint64_t chunk, Answer *A, Timing *tm) {
    const uint32_t N = S->T->n;
    const uint64_t M = S->T->m;
    if (!ns || !sel_off || !nodes_bfs) return set_error(UGP_ERR_INVALID, std::string(who) + ": no selections given");
    if (ns >= (1ull << 31)) return set_error(UGP_ERR_INVALID, std::string(who) + ": more than 2^31 selections given");
    for (uint64_t b = 0; b < ns; b++) {
        if (sel_off[b + 1] < sel_off[b]) return set_error(UGP_ERR_INVALID, std::string(who) + ": the selection offsets descend at " + std::to_string(b));
        if (sel_off[b + 1] == sel_off[b]) return set_error(UGP_ERR_INVALID, std::string(who) + ": selection " + std::to_string(b) + " is empty");
    }
    const uint64_t first = sel_off[0], nn = sel_off[ns] - first;
    if (nn >= (1ull << 31)) return set_error(UGP_ERR_INVALID, std::string(who) + ": more than 2^31 nodes given");
    for (uint64_t i = 0; i < nn; i++)
        if (nodes_bfs[first + i] >= N) return set_error(UGP_ERR_INVALID, std::string(who) + ": node " + std::to_string(first + i) + " is out of range");
    if (!S->bat) S->bat = new BatState();
    BatState *B = S->bat;
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const std::vector<uint32_t> &d2b = *S->dfs2bfs;
    UGP_HIP_TRY(hipSetDevice(S->device));

    // the windows: smallest and largest rank on the host, the climb on the device
    std::vector<uint32_t> at(nn), lo(ns), hi(ns);
    for (uint64_t b = 0; b < ns; b++) {
        uint32_t a = UINT32_MAX, z = 0;
        for (uint64_t i = sel_off[b] - first; i < sel_off[b + 1] - first; i++) {
            const uint32_t d = at[i] = S->T->bfs2dfs[nodes_bfs[first + i]];
            a = std::min(a, d); z = std::max(z, d);
        }
        lo[b] = a; hi[b] = z;
    }
    UGP_HIP_TRY(B->lo.upload(lo, st));
    UGP_HIP_TRY(B->hi.upload(hi, st));
    UGP_HIP_TRY(B->lca.alloc(ns));
    UGP_HIP_TRY(B->wlen.alloc(ns));
    UGP_HIP_TRY(B->went.alloc(ns));
    UGP_HIP_TRY(B->rpe.alloc(ns));
    k_sbat_lca<<<blocks_for(ns), kBlock, 0, st>>>(t, (uint32_t)ns, B->lo.p, B->hi.p, B->lca.p, B->wlen.p, B->went.p, B->rpe.p);
    UGP_HIP_TRY(hipGetLastError());
    std::vector<uint32_t> lca(ns), wlen(ns), went(ns), rpe(ns);
    UGP_HIP_TRY(hipMemcpyAsync(lca.data(), B->lca.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipMemcpyAsync(wlen.data(), B->wlen.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipMemcpyAsync(went.data(), B->went.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipMemcpyAsync(rpe.data(), B->rpe.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));   // lo and hi are read until here

    // the groups: whole selections while the budgets hold; a selection over a budget runs alone
    const uint64_t pos_budget = std::min<uint64_t>(group_positions ? group_positions : std::max<uint64_t>(N / 2, kBudgetFloor), 1ull << 31);
    const uint64_t ent_budget = std::max<uint64_t>(M / 2, kBudgetFloor);
    std::vector<uint64_t> starts;   // first selection of every group, and ns
    {
        uint64_t P = 0, E = 0;
        for (uint64_t b = 0; b < ns; b++) {
            const uint64_t e = (uint64_t)went[b] + rpe[b];
            if (b == 0 || P + wlen[b] > pos_budget || E + e > ent_budget) { starts.push_back(b); P = E = 0; }
            P += wlen[b]; E += e;
        }
        starts.push_back(ns);
    }
    // every member's concatenated position within its group
    std::vector<uint32_t> cpos(nn);
    for (size_t gi = 0; gi + 1 < starts.size(); gi++) {
        uint32_t P = 0;
        for (uint64_t b = starts[gi]; b < starts[gi + 1]; b++) {
            for (uint64_t i = sel_off[b] - first; i < sel_off[b + 1] - first; i++) cpos[i] = P + (at[i] - lca[b]);
            P += wlen[b];
        }
    }
    UGP_HIP_TRY(B->cpos.upload(cpos, st));

    A->kept_off.assign(ns + 1, 0);
    A->entry_off.assign(ns + 1, 0);
    A->info.assign(ns, ugp_subtree_batch_info{});
    std::vector<uint32_t> offs, koff, nsel, gath, kdfs, eoff;
    std::vector<u64> ctr;
    for (size_t gi = 0; gi + 1 < starts.size(); gi++) {
        const uint64_t b0 = starts[gi], b1 = starts[gi + 1];
        Group g;
        g.nw = (uint32_t)(b1 - b0);
        const size_t row = (size_t)g.nw + 1;
        offs.assign(3 * row, 0);
        for (uint32_t w = 0; w < g.nw; w++) {
            offs[w + 1] = offs[w] + wlen[b0 + w];
            offs[row + w + 1] = offs[row + w] + went[b0 + w];
            offs[2 * row + w + 1] = offs[2 * row + w] + rpe[b0 + w];
        }
        g.P = offs[g.nw]; g.EW = offs[row + g.nw]; g.RP = offs[2 * row + g.nw];
        g.nn = (uint32_t)(sel_off[b1] - sel_off[b0]);
        g.cpos = B->cpos.p + (sel_off[b0] - first);
        UGP_HIP_TRY(B->offs.upload(offs, st));
        g.W = WinView{g.nw, B->lca.p + b0, B->offs.p, B->offs.p + row, B->offs.p + 2 * row};
        UGP_HIP_TRY(B->wid.alloc(g.P));
        UGP_HIP_TRY(B->sel.alloc(g.P));
        UGP_HIP_TRY(B->kept.alloc(g.P));
        UGP_HIP_TRY(B->sb.alloc((size_t)g.P + 1));
        UGP_HIP_TRY(B->kb.alloc((size_t)g.P + 1));
        UGP_HIP_TRY(B->eflag.alloc(g.EW));
        UGP_HIP_TRY(B->ewid.alloc(g.EW));
        UGP_HIP_TRY(B->eb.alloc((size_t)g.EW + 1));
        UGP_HIP_TRY(B->koff.alloc(row));
        UGP_HIP_TRY(B->nsel.alloc(g.nw));
        UGP_HIP_TRY(B->gath.alloc(g.nw));
        UGP_HIP_TRY(B->ctr.alloc((size_t)g.nw * kCounters));
        if (int rc = bat_node_passes(S, B, g)) { (void)hipStreamSynchronize(st); return rc; }
        koff.resize(row); nsel.resize(g.nw); gath.resize(g.nw);
        uint32_t Gw = 0;
        UGP_HIP_TRY(hipMemcpyAsync(koff.data(), B->koff.p, row * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(nsel.data(), B->nsel.p, g.nw * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(gath.data(), B->gath.p, g.nw * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(&Gw, B->eb.p + g.EW, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));   // offs (and, in the first group, cpos) are read until here
        g.nk = koff[g.nw];
        g.G = g.RP + Gw;
        const uint32_t nk = g.nk, G = g.G;
        UGP_HIP_TRY(B->kdfs.alloc(nk));
        UGP_HIP_TRY(B->kpar.alloc(nk));
        UGP_HIP_TRY(B->kwin.alloc(nk));
        UGP_HIP_TRY(B->eoff.alloc((size_t)nk + 1));
        UGP_HIP_TRY(B->kin.alloc(G));
        UGP_HIP_TRY(B->kout.alloc(G));
        UGP_HIP_TRY(B->vin.alloc(G));
        UGP_HIP_TRY(B->vout.alloc(G));
        UGP_HIP_TRY(B->surv.alloc(G));
        UGP_HIP_TRY(B->sfirst.alloc(G));
        UGP_HIP_TRY(B->snuc.alloc(G));
        UGP_HIP_TRY(B->sv.alloc((size_t)G + 1));
        UGP_HIP_TRY(B->opos.alloc(G));
        UGP_HIP_TRY(B->ofirst.alloc(G));
        UGP_HIP_TRY(B->onuc.alloc(G));
        int rc = bat_list_passes(S, B, g);
        if (!rc) rc = bat_merge_passes(S, B, g, chunk);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        const size_t K0 = A->kept_bfs.size(), E0 = A->pos.size();
        kdfs.resize(nk); eoff.resize((size_t)nk + 1); ctr.resize((size_t)g.nw * kCounters);
        A->kept_parent.resize(K0 + nk);
        if (nk) {
            UGP_HIP_TRY(hipMemcpyAsync(kdfs.data(), B->kdfs.p, (size_t)nk * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(A->kept_parent.data() + K0, B->kpar.p, (size_t)nk * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        UGP_HIP_TRY(hipMemcpyAsync(eoff.data(), B->eoff.p, ((size_t)nk + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(ctr.data(), B->ctr.p, ctr.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        const uint32_t E = eoff[nk];
        A->pos.resize(E0 + E); A->first.resize(E0 + E); A->nuc.resize(E0 + E);
        if (E) {
            UGP_HIP_TRY(hipMemcpyAsync(A->pos.data() + E0, B->opos.p, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(A->first.data() + E0, B->ofirst.p, (size_t)E * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(A->nuc.data() + E0, B->onuc.p, E, hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipStreamSynchronize(st));
        }
        A->kept_bfs.resize(K0 + nk); A->ent_off.resize(K0 + nk);
        for (uint32_t k = 0; k < nk; k++) { A->kept_bfs[K0 + k] = d2b[kdfs[k]]; A->ent_off[K0 + k] = E0 + eoff[k]; }
        for (uint32_t w = 0; w < g.nw; w++) {
            const uint64_t b = b0 + w;
            const u64 *c = ctr.data() + (size_t)w * kCounters;
            A->kept_off[b] = K0 + koff[w];
            A->entry_off[b] = E0 + eoff[koff[w]];
            ugp_subtree_batch_info &I = A->info[b];
            I.n_selected = nsel[w];
            I.n_kept = koff[w + 1] - koff[w];
            I.n_entries = eoff[koff[w + 1]] - eoff[koff[w]];
            I.n_gathered = gath[w];
            I.n_disagree = c[kDisagree];
            I.longest_chain = c[kLongest];
            I.first_disagree = c[kDisagree] ? d2b[kdfs[(uint32_t)~c[kFirstDisagree]]] : UINT32_MAX;
            I.lca = d2b[lca[b]];
        }
        if (tm) {
            double nodes_ms = 0, merge_ms = 0;   // of this group
            if (int r2 = timed(S->stream, "ugp_subtree_batch_time", tm->reps, &nodes_ms,
                               [&] { const int c = bat_node_passes(S, B, g); return c ? c : bat_list_passes(S, B, g); })) return r2;
            if (int r2 = timed(S->stream, "ugp_subtree_batch_time", tm->reps, &merge_ms, [&] { return bat_merge_passes(S, B, g, chunk); })) return r2;
            tm->nodes_ms += nodes_ms;
            tm->merge_ms += merge_ms;
        }
    }
    A->kept_off[ns] = A->kept_bfs.size();
    A->entry_off[ns] = A->pos.size();
    return UGP_OK;
}

int bat_ready(SubState *S, const char *who) { return query_ready(S, who, "subtree"); }

int bat_answered(SubState *S, const char *who) {
    if (int rc = bat_ready(S, who)) return rc;
    if (!S->bat || !S->bat->have) return set_error(UGP_ERR_INVALID, std::string(who) + ": no batch: call ugp_subtree_batch first");
    return UGP_OK;
}

}  // namespace

int sub_batch(SubState *S, uint64_t n_sel, const uint64_t *sel_off, const uint32_t *nodes_bfs, uint64_t *kept_off, uint64_t *entry_off,
              ugp_subtree_batch_info *info, uint64_t group_positions, uint64_t chunk_items) {
    if (int rc = bat_ready(S, "ugp_subtree_batch")) return rc;
    if (!kept_off || !entry_off) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        Answer A;
        if (int rc = bat_run(S, "ugp_subtree_batch", n_sel, sel_off, nodes_bfs, group_positions, chunk_items, &A, nullptr)) return rc;
        BatState *B = S->bat;
        std::copy(A.kept_off.begin(), A.kept_off.end(), kept_off);
        std::copy(A.entry_off.begin(), A.entry_off.end(), entry_off);
        if (info) std::copy(A.info.begin(), A.info.end(), info);
        B->kept_bfs.swap(A.kept_bfs); B->kept_parent.swap(A.kept_parent); B->ent_off.swap(A.ent_off);
        B->pos.swap(A.pos); B->first.swap(A.first); B->nuc.swap(A.nuc);
        B->have = true;
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

int sub_batch_nodes(SubState *S, uint32_t *kept_bfs, uint32_t *kept_parent, uint64_t *ent_off, uint64_t cap, uint64_t *n_out) {
    if (int rc = bat_answered(S, "ugp_subtree_batch_nodes")) return rc;
    if (!n_out || (cap && (!kept_bfs || !kept_parent || !ent_off))) return set_error(UGP_ERR_INVALID, "null argument");
    const BatState *B = S->bat;
    const size_t w = (size_t)std::min<uint64_t>(cap, B->kept_bfs.size());
    std::copy_n(B->kept_bfs.begin(), w, kept_bfs);
    std::copy_n(B->kept_parent.begin(), w, kept_parent);
    std::copy_n(B->ent_off.begin(), w, ent_off);
    *n_out = B->kept_bfs.size();
    return UGP_OK;
}

int sub_batch_entries(SubState *S, int32_t *pos, uint32_t *first_entry, uint8_t *nuc, uint64_t cap, uint64_t *n_out) {
    if (int rc = bat_answered(S, "ugp_subtree_batch_entries")) return rc;
    if (!n_out || (cap && (!pos || !first_entry || !nuc))) return set_error(UGP_ERR_INVALID, "null argument");
    const BatState *B = S->bat;
    const size_t w = (size_t)std::min<uint64_t>(cap, B->pos.size());
    std::copy_n(B->pos.begin(), w, pos);
    std::copy_n(B->first.begin(), w, first_entry);
    std::copy_n(B->nuc.begin(), w, nuc);
    *n_out = B->pos.size();
    return UGP_OK;
}

int sub_batch_time(SubState *S, uint64_t n_sel, const uint64_t *sel_off, const uint32_t *nodes_bfs, uint32_t reps, double *nodes_ms,
                   double *merge_ms) {
    if (int rc = bat_ready(S, "ugp_subtree_batch_time")) return rc;
    if (!reps || !nodes_ms || !merge_ms) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        Answer A;
        Timing tm{reps, 0, 0};
        if (int rc = bat_run(S, "ugp_subtree_batch_time", n_sel, sel_off, nodes_bfs, 0, 0, &A, &tm)) return rc;
        *nodes_ms = tm.nodes_ms;
        *merge_ms = tm.merge_ms;
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

}  // namespace ugp
