// ugp_relatives.hip -- get_closest_samples (matUtils select.cpp:577-714) for a batch of samples on the device.
//
// The reference, per sample t: climb p_0 = parent(t), p_1, ...; at level j walk every child of p_j but the one the climb came
// from (c_j; c_0 = t) and collect the leaves below them with their path length to t.  On the depth-first tables (ugp_dense.hpp)
// the leaves collected at level j -- the RING -- are the leaf positions of [p_j, dend[p_j]) outside [c_j, dend[c_j]): two ranges
// of leaf ranks, and a ring leaf l is cum[t] + cum[l] - 2 cum[p_j] away.  The level bound is L_j = cum[p_0] - cum[p_j] + nm[p_j]
// (nm[t] is left out, as the reference leaves it out).
//   closest (fixed_k = false): the ring's smallest distance m_j; a strictly smaller one replaces the list, an equal one appends;
//     the climb stops after the first level with m_j < L_j.  The reference's pruning never changes the list.
//   within  (fixed_k = true, threshold k): the ring leaves at distance <= k, level by level; stops after the first L_j > k.
// Tables made at attach, all on the device:
//   lpre            prefix count of the leaf flags (scan_flags, ugp_scan.hpp): the leaf ranks of a depth-first range;
//   lcum + rc       cum of the leaves in depth-first order with a range minimum over it: minima of blocks of UGP_REL_BLOCK
//                   leaves, prefix / suffix minima inside the blocks and a sparse table over the block minima;
//   srank/sbfs/boff the leaf ranks ordered by (cum, rank), their breadth-first indices, the first slot of every cum value: the
//                   leaves of one rank range at one cum value are a slice found by two binary searches, in depth-first order;
//   snr + rn        the name ranks in that order with a second range minimum: the smallest name of a slice is one query.
// Kernels: k_rel_closest / k_rel_within (one lane per sample: the climb, the counts, the smallest rank), k_rel_scan (the 64-bit
// prefix over the counts), k_rel_fill (one wave per sample climbs again and copies the slices; within mode restores depth-first
// order inside a ring range by ranking each element against the other slices).  No pass reads a ring leaf by leaf.
// Samples run in chunks, and a chunk's lists leave the device in windows, so the workspace stays bounded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_relatives.hpp"
#include "ugp_sort.hpp"

namespace ugp {
namespace {

constexpr uint32_t kRB = UGP_REL_BLOCK;   // leaves per block of the range minima
constexpr uint32_t kScanTile = 8;         // values per thread of the scans

struct Rmq {   // range minimum over val[0, n)
    const uint32_t *val, *pre, *suf;   // pre[i] = min of val[block start .. i], suf[i] = min of val[i .. block end)
    const uint32_t *sp;                // sp[l * nb + b] = min over the blocks [b, b + 2^l)
    uint32_t n, nb;
};

struct RelView {
    uint32_t n, nl, maxcum;
    const uint32_t *dpar, *dend, *cum, *lpre;
    const uint32_t *srank, *sbfs, *boff;
    const uint32_t *rank2bfs;   // null: no name ranks
    Rmq rc, rn;
};

// min of val[a, b); kNil for an empty range.  At most kRB values are read one by one (a range inside one block).
__device__ __forceinline__ uint32_t rmq_min(const Rmq &r, uint32_t a, uint32_t b) {
    if (a >= b) return kNil;
    const uint32_t ba = a / kRB, bb = (b - 1) / kRB;
    if (ba == bb) {
        if (a % kRB == 0) return r.pre[b - 1];
        if (b % kRB == 0 || b == r.n) return r.suf[a];
        uint32_t m = r.val[a];
        for (uint32_t i = a + 1; i < b; i++) m = min(m, r.val[i]);
        return m;
    }
    uint32_t m = min(r.suf[a], r.pre[b - 1]);
    if (bb - ba > 1) {
        const uint32_t l = 31u - (uint32_t)__clz((int)(bb - ba - 1));
        const uint32_t *row = r.sp + (size_t)l * r.nb;
        m = min(m, min(row[ba + 1], row[bb - (1u << l)]));
    }
    return m;
}

// The slots [*lo, *hi) of the (cum, rank) order that hold the leaves of ranks [a, b) with cum == c.
__device__ __forceinline__ void rel_slice(const RelView &v, uint32_t c, uint32_t a, uint32_t b, uint32_t *lo, uint32_t *hi) {
    const uint32_t s0 = v.boff[c], s1 = v.boff[c + 1];
    *lo = lower_bound_u32(v.srank, s0, s1, a);
    *hi = lower_bound_u32(v.srank, *lo, s1, b);
}

// Leaves of rank < x with cmin <= cum <= cmax.
__device__ __forceinline__ uint32_t rel_below(const RelView &v, uint32_t cmin, uint32_t cmax, uint32_t x) {
    uint32_t s = 0;
    for (uint32_t c = cmin; c <= cmax; c++) { const uint32_t s0 = v.boff[c]; s += lower_bound_u32(v.srank, s0, v.boff[c + 1], x) - s0; }
    return s;
}

struct Climb {   // one sample on its way up
    uint32_t tc, cp0;    // cum[t], cum[p_0]
    uint32_t c, p;       // c_j, p_j (depth-first positions); p = kNil: past the root
    uint32_t cp, L;      // cum[p_j], L_j
    uint32_t a[2], b[2]; // the ring's two ranges of leaf ranks
};

__device__ __forceinline__ void climb_start(const RelView &v, uint32_t t, Climb *s) {
    s->tc = v.cum[t];
    s->c = t;
    s->p = v.dpar[t];
    s->cp0 = s->p != kNil ? v.cum[s->p] : 0;
}
// Fills the level's fields; `up` then moves to the next level.
__device__ __forceinline__ uint32_t climb_level(const RelView &v, Climb *s) {
    const uint32_t gp = v.dpar[s->p];
    s->cp = v.cum[s->p];
    s->L = s->cp0 - s->cp + (s->cp - (gp != kNil ? v.cum[gp] : 0));
    s->a[0] = v.lpre[s->p]; s->b[0] = v.lpre[s->c];
    s->a[1] = v.lpre[v.dend[s->c]]; s->b[1] = v.lpre[v.dend[s->p]];
    return gp;
}
__device__ __forceinline__ void climb_up(Climb *s, uint32_t gp) { s->c = s->p; s->p = gp; }

// Within mode: the cum values [*cmin, *cmax] of range r that are admissible at this level and present; false: none.
__device__ __forceinline__ bool within_span(const RelView &v, const Climb &s, uint32_t k, uint32_t r, uint32_t *cmin, uint32_t *cmax) {
    const long long bound = 2ll * (long long)s.cp + (long long)k - (long long)s.tc;
    if (bound < (long long)s.cp) return false;
    const uint32_t m = rmq_min(v.rc, s.a[r], s.b[r]);
    if (m == kNil || (long long)m > bound) return false;
    *cmin = m;
    *cmax = (uint32_t)min(bound, (long long)v.maxcum);
    return true;
}

__global__ void __launch_bounds__(kBlock) k_rel_closest(RelView v, const uint32_t *node, uint32_t ns, ugp_rel_info *info, uint32_t *cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    Climb s;
    climb_start(v, node[i], &s);
    uint32_t best = kNil, count = 0, rank = kNil, levels = 0;
    while (s.p != kNil) {
        const uint32_t gp = climb_level(v, &s);
        levels++;
        const uint32_t m = min(rmq_min(v.rc, s.a[0], s.b[0]), rmq_min(v.rc, s.a[1], s.b[1]));
        if (m != kNil) {
            const uint32_t d = s.tc + m - 2 * s.cp;
            if (d <= best) {
                if (d < best) { best = d; count = 0; rank = kNil; }
                for (uint32_t r = 0; r < 2; r++) {
                    if (s.a[r] >= s.b[r]) continue;
                    uint32_t lo, hi;
                    rel_slice(v, m, s.a[r], s.b[r], &lo, &hi);
                    count += hi - lo;
                    if (v.rank2bfs) rank = min(rank, rmq_min(v.rn, lo, hi));
                }
            }
            if (d < s.L) break;
        }
        climb_up(&s, gp);
    }
    ugp_rel_info o;
    o.dist = count ? best : 0;
    o.count = count;
    o.levels = levels;
    o.best = (count && v.rank2bfs) ? v.rank2bfs[rank] : kNil;
    info[i] = o;
    cnt[i] = count;
}

__global__ void __launch_bounds__(kBlock) k_rel_within(RelView v, const uint32_t *node, uint32_t ns, uint32_t k, ugp_rel_info *info, uint32_t *cnt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    Climb s;
    climb_start(v, node[i], &s);
    uint32_t count = 0, levels = 0;
    while (s.p != kNil) {
        const uint32_t gp = climb_level(v, &s);
        levels++;
        for (uint32_t r = 0; r < 2; r++) {
            uint32_t cmin, cmax;
            if (!within_span(v, s, k, r, &cmin, &cmax)) continue;
            count += rel_below(v, cmin, cmax, s.b[r]) - rel_below(v, cmin, cmax, s.a[r]);
        }
        if (s.L > k) break;
        climb_up(&s, gp);
    }
    ugp_rel_info o;
    o.dist = 0;
    o.count = count;
    o.levels = levels;
    o.best = kNil;
    info[i] = o;
    cnt[i] = count;
}

// off[i] = cnt[0] + ... + cnt[i - 1] in 64 bits, off[ns] = all.  One block; a thread scans kScanTile values.
__global__ void __launch_bounds__(kBlock) k_rel_scan(const uint32_t *cnt, uint32_t ns, unsigned long long *off) {
    __shared__ unsigned long long sh[kBlock / 64];
    unsigned long long carry = 0;
    for (uint64_t t0 = 0; t0 < ns; t0 += (uint64_t)kBlock * kScanTile) {
        const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kScanTile;
        uint32_t f[kScanTile];
        unsigned long long sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kScanTile; j++) { f[j] = i0 + j < ns ? cnt[i0 + j] : 0u; sum += f[j]; }
        unsigned long long tot;
        unsigned long long run = carry + block_incl_scan(sum, sh, &tot) - sum;
#pragma unroll
        for (uint32_t j = 0; j < kScanTile; j++) { if (i0 + j < ns) off[i0 + j] = run; run += f[j]; }
        carry += tot;
    }
    if (threadIdx.x == 0) off[ns] = carry;
}

// One wave per sample: the climb again over the `levels` the first pass took, and the slices of every level to
// out[off[s] - w0 ..] for the part of the list inside the window [w0, w0 + wlen).
template <bool Within>
__global__ void __launch_bounds__(kBlock) k_rel_fill(RelView v, const uint32_t *node, const ugp_rel_info *info, const unsigned long long *off,
                                                     uint32_t ns, uint32_t k, unsigned long long w0, unsigned long long wlen, uint32_t *out) {
    const uint32_t i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= ns) return;
    unsigned long long o = off[i];
    const unsigned long long end = off[i + 1], w1 = w0 + wlen;
    if (o == end || end <= w0 || o >= w1) return;
    const ugp_rel_info f = info[i];
    Climb s;
    climb_start(v, node[i], &s);
    for (uint32_t lv = 0; lv < f.levels && o < w1; lv++) {
        const uint32_t gp = climb_level(v, &s);
        for (uint32_t r = 0; r < 2; r++) {
            uint32_t cmin, cmax;
            if (Within) {
                if (!within_span(v, s, k, r, &cmin, &cmax)) continue;
            } else {   // the leaves at the final distance: one cum value
                const long long c = (long long)f.dist - (long long)s.tc + 2ll * (long long)s.cp;
                if (s.a[r] >= s.b[r] || c < (long long)s.cp || c > (long long)v.maxcum) continue;
                cmin = cmax = (uint32_t)c;
            }
            const uint32_t below = rel_below(v, cmin, cmax, s.a[r]);
            const uint32_t tot = rel_below(v, cmin, cmax, s.b[r]) - below;
            if (tot && o + tot > w0 && o < w1) {
                for (uint32_t c = cmin; c <= cmax; c++) {
                    uint32_t lo, hi;
                    rel_slice(v, c, s.a[r], s.b[r], &lo, &hi);
                    for (uint32_t e = lo + lane; e < hi; e += 64) {
                        const uint32_t pos = cmin == cmax ? e - lo : rel_below(v, cmin, cmax, v.srank[e]) - below;
                        const unsigned long long g = o + pos;
                        if (g >= w0 && g < w1) out[g - w0] = v.sbfs[e];
                    }
                }
            }
            o += tot;
        }
        climb_up(&s, gp);
    }
}

// ---- the tables ---------------------------------------------------------------------------------------------------------

// The leaves in depth-first order: their cum, their breadth-first index, and the identity for the sort.
__global__ void k_rel_leaves(uint32_t n, const uint8_t *leaf, const uint32_t *lpre, const uint32_t *cum, const uint32_t *d2b, uint32_t *lcum,
                             uint32_t *lbfs, uint32_t *iota) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !leaf[i]) return;
    const uint32_t r = lpre[i];
    lcum[r] = cum[i]; lbfs[r] = d2b[i]; iota[r] = r;
}

// boff[c] = the first slot of the sorted keys with key >= c, for c in [0, nc).
__global__ void k_rel_boff(const uint32_t *skey, uint32_t nl, uint32_t nc, uint32_t *boff) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < nc) boff[c] = lower_bound_u32(skey, 0, nl, c);
}

__global__ void k_rel_sorted(uint32_t nl, const uint32_t *srank, const uint32_t *lbfs, const uint32_t *name_rank, uint32_t *sbfs, uint32_t *snr) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nl) return;
    const uint32_t b = lbfs[srank[s]];
    sbfs[s] = b;
    if (name_rank) snr[s] = name_rank[b];
}

__global__ void k_rel_invert(uint32_t n, const uint32_t *name_rank, uint32_t *rank2bfs) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) rank2bfs[name_rank[b]] = b;
}

// One lane per block of kRB values: the prefix / suffix minima inside it and its minimum (level 0 of the sparse table).
__global__ void k_rel_rmq_blocks(uint32_t n, uint32_t nb, const uint32_t *val, uint32_t *pre, uint32_t *suf, uint32_t *sp) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint32_t lo = b * kRB, hi = min(n, lo + kRB);
    uint32_t m = kNil;
    for (uint32_t i = lo; i < hi; i++) { m = min(m, val[i]); pre[i] = m; }
    m = kNil;
    for (uint32_t i = hi; i-- > lo;) { m = min(m, val[i]); suf[i] = m; }
    sp[b] = m;
}

// Level l >= 1 of the sparse table from level l - 1 (entries whose span leaves the table are never read).
__global__ void k_rel_rmq_level(uint32_t nb, uint32_t l, uint32_t *sp) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t half = 1u << (l - 1);
    if (b + 2 * half > nb) return;
    const uint32_t *below = sp + (size_t)(l - 1) * nb;
    sp[(size_t)l * nb + b] = min(below[b], below[b + half]);
}

struct RmqBufs {
    DBuf<uint32_t> pre, suf, sp;
    uint32_t nb = 0;
    hipError_t build(const uint32_t *val, uint32_t n, hipStream_t st) {
        nb = (n + kRB - 1) / kRB;
        uint32_t levels = 1;
        while ((2u << (levels - 1)) <= nb) levels++;
        hipError_t e = pre.alloc(n);
        if (e == hipSuccess) e = suf.alloc(n);
        if (e == hipSuccess) e = sp.alloc((size_t)levels * std::max(nb, 1u));
        if (e != hipSuccess || !n) return e;
        k_rel_rmq_blocks<<<blocks_for(nb), kBlock, 0, st>>>(n, nb, val, pre.p, suf.p, sp.p);
        for (uint32_t l = 1; l < levels; l++) k_rel_rmq_level<<<blocks_for(nb), kBlock, 0, st>>>(nb, l, sp.p);
        return hipGetLastError();
    }
    Rmq view(const uint32_t *val, uint32_t n) const { return Rmq{val, pre.p, suf.p, sp.p, n, nb}; }
};

}  // namespace

struct RelState : QueryBase {
    uint32_t nl = 0, maxcum = 0;
    bool ranks = false;
    DBuf<uint32_t> lpre, lcum, srank, sbfs, boff, snr, rank2bfs;
    RmqBufs rc, rn;
    // per call
    DBuf<uint32_t> qnode, cnt, win;
    DBuf<ugp_rel_info> info;
    DBuf<unsigned long long> off;
    RelView view() const {
        return RelView{T->n, nl, maxcum, T->dpar.p, T->dend.p, T->cum.p, lpre.p, srank.p, sbfs.p, boff.p, ranks ? rank2bfs.p : nullptr,
                       rc.view(lcum.p, nl), rn.view(snr.p, ranks ? nl : 0)};
    }
};

void rel_free(RelState *s) { query_free(s); }

static int rel_build(RelState *S, const std::vector<uint32_t> &dfs2bfs, const uint32_t *name_rank) {
    const DfsTables &T = *S->T;
    const uint32_t n = T.n;
    hipStream_t st = S->stream;
    S->maxcum = *std::max_element(T.h_cum.begin(), T.h_cum.end());
    DBuf<uint32_t> d2b, lbfs, iota, skey, nrank, seg;
    DBuf<unsigned char> tmp;
    UGP_HIP_TRY(S->lpre.alloc((size_t)n + 1));
    UGP_HIP_TRY(d2b.upload(dfs2bfs.data(), n, st));
    UGP_HIP_TRY(scan_flags(seg, n, T.leaf.p, S->lpre.p, st));
    UGP_HIP_TRY(hipMemcpyAsync(&S->nl, S->lpre.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));
    const uint32_t nl = S->nl;   // at least one: the last position of a depth-first order is a leaf
    UGP_HIP_TRY(S->lcum.alloc(nl)); UGP_HIP_TRY(lbfs.alloc(nl)); UGP_HIP_TRY(iota.alloc(nl)); UGP_HIP_TRY(skey.alloc(nl));
    UGP_HIP_TRY(S->srank.alloc(nl)); UGP_HIP_TRY(S->sbfs.alloc(nl)); UGP_HIP_TRY(S->boff.alloc((size_t)S->maxcum + 2));
    k_rel_leaves<<<blocks_for(n), kBlock, 0, st>>>(n, T.leaf.p, S->lpre.p, T.cum.p, d2b.p, S->lcum.p, lbfs.p, iota.p);
    UGP_HIP_TRY(hipGetLastError());
    // a radix sort is stable: equal cum values keep their depth-first order
    UGP_HIP_TRY(sort_pairs(tmp, S->lcum.p, skey.p, iota.p, S->srank.p, nl, bits_for(S->maxcum), st));
    k_rel_boff<<<blocks_for((uint64_t)S->maxcum + 2), kBlock, 0, st>>>(skey.p, nl, S->maxcum + 2, S->boff.p);
    if (name_rank) {
        UGP_HIP_TRY(nrank.upload(name_rank, n, st));
        UGP_HIP_TRY(S->snr.alloc(nl)); UGP_HIP_TRY(S->rank2bfs.alloc(n));
        k_rel_invert<<<blocks_for(n), kBlock, 0, st>>>(n, nrank.p, S->rank2bfs.p);
    }
    k_rel_sorted<<<blocks_for(nl), kBlock, 0, st>>>(nl, S->srank.p, lbfs.p, name_rank ? nrank.p : nullptr, S->sbfs.p, S->snr.p);
    UGP_HIP_TRY(hipGetLastError());
    UGP_HIP_TRY(S->rc.build(S->lcum.p, nl, st));
    if (name_rank) UGP_HIP_TRY(S->rn.build(S->snr.p, nl, st));
    S->ranks = name_rank != nullptr;
    UGP_HIP_TRY(hipStreamSynchronize(st));   // the temporaries and the caller's ranks are read until here
    return UGP_OK;
}

int rel_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               const uint32_t *name_rank, DfsTables **tables, RelState **out) {
    return query_attach(
        "ugp_relatives_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out,
        [&](const DfsTables &T) {
            std::vector<uint8_t> seen(name_rank ? T.n : 0, 0);
            for (uint32_t j = 0; j < seen.size(); j++) {
                if (name_rank[j] >= T.n || seen[name_rank[j]]) return set_error(UGP_ERR_INVALID, "name_rank is not a permutation of 0 .. n - 1");
                seen[name_rank[j]] = 1;
            }
            return (int)UGP_OK;
        },
        [&](RelState *S) { return rel_build(S, dfs2bfs, name_rank); });
}

int rel_run(RelState *S, bool within, uint64_t n, const uint32_t *nodes, uint32_t k, ugp_rel_info *info, uint64_t *out_off,
            uint32_t *out_nodes, uint64_t cap, uint64_t *n_out, uint32_t chunk_samples, double *kernel_ms) {
    const char *who = within ? "ugp_relatives_within" : "ugp_relatives_closest";
    if (int rc = query_ready(S, who, "relatives")) return rc;
    if (!n_out || (n && !nodes) || (n && !info && !kernel_ms) || (out_off && cap && !out_nodes)) return set_error(UGP_ERR_INVALID, "null argument");
    const uint32_t N = S->T->n;
    for (uint64_t i = 0; i < n; i++)
        if (nodes[i] >= N) return set_error(UGP_ERR_INVALID, "node index out of range");
    const bool lists = out_off != nullptr || kernel_ms != nullptr;
    // workspace bounds of one chunk: samples, and list entries per window of the fill
    const uint64_t chunk = std::min<uint64_t>(chunk_samples ? chunk_samples : (1u << 20), 1u << 20);
    const uint64_t window = 16 * chunk;
    uint64_t base = 0;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0;
    try {
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        const RelView v = S->view();
        const std::vector<uint32_t> &b2d = S->T->bfs2dfs;
        const uint64_t most = std::min<uint64_t>(chunk, std::max<uint64_t>(n, 1));
        UGP_HIP_TRY(S->qnode.alloc(most)); UGP_HIP_TRY(S->cnt.alloc(most)); UGP_HIP_TRY(S->info.alloc(most)); UGP_HIP_TRY(S->off.alloc(most + 1));
        EventPair ev(st);
        if (kernel_ms) UGP_HIP_TRY(ev.create());
        std::vector<uint32_t> qn;
        std::vector<ugp_rel_info> hinfo;
        std::vector<unsigned long long> hoff;
        for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
            const uint32_t nc = (uint32_t)std::min<uint64_t>(chunk, n - c0);
            qn.resize(nc);
            for (uint32_t i = 0; i < nc; i++) qn[i] = b2d[nodes[c0 + i]];
            UGP_HIP_TRY(S->qnode.upload(qn, st));
            if (kernel_ms) UGP_HIP_TRY(ev.start());
            if (within) k_rel_within<<<blocks_for(nc), kBlock, 0, st>>>(v, S->qnode.p, nc, k, S->info.p, S->cnt.p);
            else k_rel_closest<<<blocks_for(nc), kBlock, 0, st>>>(v, S->qnode.p, nc, S->info.p, S->cnt.p);
            if (lists) k_rel_scan<<<1, kBlock, 0, st>>>(S->cnt.p, nc, S->off.p);
            UGP_HIP_TRY(hipGetLastError());
            if (kernel_ms) UGP_HIP_TRY(ev.lap(&kernel_ms[0]));
            uint64_t tot = 0;
            if (!kernel_ms) {
                hinfo.resize(nc);
                UGP_HIP_TRY(hipMemcpyAsync(hinfo.data(), S->info.p, nc * sizeof(ugp_rel_info), hipMemcpyDeviceToHost, st));
            }
            if (lists) {
                hoff.resize(kernel_ms ? 1 : (size_t)nc + 1);
                const size_t first = kernel_ms ? nc : 0;
                UGP_HIP_TRY(hipMemcpyAsync(hoff.data(), S->off.p + first, hoff.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            }
            UGP_HIP_TRY(hipStreamSynchronize(st));
            if (!kernel_ms) std::copy(hinfo.begin(), hinfo.end(), info + c0);
            if (lists) {
                tot = hoff.back();
                if (out_off) for (uint32_t i = 0; i < nc; i++) out_off[c0 + i] = base + hoff[i];
            } else {
                for (uint32_t i = 0; i < nc; i++) tot += hinfo[i].count;
            }
            // the chunk's lists, window by window; only what lies below cap leaves the device
            if (lists && tot) UGP_HIP_TRY(S->win.alloc(std::min<uint64_t>(window, tot)));
            for (uint64_t w0 = 0; lists && w0 < tot; w0 += window) {
                if (!kernel_ms && base + w0 >= cap) break;
                const uint64_t wl = std::min<uint64_t>(window, tot - w0);
                const uint32_t grid = (nc + kBlock / 64 - 1) / (kBlock / 64);
                if (kernel_ms) UGP_HIP_TRY(ev.start());
                if (within) k_rel_fill<true><<<grid, kBlock, 0, st>>>(v, S->qnode.p, S->info.p, S->off.p, nc, k, w0, wl, S->win.p);
                else k_rel_fill<false><<<grid, kBlock, 0, st>>>(v, S->qnode.p, S->info.p, S->off.p, nc, k, w0, wl, S->win.p);
                UGP_HIP_TRY(hipGetLastError());
                if (kernel_ms) { UGP_HIP_TRY(ev.lap(&kernel_ms[1])); continue; }
                const uint64_t take = std::min<uint64_t>(wl, cap - (base + w0));
                UGP_HIP_TRY(hipMemcpyAsync(out_nodes + base + w0, S->win.p, take * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                UGP_HIP_TRY(hipStreamSynchronize(st));
            }
            base += tot;
        }
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    if (out_off) out_off[n] = base;
    *n_out = base;
    return UGP_OK;
}

}  // namespace ugp
