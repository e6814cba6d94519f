// ugp_nearest.hip -- get_nearby (matUtils select.cpp:206-276) for a batch of queries on the device.
//
// The reference, per query (node, k): climb rsearch(node, true); last_anc = the last ancestor with <= k leaves (the node itself
// to begin with), anc = the first with more.  No such ancestor: the result is empty.  Otherwise the result is the leaves of
// last_anc, then the leaves l under anc with !is_ancestor(last_anc, l) -- is_ancestor starts at the parent, so only the STRICT
// descendants of last_anc are left out: a leaf last_anc is a candidate of its own search -- ascending by the number of mutation
// entries between l and anc, until k names are held.  When anc == last_anc (the node itself has more than k leaves) every leaf is
// left out and the result is all leaves of the node.
//
// On the depth-first tables (ugp_dense.hpp) the leaves of v are the leaf positions of [v, dend[v]), their number is
// lpre[dend[v]] - lpre[v] with lpre the prefix count of the leaf flags, and the distance is cum[l] - cum[anc].  So a query is "the
// `need` smallest keys cum[i] - cum[anc] over the leaf positions of [anc, dend[anc]) outside (last_anc, dend[last_anc])", ties by
// position (what a stable sort gives; the reference's std::sort leaves them to introsort):
//   (scan_flags, ugp_scan.hpp)   attach: lpre;
//   k_nk_anchor   one lane per query climbs dpar;
//   k_nk_hist     one block per (segment of kSeg positions, query) that overlaps the range: an LDS histogram of one 11-bit key
//                 digit, flushed to the query's global histogram;  k_nk_pick finds the bin that holds the need-th key.
//                 The first pass takes the LOW digit of the keys below 2^11: distances are small, so it is the only pass
//                 unless fewer than `need` keys are that small; then the digit moves up (keys below 2^22, then all) until the
//                 bin is found, and back down inside that bin: one pass, three or five;
//   k_nk_count / k_nk_offsets / k_nk_write   per-(query, segment) counts, a prefix over each query's segments, and the
//                 compaction: leaves of last_anc, keys < d*, and the first keys == d* in depth-first order, with their keys;
//   k_nk_sort     one block per query orders its candidates by (key, position): bitonic in LDS up to 4096 pairs, the same
//                 network over a global scratch for more;  k_nk_tobfs renumbers.
// Queries run in chunks, so the histograms, work lists and output rows on the device stay bounded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_nearest.hpp"

namespace ugp {
namespace {

constexpr uint32_t kBins = 2048;        // one 11-bit digit
constexpr uint32_t kDigit = 11;
constexpr uint32_t kSortLds = 4096;     // pairs the LDS sort takes

struct NkQ {
    uint32_t anc, last;        // depth-first positions; anc = kNil: empty result
    uint32_t lo, hi;           // [anc, dend[anc])
    uint32_t xlo, xhi;         // the strict descendants of last_anc
    uint32_t base;             // cum[anc]
    uint32_t nlast;            // leaves of last_anc
    uint32_t need;             // candidates to take
    uint32_t shift, prefix;    // the pass bins (key >> shift) & 2047 of the keys with key >> (shift + 11) == prefix
    uint32_t below;            // candidates known to lie below every key of the current prefix
    uint32_t done;
    uint32_t cut, n_at_cut, take;   // d*, candidates at d*, how many of them are taken
};

struct NkItem { uint32_t q, seg; };

__global__ void k_nk_anchor(DfsView t, const uint32_t *lpre, const uint32_t *node, const uint32_t *k, uint32_t nq, NkQ *Q) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const uint32_t kk = k[q];
    uint32_t last = node[q], a = last;
    while (a != kNil && lpre[t.dend[a]] - lpre[a] <= kk) { last = a; a = t.dpar[a]; }
    NkQ s;
    s.anc = a; s.last = last;
    s.nlast = lpre[t.dend[last]] - lpre[last];
    s.xlo = last + 1; s.xhi = t.dend[last];
    s.shift = 0; s.prefix = 0; s.below = 0; s.cut = 0; s.n_at_cut = 0; s.take = 0;
    if (a == kNil) { s.lo = s.hi = 0; s.base = 0; s.need = 0; }
    else { s.lo = a; s.hi = t.dend[a]; s.base = t.cum[a]; s.need = a == last ? 0 : kk - s.nlast; }
    s.done = s.need == 0 ? 1 : 0;
    Q[q] = s;
}

__device__ __forceinline__ bool nk_candidate(const DfsView &t, const NkQ &s, uint32_t i) {
    return t.leaf[i] && !(i >= s.xlo && i < s.xhi);
}

__global__ void __launch_bounds__(kBlock) k_nk_hist(DfsView t, const NkQ *Q, const NkItem *work, uint32_t *hist) {
    __shared__ uint32_t h[kBins];
    const NkItem w = work[blockIdx.x];
    const NkQ s = Q[w.q];
    if (s.done) return;
    for (uint32_t b = threadIdx.x; b < kBins; b += kBlock) h[b] = 0;
    __syncthreads();
    const uint32_t lo = max(s.lo, w.seg * kSeg), hi = min(s.hi, w.seg * kSeg + kSeg);
    const uint32_t up = s.shift + kDigit, lane = threadIdx.x & 63;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        bool c = false;
        uint32_t d = 0;
        if (i < hi && nk_candidate(t, s, i)) {
            const uint32_t key = t.cum[i] - s.base;
            if (up >= 32 || (key >> up) == s.prefix) { c = true; d = (key >> s.shift) & (kBins - 1); }
        }
        // a polytomy puts a whole wave into one bin: one add of the lane count then
        const unsigned long long m = __ballot(c);
        if (!m) continue;
        const uint32_t first = (uint32_t)__ffsll((long long)m) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)d, (int)first, 64);
        if (__ballot(c && d != d0) == 0) { if (lane == first) atomicAdd(&h[d0], (uint32_t)__popcll(m)); }
        else if (c) atomicAdd(&h[d], 1u);
    }
    __syncthreads();
    uint32_t *g = hist + (size_t)w.q * kBins;
    for (uint32_t b = threadIdx.x; b < kBins; b += kBlock) { const uint32_t v = h[b]; if (v) atomicAdd(&g[b], v); }
}

// One block per query: the bin of the pass that holds the (need - below)-th key; clears the histogram for the next pass.
__global__ void __launch_bounds__(kBlock) k_nk_pick(NkQ *Q, uint32_t *hist, uint32_t *pending) {
    __shared__ int sh[kBlock / 64];
    const uint32_t q = blockIdx.x;
    const NkQ s = Q[q];
    if (s.done) return;
    uint32_t *h = hist + (size_t)q * kBins;
    constexpr uint32_t per = kBins / kBlock;
    uint32_t v[per];
    int sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) { v[j] = h[threadIdx.x * per + j]; h[threadIdx.x * per + j] = 0; sum += (int)v[j]; }
    int tot;
    const int incl = block_incl_scan(sum, sh, &tot);
    const uint32_t rem = s.need - s.below;
    if ((uint32_t)tot < rem) {   // fewer keys that small: the digit moves up (prefix 0 still holds every key counted so far)
        if (threadIdx.x == 0) {
            if (s.shift + kDigit >= 32) Q[q].done = 1;   // (cannot happen: the last pass sees every candidate)
            else { Q[q].shift = s.shift + kDigit; atomicAdd(pending, 1u); }
        }
        return;
    }
    const uint32_t excl = (uint32_t)(incl - sum);
    if (!(excl < rem && rem <= (uint32_t)incl)) return;
    uint32_t acc = excl, b = 0, at = 0;
#pragma unroll
    for (uint32_t j = 0; j < per; j++) {
        if (at == 0 && acc + v[j] >= rem) { b = threadIdx.x * per + j; at = v[j]; }
        if (at == 0) acc += v[j];
    }
    const uint32_t below = s.below + acc;
    Q[q].below = below;
    if (s.shift == 0) {
        Q[q].cut = (s.prefix << kDigit) | b;
        Q[q].n_at_cut = at;
        Q[q].take = s.need - below;
        Q[q].done = 1;
    } else {
        Q[q].prefix = (s.prefix << kDigit) | b;
        Q[q].shift = s.shift - kDigit;
        atomicAdd(pending, 1u);
    }
}

// Flags of one position, packed for one scan: leaf of last_anc | key < d* (<< 10) | key == d* (<< 20).  A tile has 256 positions.
__device__ __forceinline__ int nk_flags(const DfsView &t, const NkQ &s, uint32_t i, uint32_t *key) {
    if (!t.leaf[i]) return 0;
    const uint32_t kq = t.cum[i] - s.base;
    *key = kq;
    int f = (i >= s.last && i < s.xhi) ? 1 : 0;
    if (s.need && !(i >= s.xlo && i < s.xhi)) f |= kq < s.cut ? 1 << 10 : (kq == s.cut ? 1 << 20 : 0);
    return f;
}

__global__ void __launch_bounds__(kBlock) k_nk_count(DfsView t, const NkQ *Q, const NkItem *work, uint32_t *cnt) {
    __shared__ int sh[kBlock / 64];
    const NkItem w = work[blockIdx.x];
    const NkQ s = Q[w.q];
    const uint32_t lo = max(s.lo, w.seg * kSeg), hi = min(s.hi, w.seg * kSeg + kSeg);
    int a = 0, b = 0, e = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) {
        uint32_t key;
        const int f = nk_flags(t, s, i, &key);
        a += f & 1; b += (f >> 10) & 1; e += (f >> 20) & 1;
    }
    int ta, tb, te;
    (void)block_incl_scan(a, sh, &ta);
    (void)block_incl_scan(b, sh, &tb);
    (void)block_incl_scan(e, sh, &te);
    if (threadIdx.x == 0) { cnt[3 * (size_t)blockIdx.x] = (uint32_t)ta; cnt[3 * (size_t)blockIdx.x + 1] = (uint32_t)tb; cnt[3 * (size_t)blockIdx.x + 2] = (uint32_t)te; }
}

// One lane per query: counts of its work items -> their offsets.
__global__ void k_nk_offsets(const uint32_t *woff, uint32_t nq, uint32_t *cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    uint32_t a = 0, b = 0, e = 0;
    for (uint32_t w = woff[q]; w < woff[q + 1]; w++) {
        const uint32_t ca = cnt[3 * (size_t)w], cb = cnt[3 * (size_t)w + 1], ce = cnt[3 * (size_t)w + 2];
        cnt[3 * (size_t)w] = a; cnt[3 * (size_t)w + 1] = b; cnt[3 * (size_t)w + 2] = e;
        a += ca; b += cb; e += ce;
    }
}

// Row q of the outputs: slots [0, nlast) the leaves of last_anc, then the keys < d*, then the taken keys == d*, each group in
// depth-first order; slots past `stride` are dropped (only a node with more than k leaves of its own has more than k).
__global__ void __launch_bounds__(kBlock) k_nk_write(DfsView t, const NkQ *Q, const NkItem *work, const uint32_t *off, uint32_t stride,
                                                     uint32_t *onode, uint32_t *odist) {
    __shared__ int sh[kBlock / 64];
    const NkItem w = work[blockIdx.x];
    const NkQ s = Q[w.q];
    const uint32_t lo = max(s.lo, w.seg * kSeg), hi = min(s.hi, w.seg * kSeg + kSeg);
    uint32_t a0 = off[3 * (size_t)blockIdx.x], b0 = off[3 * (size_t)blockIdx.x + 1], e0 = off[3 * (size_t)blockIdx.x + 2];
    uint32_t *rn = onode + (size_t)w.q * stride, *rd = odist + (size_t)w.q * stride;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        uint32_t key = 0;
        const int f = i < hi ? nk_flags(t, s, i, &key) : 0;
        int tot;
        const int incl = block_incl_scan(f, sh, &tot);
        const int ex = incl - f;
        if (f & 1) {
            const uint32_t o = a0 + (uint32_t)(ex & 1023);
            if (o < stride) { rn[o] = i; rd[o] = key; }
        }
        if (f & (1 << 10)) {
            const uint32_t o = s.nlast + b0 + (uint32_t)((ex >> 10) & 1023);
            if (o < stride) { rn[o] = i; rd[o] = key; }
        }
        if (f & (1 << 20)) {
            const uint32_t r = e0 + (uint32_t)((ex >> 20) & 1023);
            const uint32_t o = s.nlast + s.below + r;
            if (r < s.take && o < stride) { rn[o] = i; rd[o] = key; }
        }
        a0 += (uint32_t)(tot & 1023); b0 += (uint32_t)((tot >> 10) & 1023); e0 += (uint32_t)((tot >> 20) & 1023);
    }
}

// One block per query: its `need` candidates ordered by (key, position).  InLds: up to kSortLds pairs in LDS; the rest run the
// same network over `scratch` (soff[q] = the query's first slot, its padded length follows from need).
template <bool InLds>
__global__ void __launch_bounds__(kBlock) k_nk_sort(const NkQ *Q, uint32_t stride, uint32_t *onode, uint32_t *odist,
                                                    unsigned long long *scratch, const uint64_t *soff) {
    __shared__ unsigned long long lds[InLds ? kSortLds : 1];
    const uint32_t q = blockIdx.x;
    const NkQ s = Q[q];
    if (s.need < 2 || s.nlast + s.need > stride) return;
    uint32_t P = 2;
    while (P < s.need) P <<= 1;
    if (InLds != (P <= kSortLds)) return;
    unsigned long long *buf = InLds ? lds : scratch + soff[q];
    uint32_t *rn = onode + (size_t)q * stride + s.nlast, *rd = odist + (size_t)q * stride + s.nlast;
    for (uint32_t i = threadIdx.x; i < P; i += kBlock)
        buf[i] = i < s.need ? ((unsigned long long)rd[i] << 32 | rn[i]) : ~0ull;
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += kBlock) {
                const uint32_t x = i ^ j;
                if (x <= i) continue;
                const unsigned long long a = buf[i], b = buf[x];
                if ((a > b) == ((i & k2) == 0)) { buf[i] = b; buf[x] = a; }
            }
            __syncthreads();
        }
    for (uint32_t i = threadIdx.x; i < s.need; i += kBlock) { const unsigned long long v = buf[i]; rn[i] = (uint32_t)v; rd[i] = (uint32_t)(v >> 32); }
}

// Depth-first positions -> the caller's numbering, for the slots a query filled.
__global__ void k_nk_tobfs(const NkQ *Q, const uint32_t *d2b, uint32_t n, uint32_t stride, uint32_t *onode) {
    const uint32_t q = blockIdx.y, o = blockIdx.x * blockDim.x + threadIdx.x;
    const NkQ s = Q[q];
    const uint32_t cnt = s.anc == kNil ? 0 : min(stride, s.nlast + s.need);
    if (o >= cnt) return;
    const uint32_t v = onode[(size_t)q * stride + o];
    onode[(size_t)q * stride + o] = v < n ? d2b[v] : kNil;
}

}  // namespace

struct NearState : QueryBase {
    DBuf<uint32_t> lpre, d2b;
    // per call
    DBuf<uint32_t> qnode, qk, hist, pending, woff, cnt, onode, odist;
    DBuf<NkQ> Q;
    DBuf<NkItem> work;
    DBuf<unsigned long long> scratch;
    DBuf<uint64_t> soff;
};

void nk_free(NearState *s) { query_free(s); }

int nk_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, NearState **out) {
    return query_attach("ugp_nearest_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out, NoCheck(), [&](NearState *S) {
        const uint32_t n = S->T->n;
        DBuf<uint32_t> seg;   // read until the synchronize below
        hipError_t err = S->lpre.alloc((size_t)n + 1);
        if (err == hipSuccess) err = S->d2b.upload(dfs2bfs.data(), n, S->stream);
        if (err == hipSuccess) err = scan_flags(seg, n, S->T->leaf.p, S->lpre.p, S->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(S->stream);
        return hip_rc("ugp_nearest_attach", err);
    });
}

int nk_run(NearState *S, uint64_t nq, const uint32_t *nodes, const uint32_t *k, uint32_t stride, uint32_t *out_nodes, uint32_t *out_dist,
           ugp_nearest_info *info, uint32_t chunk_queries) {
    if (!S) return set_error(UGP_ERR_INVALID, "no nearest tables: call ugp_nearest_attach first");
    if (!nq) return UGP_OK;
    if (!nodes || !k || !out_nodes || !out_dist || !info) return set_error(UGP_ERR_INVALID, "null argument");
    const uint32_t N = S->T->n;
    uint32_t kmax = 0;
    for (uint64_t i = 0; i < nq; i++) {
        if (nodes[i] >= N) return set_error(UGP_ERR_INVALID, "node index out of range");
        if (k[i] == 0) return set_error(UGP_ERR_INVALID, "k must be positive");
        kmax = std::max(kmax, k[i]);
    }
    if (stride < kmax) return set_error(UGP_ERR_INVALID, "out_stride is smaller than the largest k");
    // workspace bounds of one chunk: queries, output slots, work items, pairs of the global sort
    constexpr uint64_t kMaxSlots = 1ull << 24, kMaxItems = 1ull << 20, kMaxPairs = 1ull << 24;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(chunk_queries ? chunk_queries : 1024, 32768), std::max<uint64_t>(1, kMaxSlots / stride)));
    try {
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        const DfsView t = S->T->view();
        const std::vector<uint32_t> &b2d = S->T->bfs2dfs, &d2b = *S->dfs2bfs;
        UGP_HIP_TRY(S->Q.alloc(chunk)); UGP_HIP_TRY(S->hist.alloc(chunk * kBins)); UGP_HIP_TRY(S->pending.alloc(1));
        UGP_HIP_TRY(S->woff.alloc(chunk + 1)); UGP_HIP_TRY(S->onode.alloc(chunk * stride)); UGP_HIP_TRY(S->odist.alloc(chunk * stride));
        UGP_HIP_TRY(S->soff.alloc(chunk));
        std::vector<uint32_t> qn, woff, rown, rowd;
        std::vector<NkQ> Q;
        std::vector<NkItem> work;
        std::vector<uint64_t> soff;
        for (uint64_t c0 = 0; c0 < nq;) {
            // the anchors of up to `chunk` queries, then as many of them as the work-item and sort bounds admit
            uint32_t nc = (uint32_t)std::min<uint64_t>(chunk, nq - c0);
            qn.resize(nc);
            for (uint32_t i = 0; i < nc; i++) qn[i] = b2d[nodes[c0 + i]];
            UGP_HIP_TRY(S->qnode.upload(qn, st));
            UGP_HIP_TRY(S->qk.upload(k + c0, nc, st));
            k_nk_anchor<<<(nc + kBlock - 1) / kBlock, kBlock, 0, st>>>(t, S->lpre.p, S->qnode.p, S->qk.p, nc, S->Q.p);
            UGP_HIP_TRY(hipGetLastError());
            Q.resize(nc);
            UGP_HIP_TRY(hipMemcpyAsync(Q.data(), S->Q.p, nc * sizeof(NkQ), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipStreamSynchronize(st));
            work.clear(); woff.assign(1, 0); soff.clear();
            uint64_t pairs = 0;
            uint32_t take = 0;
            for (; take < nc; take++) {
                const NkQ &s = Q[take];
                const uint64_t segs = s.hi > s.lo ? (uint64_t)(s.hi - 1) / kSeg - s.lo / kSeg + 1 : 0;
                uint64_t P = 0;
                if (s.need > kSortLds) { P = 2; while (P < s.need) P <<= 1; }
                if (take && (work.size() + segs > kMaxItems || pairs + P > kMaxPairs)) break;
                for (uint64_t g = 0; g < segs; g++) work.push_back(NkItem{take, (uint32_t)(s.lo / kSeg + g)});
                woff.push_back((uint32_t)work.size());
                soff.push_back(pairs);
                pairs += P;
            }
            nc = take;
            const uint32_t nw = (uint32_t)work.size();
            if (nw) {
                UGP_HIP_TRY(S->work.upload(work, st)); UGP_HIP_TRY(S->woff.upload(woff, st)); UGP_HIP_TRY(S->soff.upload(soff, st));
                UGP_HIP_TRY(S->cnt.alloc(3 * (size_t)nw));
                if (pairs) UGP_HIP_TRY(S->scratch.alloc(pairs));
                UGP_HIP_TRY(hipMemsetAsync(S->hist.p, 0, (size_t)nc * kBins * sizeof(uint32_t), st));
                for (int pass = 0; pass < 6; pass++) {   // one pass when the keys are small, at most five
                    uint32_t pending = 0;
                    UGP_HIP_TRY(hipMemsetAsync(S->pending.p, 0, sizeof(uint32_t), st));
                    k_nk_hist<<<nw, kBlock, 0, st>>>(t, S->Q.p, S->work.p, S->hist.p);
                    k_nk_pick<<<nc, kBlock, 0, st>>>(S->Q.p, S->hist.p, S->pending.p);
                    UGP_HIP_TRY(hipGetLastError());
                    UGP_HIP_TRY(hipMemcpyAsync(&pending, S->pending.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                    UGP_HIP_TRY(hipStreamSynchronize(st));
                    if (!pending) break;
                }
                k_nk_count<<<nw, kBlock, 0, st>>>(t, S->Q.p, S->work.p, S->cnt.p);
                k_nk_offsets<<<(nc + kBlock - 1) / kBlock, kBlock, 0, st>>>(S->woff.p, nc, S->cnt.p);
                k_nk_write<<<nw, kBlock, 0, st>>>(t, S->Q.p, S->work.p, S->cnt.p, stride, S->onode.p, S->odist.p);
                k_nk_sort<true><<<nc, kBlock, 0, st>>>(S->Q.p, stride, S->onode.p, S->odist.p, nullptr, S->soff.p);
                if (pairs) k_nk_sort<false><<<nc, kBlock, 0, st>>>(S->Q.p, stride, S->onode.p, S->odist.p, S->scratch.p, S->soff.p);
                k_nk_tobfs<<<dim3((stride + kBlock - 1) / kBlock, nc), kBlock, 0, st>>>(S->Q.p, S->d2b.p, N, stride, S->onode.p);
                UGP_HIP_TRY(hipGetLastError());
                rown.resize((size_t)nc * stride); rowd.resize((size_t)nc * stride);
                UGP_HIP_TRY(hipMemcpyAsync(rown.data(), S->onode.p, rown.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                UGP_HIP_TRY(hipMemcpyAsync(rowd.data(), S->odist.p, rowd.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
                UGP_HIP_TRY(hipMemcpyAsync(Q.data(), S->Q.p, nc * sizeof(NkQ), hipMemcpyDeviceToHost, st));
                UGP_HIP_TRY(hipStreamSynchronize(st));
            }
            for (uint32_t i = 0; i < nc; i++) {
                const NkQ &s = Q[i];
                ugp_nearest_info &o = info[c0 + i];
                o.count = s.anc == kNil ? 0 : s.nlast + s.need;
                o.anc = s.anc == kNil ? UINT32_MAX : d2b[s.anc];
                o.last_anc = d2b[s.last];
                o.cut_dist = s.cut;
                o.n_at_cut = s.n_at_cut;
                const uint32_t w = std::min(o.count, stride);
                if (w) {
                    std::copy(rown.begin() + (size_t)i * stride, rown.begin() + (size_t)i * stride + w, out_nodes + (c0 + i) * stride);
                    std::copy(rowd.begin() + (size_t)i * stride, rowd.begin() + (size_t)i * stride + w, out_dist + (c0 + i) * stride);
                }
            }
            c0 += nc;
        }
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

}  // namespace ugp
