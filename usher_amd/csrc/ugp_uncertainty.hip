// ugp_uncertainty.hip -- matUtils uncertainty (uncertainty.cpp:132-339) for a batch of tree nodes: for each node S, the
// reference's mapper2_body search (usher_mapper.cpp:167-504) over every node but S, with S's root path as the sample in the
// LITERAL order findEPPs builds it (S's own mutations, then each ancestor's; masked entries kept; never sorted), then the
// number of equally parsimonious placements, their depth-first positions and the neighborhood size (:41-130).
//
// The search is dense: every (S, X) pair is scored, no pruning ("Placement uncertainty").  The score is the closed
// form of the three loops of mapper2_body:
//   score(S, X) = nr(P) + H0(S) + C_S(P) + corr(S, X) + M0(S),   P = parent(X)
//   nr(v)    = positions whose state on root..v differs from the reference base
//   C_S(v)   = sum over the mutations m on root..v at positions of Q(S) of h(m) - h(state of parent at m's position),
//              h(s) = cost(q, s) - [s != ref]: loops 2 and 3 of the position, minus its share of nr
//   corr     = X's own mutations that loop 1 keeps (found in Q by the literal merge pointer, or a reversion it did not find)
//              replace the parent's state at their position
//   H0, M0   = what the unmatched sample rows and the masked sample rows cost at the root state.
// C_S is a prefix sum in depth-first order: every mutation at a position of Q(S) adds its term over its subtree's DFS range
// (+e at its node, -e at the end of its subtree), so per sample a difference array of N entries and one scan give C_S at
// every node.  Loop 1 -- the only order-dependent part -- is run literally per (S, X) against Q(S) in its stored order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ugp_uncertainty.hpp"

namespace ugp {
int set_error(int code, const std::string &msg);
}

namespace {

constexpr uint32_t kBlock = 256;           // threads per block of the per-segment kernels (4 waves)
constexpr uint32_t kSeg = 16384;           // depth-first positions per segment (one block per (segment, sample))
constexpr uint64_t kDiffBudget = 1ull << 31;   // bytes of the per-batch difference arrays (batch size = budget / 4N)
constexpr int32_t kNone = INT_MAX;         // score of a node that is not a candidate (not eligible, or the sample itself)

#define UNC_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return ugp::set_error(UGP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <typename T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    ~DBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t upload(const std::vector<T> &v) {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// ---- device helpers -----------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lowbit4(uint32_t a) {
    for (uint32_t b = 0; b < 4; b++) if (a & (1u << b)) return 1u << b;
    return 0;   // the reference leaves it uninitialised; the oracle (and this library) read 0
}
// Loop 2 of mapper2_body for one sample row (allele a, reference r) against the state s its position has (r: none).
__device__ __forceinline__ int row_cost(uint32_t a, uint32_t r, uint32_t s) {
    if (a & s) return 0;
    return ((a & r) ? r : lowbit4(a)) != s ? 1 : 0;
}
// Entry bits: mutated base | ref << 8 | parent state (0 = none on the root path) << 16 | [parent state != its ref] << 24
__device__ __forceinline__ uint32_t b_nuc(uint32_t b) { return b & 0xffu; }
__device__ __forceinline__ uint32_t b_ref(uint32_t b) { return (b >> 8) & 0xffu; }
__device__ __forceinline__ uint32_t b_anc(uint32_t b) { return (b >> 16) & 0xffu; }
__device__ __forceinline__ int b_ancne(uint32_t b) { return (int)((b >> 24) & 1u); }
// h(m) - h(parent state of m) for a mutation at a position of Q (sample row t = a | r << 8)
__device__ __forceinline__ int ev_term(uint32_t t, uint32_t bits) {
    const uint32_t a = t & 0xffu, r = t >> 8, nuc = b_nuc(bits), anc = b_anc(bits);
    const int hm = row_cost(a, r, nuc) - (nuc != b_ref(bits) ? 1 : 0);
    const int ha = anc ? row_cost(a, r, anc) - b_ancne(bits) : row_cost(a, r, r);
    return hm - ha;
}

__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
// Inclusive scan over the block (kBlock threads); *total = block sum.  Uses sh[kBlock / 64].
__device__ __forceinline__ int block_incl_scan(int v, int *sh, int *total) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int x = wave_incl_scan(v);
    if (lane == 63) sh[w] = x;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < (int)(kBlock / 64); k++) { const int s = sh[k]; if (k < w) pre += s; tot += s; }
    __syncthreads();
    *total = tot;
    return x + pre;
}

struct Tree {   // device tables, indexed by depth-first position
    uint32_t n;
    const uint32_t *dpar, *dend, *depth, *cum, *moff, *mbits, *mnode, *poff, *pent;
    const int32_t *nrp, *mpos;
    const uint8_t *leaf;
    uint32_t tp;   // positions 0 .. tp-1 index the per-sample table
};

struct Batch {
    uint32_t b;            // samples in this batch
    uint32_t nseg;
    const uint32_t *sdfs;  // [b] depth-first position of each sample's node
    const uint64_t *qoff;  // [b + 1] room for each sample's rows (its cum[])
    int32_t *qpos; uint16_t *qnr;   // the literal rows: position, allele | ref << 8
    uint32_t *qn;          // [b] rows
    int32_t *h0m;          // [b] H0 + M0
    int32_t *init;         // [b] the caller's initial best_set_difference: |Q| + |root mutations| + 1 (uncertainty.cpp:199)
    uint16_t *tab;         // [b][tp] row of the sample at a position (allele | ref << 8), 0 = none
    int32_t *diff;         // [b][n] difference array, then the scores
    int32_t *seg;          // [b][nseg] segment sums -> carries
    int32_t *mn;           // [b] minimum candidate score (-1: no list)
    uint32_t *scnt, *sfirst, *slast, *soff;   // [b][nseg] ties per segment, first / last position, list offset
    uint32_t *total, *shift, *lca;            // [b]
    int32_t *top;          // [b][nseg][2] the two largest neighborhood distances of each segment (-1: none)
    uint32_t *ties; uint32_t cap;            // [b][cap]
    uint32_t *epps, *nsize, *tcount;         // [b]
    uint64_t pscore;       // Tree::get_parsimony_score: mutation entries of the whole tree
    uint32_t root_muts;
};

// One thread per sample: Q(S) by walking S -> root (uncertainty.cpp:143-166), the per-position table, H0, M0.
__global__ void k_gather(Tree t, Batch B) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B.b) return;
    uint16_t *tab = B.tab + (size_t)s * t.tp;
    const uint64_t q0 = B.qoff[s], qcap = B.qoff[s + 1] - q0;
    uint64_t nq = 0;
    int h0 = 0, m0 = 0;
    uint32_t v = B.sdfs[s];
    while (v != UINT32_MAX) {
        for (uint32_t e = t.moff[v]; e < t.moff[v + 1]; e++) {
            const int32_t p = t.mpos[e];
            const uint32_t bits = t.mbits[e], a = b_nuc(bits), r = b_ref(bits);
            if (p >= 0) {
                if (tab[p]) continue;
                tab[p] = (uint16_t)(a | (r << 8));
                h0 += row_cost(a, r, r);
            } else {
                m0 += (a & r) ? 0 : (lowbit4(a) != r ? 1 : 0);
            }
            if (nq < qcap) { B.qpos[q0 + nq] = p; B.qnr[q0 + nq] = (uint16_t)(a | (r << 8)); }
            nq++;
        }
        v = t.dpar[v];
    }
    B.qn[s] = (uint32_t)nq;
    B.h0m[s] = h0 + m0;
    B.init[s] = (int32_t)(nq + B.root_muts + 1);
    B.mn[s] = kNone;
}

// One block per sample: every mutation of the tree at a position of Q(S) adds its term over its subtree.
__global__ void k_events(Tree t, Batch B) {
    const uint32_t s = blockIdx.x;
    const uint64_t q0 = B.qoff[s];
    const uint32_t nq = B.qn[s];
    const uint16_t *tab = B.tab + (size_t)s * t.tp;
    int32_t *diff = B.diff + (size_t)s * t.n;
    for (uint32_t k = threadIdx.x; k < nq; k += blockDim.x) {
        const int32_t p = B.qpos[q0 + k];
        if (p < 0) continue;
        const uint32_t row = tab[p];
        for (uint32_t i = t.poff[p]; i < t.poff[p + 1]; i++) {
            const uint32_t e = t.pent[i];
            const int ev = ev_term(row, t.mbits[e]);
            if (!ev) continue;
            const uint32_t u = t.mnode[e], end = t.dend[u];
            atomicAdd(&diff[u], ev);
            if (end < t.n) atomicAdd(&diff[end], -ev);
        }
    }
}

__global__ void k_segsum(Tree t, Batch B) {
    __shared__ int sh[kBlock / 64];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    const int32_t *diff = B.diff + (size_t)s * t.n;
    int acc = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) acc += diff[i];
    int tot;
    (void)block_incl_scan(acc, sh, &tot);
    if (threadIdx.x == 0) B.seg[(size_t)s * B.nseg + g] = tot;
}

// One thread per sample: segment sums -> exclusive carries.
__global__ void k_segscan(Batch B) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B.b) return;
    int32_t *seg = B.seg + (size_t)s * B.nseg;
    int run = 0;
    for (uint32_t g = 0; g < B.nseg; g++) { const int v = seg[g]; seg[g] = run; run += v; }
}

// The score of every node for one sample and one segment; candidates keep it, the rest read kNone.
__global__ void __launch_bounds__(kBlock) k_score(Tree t, Batch B) {
    __shared__ int sh[kBlock / 64];
    __shared__ int smin[kBlock / 64];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    int32_t *diff = B.diff + (size_t)s * t.n;
    const uint16_t *tab = B.tab + (size_t)s * t.tp;
    const uint64_t q0 = B.qoff[s];
    const uint32_t nq = B.qn[s], self = B.sdfs[s];
    const int base = B.h0m[s];
    int carry = B.seg[(size_t)s * B.nseg + g];
    int best = kNone;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const int dv = i < hi ? diff[i] : 0;
        int tot;
        const int C = carry + block_incl_scan(dv, sh, &tot);   // C_S(X): X's own terms included
        carry += tot;
        if (i >= hi) continue;
        int score = kNone;
        if (i == 0) {
            // the root: loops 2 and 3 against its own mutations, masked ones included (usher_mapper.cpp:266-269, 398-444)
            int sc = base;
            for (uint32_t e = t.moff[0]; e < t.moff[1]; e++) {
                const int32_t p = t.mpos[e];
                const uint32_t bits = t.mbits[e], nuc = b_nuc(bits), ref = b_ref(bits);
                if (p < 0) { sc += ref != nuc ? 1 : 0; continue; }
                const uint32_t row = (uint32_t)p < t.tp ? tab[p] : 0;
                if (row) sc += row_cost(row & 0xffu, row >> 8, nuc) - row_cost(row & 0xffu, row >> 8, row >> 8);
                else sc += nuc != ref ? 1 : 0;
            }
            if (i != self) score = sc;
        } else if (i != self) {
            // loop 1 (usher_mapper.cpp:190-264) literally: the merge pointer runs over Q(S) in its stored order
            uint32_t start = 0;
            int nm = 0, common = 0, corr = 0, own = 0;
            bool hu = false, stopped = false;
            for (uint32_t e = t.moff[i]; e < t.moff[i + 1]; e++) {
                const int32_t p = t.mpos[e];
                const uint32_t bits = t.mbits[e], nuc = b_nuc(bits), ref = b_ref(bits);
                const uint32_t row = p >= 0 ? tab[p] : 0;
                if (row) own += ev_term(row, bits);   // the part of C_S(X) that is X's own
                if (stopped) continue;
                nm++;
                if (p < 0) { hu = true; stopped = true; continue; }
                bool found = false, found_pos = false;
                for (uint32_t k = start; k < nq; k++) {
                    const int32_t p2 = B.qpos[q0 + k];
                    start = k;
                    if (p == p2) {
                        found_pos = true;
                        if (B.qnr[q0 + k] & nuc & 0xffu) { found = true; break; }
                    }
                    if (p < p2) break;
                }
                bool added = found;
                if (!found && !found_pos && nuc == ref) added = true;
                if (added) {
                    common++;
                    const uint32_t anc = b_anc(bits);
                    if (row) {
                        const uint32_t a = row & 0xffu, r = row >> 8;
                        corr += row_cost(a, r, nuc) - (anc ? row_cost(a, r, anc) : row_cost(a, r, r));
                    } else {
                        corr += (nuc != ref ? 1 : 0) - b_ancne(bits);
                    }
                } else {
                    hu = true;
                }
            }
            const bool lf = t.leaf[i] != 0;
            const bool elig = (hu && !lf && common > 0 && nm != common) || (lf && common > 0) || (!hu && !lf && nm == common);
            if (elig) score = t.nrp[i] + base + (C - own) + corr;
        }
        diff[i] = score;
        best = min(best, score);
    }
    // block minimum
    for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d, 64));
    if ((threadIdx.x & 63) == 0) smin[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = smin[0];
        for (int k = 1; k < (int)(kBlock / 64); k++) m = min(m, smin[k]);
        if (m != kNone) atomicMin(&B.mn[s], m);
    }
}

__global__ void k_tiecount(Tree t, Batch B) {
    __shared__ int sh[kBlock / 64];
    __shared__ uint32_t sf[kBlock / 64], sl[kBlock / 64];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    const int32_t *sc = B.diff + (size_t)s * t.n;
    const int32_t m = B.mn[s];
    int cnt = 0;
    uint32_t first = UINT32_MAX, last = 0;
    if (m != kNone)
        for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock)
            if (sc[i] == m) { cnt++; first = min(first, i); last = max(last, i); }
    for (int d = 32; d > 0; d >>= 1) { first = min(first, (uint32_t)__shfl_xor((int)first, d, 64)); last = max(last, (uint32_t)__shfl_xor((int)last, d, 64)); }
    if ((threadIdx.x & 63) == 0) { sf[threadIdx.x >> 6] = first; sl[threadIdx.x >> 6] = last; }
    int tot;
    (void)block_incl_scan(cnt, sh, &tot);   // (its barriers also publish sf / sl)
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(kBlock / 64); k++) { first = min(first, sf[k]); last = max(last, sl[k]); }
        first = min(first, sf[0]); last = max(last, sl[0]);
        const size_t o = (size_t)s * B.nseg + g;
        B.scnt[o] = (uint32_t)tot; B.sfirst[o] = first; B.slast[o] = last;
    }
}

// One thread per sample: list offsets, the reference's initial state (best = init, best_j_vec = {0}, num_best = 1), the
// lowest common ancestor of the whole tie set (that of its first and last depth-first positions).
__global__ void k_tiescan(Tree t, Batch B) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B.b) return;
    uint32_t run = 0, first = UINT32_MAX, last = 0;
    for (uint32_t g = 0; g < B.nseg; g++) {
        const size_t o = (size_t)s * B.nseg + g;
        const uint32_t c = B.scnt[o];
        B.soff[o] = run;
        run += c;
        if (c) { first = min(first, B.sfirst[o]); last = max(last, B.slast[o]); }
    }
    uint32_t shift = 0, total = run;
    const int32_t m = B.mn[s];
    if (B.qn[s] == 0) {                    // empty Q(S): the reference searches nothing (:167); reported as 0 placements
        total = 0; B.mn[s] = -1;
    } else if (m == kNone || m > B.init[s]) {   // nothing beats the initial bound: best_j_vec stays {0}
        total = 1; shift = 1; first = last = 0; B.mn[s] = -1;
    } else if (m == B.init[s]) {           // ties with the initial bound join the initial {0}
        total = run + 1; shift = 1; first = 0;
    }
    if (shift && B.cap) B.ties[(size_t)s * B.cap] = 0;
    uint32_t a = first, b = last;
    if (total > 1) {
        while (t.depth[a] > t.depth[b]) a = t.dpar[a];
        while (t.depth[b] > t.depth[a]) b = t.dpar[b];
        while (a != b) { a = t.dpar[a]; b = t.dpar[b]; }
    }
    B.total[s] = total; B.shift[s] = shift; B.lca[s] = a;
}

__device__ __forceinline__ void top2_add(int &t1, int &t2, int v) {
    if (v > t1) { t2 = t1; t1 = v; } else if (v > t2) t2 = v;
}

// Ordered list of the tied positions (up to cap) and each segment's two largest distances to the common ancestor c:
// for a tie v != c the values cum[v] - cum[a] over its ancestors a up to c; the largest two of them are cum[v] - cum[c]
// and (when v lies two or more levels below c) cum[v] - cum[child of c towards v].
__global__ void __launch_bounds__(kBlock) k_tiewrite(Tree t, Batch B) {
    __shared__ int sh[kBlock / 64];
    __shared__ int s1[kBlock], s2[kBlock];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    const int32_t *sc = B.diff + (size_t)s * t.n;
    const int32_t m = B.mn[s];
    const uint32_t total = B.total[s], c = B.lca[s];
    uint32_t base = B.shift[s] + B.soff[(size_t)s * B.nseg + g];
    int t1 = -1, t2 = -1;
    if (m >= 0 && B.scnt[(size_t)s * B.nseg + g]) {
        for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
            const uint32_t i = t0 + threadIdx.x;
            const int f = (i < hi && sc[i] == m) ? 1 : 0;
            int tot;
            const int incl = block_incl_scan(f, sh, &tot);
            if (f) {
                const uint32_t o = base + (uint32_t)(incl - 1);
                if (o < B.cap) B.ties[(size_t)s * B.cap + o] = i;
                if (total > 1 && i != c) {
                    const int top = (int)(t.cum[i] - t.cum[c]);
                    top2_add(t1, t2, top);
                    const uint32_t dc = t.depth[c];
                    if (t.depth[i] >= dc + 2) {
                        uint32_t w = i;
                        while (t.depth[w] > dc + 1) w = t.dpar[w];
                        top2_add(t1, t2, (int)(t.cum[i] - t.cum[w]));
                    }
                }
            }
            base += (uint32_t)tot;
        }
    }
    s1[threadIdx.x] = t1; s2[threadIdx.x] = t2;
    __syncthreads();
    for (uint32_t h = kBlock / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            int a1 = s1[threadIdx.x], a2 = s2[threadIdx.x];
            top2_add(a1, a2, s1[threadIdx.x + h]);
            top2_add(a1, a2, s2[threadIdx.x + h]);
            s1[threadIdx.x] = a1; s2[threadIdx.x] = a2;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const size_t o = ((size_t)s * B.nseg + g) * 2;
        B.top[o] = s1[0]; B.top[o + 1] = s2[0];
    }
}

__global__ void k_final(Batch B) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B.b) return;
    const uint32_t total = B.total[s];
    uint64_t ns = 0;
    if (total > 1) {
        int t1 = -1, t2 = -1;
        for (uint32_t g = 0; g < B.nseg; g++) {
            const size_t o = ((size_t)s * B.nseg + g) * 2;
            top2_add(t1, t2, B.top[o]);
            top2_add(t1, t2, B.top[o + 1]);
        }
        const uint64_t widest = t2 >= 0 ? (uint64_t)(t1 + t2) : 0;   // fewer than two distances: 0 (:104-113)
        ns = min(widest, B.pscore);
    }
    B.epps[s] = total;
    B.nsize[s] = (uint32_t)min<uint64_t>(ns, UINT32_MAX);
    B.tcount[s] = total;
}

}  // namespace

namespace ugp {

struct UncState {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n = 0, tp = 0, root_muts = 0;
    uint64_t pscore = 0;
    std::vector<uint32_t> h_cum, bfs2dfs;
    DBuf<uint32_t> dpar, dend, depth, cum, moff, mbits, mnode, poff, pent;
    DBuf<int32_t> nrp, mpos;
    DBuf<uint8_t> leaf;
    // per-batch workspace
    DBuf<uint32_t> sdfs, qn, scnt, sfirst, slast, soff, total, shift, lca, ties, epps, nsize, tcount;
    DBuf<uint64_t> qoff;
    DBuf<int32_t> qpos, h0m, init, diff, seg, mn, top;
    DBuf<uint16_t> qnr, tab;
    ~UncState() {
        if (stream) { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    }
};

void unc_free(UncState *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int unc_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device, UncState **out) {
    if (!tree || !out || !tree->parent || !tree->mut_off) return set_error(UGP_ERR_INVALID, "null argument");
    const uint64_t N = tree->n_nodes;
    if (N == 0 || N >= (1ull << 31) || dfs2bfs.size() != N || bfs2dfs.size() != N) return set_error(UGP_ERR_INVALID, "tree does not match the handle");
    const uint64_t M = tree->mut_off[N];
    if (M >= (1ull << 32)) return set_error(UGP_ERR_UNSUPPORTED, "more than 2^32 mutation entries");
    if (M && (!tree->mut_pos || !tree->mut_ref || !tree->mut_nuc)) return set_error(UGP_ERR_INVALID, "null mutation arrays");
    UncState *S = nullptr;
    try {
        S = new UncState();
        S->device = device;
        S->n = (uint32_t)N;
        S->pscore = M;
        S->root_muts = (uint32_t)(tree->mut_off[1] - tree->mut_off[0]);
        S->bfs2dfs = bfs2dfs;
        std::vector<uint32_t> dpar(N), dend(N), depth(N), cum(N), moff(N + 1), mbits(M), mnode(M);
        std::vector<int32_t> mpos(M), nrp(N, 0);
        std::vector<uint8_t> leaf(N, 1);
        int32_t maxpos = -1;
        uint64_t e = 0;
        for (uint64_t i = 0; i < N; i++) {
            const uint32_t b = dfs2bfs[i];
            if (b >= N || bfs2dfs[b] != i) { delete S; return set_error(UGP_ERR_INVALID, "depth-first order is not a permutation"); }
            dpar[i] = i ? bfs2dfs[tree->parent[b]] : UINT32_MAX;
            if (i && dpar[i] >= i) { delete S; return set_error(UGP_ERR_INVALID, "parent after child in depth-first order"); }
            moff[i] = (uint32_t)e;
            for (uint64_t k = tree->mut_off[b]; k < tree->mut_off[b + 1]; k++, e++) {
                mpos[e] = tree->mut_pos[k];
                mbits[e] = (uint32_t)tree->mut_nuc[k] | (uint32_t)tree->mut_ref[k] << 8;
                mnode[e] = (uint32_t)i;
                maxpos = std::max(maxpos, tree->mut_pos[k]);
            }
            depth[i] = i ? depth[dpar[i]] + 1 : 0;
            cum[i] = (i ? cum[dpar[i]] : 0) + (uint32_t)(tree->mut_off[b + 1] - tree->mut_off[b]);
            if (i) leaf[dpar[i]] = 0;
        }
        moff[N] = (uint32_t)e;
        if (maxpos >= (1 << 28)) { delete S; return set_error(UGP_ERR_UNSUPPORTED, "mutation position above 2^28"); }
        // subtree ends: size by a reverse sweep
        {
            std::vector<uint32_t> sz(N, 1);
            for (uint64_t i = N; i-- > 1;) sz[dpar[i]] += sz[i];
            for (uint64_t i = 0; i < N; i++) dend[i] = (uint32_t)(i + sz[i]);
        }
        // non-masked entries by position (in depth-first order of their node), and the parent state of every entry:
        // the nearest entry above it at its position -- a stack per position whose top's subtree still contains the node
        const uint32_t tp = (uint32_t)(maxpos + 1);
        std::vector<uint32_t> poff(tp + 1, 0), pent;
        for (uint64_t k = 0; k < M; k++) if (mpos[k] >= 0) poff[mpos[k] + 1]++;
        for (uint32_t p = 0; p < tp; p++) poff[p + 1] += poff[p];
        pent.resize(poff[tp]);
        {
            std::vector<uint32_t> fill(poff.begin(), poff.end() - 1);
            for (uint64_t k = 0; k < M; k++) if (mpos[k] >= 0) pent[fill[mpos[k]]++] = (uint32_t)k;
        }
        std::vector<uint32_t> st;
        for (uint32_t p = 0; p < tp; p++) {
            st.clear();
            for (uint32_t x = poff[p]; x < poff[p + 1]; x++) {
                const uint32_t k = pent[x], u = mnode[k];
                while (!st.empty() && dend[mnode[st.back()]] <= u) st.pop_back();
                if (!st.empty() && mnode[st.back()] == u) { delete S; return set_error(UGP_ERR_UNSUPPORTED, "two mutations at one position on one branch"); }
                if (!st.empty()) {
                    const uint32_t a = st.back(), an = mbits[a] & 0xffu, ar = (mbits[a] >> 8) & 0xffu;
                    mbits[k] |= an << 16 | (uint32_t)(an != ar) << 24;
                }
                st.push_back(k);
            }
        }
        // nr(parent): positions off the reference on the parent's root path
        {
            std::vector<int32_t> nr(N, 0);
            for (uint64_t i = 0; i < N; i++) {
                int32_t v = i ? nr[dpar[i]] : 0;
                for (uint32_t k = moff[i]; k < moff[i + 1]; k++) {
                    if (mpos[k] < 0) continue;
                    const uint32_t b = mbits[k];
                    v += ((b & 0xffu) != ((b >> 8) & 0xffu) ? 1 : 0) - (int32_t)((b >> 24) & 1u);
                }
                nr[i] = v;
                nrp[i] = i ? nr[dpar[i]] : 0;
            }
        }
        S->tp = tp;
        S->h_cum = cum;
        if (hipSetDevice(device) != hipSuccess) { delete S; return set_error(UGP_ERR_HIP, "hipSetDevice failed"); }
        hipError_t err = hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking);
        if (err == hipSuccess) err = S->dpar.upload(dpar);
        if (err == hipSuccess) err = S->dend.upload(dend);
        if (err == hipSuccess) err = S->depth.upload(depth);
        if (err == hipSuccess) err = S->cum.upload(cum);
        if (err == hipSuccess) err = S->moff.upload(moff);
        if (err == hipSuccess) err = S->mbits.upload(mbits);
        if (err == hipSuccess) err = S->mnode.upload(mnode);
        if (err == hipSuccess) err = S->poff.upload(poff);
        if (err == hipSuccess) err = S->pent.upload(pent);
        if (err == hipSuccess) err = S->nrp.upload(nrp);
        if (err == hipSuccess) err = S->mpos.upload(mpos);
        if (err == hipSuccess) err = S->leaf.upload(leaf);
        if (err != hipSuccess) { delete S; return set_error(UGP_ERR_HIP, std::string("uncertainty tables: ") + hipGetErrorString(err)); }
    } catch (const std::bad_alloc &) {
        delete S;
        return set_error(UGP_ERR_NOMEM, "out of host memory");
    }
    unc_free(*out);
    *out = S;
    return UGP_OK;
}

int unc_run(UncState *S, const uint32_t *nodes, uint64_t n, uint32_t cap, uint32_t *epps, uint32_t *nsize, uint32_t *tie_dfs, uint32_t *tie_count) {
    if (!S) return set_error(UGP_ERR_INVALID, "no uncertainty tables: call ugp_uncertainty_attach first");
    if (n && (!nodes || !epps || !nsize || !tie_count || (cap && !tie_dfs))) return set_error(UGP_ERR_INVALID, "null argument");
    for (uint64_t i = 0; i < n; i++) if (nodes[i] >= S->n) return set_error(UGP_ERR_INVALID, "node index out of range");
    if (!n) return UGP_OK;
    UNC_TRY(hipSetDevice(S->device));
    const uint32_t N = S->n, nseg = (N + kSeg - 1) / kSeg;
    const uint64_t bmax = std::max<uint64_t>(1, std::min<uint64_t>(4096, kDiffBudget / (4ull * N)));
    hipStream_t st = S->stream;
    Tree t{N, S->dpar.p, S->dend.p, S->depth.p, S->cum.p, S->moff.p, S->mbits.p, S->mnode.p, S->poff.p, S->pent.p,
           S->nrp.p, S->mpos.p, S->leaf.p, S->tp};
    std::vector<uint32_t> sdfs, cnt;
    std::vector<uint64_t> qoff;
    for (uint64_t b0 = 0; b0 < n; b0 += bmax) {
        const uint32_t b = (uint32_t)std::min<uint64_t>(bmax, n - b0);
        sdfs.resize(b); qoff.assign(b + 1, 0);
        for (uint32_t s = 0; s < b; s++) {
            sdfs[s] = S->bfs2dfs[nodes[b0 + s]];
            qoff[s + 1] = qoff[s] + S->h_cum[sdfs[s]];
        }
        const size_t bs = (size_t)b * nseg;
        UNC_TRY(S->sdfs.upload(sdfs));
        UNC_TRY(S->qoff.upload(qoff));
        UNC_TRY(S->qpos.alloc(qoff[b])); UNC_TRY(S->qnr.alloc(qoff[b]));
        UNC_TRY(S->qn.alloc(b)); UNC_TRY(S->h0m.alloc(b)); UNC_TRY(S->init.alloc(b)); UNC_TRY(S->mn.alloc(b));
        UNC_TRY(S->tab.alloc((size_t)b * S->tp)); UNC_TRY(S->diff.alloc((size_t)b * N)); UNC_TRY(S->seg.alloc(bs));
        UNC_TRY(S->scnt.alloc(bs)); UNC_TRY(S->sfirst.alloc(bs)); UNC_TRY(S->slast.alloc(bs)); UNC_TRY(S->soff.alloc(bs));
        UNC_TRY(S->top.alloc(bs * 2));
        UNC_TRY(S->total.alloc(b)); UNC_TRY(S->shift.alloc(b)); UNC_TRY(S->lca.alloc(b));
        UNC_TRY(S->ties.alloc((size_t)b * cap)); UNC_TRY(S->epps.alloc(b)); UNC_TRY(S->nsize.alloc(b)); UNC_TRY(S->tcount.alloc(b));
        Batch B{b, nseg, S->sdfs.p, S->qoff.p, S->qpos.p, S->qnr.p, S->qn.p, S->h0m.p, S->init.p, S->tab.p, S->diff.p, S->seg.p, S->mn.p,
                S->scnt.p, S->sfirst.p, S->slast.p, S->soff.p, S->total.p, S->shift.p, S->lca.p, S->top.p, S->ties.p, cap,
                S->epps.p, S->nsize.p, S->tcount.p, S->pscore, S->root_muts};
        UNC_TRY(hipMemsetAsync(S->tab.p, 0, (size_t)b * S->tp * sizeof(uint16_t), st));
        UNC_TRY(hipMemsetAsync(S->diff.p, 0, (size_t)b * N * sizeof(int32_t), st));
        const dim3 per_sample((b + 63) / 64), grid(nseg, b);
        k_gather<<<per_sample, 64, 0, st>>>(t, B);
        k_events<<<b, kBlock, 0, st>>>(t, B);
        k_segsum<<<grid, kBlock, 0, st>>>(t, B);
        k_segscan<<<per_sample, 64, 0, st>>>(B);
        k_score<<<grid, kBlock, 0, st>>>(t, B);
        k_tiecount<<<grid, kBlock, 0, st>>>(t, B);
        k_tiescan<<<per_sample, 64, 0, st>>>(t, B);
        k_tiewrite<<<grid, kBlock, 0, st>>>(t, B);
        k_final<<<per_sample, 64, 0, st>>>(B);
        UNC_TRY(hipGetLastError());
        UNC_TRY(hipMemcpyAsync(epps + b0, S->epps.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UNC_TRY(hipMemcpyAsync(nsize + b0, S->nsize.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UNC_TRY(hipMemcpyAsync(tie_count + b0, S->tcount.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (cap) UNC_TRY(hipMemcpyAsync(tie_dfs + b0 * cap, S->ties.p, (size_t)b * cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UNC_TRY(hipStreamSynchronize(st));
    }
    return UGP_OK;
}

}  // namespace ugp
