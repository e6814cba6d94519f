// ugp_uncertainty.hip -- matUtils uncertainty (uncertainty.cpp:132-339) for a batch of tree nodes: for each node S, the
// reference's mapper2_body search (usher_mapper.cpp:167-504) over every node but S, with S's root path as the sample in the
// LITERAL order findEPPs builds it (S's own mutations, then each ancestor's; masked entries kept; never sorted), then the
// number of equally parsimonious placements, their depth-first positions and the neighborhood size (:41-130).
//
// The search is dense: every (S, X) pair is scored, no pruning.  The score is the closed form of DESIGN.md 9, written once in
// ugp_dense.hpp (literal_score) with one row per position of Q(S); the depth-first tables are the handle's (ugp_dense.hpp).
// C_S is a prefix sum in depth-first order: every mutation at a position of Q(S) adds its term over its subtree's DFS range
// (+e at its node, -e at the end of its subtree), so per sample a difference array of N entries and one scan give C_S at
// every node.  Loop 1 -- the only order-dependent part -- is run literally per (S, X) against Q(S) in its stored order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_uncertainty.hpp"

namespace ugp {
namespace {

constexpr uint64_t kDiffBudget = 1ull << 31;   // bytes of the per-batch difference arrays (batch size = budget / 4N)

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
__global__ void k_gather(DfsView t, Batch B) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B.b) return;
    uint16_t *tab = B.tab + (size_t)s * t.tp;
    const uint64_t q0 = B.qoff[s], qcap = B.qoff[s + 1] - q0;
    uint64_t nq = 0;
    int h0 = 0, m0 = 0;
    uint32_t v = B.sdfs[s];
    while (v != kNil) {
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
__global__ void k_events(DfsView t, Batch B) {
    const uint32_t s = blockIdx.x;
    const uint64_t q0 = B.qoff[s];
    const uint32_t nq = B.qn[s];
    const OneRow R{B.tab + (size_t)s * t.tp};
    int32_t *diff = B.diff + (size_t)s * t.n;
    for (uint32_t k = threadIdx.x; k < nq; k += blockDim.x) {
        const int32_t p = B.qpos[q0 + k];
        if (p < 0) continue;
        const uint32_t row = R.at(p);
        for (uint32_t i = t.poff[p]; i < t.poff[p + 1]; i++) {
            const uint32_t e = t.pent[i];
            const int ev = ev_term(R, row, t.mbits[e]);
            if (!ev) continue;
            const uint32_t u = t.mnode[e], end = t.dend[u];
            atomicAdd(&diff[u], ev);
            if (end < t.n) atomicAdd(&diff[end], -ev);
        }
    }
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
__global__ void __launch_bounds__(kBlock) k_score(DfsView t, Batch B) {
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const uint64_t q0 = B.qoff[s];
    const Literal q{B.qpos + q0, B.qnr + q0, B.qn[s], B.h0m[s], B.sdfs[s]};
    score_segment(t, OneRow{B.tab + (size_t)s * t.tp}, q, B.diff + (size_t)s * t.n, B.seg[(size_t)s * B.nseg + g], g, &B.mn[s]);
}

__global__ void k_tiecount(DfsView t, Batch B) {
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
__global__ void k_tiescan(DfsView t, Batch B) {
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
__global__ void __launch_bounds__(kBlock) k_tiewrite(DfsView t, Batch B) {
    __shared__ int s1[kBlock], s2[kBlock];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const int32_t m = B.mn[s];
    const uint32_t total = B.total[s], c = B.lca[s];
    int t1 = -1, t2 = -1;
    if (m >= 0 && B.scnt[(size_t)s * B.nseg + g])
        write_ties(B.diff + (size_t)s * t.n, t.n, g, m, B.shift[s] + B.soff[(size_t)s * B.nseg + g], B.ties + (size_t)s * B.cap, B.cap,
                   [&](uint32_t i) {
                       if (total > 1 && i != c) {
                           top2_add(t1, t2, (int)(t.cum[i] - t.cum[c]));
                           const uint32_t dc = t.depth[c];
                           if (t.depth[i] >= dc + 2) {
                               uint32_t w = i;
                               while (t.depth[w] > dc + 1) w = t.dpar[w];
                               top2_add(t1, t2, (int)(t.cum[i] - t.cum[w]));
                           }
                       }
                   });
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

struct UncState : QueryBase {
    // per-batch workspace
    DBuf<uint32_t> sdfs, qn, scnt, sfirst, slast, soff, total, shift, lca, ties, epps, nsize, tcount;
    DBuf<uint64_t> qoff;
    DBuf<int32_t> qpos, h0m, init, diff, seg, mn, top;
    DBuf<uint16_t> qnr, tab;
};

void unc_free(UncState *s) { query_free(s); }

int unc_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, UncState **out) {
    return query_attach(
        "ugp_uncertainty_attach", tree, dfs2bfs, bfs2dfs, device, 32, tables, out,
        [](const DfsTables &T) { return T.literal_ok ? (int)UGP_OK : set_error(UGP_ERR_UNSUPPORTED, "two mutations at one position on one branch"); },
        [](UncState *) { return (int)UGP_OK; });
}

int unc_run(UncState *S, const uint32_t *nodes, uint64_t n, uint32_t cap, uint32_t *epps, uint32_t *nsize, uint32_t *tie_dfs, uint32_t *tie_count) {
    if (!S) return set_error(UGP_ERR_INVALID, "no uncertainty tables: call ugp_uncertainty_attach first");
    if (n && (!nodes || !epps || !nsize || !tie_count || (cap && !tie_dfs))) return set_error(UGP_ERR_INVALID, "null argument");
    const DfsTables &T = *S->T;
    for (uint64_t i = 0; i < n; i++) if (nodes[i] >= T.n) return set_error(UGP_ERR_INVALID, "node index out of range");
    if (!n) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(S->device));
    const uint32_t N = T.n, nseg = (N + kSeg - 1) / kSeg;
    const uint64_t bmax = std::max<uint64_t>(1, std::min<uint64_t>(4096, kDiffBudget / (4ull * N)));
    hipStream_t st = S->stream;
    const DfsView t = T.view();
    std::vector<uint32_t> sdfs, cnt;
    std::vector<uint64_t> qoff;
    for (uint64_t b0 = 0; b0 < n; b0 += bmax) {
        const uint32_t b = (uint32_t)std::min<uint64_t>(bmax, n - b0);
        sdfs.resize(b); qoff.assign(b + 1, 0);
        for (uint32_t s = 0; s < b; s++) {
            sdfs[s] = T.bfs2dfs[nodes[b0 + s]];
            qoff[s + 1] = qoff[s] + T.h_cum[sdfs[s]];
        }
        const size_t bs = (size_t)b * nseg;
        UGP_HIP_TRY(S->sdfs.upload(sdfs));
        UGP_HIP_TRY(S->qoff.upload(qoff));
        UGP_HIP_TRY(S->qpos.alloc(qoff[b])); UGP_HIP_TRY(S->qnr.alloc(qoff[b]));
        UGP_HIP_TRY(S->qn.alloc(b)); UGP_HIP_TRY(S->h0m.alloc(b)); UGP_HIP_TRY(S->init.alloc(b)); UGP_HIP_TRY(S->mn.alloc(b));
        UGP_HIP_TRY(S->tab.alloc((size_t)b * T.tp)); UGP_HIP_TRY(S->diff.alloc((size_t)b * N)); UGP_HIP_TRY(S->seg.alloc(bs));
        UGP_HIP_TRY(S->scnt.alloc(bs)); UGP_HIP_TRY(S->sfirst.alloc(bs)); UGP_HIP_TRY(S->slast.alloc(bs)); UGP_HIP_TRY(S->soff.alloc(bs));
        UGP_HIP_TRY(S->top.alloc(bs * 2));
        UGP_HIP_TRY(S->total.alloc(b)); UGP_HIP_TRY(S->shift.alloc(b)); UGP_HIP_TRY(S->lca.alloc(b));
        UGP_HIP_TRY(S->ties.alloc((size_t)b * cap)); UGP_HIP_TRY(S->epps.alloc(b)); UGP_HIP_TRY(S->nsize.alloc(b)); UGP_HIP_TRY(S->tcount.alloc(b));
        Batch B{b, nseg, S->sdfs.p, S->qoff.p, S->qpos.p, S->qnr.p, S->qn.p, S->h0m.p, S->init.p, S->tab.p, S->diff.p, S->seg.p, S->mn.p,
                S->scnt.p, S->sfirst.p, S->slast.p, S->soff.p, S->total.p, S->shift.p, S->lca.p, S->top.p, S->ties.p, cap,
                S->epps.p, S->nsize.p, S->tcount.p, T.m, T.root_muts};
        UGP_HIP_TRY(hipMemsetAsync(S->tab.p, 0, (size_t)b * T.tp * sizeof(uint16_t), st));
        UGP_HIP_TRY(hipMemsetAsync(S->diff.p, 0, (size_t)b * N * sizeof(int32_t), st));
        const dim3 per_sample((b + 63) / 64), grid(nseg, b);
        k_gather<<<per_sample, 64, 0, st>>>(t, B);
        k_events<<<b, kBlock, 0, st>>>(t, B);
        k_segsum<><<<grid, kBlock, 0, st>>>(N, nseg, B.diff, B.seg);
        k_segscan<<<per_sample, 64, 0, st>>>(B);
        k_score<<<grid, kBlock, 0, st>>>(t, B);
        k_tiecount<<<grid, kBlock, 0, st>>>(t, B);
        k_tiescan<<<per_sample, 64, 0, st>>>(t, B);
        k_tiewrite<<<grid, kBlock, 0, st>>>(t, B);
        k_final<<<per_sample, 64, 0, st>>>(B);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(hipMemcpyAsync(epps + b0, S->epps.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(nsize + b0, S->nsize.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(tie_count + b0, S->tcount.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (cap) UGP_HIP_TRY(hipMemcpyAsync(tie_dfs + b0 * cap, S->ties.p, (size_t)b * cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
    }
    return UGP_OK;
}

}  // namespace ugp
