// ugp_coarse.hip -- k_coarse_sparse: the locality pre-pass of a plain batch from the samples' own rows (ugp_coarse.hpp has the
// algebra, the record layouts and the host restatement the tests hold against the oracle).
#include <hip/hip_runtime.h>

#include "ugp_coarse.hpp"
#include "ugp_kernels.hpp"

namespace ugp {

namespace {
constexpr int CS_LANES = 16;   // lanes per sample: a sample has a few dozen rows and boundaries -- as k_descend<16>
constexpr int CS_GROUPS = 64 / CS_LANES;

__device__ __forceinline__ uint32_t group_min(uint32_t v) {
#pragma unroll
    for (int m = CS_LANES / 2; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, CS_LANES));
    return v;
}
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
    for (int m = CS_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, CS_LANES);
    return v;
}
}  // namespace

// One sample per group of 16 lanes, one-wave blocks (next to the persistent walks of the batches in front a CU has room for about
// one more wave: see k_descend).  LDS per group: cap boundary records (4 bytes) and their running shifts (2 bytes); cap is a power
// of two and at least twice the largest number of events a sample of the call can have (the plan's capacity rule) -- the launcher
// checks that, so no record is ever dropped (the bounds test in front of the store only keeps a broken caller inside the LDS).
__global__ void __launch_bounds__(64) k_coarse_sparse(CoarseSparseArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cs_lds[];
    __shared__ uint32_t cs_count[CS_GROUPS];
    const uint32_t lane = threadIdx.x, g = lane / CS_LANES, gl = lane % CS_LANES;
    uint32_t *rec = cs_lds + (size_t)g * a.cap;
    int16_t *pre = (int16_t *)(cs_lds + (size_t)CS_GROUPS * a.cap) + (size_t)g * a.cap;
    const uint32_t q = blockIdx.x * CS_GROUPS + g;
    const bool live = q < a.n_queries;
    if (gl == 0) cs_count[g] = 0;
    __syncthreads();

    // 1. D(bottom) and the boundary records of the rows that hit a coarse site
    // (a set without rows has no row arrays, or those of the batch before it: nothing of them is read.  A set whose row check
    // failed is placed as if it had no rows, as the scatter kernels build it)
    const bool no_rows = a.n_ent == 0 || !a.ent_off || (a.err && *a.err != ~0ull);
    const uint64_t rb = (live && !no_rows) ? a.ent_off[q] : 0, re = (live && !no_rows) ? min((uint64_t)a.ent_off[q + 1], a.n_ent) : rb;
    int mism = 0;
    for (uint64_t r = rb + gl; r < re; r += CS_LANES) {
        const int32_t p = a.pos[r];
        const uint32_t miss = a.is_missing[r], S = miss ? 15u : (uint32_t)a.nuc[r];
        if (!miss && (S & a.ref[r]) == 0) mism++;
        const int32_t site = (p >= 0 && (uint32_t)p <= a.max_pos) ? a.pos2site[p] : -1;
        if (site < 0) continue;
        const uint32_t e0 = a.site_off[site], e1 = a.site_off[site + 1];
        if (e0 == e1) continue;
        uint32_t at = atomicAdd(&cs_count[g], 2u * (e1 - e0));
        for (uint32_t e = e0; e < e1; e++, at += 2) {
            const uint2 ev = a.events[e];
            uint32_t s, en;
            coarse_boundaries(ev.x, ev.y, S, s, en);
            if (at + 2 <= a.cap) { rec[at] = s; rec[at + 1] = en; }
        }
    }
    const int d_bottom = group_sum(mism);
    __syncthreads();
    const uint32_t n = min(cs_count[g], a.cap);

    // 2. sort: a bitonic network over the largest count of the wave's four samples (the loops stay wave-uniform)
    uint32_t n_max = max(n, (uint32_t)__shfl_xor((int)n, 16));
    n_max = max(n_max, (uint32_t)__shfl_xor((int)n_max, 32));
    uint32_t np = 2;
    while (np < n_max) np <<= 1;   // (np <= cap: cap is a power of two >= every count)
    for (uint32_t i = n + gl; i < np; i += CS_LANES) rec[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t k = 2; k <= np; k <<= 1)
        for (uint32_t j = k >> 1; j >= 1; j >>= 1) {
            for (uint32_t t = gl; t < np / 2; t += CS_LANES) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;   // the t-th pair of this step
                const uint32_t x = rec[i], y = rec[l];
                if ((x > y) == ((i & k) == 0)) { rec[i] = y; rec[l] = x; }
            }
            __syncthreads();
        }

    // 3. the running shift behind every boundary
    {
        const uint32_t per = max(np / CS_LANES, 1u), b = gl * per, e = min(b + per, n);
        int sum = 0;
        for (uint32_t i = b; i < e; i++) sum += coarse_rec_shift(rec[i]);
        int run = sum;   // inclusive scan over the group's lanes
#pragma unroll
        for (int d = 1; d < CS_LANES; d <<= 1) { const int v = __shfl_up(run, d, CS_LANES); if ((int)gl >= d) run += v; }
        run -= sum;
        for (uint32_t i = b; i < e; i++) { run += coarse_rec_shift(rec[i]); pre[i] = (int16_t)run; }
    }
    __syncthreads();

    // 4.-6. one candidate per stretch between two boundaries (the stretch in front of the first and the tail included; the root
    // is part of the first stretch unless it carries an event), and one per event node
    uint32_t best = kCoarseNoKey;
    for (uint32_t i = gl; i <= n; i += CS_LANES) {
        const uint32_t r0 = i ? rec[i - 1] : 0u, r1 = i < n ? rec[i] : 0u;
        const uint32_t lo = i ? coarse_rec_pos(r0) + (coarse_rec_is_start(r0) ? 1u : 0u) : 0u;
        const uint32_t hi = i < n ? coarse_rec_pos(r1) : a.n_nodes;
        const int before = i ? (int)pre[i - 1] : 0;
        best = min(best, coarse_range_candidate(a.rmq, a.n_nodes, lo, min(hi, a.n_nodes), before + d_bottom));
        if (i < n && coarse_rec_is_start(r1) && (i == 0 || (r0 >> kCoarseKeyShift) != (r1 >> kCoarseKeyShift))) {   // the first event of a node
            int sum_shift = 0, sum_dneg = 0, sum_dcom = 0;
            for (uint32_t k = i; k < n; k++) {
                const uint32_t rk = rec[k];
                if ((rk >> kCoarseKeyShift) != (r1 >> kCoarseKeyShift)) break;
                sum_shift += coarse_rec_shift(rk); sum_dneg += coarse_rec_dneg(rk); sum_dcom += coarse_rec_dcom(rk);
            }
            const uint32_t d = min(coarse_rec_pos(r1), a.n_nodes - 1);
            const uint2 nd = a.node[d];
            best = min(best, coarse_node_candidate(nd.x, nd.y, d, coarse_rec_root(r1), d_bottom, before, sum_shift, sum_dneg, sum_dcom));
        }
    }

    // 7. the smallest cost, at equal costs the first node of the depth-first order: the node the walked pass names
    best = group_min(best);
    if (live && gl == 0) a.out[q] = ugp_result{(int32_t)(best >> 16), 1u, a.dfs2bfs[min(best & 0xFFFFu, a.n_nodes - 1)], 0u};
}

size_t coarse_sparse_lds_bytes(uint32_t cap) { return (size_t)CS_GROUPS * cap * 6; }

hipError_t launch_coarse_sparse(const CoarseSparseArgs &a, hipStream_t s) {
    if (!a.n_queries) return hipSuccess;
    if (a.cap < 2 || (a.cap & (a.cap - 1)) || a.cap > 2 * kCoarseSparseMaxEvents || !a.n_nodes || a.n_nodes > kCoarseSparseMaxNodes) return hipErrorInvalidValue;
    if (2 * a.max_rows * a.max_per_pos > a.cap) return hipErrorInvalidValue;   // (every sample's records fit: none is ever dropped)
    hipLaunchKernelGGL(k_coarse_sparse, dim3((a.n_queries + CS_GROUPS - 1) / CS_GROUPS), dim3(64), coarse_sparse_lds_bytes(a.cap), s, a);
    return hipGetLastError();
}

}  // namespace ugp
