// ugp_scan.hpp -- the block scans and the segmented flag scan that the dense searches and the matUtils queries share.
// Part of ugp_dense.hpp, which includes it behind DBuf, kBlock and kSeg; it is not included on its own.
#pragma once

namespace ugp {

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }
inline uint32_t segs_for(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, (n + kSeg - 1) / kSeg); }
inline unsigned bits_for(uint64_t v) { unsigned b = 1; while (b < 64 && (v >> b)) b++; return b; }   // v < 2^b

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
// Inclusive scan over the block (kBlock threads); *total = block sum.  Uses sh[kBlock / 64].  Unsigned sums wrap.
template <typename T>
__device__ __forceinline__ T block_incl_scan(T v, T *sh, T *total) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const T x = wave_incl_scan(v);
    if (lane == 63) sh[w] = x;
    __syncthreads();
    T pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < (int)(kBlock / 64); k++) { const T s = sh[k]; if (k < w) pre += s; tot += s; }
    __syncthreads();
    *total = tot;
    return x + pre;
}

// One block per (segment blockIdx.x, row blockIdx.y): the sum of the row's array x ([rows][n]) over the segment.  (The kernels
// here are templates so that they are compiled where they are launched.)
template <typename T>
__global__ void __launch_bounds__(kBlock) k_segsum(uint32_t n, uint32_t nseg, const T *x, T *seg) {
    __shared__ T sh[kBlock / 64];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const uint32_t lo = g * kSeg, hi = min(n, lo + kSeg);
    x += (size_t)s * n;
    T acc = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) acc += x[i];
    T tot;
    (void)block_incl_scan(acc, sh, &tot);
    if (threadIdx.x == 0) seg[(size_t)s * nseg + g] = tot;
}

// The sum of the segments before g (the carry), by the whole block.
template <typename T>
__device__ __forceinline__ T seg_carry(const T *seg, uint32_t g, T *sh) {
    T acc = 0;
    for (uint32_t k = threadIdx.x; k < g; k += kBlock) acc += seg[k];
    T tot;
    (void)block_incl_scan(acc, sh, &tot);
    return tot;
}

// ---- the flag scan: per item the flags set in front of it, kSeg items per block ---------------------------------------------

// One block per segment: the flags set in it.
template <typename = void>
__global__ void __launch_bounds__(kBlock) k_flag_segsum(uint32_t n, const uint8_t *flag, uint32_t *seg) {
    __shared__ uint32_t sh[kBlock / 64];
    const uint32_t lo = blockIdx.x * kSeg, hi = min(n, lo + kSeg);
    uint32_t acc = 0, tot;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) acc += flag[i] ? 1 : 0;
    (void)block_incl_scan(acc, sh, &tot);
    if (threadIdx.x == 0) seg[blockIdx.x] = tot;
}

// The block walks the items i of segment g: f(i, before, set) sees every one with the flags set before it (the carry: the
// segments before).  Returns the flags set up to the end of the segment.
template <class F>
__device__ __forceinline__ uint32_t scan_flag_segment(uint32_t n, const uint8_t *flag, const uint32_t *seg, uint32_t g, F f) {
    __shared__ uint32_t sh[kBlock / 64];
    const uint32_t lo = g * kSeg, hi = min(n, lo + kSeg);
    uint32_t carry = seg_carry(seg, g, sh), tot;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const uint32_t s = (i < hi && flag[i]) ? 1 : 0;
        const uint32_t incl = block_incl_scan(s, sh, &tot);
        if (i < hi) f(i, carry + (incl - s), s != 0);
        carry += tot;
    }
    return carry;
}
// Does segment g hold the last of n items?  Its block writes the total.
__device__ __forceinline__ bool last_segment(uint32_t n, uint32_t g) { return min(n, g * kSeg + kSeg) == n; }

// One block per segment: out[i] = flags set before i, out[n] = all of them.
template <typename = void>
__global__ void __launch_bounds__(kBlock) k_flag_scan(uint32_t n, const uint8_t *flag, const uint32_t *seg, uint32_t *out) {
    const uint32_t all = scan_flag_segment(n, flag, seg, blockIdx.x, [=](uint32_t i, uint32_t before, bool) { out[i] = before; });
    if (last_segment(n, blockIdx.x) && threadIdx.x == 0) out[n] = all;
}

// out[i] = flags set before i, out[n] = all (n + 1 values); seg is the workspace.
template <typename = void>
hipError_t scan_flags(DBuf<uint32_t> &seg, uint32_t n, const uint8_t *flag, uint32_t *out, hipStream_t st) {
    const uint32_t nseg = segs_for(n);
    const hipError_t e = seg.alloc(nseg);
    if (e != hipSuccess) return e;
    k_flag_segsum<<<nseg, kBlock, 0, st>>>(n, flag, seg.p);
    k_flag_scan<<<nseg, kBlock, 0, st>>>(n, flag, seg.p, out);
    return hipGetLastError();
}

}  // namespace ugp
