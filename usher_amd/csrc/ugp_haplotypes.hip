// ugp_haplotypes.hip -- matUtils summary --haplotype (matUtils/summary.cpp: count_haplotypes :182-218, write_haplotype_table :244-264)
// on the device.
//
// The reference copies a std::map<int,int8_t> from the parent into every node and counts the leaves in a map keyed by whole maps.
// Here the haplotype of a node -- the (position, allele) pairs off the reference at the end of its root path (usher_amd.h) -- differs
// from its parent's by something local to the node's own entries: an entry off its reference adds its pair, and when the state above
// it was off its reference (mbits bits 16-24, from the owner above) that pair leaves.  With H a fixed 128-bit mix of a pair, the sum
// of H over the set is a FINGERPRINT that a prefix sum over the depth-first order gives for every node at once: +d(v) at position v,
// -d(v) at dend[v], d(v) the sum of the node's own differences.  All sums wrap modulo 2^64, so their order is free.
//   k_hp_diff                      per node d(v) in three lanes (two of the mix, one the size of the set), added at v and taken away at
//                                  dend[v] with integer atomics;
//   k_segsum / k_hp_scan           the inclusive scan over the depth-first positions, in place, kSeg positions per block (the
//                                  segment sums, the carry and the block scan are those of ugp_scan.hpp, over 64-bit wrapping sums);
//   k_hp_gather / (rocprim radix sort, twice)     the leaves ordered by (fingerprint, depth-first rank): the low lane, then stably
//                                  the high lane;
//   k_hp_heads / (scan_flags, ugp_scan.hpp)       the first leaf of every run of equal fingerprints and the runs in front of each;
//   k_hp_verify                    every other leaf against the leaf in front of it, exactly: up both paths to the lowest common
//                                  ancestor, every entry's position looked up for both leaves among the position's owners;
//   k_hp_runs / (radix sort) / k_hp_emit          one record per run, in depth-first order of the run's first leaf;
//   k_hp_sizes / k_hp_fill / (rocprim segmented sort)     the sets of given leaves: sizes from the third lane, pairs by a climb of the
//                                  root path that keeps an entry when the lookup from the leaf names that very entry.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_haplotypes.hpp"
#include "ugp_sort.hpp"
#include "ugp_translate.hpp"

namespace ugp {
namespace {

constexpr uint64_t kSeedA = 0x9e3779b97f4a7c15ull, kSeedB = 0xd6e8feb86659fd93ull;   // fixed: the fingerprints are reproducible
constexpr uint64_t kDefaultLeaves = 1ull << 18;   // leaves per launch window of the sets
constexpr uint64_t kWindowEntries = 1ull << 27;   // set entries per launch window, at most (a window holds at least one leaf)

__device__ __forceinline__ uint64_t mix64(uint64_t x) {   // the finalizer of splitmix64
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// H(pos, allele): two independent mixes
__device__ __forceinline__ void pair_hash(int32_t pos, uint32_t nuc, uint64_t *a, uint64_t *b) {
    const uint64_t x = ((uint64_t)(uint32_t)pos << 8) | nuc;
    *a = mix64(x + kSeedA);
    *b = mix64((x ^ kSeedB) * 0xff51afd7ed558ccdull + kSeedB);
}

// Per node: its difference, added at its own position and taken away where its subtree ends.  x* are zero before.
__global__ void k_hp_diff(DfsView t, unsigned long long *xa, unsigned long long *xb, unsigned long long *xs) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= t.n) return;
    uint64_t da = 0, db = 0, ds = 0;
    for (uint32_t e = t.moff[v], end = t.moff[v + 1]; e < end; e++) {
        const int32_t p = t.mpos[e];
        if (p < 0) continue;
        const uint32_t bits = t.mbits[e];
        uint64_t a, b;
        if (b_nuc(bits) != b_ref(bits)) { pair_hash(p, b_nuc(bits), &a, &b); da += a; db += b; ds += 1; }
        if (b_ancne(bits)) { pair_hash(p, b_anc(bits), &a, &b); da -= a; db -= b; ds -= 1; }
    }
    if (!(da | db | ds)) return;
    atomicAdd(&xa[v], da); atomicAdd(&xb[v], db); atomicAdd(&xs[v], ds);
    const uint32_t end = t.dend[v];
    if (end < t.n) { atomicAdd(&xa[end], 0ull - da); atomicAdd(&xb[end], 0ull - db); atomicAdd(&xs[end], 0ull - ds); }
}

// One block per (segment, lane): the inclusive scan of the lane's array, in place (the carry: the segments before).
__global__ void __launch_bounds__(kBlock) k_hp_scan(uint32_t n, uint32_t nseg, uint64_t *x, const uint64_t *seg) {
    __shared__ uint64_t sh[kBlock / 64];
    const uint32_t g = blockIdx.x, lo = g * kSeg, hi = min(n, lo + kSeg);
    x += (size_t)blockIdx.y * n;
    seg += (size_t)blockIdx.y * nseg;
    uint64_t carry = seg_carry(seg, g, sh), tot;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const uint64_t incl = block_incl_scan<uint64_t>(i < hi ? x[i] : 0, sh, &tot);
        if (i < hi) x[i] = carry + incl;
        carry += tot;
    }
}

// Sort input x: the leaf of rank vin[x] (vin NULL: rank x) with the masked lane of its fingerprint.
__global__ void k_hp_gather(uint32_t nl, const uint32_t *ldfs, const uint64_t *f, uint64_t mask, const uint32_t *vin, uint64_t *key, uint32_t *val) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nl) return;
    const uint32_t r = vin ? vin[x] : x;
    key[x] = f[ldfs[r]] & mask;
    val[x] = r;
}

// Per place x of the sorted leaves: is it the first of its masked fingerprint.
__global__ void k_hp_heads(uint32_t nl, const uint32_t *ldfs, const uint32_t *ord, const uint64_t *fa, const uint64_t *fb, uint64_t ma, uint64_t mb,
                           uint8_t *head) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nl) return;
    uint8_t h = 1;
    if (x) {
        const uint32_t u = ldfs[ord[x - 1]], v = ldfs[ord[x]];
        h = (((fa[u] ^ fa[v]) & ma) | ((fb[u] ^ fb[v]) & mb)) ? 1 : 0;
    }
    head[x] = h;
}

// The owner (kNil: none) in force at position p for node v, v's own included: the last owner of p not behind v in depth-first
// order, then up the owners above until one contains v.  (allele_above of ugp_translate.hip, inclusive.)
__device__ __forceinline__ uint32_t owner_at(const DfsView &t, const uint32_t *onode, uint32_t v, int32_t p) {
    if ((uint32_t)p >= t.tp) return kNil;
    const uint32_t lo = t.poff[p], x = lower_bound_u32(onode, lo, t.poff[p + 1], v + 1);
    uint32_t cur = x > lo ? t.pent[x - 1] : kNil;
    while (cur != kNil && v >= t.dend[t.mnode[cur]]) cur = t.mlink[cur];
    return cur;
}
// The allele of owner e when it is off its own reference, else 0.
__device__ __forceinline__ uint32_t off_ref(const DfsView &t, uint32_t e) {
    if (e == kNil) return 0;
    const uint32_t bits = t.mbits[e];
    return b_nuc(bits) != b_ref(bits) ? b_nuc(bits) : 0u;
}
// Do u and v agree at every position with an entry on the path from `from` up to (not including) the first node that holds `other`?
__device__ __forceinline__ bool paths_agree(const DfsView &t, const uint32_t *onode, uint32_t from, uint32_t other, uint32_t u, uint32_t v,
                                            uint32_t *visited) {
    for (uint32_t cur = from; !(cur <= other && other < t.dend[cur]); cur = t.dpar[cur]) {   // the root holds every node
        for (uint32_t e = t.moff[cur], end = t.moff[cur + 1]; e < end; e++) {
            const int32_t p = t.mpos[e];
            if (p < 0) continue;
            (*visited)++;
            if (off_ref(t, owner_at(t, onode, u, p)) != off_ref(t, owner_at(t, onode, v, p))) return false;
        }
    }
    return true;
}

// Places [1, nl) of the sorted leaves: a leaf that is not the first of its run against the leaf in front of it.
// counters[0] += the leaves that differ, counters[1] += the entries read.
__global__ void __launch_bounds__(kBlock) k_hp_verify(DfsView t, const uint32_t *onode, uint32_t nl, const uint32_t *ldfs, const uint32_t *ord,
                                                      const uint8_t *head, const uint64_t *fs, unsigned long long *counters) {
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    uint32_t visited = 0;
    if (x > 0 && x < nl && !head[x]) {
        const uint32_t u = ldfs[ord[x - 1]], v = ldfs[ord[x]];
        bad = (uint32_t)fs[u] != (uint32_t)fs[v] || !paths_agree(t, onode, u, v, u, v, &visited) || !paths_agree(t, onode, v, u, u, v, &visited);
    }
    // one atomic per wave and counter
    const unsigned long long votes = __ballot(bad);
    uint32_t sum = visited;
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63u) == 0) {
        if (votes) atomicAdd(&counters[0], (unsigned long long)__popcll(votes));
        if (sum) atomicAdd(&counters[1], (unsigned long long)sum);
    }
}

// hidx = heads before x.  Run r = hidx[x] of a head x: its first leaf's rank (the key of the second sort), its start; rstart[runs] = nl.
__global__ void k_hp_runs(uint32_t nl, const uint32_t *ord, const uint8_t *head, const uint32_t *hidx, uint32_t *rkey, uint32_t *rval, uint32_t *rstart) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x > nl) return;
    if (x == nl) { rstart[hidx[nl]] = nl; return; }
    if (!head[x]) return;
    const uint32_t r = hidx[x];
    rkey[r] = ord[x];
    rval[r] = r;
    rstart[r] = x;
}

// Record j of the runs sorted by their first leaf's rank, while below `fill`.
__global__ void k_hp_emit(uint32_t fill, const uint32_t *rkey, const uint32_t *rval, const uint32_t *rstart, const uint32_t *ldfs,
                          const uint32_t *d2b, const uint64_t *fs, ugp_hp_group *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= fill) return;
    const uint32_t r = rval[j], v = ldfs[rkey[j]];
    out[j] = ugp_hp_group{d2b[v], rstart[r + 1] - rstart[r], (uint32_t)fs[v], 0u};
}

__global__ void k_hp_sizes(uint32_t n, const uint32_t *node, const uint64_t *fs, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)fs[node[i]];
}

// Leaves [0, cnt) of a window: the pairs of leaf j go to kpos / knuc[woff[j] .. woff[j + 1]) in the order of the climb.
// *wrong += the leaves whose pairs are not as many as their size lane says.
__global__ void __launch_bounds__(kBlock) k_hp_fill(DfsView t, const uint32_t *onode, uint32_t cnt, const uint32_t *node, const uint32_t *woff,
                                                    uint32_t *kpos, uint8_t *knuc, uint32_t *wrong) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t v = node[j], end = woff[j + 1];
    uint32_t o = woff[j], extra = 0;
    for (uint32_t cur = v; cur != kNil; cur = t.dpar[cur]) {
        for (uint32_t e = t.moff[cur], eend = t.moff[cur + 1]; e < eend; e++) {
            const int32_t p = t.mpos[e];
            if (p < 0) continue;
            const uint32_t bits = t.mbits[e];
            if (b_nuc(bits) == b_ref(bits) || owner_at(t, onode, v, p) != e) continue;
            if (o < end) { kpos[o] = (uint32_t)p; knuc[o] = (uint8_t)b_nuc(bits); o++; }
            else extra++;
        }
    }
    if (o != end || extra) atomicAdd(wrong, 1u);
}

inline uint64_t low_mask(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; }

}  // namespace

struct HpState : QueryBase {
    std::vector<uint8_t> h_leaf;                  // by BFS index
    uint32_t nleaves = 0;
    uint64_t ndup = 0;
    uint32_t first_dup = kNil;                    // BFS index
    bool have_fp = false;
    DBuf<uint32_t> ldfs, d2b;                     // the depth-first position of leaf rank r; dfs2bfs
    DBuf<uint64_t> f, seg;                        // [3 n]: the fingerprint lanes a, b and the size lane, by depth-first position
    // per call
    DBuf<uint64_t> k0, k1;
    DBuf<uint32_t> v0, v1, v2, hidx, fseg, rkey, rkey2, rval, rval2, rstart;
    DBuf<uint8_t> head;
    DBuf<unsigned long long> counters;
    DBuf<ugp_hp_group> gout;
    DBuf<uint32_t> qnode, qsz, woff, kpos, spos, wrong;
    DBuf<uint8_t> knuc, snuc;
    DBuf<unsigned char> tmp;
    const uint32_t *ord = nullptr;                // the leaves' ranks in sorted order: v0, v1 or v2
    const uint64_t *fa() const { return f.p; }
    const uint64_t *fb() const { return f.p + T->n; }
    const uint64_t *fs() const { return f.p + 2 * (size_t)T->n; }
};

void hp_free(HpState *s) { query_free(s); }

int hp_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, HpState **out) {
    return query_attach("ugp_haplotypes_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out, NoCheck(), [&](HpState *S) {
        const uint32_t N = S->T->n;
        LeafRanks lr;
        leaf_ranks(tree, dfs2bfs, bfs2dfs, &lr);
        S->nleaves = (uint32_t)lr.leaf_dfs.size();
        S->h_leaf.assign(N, 0);
        for (uint32_t i : lr.leaf_dfs) S->h_leaf[dfs2bfs[i]] = 1;
        // the duplicate nodes: two non-masked entries at one position
        std::vector<int32_t> seen;
        for (uint32_t i = 0; i < N; i++) {
            const uint32_t b = dfs2bfs[i];
            seen.clear();
            bool dup = false;
            for (uint64_t k = tree->mut_off[b]; k < tree->mut_off[b + 1]; k++) {
                const int32_t p = tree->mut_pos[k];
                if (p < 0) continue;
                if (std::find(seen.begin(), seen.end(), p) != seen.end()) dup = true;
                else seen.push_back(p);
            }
            if (dup && !S->ndup++) S->first_dup = b;
        }
        const StreamDrain drain{S->stream};   // lr
        UGP_HIP_TRY(S->ldfs.upload(lr.leaf_dfs, S->stream));
        UGP_HIP_TRY(S->d2b.upload(dfs2bfs.data(), N, S->stream));
        UGP_HIP_TRY(hipStreamSynchronize(S->stream));   // lr is read until here
        return tr_owner_nodes(*tables, S->stream);
    });
}

// The fingerprints of every node: S->f.
static int pass_scan(HpState *S) {
    const DfsView t = S->T->view();
    const uint32_t N = t.n, nseg = segs_for(N);
    hipStream_t st = S->stream;
    UGP_HIP_TRY(S->f.alloc(3 * (size_t)N)); UGP_HIP_TRY(S->seg.alloc(3 * (size_t)nseg));
    UGP_HIP_TRY(hipMemsetAsync(S->f.p, 0, 3 * (size_t)N * sizeof(uint64_t), st));
    unsigned long long *x = reinterpret_cast<unsigned long long *>(S->f.p);
    k_hp_diff<<<blocks_for(N), kBlock, 0, st>>>(t, x, x + N, x + 2 * (size_t)N);
    k_segsum<<<dim3(nseg, 3), kBlock, 0, st>>>(N, nseg, S->f.p, S->seg.p);
    k_hp_scan<<<dim3(nseg, 3), kBlock, 0, st>>>(N, nseg, S->f.p, S->seg.p);
    UGP_HIP_TRY(hipGetLastError());
    S->have_fp = true;
    return UGP_OK;
}

static int sort_workspace(HpState *S) {
    const size_t L = S->nleaves;
    UGP_HIP_TRY(S->k0.alloc(L)); UGP_HIP_TRY(S->k1.alloc(L)); UGP_HIP_TRY(S->v0.alloc(L)); UGP_HIP_TRY(S->v1.alloc(L)); UGP_HIP_TRY(S->v2.alloc(L));
    UGP_HIP_TRY(S->head.alloc(L)); UGP_HIP_TRY(S->hidx.alloc(L + 1)); UGP_HIP_TRY(S->fseg.alloc(segs_for(L)));
    UGP_HIP_TRY(S->counters.alloc(2));
    return UGP_OK;
}

// The leaves by (low hash_bits of the fingerprint, rank): S->ord; the heads of their runs: S->head.
static int pass_sort(HpState *S, uint32_t hash_bits) {
    const uint32_t L = S->nleaves;
    hipStream_t st = S->stream;
    const uint32_t bits_a = std::min<uint32_t>(hash_bits, 64), bits_b = hash_bits - bits_a;
    const uint64_t ma = low_mask(bits_a), mb = low_mask(bits_b);
    k_hp_gather<<<blocks_for(L), kBlock, 0, st>>>(L, S->ldfs.p, S->fa(), ma, nullptr, S->k0.p, S->v0.p);
    UGP_HIP_TRY(hipGetLastError());
    S->ord = S->v0.p;
    if (bits_a) {
        UGP_HIP_TRY(sort_pairs(S->tmp, S->k0.p, S->k1.p, S->v0.p, S->v1.p, L, bits_a, st));
        S->ord = S->v1.p;
    }
    if (bits_b) {   // stable: equal high lanes keep the order of the low lane, equal fingerprints that of the ranks
        k_hp_gather<<<blocks_for(L), kBlock, 0, st>>>(L, S->ldfs.p, S->fb(), mb, S->v1.p, S->k0.p, S->v0.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(sort_pairs(S->tmp, S->k0.p, S->k1.p, S->v0.p, S->v2.p, L, bits_b, st));
        S->ord = S->v2.p;
    }
    k_hp_heads<<<blocks_for(L), kBlock, 0, st>>>(L, S->ldfs.p, S->ord, S->fa(), S->fb(), ma, mb, S->head.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

static int pass_verify(HpState *S) {
    hipStream_t st = S->stream;
    UGP_HIP_TRY(hipMemsetAsync(S->counters.p, 0, 2 * sizeof(unsigned long long), st));
    k_hp_verify<<<blocks_for(S->nleaves), kBlock, 0, st>>>(S->T->view(), S->T->onode.p, S->nleaves, S->ldfs.p, S->ord, S->head.p, S->fs(), S->counters.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

static int hp_ready(HpState *S, const char *who) { return query_ready(S, who, "haplotypes"); }

static int refuse_duplicates(const HpState *S, const char *who) {
    return set_error(UGP_ERR_UNSUPPORTED, std::string(who) + ": " + std::to_string(S->ndup) +
                                              " nodes with two entries at one position: the closed form does not hold");
}

int hp_groups(HpState *S, ugp_hp_group *out, uint64_t cap, uint64_t *n_out, ugp_hp_info *info, uint32_t hash_bits) {
    if (int rc = hp_ready(S, "ugp_haplotype_groups")) return rc;
    if (!n_out || (cap && !out)) return set_error(UGP_ERR_INVALID, "null argument");
    if (hash_bits > 128) return set_error(UGP_ERR_INVALID, "hash_bits above 128");
    *n_out = 0;
    const uint32_t L = S->nleaves;
    ugp_hp_info I{L, 0, 0, S->ndup, 0, S->first_dup, 0};
    if (info) *info = I;
    if (S->ndup) return refuse_duplicates(S, "ugp_haplotype_groups");
    UGP_HIP_TRY(hipSetDevice(S->device));
    hipStream_t st = S->stream;
    if (int rc = sort_workspace(S)) return rc;
    if (int rc = pass_scan(S)) return rc;
    if (int rc = pass_sort(S, hash_bits)) return rc;
    if (int rc = pass_verify(S)) return rc;
    UGP_HIP_TRY(scan_flags(S->fseg, L, S->head.p, S->hidx.p, st));
    uint32_t runs = 0;
    unsigned long long counters[2] = {0, 0};
    UGP_HIP_TRY(hipMemcpyAsync(&runs, S->hidx.p + L, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipMemcpyAsync(counters, S->counters.p, sizeof(counters), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));
    I.n_groups = runs;
    I.n_collisions = counters[0];
    I.n_visited = counters[1];
    if (info) *info = I;
    if (I.n_collisions)
        return set_error(UGP_ERR_UNSUPPORTED, "ugp_haplotype_groups: " + std::to_string(I.n_collisions) +
                                                  " leaves differ from the leaf their fingerprint groups them with: no table");
    *n_out = runs;
    const uint32_t fill = (uint32_t)std::min<uint64_t>(cap, runs);
    if (!fill) return UGP_OK;
    UGP_HIP_TRY(S->rkey.alloc(runs)); UGP_HIP_TRY(S->rkey2.alloc(runs)); UGP_HIP_TRY(S->rval.alloc(runs)); UGP_HIP_TRY(S->rval2.alloc(runs));
    UGP_HIP_TRY(S->rstart.alloc((size_t)runs + 1)); UGP_HIP_TRY(S->gout.alloc(fill));
    k_hp_runs<<<blocks_for((uint64_t)L + 1), kBlock, 0, st>>>(L, S->ord, S->head.p, S->hidx.p, S->rkey.p, S->rval.p, S->rstart.p);
    UGP_HIP_TRY(hipGetLastError());
    UGP_HIP_TRY(sort_pairs(S->tmp, S->rkey.p, S->rkey2.p, S->rval.p, S->rval2.p, runs, bits_for(L), st));
    k_hp_emit<<<blocks_for(fill), kBlock, 0, st>>>(fill, S->rkey2.p, S->rval2.p, S->rstart.p, S->ldfs.p, S->d2b.p, S->fs(), S->gout.p);
    UGP_HIP_TRY(hipGetLastError());
    UGP_HIP_TRY(hipMemcpyAsync(out, S->gout.p, (size_t)fill * sizeof(ugp_hp_group), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));
    return UGP_OK;
}

int hp_sets(HpState *S, const uint32_t *leaves, uint64_t n, uint64_t *off, int32_t *pos, uint8_t *nuc, uint64_t cap, uint64_t *n_out,
            uint64_t chunk_leaves) {
    if (int rc = hp_ready(S, "ugp_haplotype_sets")) return rc;
    if (!n_out || !off || (n && !leaves) || (cap && (!pos || !nuc))) return set_error(UGP_ERR_INVALID, "null argument");
    const uint32_t N = S->T->n;
    if (n >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "more than 2^31 leaves listed");
    for (uint64_t i = 0; i < n; i++) {
        if (leaves[i] >= N) return set_error(UGP_ERR_INVALID, "ugp_haplotype_sets: node index out of range");
        if (!S->h_leaf[leaves[i]]) return set_error(UGP_ERR_INVALID, "ugp_haplotype_sets: node " + std::to_string(leaves[i]) + " is not a leaf");
    }
    *n_out = 0;
    if (S->ndup) return refuse_duplicates(S, "ugp_haplotype_sets");
    off[0] = 0;
    if (!n) return UGP_OK;
    try {
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        if (!S->have_fp) if (int rc = pass_scan(S)) return rc;
        std::vector<uint32_t> node(n), sz(n), woff;
        for (uint64_t i = 0; i < n; i++) node[i] = S->T->bfs2dfs[leaves[i]];
        UGP_HIP_TRY(S->qnode.upload(node, st)); UGP_HIP_TRY(S->qsz.alloc(n)); UGP_HIP_TRY(S->wrong.alloc(1));
        UGP_HIP_TRY(hipMemsetAsync(S->wrong.p, 0, sizeof(uint32_t), st));
        k_hp_sizes<<<blocks_for(n), kBlock, 0, st>>>((uint32_t)n, S->qnode.p, S->fs(), S->qsz.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(hipMemcpyAsync(sz.data(), S->qsz.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + sz[i];
        *n_out = off[n];
        const uint64_t win = std::min<uint64_t>(chunk_leaves ? chunk_leaves : kDefaultLeaves, n);
        const DfsView t = S->T->view();
        const unsigned pbits = bits_for(t.tp);
        for (uint64_t i0 = 0; i0 < n && off[i0] < cap;) {
            uint64_t i1 = i0 + 1;
            while (i1 < n && i1 - i0 < win && off[i1 + 1] - off[i0] <= kWindowEntries) i1++;
            const uint32_t cnt = (uint32_t)(i1 - i0);
            const uint64_t went = off[i1] - off[i0];
            if (went >= (1ull << 31)) return set_error(UGP_ERR_UNSUPPORTED, "ugp_haplotype_sets: a set of more than 2^31 pairs");
            if (went) {
                woff.resize((size_t)cnt + 1);
                for (uint32_t j = 0; j <= cnt; j++) woff[j] = (uint32_t)(off[i0 + j] - off[i0]);
                UGP_HIP_TRY(S->woff.upload(woff, st));
                UGP_HIP_TRY(S->kpos.alloc(went)); UGP_HIP_TRY(S->spos.alloc(went)); UGP_HIP_TRY(S->knuc.alloc(went)); UGP_HIP_TRY(S->snuc.alloc(went));
                k_hp_fill<<<blocks_for(cnt), kBlock, 0, st>>>(t, S->T->onode.p, cnt, S->qnode.p + i0, S->woff.p, S->kpos.p, S->knuc.p, S->wrong.p);
                UGP_HIP_TRY(hipGetLastError());
                size_t bytes = 0;
                UGP_HIP_TRY(rocprim::segmented_radix_sort_pairs(nullptr, bytes, S->kpos.p, S->spos.p, S->knuc.p, S->snuc.p, (unsigned)went, cnt,
                                                                S->woff.p, S->woff.p + 1, 0u, pbits, st));
                UGP_HIP_TRY(S->tmp.alloc(bytes));
                UGP_HIP_TRY(rocprim::segmented_radix_sort_pairs(S->tmp.p, bytes, S->kpos.p, S->spos.p, S->knuc.p, S->snuc.p, (unsigned)went, cnt,
                                                                S->woff.p, S->woff.p + 1, 0u, pbits, st));
                const uint64_t take = std::min<uint64_t>(went, cap - off[i0]);
                UGP_HIP_TRY(hipMemcpyAsync(pos + off[i0], S->spos.p, take * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                UGP_HIP_TRY(hipMemcpyAsync(nuc + off[i0], S->snuc.p, take, hipMemcpyDeviceToHost, st));
                UGP_HIP_TRY(hipStreamSynchronize(st));   // woff is read until here
            }
            i0 = i1;
        }
        uint32_t wrong = 0;
        UGP_HIP_TRY(hipMemcpyAsync(&wrong, S->wrong.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        if (wrong) return set_error(UGP_ERR_HIP, "ugp_haplotype_sets: " + std::to_string(wrong) + " sets do not have the size their fingerprint carries");
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

int hp_time(HpState *S, uint32_t reps, double *scan_ms, double *sort_ms, double *verify_ms) {
    if (int rc = hp_ready(S, "ugp_haplotype_time")) return rc;
    if (!reps || !scan_ms || !sort_ms || !verify_ms) return set_error(UGP_ERR_INVALID, "null argument");
    *scan_ms = *sort_ms = *verify_ms = 0;
    if (S->ndup) return refuse_duplicates(S, "ugp_haplotype_time");
    UGP_HIP_TRY(hipSetDevice(S->device));
    hipStream_t st = S->stream;
    if (int rc = sort_workspace(S)) return rc;
    const char *who = "ugp_haplotype_time";   // each stage reads what the stage before it left
    if (int rc = timed(st, who, reps, scan_ms, [&] { return pass_scan(S); })) return rc;
    if (int rc = timed(st, who, reps, sort_ms, [&] { return pass_sort(S, 128); })) return rc;
    return timed(st, who, reps, verify_ms, [&] { return pass_verify(S); });
}

}  // namespace ugp
