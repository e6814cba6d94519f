// ugp_dense.hpp -- what the device query families share on the device and in their tables (ugp_query.hpp: the host code around
// them), and the helpers RIPPLES (ugp_ripples.hip) reads too: device buffers, the error macro, the entry bits and loop 2 of mapper2_body, the scans (ugp_scan.hpp), the
// depth-first tables of a handle's tree and the literal score of one node against one sample.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "usher_amd.h"

namespace ugp {

int set_error(int code, const std::string &msg);   // ugp_capi.cpp

#define UGP_HIP_TRY(expr)                                                                                     \
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
    hipError_t upload(const T *v, size_t count, hipStream_t st) {
        hipError_t e = alloc(count);
        if (e != hipSuccess || !count) return e;
        return hipMemcpyAsync(p, v, count * sizeof(T), hipMemcpyHostToDevice, st);
    }
    hipError_t upload(const std::vector<T> &v, hipStream_t st) { return upload(v.data(), v.size(), st); }
};

constexpr uint32_t kBlock = 256;     // threads per block (4 waves)
constexpr uint32_t kSeg = 16384;     // depth-first positions per segment of the dense searches
constexpr int32_t kNone = INT_MAX;   // score of a node that is not a candidate
constexpr uint32_t kNil = UINT32_MAX;

// ---- entry bits and loop 2 ----------------------------------------------------------------------------------------

// Entry bits: mutated base | ref << 8 | parent state (0 = none on the root path) << 16 | [parent state != its ref] << 24
__device__ __forceinline__ uint32_t b_nuc(uint32_t b) { return b & 0xffu; }
__device__ __forceinline__ uint32_t b_ref(uint32_t b) { return (b >> 8) & 0xffu; }
__device__ __forceinline__ uint32_t b_anc(uint32_t b) { return (b >> 16) & 0xffu; }
__device__ __forceinline__ int b_ancne(uint32_t b) { return (int)((b >> 24) & 1u); }

__host__ __device__ __forceinline__ uint32_t lowbit4(uint32_t a) {
    for (uint32_t b = 0; b < 4; b++) if (a & (1u << b)) return 1u << b;
    return 0;   // the reference leaves it uninitialised; the oracle (and this library) read 0
}
// Loop 2 of mapper2_body for one sample row (allele a, reference r) against the state s its position has (r: none).
__host__ __device__ __forceinline__ int row_cost(uint32_t a, uint32_t r, uint32_t s) {
    if (a & s) return 0;
    return ((a & r) ? r : lowbit4(a)) != s ? 1 : 0;
}

}  // namespace ugp

// ---- scans: block_incl_scan, k_segsum, seg_carry, the flag scan and the launch sizes ------------------------------
#include "ugp_scan.hpp"

namespace ugp {

// First index in [lo, hi) of the sorted xs with xs[k] >= v.
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *xs, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (xs[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the depth-first tables of a handle's tree --------------------------------------------------------------------

// Entry flags
constexpr uint8_t kCounts = 1;   // annotate's walk takes it and it has ref != mut
constexpr uint8_t kOwner = 2;    // first non-masked entry of its position on its node

struct DfsView {   // device tables, indexed by depth-first position / depth-first entry index
    uint32_t n, tp;   // nodes; positions 0 .. tp-1 carry entries
    const uint32_t *dpar, *dend, *depth, *cum, *moff, *mbits, *mnode, *mlink, *morig, *poff, *pent;
    const int32_t *mpos, *nrp;
    const uint8_t *mflag, *leaf;
};

// Built by the first attach of a handle, of whichever family, and read by all.  Entries follow their nodes' depth-first
// order, and their stored order within a node (morig: index in the caller's CSR).  The OWNER of a position on a node is its
// first non-masked entry there; poff / pent list the owners by position, in depth-first order of their node.  An owner's
// parent state (mbits bits 16-24) and mlink come from the nearest owner above it at its position.  nrp[v] counts the
// positions off the reference on the root path of v's parent; cum[v] the entries on v's root path.  When no branch has two
// non-masked entries at one position (literal_ok), the owners are exactly the non-masked entries.
struct DfsTables {
    int device = 0;
    uint32_t n = 0, tp = 0, root_muts = 0;
    uint64_t m = 0;
    bool literal_ok = true;
    std::vector<uint32_t> bfs2dfs, h_cum;
    DBuf<uint32_t> dpar, dend, depth, cum, moff, mbits, mnode, mlink, morig, poff, pent;
    DBuf<int32_t> mpos, nrp;
    DBuf<uint8_t> mflag, leaf;
    DBuf<uint32_t> onode;      // per slot of pent the owner's node; made by the first translate or select attach (tr_owner_nodes)
    bool have_onode = false;
    DfsView view() const {
        return DfsView{n, tp, dpar.p, dend.p, depth.p, cum.p, moff.p, mbits.p, mnode.p, mlink.p, morig.p, poff.p, pent.p,
                       mpos.p, nrp.p, mflag.p, leaf.p};
    }
};

// Checks `tree` (fewer than 2^entry_bits mutation entries) and, unless *tables exists, builds the tables on `device`.
int dfs_tables(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               int entry_bits, DfsTables **tables);
void dfs_tables_free(DfsTables *t);
// The handle's tables may be older than the attach that reads the caller's arrays THROUGH them (morig, pent): UGP_OK when `t` was
// built from exactly the mutation arrays of `tree` (compared entry by entry, and each node's first entry with its offset: the same
// entries on other nodes are other arrays), else UGP_ERR_INVALID naming the call `who`.  Every dense attach calls it.
int dfs_tables_same_arrays(const DfsTables &t, const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const char *who);

// The leaf-rank ranges select and mask read: leaf r is the r-th leaf in depth-first order, lbefore[i] ([n + 1]) the leaves in front of
// depth-first position i, dend[i] ([n]) the end of position i's subtree, leaf_dfs[r] the depth-first position of leaf r.
struct LeafRanks { std::vector<uint32_t> lbefore, dend, leaf_dfs; };
void leaf_ranks(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, LeafRanks *out);

// What mask and subtree read: per depth-first entry (its node's depth-first order, stored order within the node) the stored parent
// allele << 4 | allele.  Refuses an allele above 15, naming the call `who`.
int stored_alleles(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const DfsTables &T, const char *who, std::vector<uint8_t> *mpn);
// What genotypes, summary and translate ask of the caller's arrays: mut_par is there (else UGP_ERR_INVALID with the sentence `needs`)
// and the codes of every non-masked entry lie in 1 .. 15.
int coded_alleles(const ugp_tree_desc *tree, const DfsTables &T, const std::string &needs);

// ---- the literal score: loop 1 run literally, loops 2 and 3 in closed form, the eligibility ------------------------

// Row-cost policies.  A handle h != 0 stands for the sample's rows at one position (0: no row there).
struct OneRow {   // uncertainty: one row per position, h = allele | ref << 8
    const uint16_t *tab;
    __device__ __forceinline__ uint32_t at(int32_t p) const { return tab[p]; }
    __device__ __forceinline__ int cost(uint32_t h, uint32_t s) const { return row_cost(h & 0xffu, h >> 8, s); }
    __device__ __forceinline__ int cost_ref(uint32_t h) const { return row_cost(h & 0xffu, h >> 8, h >> 8); }
};
struct RowGroups {   // annotate: any number of rows per position, h = 1 + their group; loop 2 runs once per row
    const uint32_t *tab;
    const uint32_t *goff;
    const uint16_t *grow;
    __device__ __forceinline__ uint32_t at(int32_t p) const { return tab[p]; }
    __device__ __forceinline__ int cost(uint32_t h, uint32_t s) const {   // s = 0: each row against its own reference
        int c = 0;
        for (uint32_t k = goff[h - 1]; k < goff[h]; k++) {
            const uint32_t a = grow[k] & 0xffu, r = grow[k] >> 8;
            c += row_cost(a, r, s ? s : r);
        }
        return c;
    }
    __device__ __forceinline__ int cost_ref(uint32_t h) const { return cost(h, 0); }
};

// h(m) - h(parent state of m) for an entry at a position with rows h, h(s) = cost(s) - [s != ref]
template <class Rows>
__device__ __forceinline__ int ev_term(const Rows &R, uint32_t h, uint32_t bits) {
    const uint32_t nuc = b_nuc(bits), anc = b_anc(bits);
    const int hm = R.cost(h, nuc) - (nuc != b_ref(bits) ? 1 : 0);
    const int ha = anc ? R.cost(h, anc) - b_ancne(bits) : R.cost_ref(h);
    return hm - ha;
}

struct Literal {   // one sample: its rows in stored order
    const int32_t *qpos;
    const uint16_t *qnr;   // allele | ref << 8
    uint32_t nq;
    int base;              // H0 + M0: every row against the root state
    uint32_t self;         // a node that is never a candidate (kNil: none)
};

// The score of node i: nr(parent) + base + (C - own) + corr when i is eligible, else kNone.  C = C(i), i's own terms included.
template <class Rows>
__device__ __forceinline__ int literal_score(const DfsView &t, const Rows &R, const Literal &q, uint32_t i, int C) {
    if (i == q.self) return kNone;
    if (i == 0) {
        // the root: loops 2 and 3 against its own mutations, masked ones included (usher_mapper.cpp:266-269, 398-444)
        int sc = q.base;
        for (uint32_t e = t.moff[0]; e < t.moff[1]; e++) {
            const int32_t p = t.mpos[e];
            const uint32_t bits = t.mbits[e], nuc = b_nuc(bits), ref = b_ref(bits);
            if (p < 0) { sc += ref != nuc ? 1 : 0; continue; }
            const uint32_t h = R.at(p);
            if (h) sc += R.cost(h, nuc) - R.cost_ref(h);
            else sc += nuc != ref ? 1 : 0;
        }
        return sc;
    }
    // loop 1 (usher_mapper.cpp:190-264) literally: the merge pointer runs over the rows in their stored order
    uint32_t start = 0;
    int nm = 0, common = 0, corr = 0, own = 0;
    bool hu = false, stopped = false;
    for (uint32_t e = t.moff[i]; e < t.moff[i + 1]; e++) {
        const int32_t p = t.mpos[e];
        const uint32_t bits = t.mbits[e], nuc = b_nuc(bits), ref = b_ref(bits);
        const uint32_t h = p >= 0 ? R.at(p) : 0;
        if (h) own += ev_term(R, h, bits);   // the part of C(i) that is i's own
        if (stopped) continue;
        nm++;
        if (p < 0) { hu = true; stopped = true; continue; }
        bool found = false, found_pos = false;
        for (uint32_t k = start; k < q.nq; k++) {
            const int32_t p2 = q.qpos[k];
            start = k;
            if (p == p2) {
                found_pos = true;
                if (q.qnr[k] & nuc & 0xffu) { found = true; break; }
            }
            if (p < p2) break;
        }
        bool added = found;
        if (!found && !found_pos && nuc == ref) added = true;
        if (added) {
            common++;
            const uint32_t anc = b_anc(bits);
            if (h) corr += R.cost(h, nuc) - (anc ? R.cost(h, anc) : R.cost_ref(h));
            else corr += (nuc != ref ? 1 : 0) - b_ancne(bits);
        } else {
            hu = true;
        }
    }
    const bool lf = t.leaf[i] != 0;
    const bool elig = (hu && !lf && common > 0 && nm != common) || (lf && common > 0) || (!hu && !lf && nm == common);
    return elig ? t.nrp[i] + q.base + (C - own) + corr : kNone;
}

// One block per segment g of one sample: the scores of the segment's nodes replace their entries of the difference array
// (carry: the sum of the earlier segments), and the smallest candidate score goes to *mn.
template <class Rows>
__device__ __forceinline__ void score_segment(const DfsView &t, const Rows &R, const Literal &q, int32_t *diff, int carry,
                                              uint32_t g, int32_t *mn) {
    __shared__ int sh[kBlock / 64];
    __shared__ int smin[kBlock / 64];
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    int best = kNone;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const int dv = i < hi ? diff[i] : 0;
        int tot;
        const int C = carry + block_incl_scan(dv, sh, &tot);
        carry += tot;
        if (i >= hi) continue;
        const int score = literal_score(t, R, q, i, C);
        diff[i] = score;
        best = min(best, score);
    }
    for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d, 64));
    if ((threadIdx.x & 63) == 0) smin[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = smin[0];
        for (int k = 1; k < (int)(kBlock / 64); k++) m = min(m, smin[k]);
        if (m != kNone) atomicMin(mn, m);
    }
}

// The positions i of segment g with sc[i] == m, in ascending order, to ties[base ..] while below cap; f(i) sees every one.
template <class F>
__device__ __forceinline__ void write_ties(const int32_t *sc, uint32_t n, uint32_t g, int32_t m, uint32_t base, uint32_t *ties,
                                           uint32_t cap, F f) {
    __shared__ int sh[kBlock / 64];
    const uint32_t lo = g * kSeg, hi = min(n, lo + kSeg);
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const int flag = (i < hi && sc[i] == m) ? 1 : 0;
        int tot;
        const int incl = block_incl_scan(flag, sh, &tot);
        if (flag) {
            const uint32_t o = base + (uint32_t)(incl - 1);
            if (o < cap) ties[o] = i;
            f(i);
        }
        base += (uint32_t)tot;
    }
}

}  // namespace ugp
