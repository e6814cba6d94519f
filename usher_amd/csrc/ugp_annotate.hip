// ugp_annotate.hip -- matUtils annotate (annotate.cpp) on the device.
//
// Clade allele counts (parse_clade_names, :355-390).  Every exemplar walks its root path (rsearch(n, true)) and takes the first
// non-masked entry at each position, every masked entry, and counts those with ref != mut.  In closed form: call an entry the
// OWNER of its position on its node when it is the first non-masked entry there in stored order.  With cnt_c(u) = the clade's
// exemplars in u's subtree (u included), an owner e at node u is taken by exactly the exemplars below u whose path meets no
// nearer owner of the same position, so
//     count(e) = cnt_c(u) - sum of cnt_c(v) over the owners f at v whose nearest owning ancestor entry is e,
// a masked entry counts cnt_c(u), any other entry 0.  Only nodes with cnt_c(u) > 0 -- the union of the exemplars'
// root paths -- can count; with the exemplars sorted by depth-first position, exemplar i walks up until it meets an ancestor of
// exemplar i - 1, so every node of the union is visited once, and the nodes exemplar i adds all lie after those of i - 1: written
// top-down, each clade's visited list is sorted by depth-first position, which is how a link target finds its slot.
//
// Descendant counts (get_freq_overlap / is_ancestor, :466-481; mutation_annotated_tree.cpp:920-929): exemplars strictly below a
// node = a range count over the clade's sorted depth-first positions.
//
// Literal search (:611-638 for clade rows the packed search refuses: repeated positions, masked rows).  mapper2_body over every
// node in depth-first order with best = 1e9, dense, the closed form of ugp_uncertainty.hip with one change: the cost of the
// rows at a position against a state is the SUM over all rows at that position (loop 2 of usher_mapper.cpp:292-350 runs per
// row, loop 3 only asks whether a row exists there), and loop 1 runs literally over the rows in their stored order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ugp_annotate.hpp"

namespace ugp {
int set_error(int code, const std::string &msg);
}

namespace {

constexpr uint32_t kBlock = 256;   // threads per block (4 waves)
constexpr uint32_t kSeg = 16384;   // depth-first positions per segment of the literal search
constexpr int32_t kNone = INT_MAX; // score of a node that is not an eligible placement
constexpr uint32_t kNil = UINT32_MAX;

#define ANN_TRY(expr)                                                                                         \
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
    hipError_t upload(const T *v, size_t count, hipStream_t st) {
        hipError_t e = alloc(count);
        if (e != hipSuccess || !count) return e;
        return hipMemcpyAsync(p, v, count * sizeof(T), hipMemcpyHostToDevice, st);
    }
    hipError_t upload(const std::vector<T> &v, hipStream_t st) { return upload(v.data(), v.size(), st); }
};

// Entry flags
constexpr uint8_t kCounts = 1;   // the walk takes it and it has ref != mut
constexpr uint8_t kOwner = 2;    // first non-masked entry of its position on its node

// ---- device helpers -----------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lowbit4(uint32_t a) {
    for (uint32_t b = 0; b < 4; b++) if (a & (1u << b)) return 1u << b;
    return 0;
}
// Loop 2 of mapper2_body for one row (allele a, reference r) against the state s of its position (r: none on the path).
__device__ __forceinline__ int row_cost(uint32_t a, uint32_t r, uint32_t s) {
    if (a & s) return 0;
    return ((a & r) ? r : lowbit4(a)) != s ? 1 : 0;
}
// Entry bits: mutated base | ref << 8 | parent state (0 = none on the root path) << 16 | [parent state != its ref] << 24
__device__ __forceinline__ uint32_t b_nuc(uint32_t b) { return b & 0xffu; }
__device__ __forceinline__ uint32_t b_ref(uint32_t b) { return (b >> 8) & 0xffu; }
__device__ __forceinline__ uint32_t b_anc(uint32_t b) { return (b >> 16) & 0xffu; }
__device__ __forceinline__ int b_ancne(uint32_t b) { return (int)((b >> 24) & 1u); }

// First index in [lo, hi) of the sorted xs with xs[k] >= v.
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *xs, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (xs[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
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

struct Tree {   // device tables, indexed by depth-first position / depth-first entry index
    uint32_t n, tp;
    const uint32_t *dpar, *dend, *moff, *mbits, *mnode, *mlink, *morig, *poff, *pent;
    const int32_t *mpos, *nrp;
    const uint8_t *mflag, *leaf;
};

// ---- clade allele counts ------------------------------------------------------------------------------------------

struct Alleles {
    uint32_t nx;           // exemplars of all clades
    const uint32_t *xs;    // [nx] depth-first positions, sorted within each clade
    const uint32_t *cid;   // [nx] clade of each exemplar
    const uint32_t *coff;  // [n_clades + 1] exemplar offsets
    uint32_t *len, *ecnt;  // [nx] nodes / entries each exemplar's walk adds
    const uint32_t *voff, *eoff;   // [nx + 1] their exclusive scans
    const uint32_t *cvoff; // [n_clades + 1] visited-slot range of each clade
    uint32_t *vis, *vcl, *veoff;   // [V] visited node, its clade, its first entry slot
    uint32_t *oent;        // [E] tree entry index
    int32_t *ocnt;         // [E] count
};

// One thread per exemplar: walk up until the node is an ancestor of the clade's previous exemplar.  emit = 0: sizes only;
// emit = 1: the nodes, top-down, and the first entry slot of each.
__global__ void k_walk(Tree t, Alleles A, int emit) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.nx) return;
    const uint32_t c = A.cid[i];
    const uint32_t x = A.xs[i], prev = i > A.coff[c] ? A.xs[i - 1] : kNil;
    if (!emit) {
        uint32_t len = 0, ent = 0, u = x;
        while (u != kNil && !(prev != kNil && u <= prev && prev < t.dend[u])) {
            len++;
            ent += t.moff[u + 1] - t.moff[u];
            u = t.dpar[u];
        }
        A.len[i] = len; A.ecnt[i] = ent;
        return;
    }
    const uint32_t len = A.voff[i + 1] - A.voff[i], ent = A.eoff[i + 1] - A.eoff[i];
    uint32_t u = x, ecum = 0;
    for (uint32_t k = 0; k < len; k++) {
        ecum += t.moff[u + 1] - t.moff[u];
        const uint32_t s = A.voff[i] + len - 1 - k;
        A.vis[s] = u; A.vcl[s] = c; A.veoff[s] = A.eoff[i] + ent - ecum;
        u = t.dpar[u];
    }
}

// One thread per visited node: its entries and their cnt_c(u); each owner takes cnt_c(u) off its nearest owning ancestor.
__global__ void k_count(Tree t, Alleles A, uint32_t V) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const uint32_t u = A.vis[v], c = A.vcl[v];
    const uint32_t lo = A.coff[c], hi = A.coff[c + 1];
    const int rc = (int)(lower_bound_u32(A.xs, lo, hi, t.dend[u]) - lower_bound_u32(A.xs, lo, hi, u));
    const uint32_t m0 = t.moff[u], base = A.veoff[v];
    for (uint32_t e = m0; e < t.moff[u + 1]; e++) {
        const uint32_t s = base + (e - m0);
        A.oent[s] = t.morig[e];
        const uint8_t f = t.mflag[e];
        if (f & kCounts) atomicAdd(&A.ocnt[s], rc);
        const uint32_t g = t.mlink[e];
        if (!(f & kOwner) || g == kNil || !(t.mflag[g] & kCounts)) continue;
        const uint32_t a = t.mnode[g], v0 = A.cvoff[c], v1 = A.cvoff[c + 1];
        const uint32_t k = lower_bound_u32(A.vis, v0, v1, a);
        if (k < v1 && A.vis[k] == a) atomicAdd(&A.ocnt[A.veoff[k] + (g - t.moff[a])], -rc);
    }
}

// ---- descendant counts --------------------------------------------------------------------------------------------

__global__ void k_desc(Tree t, const uint32_t *xs, const uint32_t *coff, const uint32_t *pc, const uint32_t *pu, uint32_t np,
                       uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const uint32_t c = pc[i], u = pu[i], lo = coff[c], hi = coff[c + 1];
    out[i] = lower_bound_u32(xs, lo, hi, t.dend[u]) - lower_bound_u32(xs, lo, hi, u + 1);
}

// ---- literal search -----------------------------------------------------------------------------------------------

struct Search {
    uint32_t nq, ng, nseg, cap;
    const int32_t *qpos;      // [nq] rows in stored order
    const uint16_t *qnr;      // [nq] allele | ref << 8
    const int32_t *gpos;      // [ng] distinct row positions < tp, ascending
    const uint32_t *goff;     // [ng + 1] rows of each position ...
    const uint16_t *grow;     // ... allele | ref << 8
    uint32_t *tab;            // [tp] 1 + group of a position, 0 = no row there
    int32_t base;             // every row against the reference state: H0 + M0
    int32_t *diff;            // [n] difference array, then the scores
    int32_t *seg;             // [nseg] segment sums -> carries
    int32_t *mn;              // [1] best score
    uint32_t *scnt, *soff;    // [nseg] ties per segment, list offset
    uint32_t *total;          // [1]
    uint32_t *ties;           // [cap]
};

// Loop 2 of every row of group g against state s (0 = none: each row's own reference).
__device__ __forceinline__ int gcost(const Search &S, uint32_t g, uint32_t s) {
    int c = 0;
    for (uint32_t k = S.goff[g]; k < S.goff[g + 1]; k++) {
        const uint32_t a = S.grow[k] & 0xffu, r = S.grow[k] >> 8;
        c += row_cost(a, r, s ? s : r);
    }
    return c;
}
// h(m) - h(parent state of m) for an owner at a row position (group g)
__device__ __forceinline__ int gev(const Search &S, uint32_t g, uint32_t bits) {
    const uint32_t nuc = b_nuc(bits), anc = b_anc(bits);
    const int hm = gcost(S, g, nuc) - (nuc != b_ref(bits) ? 1 : 0);
    const int ha = anc ? gcost(S, g, anc) - b_ancne(bits) : gcost(S, g, 0);
    return hm - ha;
}

__global__ void k_tab(Search S, int set) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < S.ng) S.tab[S.gpos[g]] = set ? g + 1 : 0;
}

// One thread per row position: every owner there adds its term over its subtree.
__global__ void k_events(Tree t, Search S) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.ng) return;
    const int32_t p = S.gpos[g];
    for (uint32_t i = t.poff[p]; i < t.poff[p + 1]; i++) {
        const uint32_t e = t.pent[i];
        const int ev = gev(S, g, t.mbits[e]);
        if (!ev) continue;
        const uint32_t u = t.mnode[e], end = t.dend[u];
        atomicAdd(&S.diff[u], ev);
        if (end < t.n) atomicAdd(&S.diff[end], -ev);
    }
}

__global__ void __launch_bounds__(kBlock) k_segsum(Tree t, Search S) {
    __shared__ int sh[kBlock / 64];
    const uint32_t g = blockIdx.x;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    int acc = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) acc += S.diff[i];
    int tot;
    (void)block_incl_scan(acc, sh, &tot);
    if (threadIdx.x == 0) S.seg[g] = tot;
}

__global__ void k_segscan(Search S) {
    if (blockIdx.x || threadIdx.x) return;
    int run = 0;
    for (uint32_t g = 0; g < S.nseg; g++) { const int v = S.seg[g]; S.seg[g] = run; run += v; }
    S.mn[0] = kNone;
}

// The score of every node; eligible ones keep it, the rest read kNone.
__global__ void __launch_bounds__(kBlock) k_score(Tree t, Search S) {
    __shared__ int sh[kBlock / 64];
    __shared__ int smin[kBlock / 64];
    const uint32_t g = blockIdx.x;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    int carry = S.seg[g];
    int best = kNone;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const int dv = i < hi ? S.diff[i] : 0;
        int tot;
        const int C = carry + block_incl_scan(dv, sh, &tot);   // C(X): X's own terms included
        carry += tot;
        if (i >= hi) continue;
        int score = kNone;
        if (i == 0) {
            // the root: loops 2 and 3 against its own mutations, masked ones included (usher_mapper.cpp:266-269, 398-444)
            int sc = S.base;
            for (uint32_t e = t.moff[0]; e < t.moff[1]; e++) {
                const int32_t p = t.mpos[e];
                const uint32_t bits = t.mbits[e], nuc = b_nuc(bits), ref = b_ref(bits);
                if (p < 0) { sc += ref != nuc ? 1 : 0; continue; }
                const uint32_t gr = S.tab[p];
                if (gr) sc += gcost(S, gr - 1, nuc) - gcost(S, gr - 1, 0);
                else sc += nuc != ref ? 1 : 0;
            }
            score = sc;
        } else {
            // loop 1 (usher_mapper.cpp:190-264) literally: the merge pointer runs over the rows in their stored order
            uint32_t start = 0;
            int nm = 0, common = 0, corr = 0, own = 0;
            bool hu = false, stopped = false;
            for (uint32_t e = t.moff[i]; e < t.moff[i + 1]; e++) {
                const int32_t p = t.mpos[e];
                const uint32_t bits = t.mbits[e], nuc = b_nuc(bits), ref = b_ref(bits);
                const uint32_t gr = p >= 0 ? S.tab[p] : 0;
                if (gr) own += gev(S, gr - 1, bits);   // the part of C(X) that is X's own
                if (stopped) continue;
                nm++;
                if (p < 0) { hu = true; stopped = true; continue; }
                bool found = false, found_pos = false;
                for (uint32_t k = start; k < S.nq; k++) {
                    const int32_t p2 = S.qpos[k];
                    start = k;
                    if (p == p2) {
                        found_pos = true;
                        if (S.qnr[k] & nuc & 0xffu) { found = true; break; }
                    }
                    if (p < p2) break;
                }
                bool added = found;
                if (!found && !found_pos && nuc == ref) added = true;
                if (added) {
                    common++;
                    const uint32_t anc = b_anc(bits);
                    if (gr) corr += gcost(S, gr - 1, nuc) - gcost(S, gr - 1, anc);
                    else corr += (nuc != ref ? 1 : 0) - b_ancne(bits);
                } else {
                    hu = true;
                }
            }
            const bool lf = t.leaf[i] != 0;
            const bool elig = (hu && !lf && common > 0 && nm != common) || (lf && common > 0) || (!hu && !lf && nm == common);
            if (elig) score = t.nrp[i] + S.base + (C - own) + corr;
        }
        S.diff[i] = score;
        best = min(best, score);
    }
    for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d, 64));
    if ((threadIdx.x & 63) == 0) smin[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = smin[0];
        for (int k = 1; k < (int)(kBlock / 64); k++) m = min(m, smin[k]);
        if (m != kNone) atomicMin(S.mn, m);
    }
}

__global__ void __launch_bounds__(kBlock) k_tiecount(Tree t, Search S) {
    __shared__ int sh[kBlock / 64];
    const uint32_t g = blockIdx.x;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    const int32_t m = S.mn[0];
    int cnt = 0;
    if (m != kNone)
        for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) cnt += S.diff[i] == m ? 1 : 0;
    int tot;
    (void)block_incl_scan(cnt, sh, &tot);
    if (threadIdx.x == 0) S.scnt[g] = (uint32_t)tot;
}

__global__ void k_tiescan(Search S) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t run = 0;
    for (uint32_t g = 0; g < S.nseg; g++) { S.soff[g] = run; run += S.scnt[g]; }
    S.total[0] = run;
}

// The tied depth-first positions in ascending order, up to cap.
__global__ void __launch_bounds__(kBlock) k_tiewrite(Tree t, Search S) {
    __shared__ int sh[kBlock / 64];
    const uint32_t g = blockIdx.x;
    const uint32_t lo = g * kSeg, hi = min(t.n, lo + kSeg);
    const int32_t m = S.mn[0];
    if (m == kNone || !S.scnt[g]) return;
    uint32_t base = S.soff[g];
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const int f = (i < hi && S.diff[i] == m) ? 1 : 0;
        int tot;
        const int incl = block_incl_scan(f, sh, &tot);
        if (f) {
            const uint32_t o = base + (uint32_t)(incl - 1);
            if (o < S.cap) S.ties[o] = i;
        }
        base += (uint32_t)tot;
    }
}

uint32_t h_lowbit4(uint32_t a) {
    for (uint32_t b = 0; b < 4; b++) if (a & (1u << b)) return 1u << b;
    return 0;
}
int h_row_cost(uint32_t a, uint32_t r, uint32_t s) {
    if (a & s) return 0;
    return ((a & r) ? r : h_lowbit4(a)) != s ? 1 : 0;
}

}  // namespace

namespace ugp {

struct AnnState {
    int device = 0;
    uint32_t n = 0, tp = 0;
    uint64_t m = 0;
    bool literal_ok = true;         // no branch carries two non-masked mutations at one position
    hipStream_t stream = nullptr;
    std::vector<uint32_t> bfs2dfs;
    DBuf<uint32_t> dpar, dend, moff, mbits, mnode, mlink, morig, poff, pent;
    DBuf<int32_t> mpos, nrp;
    DBuf<uint8_t> mflag, leaf;
    // per call
    DBuf<uint32_t> xs, cid, coff, len, ecnt, voff, eoff, cvoff, vis, vcl, veoff, oent, pc, pu, dout;
    DBuf<int32_t> ocnt;
    DBuf<int32_t> qpos, gpos, diff, seg, mn;
    DBuf<uint16_t> qnr, grow;
    DBuf<uint32_t> goff, tab, scnt, soff, total, ties;
    ~AnnState() { if (stream) (void)hipStreamDestroy(stream); }
    Tree tree() const {
        return Tree{n, tp, dpar.p, dend.p, moff.p, mbits.p, mnode.p, mlink.p, morig.p, poff.p, pent.p, mpos.p, nrp.p, mflag.p, leaf.p};
    }
};

void ann_free(AnnState *s) { delete s; }

int ann_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device, AnnState **out) {
    if (!tree || !out || !tree->parent || !tree->mut_off) return set_error(UGP_ERR_INVALID, "null argument");
    const uint64_t N = tree->n_nodes;
    if (N == 0 || N >= (1ull << 31) || dfs2bfs.size() != N || bfs2dfs.size() != N) return set_error(UGP_ERR_INVALID, "tree does not match the handle");
    const uint64_t M = tree->mut_off[N];
    if (M >= (1ull << 31)) return set_error(UGP_ERR_UNSUPPORTED, "more than 2^31 mutation entries");
    if (M && (!tree->mut_pos || !tree->mut_ref || !tree->mut_nuc)) return set_error(UGP_ERR_INVALID, "null mutation arrays");
    AnnState *S = nullptr;
    try {
        S = new AnnState();
        S->device = device;
        S->n = (uint32_t)N;
        S->m = M;
        S->bfs2dfs = bfs2dfs;
        std::vector<uint32_t> dpar(N), dend(N), moff(N + 1), mbits(M), mnode(M), mlink(M, kNil), morig(M);
        std::vector<int32_t> mpos(M), nrp(N, 0);
        std::vector<uint8_t> mflag(M, 0), leaf(N, 1);
        int32_t maxpos = -1;
        uint64_t e = 0;
        std::vector<int32_t> seen;   // positions of the current node's owners
        for (uint64_t i = 0; i < N; i++) {
            const uint32_t b = dfs2bfs[i];
            if (b >= N || bfs2dfs[b] != i) { delete S; return set_error(UGP_ERR_INVALID, "depth-first order is not a permutation"); }
            dpar[i] = i ? bfs2dfs[tree->parent[b]] : kNil;
            if (i && dpar[i] >= i) { delete S; return set_error(UGP_ERR_INVALID, "parent after child in depth-first order"); }
            moff[i] = (uint32_t)e;
            seen.clear();
            for (uint64_t k = tree->mut_off[b]; k < tree->mut_off[b + 1]; k++, e++) {
                const int32_t p = tree->mut_pos[k];
                mpos[e] = p;
                mbits[e] = (uint32_t)tree->mut_nuc[k] | (uint32_t)tree->mut_ref[k] << 8;
                mnode[e] = (uint32_t)i;
                morig[e] = (uint32_t)k;
                maxpos = std::max(maxpos, p);
                bool take = p < 0;
                if (p >= 0) {
                    if (std::find(seen.begin(), seen.end(), p) == seen.end()) { seen.push_back(p); take = true; mflag[e] |= kOwner; }
                    else S->literal_ok = false;
                }
                if (take && tree->mut_ref[k] != tree->mut_nuc[k]) mflag[e] |= kCounts;
            }
            if (i) leaf[dpar[i]] = 0;
        }
        moff[N] = (uint32_t)e;
        if (maxpos >= (1 << 28)) { delete S; return set_error(UGP_ERR_UNSUPPORTED, "mutation position above 2^28"); }
        {
            std::vector<uint32_t> sz(N, 1);
            for (uint64_t i = N; i-- > 1;) sz[dpar[i]] += sz[i];
            for (uint64_t i = 0; i < N; i++) dend[i] = (uint32_t)(i + sz[i]);
        }
        // owners by position, in depth-first order of their node; the nearest owning ancestor of each (a stack per position
        // whose top's subtree still contains the node) and its allele, the parent state of the literal search
        const uint32_t tp = (uint32_t)(maxpos + 1);
        std::vector<uint32_t> poff(tp + 1, 0), pent;
        for (uint64_t k = 0; k < M; k++) if (mflag[k] & kOwner) poff[mpos[k] + 1]++;
        for (uint32_t p = 0; p < tp; p++) poff[p + 1] += poff[p];
        pent.resize(poff[tp]);
        {
            std::vector<uint32_t> fill(poff.begin(), poff.end() - 1);
            for (uint64_t k = 0; k < M; k++) if (mflag[k] & kOwner) pent[fill[mpos[k]]++] = (uint32_t)k;
        }
        std::vector<uint32_t> st;
        for (uint32_t p = 0; p < tp; p++) {
            st.clear();
            for (uint32_t x = poff[p]; x < poff[p + 1]; x++) {
                const uint32_t k = pent[x], u = mnode[k];
                while (!st.empty() && dend[mnode[st.back()]] <= u) st.pop_back();
                if (!st.empty()) {
                    const uint32_t a = st.back(), an = mbits[a] & 0xffu, ar = (mbits[a] >> 8) & 0xffu;
                    mbits[k] |= an << 16 | (uint32_t)(an != ar) << 24;
                    mlink[k] = a;
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
                    if (!(mflag[k] & kOwner)) continue;
                    const uint32_t b = mbits[k];
                    v += ((b & 0xffu) != ((b >> 8) & 0xffu) ? 1 : 0) - (int32_t)((b >> 24) & 1u);
                }
                nr[i] = v;
                nrp[i] = i ? nr[dpar[i]] : 0;
            }
        }
        S->tp = tp;
        if (hipSetDevice(device) != hipSuccess) { delete S; return set_error(UGP_ERR_HIP, "hipSetDevice failed"); }
        hipStream_t s = nullptr;
        hipError_t err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (err == hipSuccess) {
            S->stream = s;
            for (auto pr : {std::make_pair(&S->dpar, &dpar), std::make_pair(&S->dend, &dend), std::make_pair(&S->moff, &moff),
                            std::make_pair(&S->mbits, &mbits), std::make_pair(&S->mnode, &mnode), std::make_pair(&S->mlink, &mlink),
                            std::make_pair(&S->morig, &morig), std::make_pair(&S->poff, &poff), std::make_pair(&S->pent, &pent)})
                if (err == hipSuccess) err = pr.first->upload(*pr.second, s);
        }
        if (err == hipSuccess) err = S->mpos.upload(mpos, s);
        if (err == hipSuccess) err = S->nrp.upload(nrp, s);
        if (err == hipSuccess) err = S->mflag.upload(mflag, s);
        if (err == hipSuccess) err = S->leaf.upload(leaf, s);
        if (err == hipSuccess) err = S->tab.alloc(std::max<uint32_t>(tp, 1));
        if (err == hipSuccess) err = hipMemsetAsync(S->tab.p, 0, (size_t)std::max<uint32_t>(tp, 1) * sizeof(uint32_t), s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);   // the host vectors go out of scope
        if (err != hipSuccess) { delete S; return set_error(UGP_ERR_HIP, std::string("annotate tables: ") + hipGetErrorString(err)); }
    } catch (const std::bad_alloc &) {
        delete S;
        return set_error(UGP_ERR_NOMEM, "out of host memory");
    }
    delete *out;
    *out = S;
    return UGP_OK;
}

namespace {
// The clades' exemplars as sorted depth-first positions (CSR) on the device.
int upload_clades(AnnState *S, const uint64_t *clade_off, const uint32_t *nodes, uint64_t nc, std::vector<uint32_t> &xs,
                  std::vector<uint32_t> &coff) {
    if (nc >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "too many clades");
    const uint64_t nx = clade_off[nc];
    if (clade_off[0] != 0 || nx >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "bad clade offsets");
    if (nx && !nodes) return set_error(UGP_ERR_INVALID, "null argument");
    xs.resize(nx); coff.resize(nc + 1);
    for (uint64_t c = 0; c < nc; c++) {
        if (clade_off[c + 1] < clade_off[c]) return set_error(UGP_ERR_INVALID, "bad clade offsets");
        coff[c] = (uint32_t)clade_off[c];
        for (uint64_t k = clade_off[c]; k < clade_off[c + 1]; k++) {
            if (nodes[k] >= S->n) return set_error(UGP_ERR_INVALID, "node index out of range");
            xs[k] = S->bfs2dfs[nodes[k]];
        }
        std::sort(xs.begin() + clade_off[c], xs.begin() + clade_off[c + 1]);
    }
    coff[nc] = (uint32_t)nx;
    ANN_TRY(hipSetDevice(S->device));
    ANN_TRY(S->xs.upload(xs, S->stream));
    ANN_TRY(S->coff.upload(coff, S->stream));
    return UGP_OK;
}
}  // namespace

int ann_alleles(AnnState *S, const uint64_t *clade_off, const uint32_t *nodes, uint64_t nc, uint64_t *out_off, uint32_t *out_ent,
                uint32_t *out_cnt, uint64_t cap, uint64_t *n_out) {
    if (!S) return set_error(UGP_ERR_INVALID, "no annotate tables: call ugp_annotate_attach first");
    if (!clade_off || !out_off || !n_out || (cap && (!out_ent || !out_cnt))) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        std::vector<uint32_t> xs, coff;
        int rc = upload_clades(S, clade_off, nodes, nc, xs, coff);
        if (rc) return rc;
        const uint32_t nx = (uint32_t)xs.size();
        hipStream_t st = S->stream;
        std::vector<uint32_t> cid(nx);
        for (uint64_t c = 0; c < nc; c++) for (uint32_t k = coff[c]; k < coff[c + 1]; k++) cid[k] = (uint32_t)c;
        ANN_TRY(S->cid.upload(cid, st));
        ANN_TRY(S->len.alloc(nx)); ANN_TRY(S->ecnt.alloc(nx));
        Tree t = S->tree();
        Alleles A{nx, S->xs.p, S->cid.p, S->coff.p, S->len.p, S->ecnt.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        const uint32_t gx = (nx + kBlock - 1) / kBlock;
        if (nx) k_walk<<<gx, kBlock, 0, st>>>(t, A, 0);
        std::vector<uint32_t> len(nx), ecnt(nx);
        if (nx) {
            ANN_TRY(hipMemcpyAsync(len.data(), S->len.p, nx * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            ANN_TRY(hipMemcpyAsync(ecnt.data(), S->ecnt.p, nx * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        ANN_TRY(hipStreamSynchronize(st));
        std::vector<uint32_t> voff(nx + 1, 0), eoff(nx + 1, 0), cvoff(nc + 1);
        uint64_t V = 0, E = 0;
        for (uint32_t i = 0; i < nx; i++) {
            voff[i] = (uint32_t)V; eoff[i] = (uint32_t)E;
            V += len[i]; E += ecnt[i];
            if (V >= (1ull << 32) || E >= (1ull << 32)) return set_error(UGP_ERR_UNSUPPORTED, "more than 2^32 visited entries in one call");
        }
        voff[nx] = (uint32_t)V; eoff[nx] = (uint32_t)E;
        for (uint64_t c = 0; c <= nc; c++) cvoff[c] = voff[coff[c]];
        ANN_TRY(S->voff.upload(voff, st)); ANN_TRY(S->eoff.upload(eoff, st)); ANN_TRY(S->cvoff.upload(cvoff, st));
        ANN_TRY(S->vis.alloc(V)); ANN_TRY(S->vcl.alloc(V)); ANN_TRY(S->veoff.alloc(V));
        ANN_TRY(S->oent.alloc(E)); ANN_TRY(S->ocnt.alloc(E));
        if (E) ANN_TRY(hipMemsetAsync(S->ocnt.p, 0, E * sizeof(int32_t), st));
        A.voff = S->voff.p; A.eoff = S->eoff.p; A.cvoff = S->cvoff.p;
        A.vis = S->vis.p; A.vcl = S->vcl.p; A.veoff = S->veoff.p; A.oent = S->oent.p; A.ocnt = S->ocnt.p;
        if (nx) k_walk<<<gx, kBlock, 0, st>>>(t, A, 1);
        if (V) k_count<<<(uint32_t)((V + kBlock - 1) / kBlock), kBlock, 0, st>>>(t, A, (uint32_t)V);
        ANN_TRY(hipGetLastError());
        std::vector<uint32_t> oent(E);
        std::vector<int32_t> ocnt(E);
        if (E) {
            ANN_TRY(hipMemcpyAsync(oent.data(), S->oent.p, E * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            ANN_TRY(hipMemcpyAsync(ocnt.data(), S->ocnt.p, E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        ANN_TRY(hipStreamSynchronize(st));
        // entries that some walk takes, per clade in depth-first order of their node, then stored order
        uint64_t w = 0;
        for (uint64_t c = 0; c < nc; c++) {
            out_off[c] = w;
            for (uint32_t s = eoff[coff[c]]; s < eoff[coff[c + 1]]; s++) {
                if (ocnt[s] <= 0) continue;
                if (w < cap) { out_ent[w] = oent[s]; out_cnt[w] = (uint32_t)ocnt[s]; }
                w++;
            }
        }
        out_off[nc] = w;
        *n_out = w;
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

int ann_descendants(AnnState *S, const uint64_t *clade_off, const uint32_t *nodes, uint64_t nc, const uint32_t *pair_clade,
                    const uint32_t *pair_node, uint64_t np, uint32_t *out) {
    if (!S) return set_error(UGP_ERR_INVALID, "no annotate tables: call ugp_annotate_attach first");
    if (!clade_off || (np && (!pair_clade || !pair_node || !out))) return set_error(UGP_ERR_INVALID, "null argument");
    if (np >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "too many pairs");
    try {
        std::vector<uint32_t> xs, coff;
        int rc = upload_clades(S, clade_off, nodes, nc, xs, coff);
        if (rc) return rc;
        if (!np) return UGP_OK;
        std::vector<uint32_t> pu(np);
        for (uint64_t i = 0; i < np; i++) {
            if (pair_clade[i] >= nc) return set_error(UGP_ERR_INVALID, "clade index out of range");
            if (pair_node[i] >= S->n) return set_error(UGP_ERR_INVALID, "node index out of range");
            pu[i] = S->bfs2dfs[pair_node[i]];
        }
        hipStream_t st = S->stream;
        ANN_TRY(S->pc.upload(pair_clade, np, st));
        ANN_TRY(S->pu.upload(pu, st));
        ANN_TRY(S->dout.alloc(np));
        k_desc<<<(uint32_t)((np + kBlock - 1) / kBlock), kBlock, 0, st>>>(S->tree(), S->xs.p, S->coff.p, S->pc.p, S->pu.p, (uint32_t)np, S->dout.p);
        ANN_TRY(hipGetLastError());
        ANN_TRY(hipMemcpyAsync(out, S->dout.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        ANN_TRY(hipStreamSynchronize(st));
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

int ann_search(AnnState *S, const ugp_queries *q, uint32_t cap, int32_t *best, uint32_t *tie_dfs, uint32_t *tie_count) {
    if (!S) return set_error(UGP_ERR_INVALID, "no annotate tables: call ugp_annotate_attach first");
    if (!q || !best || !tie_count || (cap && !tie_dfs)) return set_error(UGP_ERR_INVALID, "null argument");
    if (!q->n_queries) return UGP_OK;
    if (!q->ent_off) return set_error(UGP_ERR_INVALID, "null argument");
    if (!S->literal_ok) return set_error(UGP_ERR_UNSUPPORTED, "two mutations at one position on one branch");
    const uint64_t nent = q->ent_off[q->n_queries];
    if (nent && (!q->pos || !q->ref || !q->nuc)) return set_error(UGP_ERR_INVALID, "null row arrays");
    try {
        ANN_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        const uint32_t N = S->n, nseg = (N + kSeg - 1) / kSeg;
        ANN_TRY(S->diff.alloc(N)); ANN_TRY(S->seg.alloc(nseg)); ANN_TRY(S->mn.alloc(1));
        ANN_TRY(S->scnt.alloc(nseg)); ANN_TRY(S->soff.alloc(nseg)); ANN_TRY(S->total.alloc(1)); ANN_TRY(S->ties.alloc(std::max<uint32_t>(cap, 1)));
        const Tree t = S->tree();
        std::vector<int32_t> qpos, gpos;
        std::vector<uint16_t> qnr, grow;
        std::vector<uint32_t> goff, order;
        for (uint64_t s = 0; s < q->n_queries; s++) {
            const uint64_t r0 = q->ent_off[s], r1 = q->ent_off[s + 1];
            if (r1 < r0 || r1 > nent || r1 - r0 >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "bad row offsets");
            const uint32_t nq = (uint32_t)(r1 - r0);
            qpos.assign(q->pos + r0, q->pos + r1);
            qnr.resize(nq);
            int base = 0;
            for (uint32_t k = 0; k < nq; k++) {
                if (q->is_missing && q->is_missing[r0 + k]) return set_error(UGP_ERR_INVALID, "the literal search takes rows with is_missing = 0");
                const uint32_t a = (uint8_t)q->nuc[r0 + k], r = (uint8_t)q->ref[r0 + k];
                if (a == 0 || a > 15 || r > 15) return set_error(UGP_ERR_INVALID, "allele outside 1..15");
                qnr[k] = (uint16_t)(a | r << 8);
                base += h_row_cost(a, r, r);
            }
            // rows grouped by position (the positions the tree has entries at)
            order.resize(nq);
            for (uint32_t k = 0; k < nq; k++) order[k] = k;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return qpos[a] < qpos[b]; });
            gpos.clear(); goff.assign(1, 0); grow.clear();
            for (uint32_t k : order) {
                const int32_t p = qpos[k];
                if (p < 0 || (uint32_t)p >= S->tp) continue;
                if (gpos.empty() || gpos.back() != p) { gpos.push_back(p); goff.push_back(goff.back()); }
                grow.push_back(qnr[k]);
                goff.back()++;
            }
            const uint32_t ng = (uint32_t)gpos.size();
            ANN_TRY(S->qpos.upload(qpos, st)); ANN_TRY(S->qnr.upload(qnr, st));
            ANN_TRY(S->gpos.upload(gpos, st)); ANN_TRY(S->goff.upload(goff, st)); ANN_TRY(S->grow.upload(grow, st));
            Search B{nq, ng, nseg, cap, S->qpos.p, S->qnr.p, S->gpos.p, S->goff.p, S->grow.p, S->tab.p, base,
                     S->diff.p, S->seg.p, S->mn.p, S->scnt.p, S->soff.p, S->total.p, S->ties.p};
            const uint32_t gg = (ng + kBlock - 1) / kBlock;
            ANN_TRY(hipMemsetAsync(S->diff.p, 0, (size_t)N * sizeof(int32_t), st));
            if (ng) k_tab<<<gg, kBlock, 0, st>>>(B, 1);
            if (ng) k_events<<<gg, kBlock, 0, st>>>(t, B);
            k_segsum<<<nseg, kBlock, 0, st>>>(t, B);
            k_segscan<<<1, 64, 0, st>>>(B);
            k_score<<<nseg, kBlock, 0, st>>>(t, B);
            k_tiecount<<<nseg, kBlock, 0, st>>>(t, B);
            k_tiescan<<<1, 64, 0, st>>>(B);
            k_tiewrite<<<nseg, kBlock, 0, st>>>(t, B);
            if (ng) k_tab<<<gg, kBlock, 0, st>>>(B, 0);
            ANN_TRY(hipGetLastError());
            ANN_TRY(hipMemcpyAsync(best + s, S->mn.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            ANN_TRY(hipMemcpyAsync(tie_count + s, S->total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            ANN_TRY(hipStreamSynchronize(st));
            const uint32_t k = std::min(cap, tie_count[s]);
            if (k) ANN_TRY(hipMemcpy(tie_dfs + (size_t)s * cap, S->ties.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

}  // namespace ugp
