// ugp_ripples.hip -- RIPPLES' recombination search (ripples/main.cpp:300-680) for a list of branches: for a branch nid with
// pruned sample Q (its root path, sorted by position, M rows), pass 1 scores every candidate node k (>= n_desc subtree nodes)
// with mapper2_body, every breakpoint pair (i, j) splits Q into donor rows [i, j) and acceptor rows, and the pair's event is
// the first (donor, acceptor) of the two sorted candidate lists whose unmatched counts fit the parsimony budget.
//
// Both node passes of a pair read one set per candidate: U_k, the excess mutations of k (mapper2_body's vector) that match none
// of k's own mutations (main.cpp:436-457).  Its entries sit at positions; a pair counts those in [pos[i], pos[j-1]] (donor) and
// the rest (acceptor).  So per candidate the counts of U_k in 2M + 1 buckets -- below pos[0], at pos[0], between pos[0] and
// pos[1], ..., above pos[M-1] -- answer every pair: in(i, j) = S[2j] - S[2i+1] with S the bucket prefix sums.
//
// U_k in closed form ("RIPPLES"): with g(p) the ancestral state mapper2_body uses at position p,
//   a sample position p (row s, ref r):  one entry iff s & (g(p) or r) == 0;   a position outside Q:  iff g(p) not in {none, r};
//   masked sample rows:  iff s & r == 0;   the root's masked mutations (k = root only):  iff nuc != ref.
// g(p) is the parent's genotype except at k's own mutations that loop 1 keeps, so the bucket counts are the parent-genotype
// counts (each mutation on root..parent(k) adds term(new state) - term(state it replaced) at its bucket: a telescoping sum
// along the root path) plus a correction at each own mutation, which also applies the own-mutation match of :436-449.  The
// same terms, without that match, are loops 2 and 3 of mapper2_body: their total is the pass-1 set difference.
//
// Kernels per branch: k_count (one thread per candidate: bucket counts -> prefix sums, pass-1 score and flags, the minimum
// eligible score), k_pairs (one thread per pair, candidates in LDS tiles: the top-3 donors and acceptors by
// count << 32 | name rank, per block), k_merge (per pair over the blocks).  The host applies the selection of :594-606 to the
// top-3 lists: with nid removed, the chosen pair depends on the first two entries of each list only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_set>
#include <vector>

#include "ugp_dense.hpp"
#include "ugp_ripples.hpp"

namespace ugp {
namespace {

constexpr uint64_t kKeyMax = ~0ull;
constexpr uint64_t kCountBudget = 1ull << 29;   // bytes of bucket prefix sums per candidate chunk
constexpr uint64_t kSlabBudget = 1ull << 28;    // bytes of per-block top-3 partials
constexpr uint64_t kLdsInts = 12288;            // 48 KiB of bucket sums per candidate tile
constexpr uint32_t kTileMax = 64;
// flags of a candidate
constexpr uint8_t kElig = 1, kHasUnique = 2, kUnder = 4, kLeaf = 8;

// Entry bits (b_nuc / b_ref / b_anc of ugp_dense.hpp): mutated base | ref << 8 | parent state (0 = none on the root path) << 16

struct Tree {   // device tables, BFS-indexed
    uint32_t n, tp;
    const uint32_t *parent, *moff, *mbits, *dfs, *dend, *rank;
    const int32_t *mpos;
    const uint8_t *leaf;
};

struct Branch {
    uint32_t nid, M, nb, C, c0, Cc;   // branch node, sample rows, buckets (2M + 1), candidates, this chunk
    const int32_t *qpos;      // [M] sample positions, ascending (masked first)
    const uint8_t *qnuc;      // [M]
    const uint32_t *btab;     // [tp] bucket of a position >= 0
    const uint16_t *srow;     // [tp] sample row at a position: nuc | ref << 8, 0 = none
    const int32_t *base0;     // [nb] counts with no mutation on the path; base0[nb] = their total
    const uint32_t *cand;     // [C] candidate nodes (BFS)
    int32_t *S;               // [(nb + 1) * Cc] bucket prefix sums of the chunk, bucket-major
    int32_t *score;           // [C] node_set_difference
    uint8_t *flags;           // [C]
    int32_t *minE;            // [1] smallest set difference of an eligible candidate
};

__device__ __forceinline__ uint32_t bucket_of(const Tree &t, const Branch &b, int32_t p) {
    if (p >= 0) return b.btab[p];
    uint32_t lo = 0, hi = b.M;   // lower bound among the (masked, negative) sample positions
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (b.qpos[mid] < p) lo = mid + 1; else hi = mid; }
    return 2 * lo + ((lo < b.M && b.qpos[lo] == p) ? 1u : 0u);
}
// Is there an unmatched entry at p (>= 0) when the ancestral state there is st (0: none)?
__device__ __forceinline__ int term(const Tree &t, const Branch &b, int32_t p, uint32_t ref, uint32_t st) {
    const uint32_t row = (uint32_t)p < t.tp ? b.srow[p] : 0u;
    if (row) return ((row & 0xffu) & (st ? st : (row >> 8))) == 0 ? 1 : 0;
    return (st != 0 && st != ref) ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_count(Tree t, Branch b) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= b.Cc) return;
    const uint32_t k = b.cand[b.c0 + c];
    int32_t *col = b.S + c;   // bucket x of this candidate: col[(x + 1) * Cc] (slot 0 stays the zero prefix)
    const size_t st = b.Cc;
    col[0] = 0;
    for (uint32_t x = 0; x < b.nb; x++) col[(x + 1) * st] = b.base0[x];
    int E = b.base0[b.nb];
    // the parent's genotype: every mutation strictly above k, against the state it replaced
    for (uint32_t v = t.parent[k]; v != kNil; v = t.parent[v]) {
        for (uint32_t e = t.moff[v]; e < t.moff[v + 1]; e++) {
            const int32_t p = t.mpos[e];
            if (p < 0) continue;
            const uint32_t bits = t.mbits[e];
            const int d = term(t, b, p, b_ref(bits), b_nuc(bits)) - term(t, b, p, b_ref(bits), b_anc(bits));
            if (d) { col[(b.btab[p] + 1) * st] += d; E += d; }
        }
    }
    // k's own mutations: loop 1 literally (usher_mapper.cpp:190-264) decides which replace the parent's state
    const bool root = k == 0;
    uint32_t start = 0;
    int nm = 0, common = 0;
    bool hu = false, stopped = root;
    for (uint32_t e = t.moff[k]; e < t.moff[k + 1]; e++) {
        const int32_t p = t.mpos[e];
        const uint32_t bits = t.mbits[e], nuc = b_nuc(bits), ref = b_ref(bits);
        bool kept = root;
        if (!stopped) {
            nm++;
            if (p < 0) {
                hu = true; stopped = true;
            } else {
                bool found = false, found_pos = false;
                for (uint32_t q = start; q < b.M; q++) {
                    const int32_t p2 = b.qpos[q];
                    start = q;
                    if (p == p2) {
                        found_pos = true;
                        if (b.qnuc[q] & nuc) { found = true; break; }
                    }
                    if (p < p2) break;
                }
                kept = found || (!found_pos && nuc == ref);
                if (kept) common++; else hu = true;
            }
        }
        if (p < 0) {
            if (root && nuc != ref) { col[(bucket_of(t, b, p) + 1) * st] += 1; E += 1; }   // loop 3 (:446-470)
            continue;
        }
        const uint32_t anc = root ? 0u : b_anc(bits);
        const int ek = term(t, b, p, ref, kept ? nuc : anc), eb = term(t, b, p, ref, anc);
        const uint32_t row = (uint32_t)p < t.tp ? b.srow[p] : 0u;
        uint32_t bq = ref;   // the entry's allele: the sample's row (loop 2) or the reference (loop 3)
        if (row) { const uint32_t s = row & 0xffu, sr = row >> 8; bq = (s & sr) ? sr : lowbit4(s); }
        const int uk = (ek && nuc != bq) ? 1 : 0;   // an own mutation equal to the entry hides it (main.cpp:436-449)
        col[(b.btab[p] + 1) * st] += uk - eb;
        E += ek - eb;
    }
    const bool lf = t.leaf[k] != 0;
    const bool elig = root || (hu && !lf && common > 0 && nm != common) || (lf && common > 0) || (!hu && !lf && nm == common);
    const bool under = t.dfs[b.nid] < t.dfs[k] && t.dfs[k] < t.dend[b.nid];
    b.score[b.c0 + c] = E + (elig ? 0 : 1);
    b.flags[b.c0 + c] = (uint8_t)((elig ? kElig : 0) | ((hu && !root) ? kHasUnique : 0) | (under ? kUnder : 0) | (lf ? kLeaf : 0));
    if (elig) atomicMin(b.minE, E);
    int acc = 0;
    for (uint32_t x = 1; x <= b.nb; x++) { acc += col[x * st]; col[x * st] = acc; }
}

__device__ __forceinline__ void ins3(uint64_t &a, uint64_t &m, uint64_t &z, uint64_t key) {   // keep the 3 smallest, sorted
    const bool l0 = key < a, l1 = key < m, l2 = key < z;
    const uint64_t na = l0 ? key : a, nm = l0 ? a : (l1 ? key : m), nz = l1 ? m : (l2 ? key : z);
    a = na; m = nm; z = nz;
}

struct Pairs {
    uint32_t P, tile, ntiles;
    int32_t B;
    const uint32_t *ij;   // [P] i | j << 16
    uint64_t *slab;       // [gridDim.x][P][6]: donors 0-2, acceptors 3-5
};

// One thread per pair, the candidates of a tile in LDS; each block folds its tiles into its slab row.
__global__ void __launch_bounds__(kBlock) k_pairs(Tree t, Branch b, Pairs pr) {
    // [(nb + 1) rows of tile + 1] bucket sums (the padding puts rows 2j and 2i + 1 of one candidate in different banks), then
    // [tile] rank (kNil: not a candidate here)
    extern __shared__ int32_t lds[];
    const uint32_t T = pr.tile, TP = T + 1, W = b.nb + 1;
    uint32_t *lrank = (uint32_t *)(lds + (size_t)W * TP);
    for (uint32_t g = blockIdx.x; g < pr.ntiles; g += gridDim.x) {
        const uint32_t c0 = g * T, cn = min(T, b.Cc - c0);
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < W * T; x += blockDim.x) {
            const uint32_t row = x / T, c = x % T;
            lds[row * TP + c] = c < cn ? b.S[(size_t)row * b.Cc + c0 + c] : 0;
        }
        for (uint32_t c = threadIdx.x; c < T; c += blockDim.x) {
            uint32_t r = kNil;
            if (c < cn && !(b.flags[b.c0 + c0 + c] & kUnder)) r = t.rank[b.cand[b.c0 + c0 + c]];
            lrank[c] = r;
        }
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < pr.P; q += blockDim.x) {
            const uint32_t i = pr.ij[q] & 0xffffu, j = pr.ij[q] >> 16;
            uint64_t *o = pr.slab + ((size_t)blockIdx.x * pr.P + q) * 6;
            uint64_t d0 = o[0], d1 = o[1], d2 = o[2], a0 = o[3], a1 = o[4], a2 = o[5];
            const int32_t *hi = lds + (size_t)(2 * j) * TP, *lo = lds + (size_t)(2 * i + 1) * TP, *tot = lds + (size_t)(W - 1) * TP;
            for (uint32_t c = 0; c < cn; c++) {
                const uint32_t r = lrank[c];
                if (r == kNil) continue;
                const int32_t in = hi[c] - lo[c], out = tot[c] - in;
                if (in <= pr.B) ins3(d0, d1, d2, (uint64_t)(uint32_t)in << 32 | r);
                if (out <= pr.B) ins3(a0, a1, a2, (uint64_t)(uint32_t)out << 32 | r);
            }
            o[0] = d0; o[1] = d1; o[2] = d2; o[3] = a0; o[4] = a1; o[5] = a2;
        }
    }
}

// Per pair: the top-3 of each list over every block's partial (the keys are distinct, so any merge order gives these).
__global__ void k_merge(Pairs pr, uint32_t nblk, uint64_t *top) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= pr.P) return;
    uint64_t d0 = kKeyMax, d1 = kKeyMax, d2 = kKeyMax, a0 = kKeyMax, a1 = kKeyMax, a2 = kKeyMax;
    for (uint32_t g = 0; g < nblk; g++) {
        const uint64_t *o = pr.slab + ((size_t)g * pr.P + q) * 6;
        ins3(d0, d1, d2, o[0]); ins3(d0, d1, d2, o[1]); ins3(d0, d1, d2, o[2]);
        ins3(a0, a1, a2, o[3]); ins3(a0, a1, a2, o[4]); ins3(a0, a1, a2, o[5]);
    }
    uint64_t *w = top + (size_t)q * 6;
    w[0] = d0; w[1] = d1; w[2] = d2; w[3] = a0; w[4] = a1; w[5] = a2;
}

__global__ void k_fetch(const uint32_t *idx, uint32_t n, const int32_t *score, const uint8_t *flags, int32_t *os, uint8_t *of) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    os[x] = score[idx[x]];
    of[x] = flags[idx[x]];
}

}  // namespace

struct RipState {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n = 0, tp = 0;
    std::vector<uint32_t> parent, moff, rank, inv_rank, size, cand_of;
    std::vector<int32_t> mpos;
    std::vector<uint32_t> mbits;
    DBuf<uint32_t> d_parent, d_moff, d_mbits, d_dfs, d_dend, d_rank;
    DBuf<int32_t> d_mpos;
    DBuf<uint8_t> d_leaf;
    // candidates of the last num_descendants
    uint32_t cand_nd = kNil;
    std::vector<uint32_t> cand;
    DBuf<uint32_t> d_cand;
    // per-branch workspace
    DBuf<int32_t> qpos, base0, S, score, minE, fscore;
    DBuf<uint8_t> qnuc, flags, fflags;
    DBuf<uint32_t> btab, ij, fidx;
    DBuf<uint16_t> srow;
    DBuf<uint64_t> slab, top;
    ~RipState() {
        if (stream) { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    }
};

void rip_free(RipState *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int rip_attach(const ugp_tree_desc *tree, const uint32_t *name_rank, const std::vector<uint32_t> &bfs2dfs, int device, RipState **out) {
    if (!tree || !out || !tree->parent || !tree->mut_off || !name_rank) return set_error(UGP_ERR_INVALID, "null argument");
    const uint64_t N = tree->n_nodes;
    if (N == 0 || N >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "node count out of range");
    if (bfs2dfs.size() != N) return set_error(UGP_ERR_INVALID, "tree does not match the handle");
    const uint64_t Mu = tree->mut_off[N];
    if (Mu >= (1ull << 32)) return set_error(UGP_ERR_UNSUPPORTED, "more than 2^32 mutation entries");
    if (Mu && (!tree->mut_pos || !tree->mut_ref || !tree->mut_nuc)) return set_error(UGP_ERR_INVALID, "null mutation arrays");
    RipState *S = nullptr;
    try {
        S = new RipState();
        S->device = device;
        S->n = (uint32_t)N;
        S->parent.assign(tree->parent, tree->parent + N);
        S->parent[0] = kNil;
        for (uint64_t j = 1; j < N; j++)
            if (S->parent[j] >= j) { delete S; return set_error(UGP_ERR_INVALID, "parent[] is not in breadth-first order"); }
        S->rank.assign(name_rank, name_rank + N);
        S->inv_rank.assign(N, kNil);
        for (uint64_t j = 0; j < N; j++) {
            if (S->rank[j] >= N || S->inv_rank[S->rank[j]] != kNil) { delete S; return set_error(UGP_ERR_INVALID, "name_rank is not a permutation"); }
            S->inv_rank[S->rank[j]] = (uint32_t)j;
        }
        S->moff.resize(N + 1);
        S->mpos.resize(Mu);
        S->mbits.resize(Mu);
        int32_t maxpos = -1;
        for (uint64_t j = 0; j <= N; j++) S->moff[j] = (uint32_t)tree->mut_off[j];
        for (uint64_t e = 0; e < Mu; e++) {
            S->mpos[e] = tree->mut_pos[e];
            S->mbits[e] = (uint32_t)tree->mut_nuc[e] | (uint32_t)tree->mut_ref[e] << 8;
            maxpos = std::max(maxpos, tree->mut_pos[e]);
        }
        if (maxpos >= (1 << 28)) { delete S; return set_error(UGP_ERR_UNSUPPORTED, "mutation position above 2^28"); }
        S->tp = (uint32_t)(maxpos + 1);
        // subtree sizes (tree_num_leaves of main.cpp:280-289: nodes, self included), leaves, the handle's preorder for "under nid"
        const std::vector<uint32_t> &dfs = bfs2dfs;
        std::vector<uint32_t> sz(N, 1), dend(N);
        std::vector<uint8_t> leaf(N, 1);
        for (uint64_t j = N; j-- > 1;) { sz[S->parent[j]] += sz[j]; leaf[S->parent[j]] = 0; }
        for (uint64_t j = 0; j < N; j++) dend[j] = dfs[j] + sz[j];
        S->size = sz;
        // parent state of every non-masked entry: the nearest entry above it at its position (per position, entries in preorder)
        {
            const uint32_t tp = S->tp;
            std::vector<uint32_t> poff(tp + 1, 0), pent, node_of(Mu);
            for (uint64_t j = 0; j < N; j++) for (uint32_t e = S->moff[j]; e < S->moff[j + 1]; e++) node_of[e] = (uint32_t)j;
            for (uint64_t e = 0; e < Mu; e++) if (S->mpos[e] >= 0) poff[S->mpos[e] + 1]++;
            for (uint32_t p = 0; p < tp; p++) poff[p + 1] += poff[p];
            pent.resize(poff[tp]);
            std::vector<uint32_t> fill(poff.begin(), poff.end() - 1);
            for (uint64_t e = 0; e < Mu; e++) if (S->mpos[e] >= 0) pent[fill[S->mpos[e]]++] = (uint32_t)e;
            std::vector<uint32_t> st;
            for (uint32_t p = 0; p < tp; p++) {
                std::sort(pent.begin() + poff[p], pent.begin() + poff[p + 1],
                          [&](uint32_t a, uint32_t c) { return dfs[node_of[a]] < dfs[node_of[c]]; });
                st.clear();
                for (uint32_t x = poff[p]; x < poff[p + 1]; x++) {
                    const uint32_t e = pent[x], u = node_of[e];
                    while (!st.empty() && dend[node_of[st.back()]] <= dfs[u]) st.pop_back();
                    if (!st.empty() && node_of[st.back()] == u) { delete S; return set_error(UGP_ERR_UNSUPPORTED, "two mutations at one position on one branch"); }
                    if (!st.empty()) S->mbits[e] |= (S->mbits[st.back()] & 0xffu) << 16;
                    st.push_back(e);
                }
            }
        }
        if (hipSetDevice(device) != hipSuccess) { delete S; return set_error(UGP_ERR_HIP, "hipSetDevice failed"); }
        hipStream_t s = nullptr;
        hipError_t err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        S->stream = s;
        if (err == hipSuccess) err = S->d_parent.upload(S->parent, s);
        if (err == hipSuccess) err = S->d_moff.upload(S->moff, s);
        if (err == hipSuccess) err = S->d_mbits.upload(S->mbits, s);
        if (err == hipSuccess) err = S->d_mpos.upload(S->mpos, s);
        if (err == hipSuccess) err = S->d_dfs.upload(dfs, s);
        if (err == hipSuccess) err = S->d_dend.upload(dend, s);
        if (err == hipSuccess) err = S->d_rank.upload(S->rank, s);
        if (err == hipSuccess) err = S->d_leaf.upload(leaf, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        if (err != hipSuccess) { delete S; return set_error(UGP_ERR_HIP, std::string("ripples tables: ") + hipGetErrorString(err)); }
    } catch (const std::bad_alloc &) {
        delete S;
        return set_error(UGP_ERR_NOMEM, "out of host memory");
    }
    rip_free(*out);
    *out = S;
    return UGP_OK;
}

namespace {
struct Row { int32_t pos; uint8_t ref, nuc; };
}

int rip_run(RipState *S, const ugp_ripples_opts *o, const uint32_t *branches, uint64_t n, ugp_ripples_event *out, uint64_t cap,
            uint64_t *n_out) {
    if (!S) return set_error(UGP_ERR_INVALID, "no ripples tables: call ugp_ripples_attach first");
    if (!o || !n_out || (n && !branches) || (cap && !out)) return set_error(UGP_ERR_INVALID, "null argument");
    if (o->branch_len < 1 || o->parsimony_improvement < 0) return set_error(UGP_ERR_INVALID, "branch_len must be >= 1 and parsimony_improvement >= 0");
    for (uint64_t i = 0; i < n; i++) if (branches[i] >= S->n) return set_error(UGP_ERR_INVALID, "branch index out of range");
    *n_out = 0;
    if (!n) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(S->device));
    hipStream_t st = S->stream;
    const uint32_t N = S->n;
    // UGP_RIPPLES_LIMITS="count_bytes,slab_bytes,lds_ints" lowers the workspace limits (a test hook: small trees then take the
    // candidate-chunk, slab-clamp and one-candidate-tile paths that otherwise only very large inputs reach)
    struct { uint64_t count = kCountBudget, slab = kSlabBudget, lds = kLdsInts; } lim;
    if (const char *env = getenv("UGP_RIPPLES_LIMITS")) {
        unsigned long long a = 0, b = 0, c = 0;
        if (sscanf(env, "%llu,%llu,%llu", &a, &b, &c) == 3) {
            lim.count = std::max<uint64_t>(1, std::min<uint64_t>(a, kCountBudget));
            lim.slab = std::max<uint64_t>(1, std::min<uint64_t>(b, kSlabBudget));
            lim.lds = std::max<uint64_t>(1, std::min<uint64_t>(c, kLdsInts));
        }
    }
    if (S->cand_nd != o->num_descendants) {
        S->cand.clear();
        S->cand_of.assign(N, kNil);
        for (uint32_t k = 0; k < N; k++)
            if (S->size[k] >= o->num_descendants) { S->cand_of[k] = (uint32_t)S->cand.size(); S->cand.push_back(k); }
        UGP_HIP_TRY(S->d_cand.upload(S->cand, st));
        S->cand_nd = o->num_descendants;
    }
    const uint32_t C = (uint32_t)S->cand.size();
    Tree t{N, S->tp, S->d_parent.p, S->d_moff.p, S->d_mbits.p, S->d_dfs.p, S->d_dend.p, S->d_rank.p, S->d_mpos.p, S->d_leaf.p};
    std::vector<Row> rows;
    std::unordered_set<int32_t> seen;
    std::vector<int32_t> qpos, base0;
    std::vector<uint8_t> qnuc;
    std::vector<uint32_t> btab(S->tp), ij, fidx;
    std::vector<uint16_t> srow(S->tp);
    std::vector<uint64_t> top;
    std::vector<ugp_ripples_event> ev;
    std::vector<int32_t> fscore;
    std::vector<uint8_t> fflags;
    uint64_t total = 0;
    for (uint64_t bi = 0; bi < n; bi++) {
        const uint32_t nid = branches[bi];
        const int orig = (int)(S->moff[nid + 1] - S->moff[nid]);
        const int B = orig - o->parsimony_improvement;
        // Pruned_Sample of the root path (main.cpp:68-90, 317-325): the lowest occurrence of a position wins
        rows.clear(); seen.clear();
        for (uint32_t v = nid; v != kNil; v = S->parent[v])
            for (uint32_t e = S->moff[v]; e < S->moff[v + 1]; e++) {
                const int32_t p = S->mpos[e];
                const uint8_t nuc = (uint8_t)(S->mbits[e] & 0xffu), ref = (uint8_t)((S->mbits[e] >> 8) & 0xffu);
                if (ref != nuc && !seen.count(p)) rows.push_back({p, ref, nuc});
                seen.insert(p);
            }
        std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &c) { return a.pos < c.pos; });
        const uint32_t M = (uint32_t)rows.size();
        if (M >= 0xffffu) return set_error(UGP_ERR_UNSUPPORTED, "a branch's root path carries 65535 or more sample rows");
        // valid breakpoint pairs (:383-413)
        ij.clear();
        for (uint32_t i = 0; i < M; i++)
            for (uint32_t j = i; j < M; j++) {
                const int64_t el = j >= 1 ? rows[j - 1].pos : 0, span = el - (int64_t)rows[i].pos;
                if (j - i < o->branch_len || M - (j - i) < o->branch_len || span < o->min_range || span > o->max_range) continue;
                ij.push_back(i | j << 16);
            }
        if (ij.empty() || B < 0 || C == 0) continue;
        const uint32_t P = (uint32_t)ij.size(), nb = 2 * M + 1;
        qpos.resize(M); qnuc.resize(M);
        std::fill(srow.begin(), srow.end(), 0);
        base0.assign(nb + 1, 0);
        for (uint32_t q = 0; q < M; q++) {
            qpos[q] = rows[q].pos; qnuc[q] = rows[q].nuc;
            if (rows[q].pos >= 0) srow[rows[q].pos] = (uint16_t)(rows[q].nuc | rows[q].ref << 8);
            if (!(rows[q].nuc & rows[q].ref)) { base0[2 * q + 1]++; base0[nb]++; }   // loop 2 of a row against the root state
        }
        {
            uint32_t lb = 0;
            for (uint32_t p = 0; p < S->tp; p++) {
                while (lb < M && rows[lb].pos < (int32_t)p) lb++;
                btab[p] = 2 * lb + ((lb < M && rows[lb].pos == (int32_t)p) ? 1u : 0u);
            }
        }
        UGP_HIP_TRY(S->qpos.upload(qpos, st)); UGP_HIP_TRY(S->qnuc.upload(qnuc, st));
        UGP_HIP_TRY(S->btab.upload(btab, st)); UGP_HIP_TRY(S->srow.upload(srow, st));
        UGP_HIP_TRY(S->base0.upload(base0, st)); UGP_HIP_TRY(S->ij.upload(ij, st));
        UGP_HIP_TRY(S->score.alloc(C)); UGP_HIP_TRY(S->flags.alloc(C)); UGP_HIP_TRY(S->minE.alloc(1));
        UGP_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)S->minE.p, INT_MAX, 1, st));
        if (48ull * P > kSlabBudget) return set_error(UGP_ERR_UNSUPPORTED, "a branch has more than 5,592,405 valid breakpoint pairs");
        const uint32_t Cc = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(C, lim.count / (4ull * (nb + 1))));
        const uint32_t fit = (uint32_t)(lim.lds / (nb + 1)), tile = fit >= 2 ? std::min(kTileMax, fit - 1) : 1u;
        const size_t lds = (size_t)(nb + 1) * (tile + 1) * sizeof(int32_t) + tile * sizeof(uint32_t);
        if (lds > 64 * 1024) return set_error(UGP_ERR_UNSUPPORTED, "too many sample rows for one LDS tile");
        const uint32_t tiles_all = (C + tile - 1) / tile;
        const uint32_t nblk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({1024, tiles_all, lim.slab / (48ull * P)}));
        UGP_HIP_TRY(S->S.alloc((size_t)(nb + 1) * Cc));
        UGP_HIP_TRY(S->slab.alloc((size_t)nblk * P * 6)); UGP_HIP_TRY(S->top.alloc((size_t)P * 6));
        UGP_HIP_TRY(hipMemsetAsync(S->slab.p, 0xff, (size_t)nblk * P * 6 * sizeof(uint64_t), st));
        Pairs pr{P, tile, 0, B, S->ij.p, S->slab.p};
        for (uint32_t c0 = 0; c0 < C; c0 += Cc) {
            const uint32_t cc = std::min(Cc, C - c0);
            Branch b{nid, M, nb, C, c0, cc, S->qpos.p, S->qnuc.p, S->btab.p, S->srow.p, S->base0.p, S->d_cand.p, S->S.p,
                     S->score.p, S->flags.p, S->minE.p};
            k_count<<<(cc + kBlock - 1) / kBlock, kBlock, 0, st>>>(t, b);
            pr.ntiles = (cc + tile - 1) / tile;
            k_pairs<<<std::min(nblk, pr.ntiles), kBlock, lds, st>>>(t, b, pr);
        }
        k_merge<<<(P + kBlock - 1) / kBlock, kBlock, 0, st>>>(pr, nblk, S->top.p);
        UGP_HIP_TRY(hipGetLastError());
        top.resize((size_t)P * 6);
        int32_t minE = 0;
        UGP_HIP_TRY(hipMemcpyAsync(top.data(), S->top.p, top.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(&minE, S->minE.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        // the donor-acceptor choice (:594-606) on the top-3 lists: nid removed, the first two of each list decide
        ev.clear(); fidx.clear();
        const uint32_t nid_rank = S->rank[nid];
        for (uint32_t q = 0; q < P; q++) {
            uint64_t d[2], a[2];
            uint32_t nd = 0, na = 0;
            for (uint32_t x = 0; x < 3; x++) {
                const uint64_t kd = top[(size_t)q * 6 + x], ka = top[(size_t)q * 6 + 3 + x];
                if (kd != kKeyMax && (uint32_t)kd != nid_rank && nd < 2) d[nd++] = kd;
                if (ka != kKeyMax && (uint32_t)ka != nid_rank && na < 2) a[na++] = ka;
            }
            bool hit = false;
            for (uint32_t x = 0; x < nd && !hit; x++)
                for (uint32_t y = 0; y < na && !hit; y++) {
                    if ((uint32_t)d[x] == (uint32_t)a[y] || (int64_t)(d[x] >> 32) + (int64_t)(a[y] >> 32) > B) continue;
                    hit = true;
                    ugp_ripples_event e;
                    std::memset(&e, 0, sizeof(e));
                    e.branch = bi; e.i = ij[q] & 0xffffu; e.j = ij[q] >> 16;
                    e.donor = S->inv_rank[(uint32_t)d[x]]; e.acceptor = S->inv_rank[(uint32_t)a[y]];
                    e.donor_count = (uint32_t)(d[x] >> 32); e.acceptor_count = (uint32_t)(a[y] >> 32);
                    ev.push_back(e);
                    fidx.push_back(S->cand_of[e.donor]); fidx.push_back(S->cand_of[e.acceptor]);
                }
        }
        if (ev.empty()) continue;
        const uint32_t nf = (uint32_t)fidx.size();
        UGP_HIP_TRY(S->fidx.upload(fidx, st)); UGP_HIP_TRY(S->fscore.alloc(nf)); UGP_HIP_TRY(S->fflags.alloc(nf));
        k_fetch<<<(nf + kBlock - 1) / kBlock, kBlock, 0, st>>>(S->fidx.p, nf, S->score.p, S->flags.p, S->fscore.p, S->fflags.p);
        UGP_HIP_TRY(hipGetLastError());
        fscore.resize(nf); fflags.resize(nf);
        UGP_HIP_TRY(hipMemcpyAsync(fscore.data(), S->fscore.p, nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(fflags.data(), S->fflags.p, nf, hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        // is_sibling: a leaf, or one of the final ties (eligible, set difference = the minimum) that has a unique mutation
        auto sib = [&](uint32_t x) {
            const uint8_t f = fflags[x];
            const int32_t E = fscore[x] - ((f & kElig) ? 0 : 1);
            return (uint8_t)(((f & kLeaf) || ((f & kElig) && E == minE && (f & kHasUnique))) ? 1 : 0);
        };
        for (size_t x = 0; x < ev.size(); x++) {
            ugp_ripples_event &e = ev[x];
            e.donor_score = fscore[2 * x]; e.acceptor_score = fscore[2 * x + 1];
            e.donor_sibling = sib((uint32_t)(2 * x)); e.acceptor_sibling = sib((uint32_t)(2 * x + 1));
            if (total < cap) out[total] = e;
            total++;
        }
    }
    *n_out = total;
    return UGP_OK;
}

}  // namespace ugp
