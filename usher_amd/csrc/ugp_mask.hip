// ugp_mask.hip -- matUtils mask on the device (mask.cpp: restrictSamples :802-905, restrictMutationsLocally with
// mask_mutation_on_branch and match_mutations :703-800), both as closed forms over depth-first ranges.
//
// Restricted samples, every named node a leaf.  Leaf r is the r-th leaf in depth-first order; the leaves below v are the ranks
// [lbefore[v], lbefore[dend[v]]).  full[v]: all of them are named.  F: the inner nodes that are full and have a leaf child.
//   k_msk_names      one lane per name: its bit of the bitmap over leaf ranks
//   k_msk_segsum / k_msk_wordscan   the named ranks in front of every word of the bitmap (seg_carry, block_incl_scan: ugp_scan.hpp)
//   k_msk_full       one lane per node: full[v]; a node of F adds +1 at v and -1 at dend[v] to a difference array
//   k_msk_segsum / k_msk_cover      A[v] = the nodes of F on v's root path, v included, by a scan over depth-first order.  A root is a
//                    node of F with A = 1, or a named leaf whose parent is not full; v is covered when A >= 1 or it is such a leaf
//                    (a leaf below a node of F has a full parent, so the two kinds of root never nest)
//   k_msk_mark       one lane per entry: a non-masked entry on an uncovered node marks table[position, parent allele, allele]
//   k_msk_read       one lane per entry: a non-masked entry on a covered node is masked when its key is not marked
// Mutations: one lane per entry.  The lines of a batch are sorted by position (file order within one position); the lane finds the
// lines of its position by binary search and takes the first whose alleles match, whose target's range holds its node and none of
// whose exclusion ranges (strict descendants of the target, filtered on the host) does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "ugp_mask.hpp"
#include "ugp_query.hpp"

namespace ugp {
namespace {

constexpr uint32_t kDefaultLines = 1u << 16;   // lines staged per launch
constexpr uint32_t kMaxTablePos = 1u << 22;    // positions the direct key table takes (256 bytes each: 1 GiB)
constexpr uint8_t kCover = 1, kRoot = 2;       // node flags of the restricted pass
typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "bitmap words and counts are 64-bit");

__global__ void __launch_bounds__(kBlock) k_msk_names(uint32_t nn, const uint32_t *ranks, u64 *words) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < nn) atomicOr(&words[ranks[i] >> 6], 1ull << (ranks[i] & 63u));
}

struct WordBits {   // scan input: the bits set in word i
    const u64 *words;
    __device__ __forceinline__ int operator()(uint32_t i) const { return __popcll(words[i]); }
};
struct DiffAt {     // scan input: the difference array
    const int32_t *diff;
    __device__ __forceinline__ int operator()(uint32_t i) const { return diff[i]; }
};

// One block per segment: the sum of in(i) over it.
template <class In>
__global__ void __launch_bounds__(kBlock) k_msk_segsum(uint32_t n, In in, int32_t *seg) {
    __shared__ int sh[kBlock / 64];
    const uint32_t lo = blockIdx.x * kSeg, hi = min(n, lo + kSeg);
    int acc = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kBlock) acc += in(i);
    int tot;
    (void)block_incl_scan(acc, sh, &tot);
    if (threadIdx.x == 0) seg[blockIdx.x] = tot;
}

// One block per segment: wpre[i] = the bits set in the words before word i.
__global__ void __launch_bounds__(kBlock) k_msk_wordscan(uint32_t n, const u64 *words, const int32_t *seg, uint32_t *wpre) {
    __shared__ int sh[kBlock / 64];
    const uint32_t g = blockIdx.x, lo = g * kSeg, hi = min(n, lo + kSeg);
    int carry = seg_carry(seg, g, sh), tot;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t i = t0 + threadIdx.x;
        const int f = i < hi ? __popcll(words[i]) : 0;
        const int incl = block_incl_scan(f, sh, &tot);
        if (i < hi) wpre[i] = (uint32_t)(carry + incl - f);
        carry += tot;
    }
}

// The named ranks below r (r <= nleaf: the bitmap has a zero word past the last leaf).
__device__ __forceinline__ uint32_t named_before(const u64 *words, const uint32_t *wpre, uint32_t r) {
    return wpre[r >> 6] + (uint32_t)__popcll(words[r >> 6] & ((1ull << (r & 63u)) - 1ull));
}

__global__ void __launch_bounds__(kBlock) k_msk_full(DfsView t, const uint32_t *lbefore, const uint8_t *hasleaf, const u64 *words,
                                                     const uint32_t *wpre, uint8_t *full, int32_t *diff) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= t.n) return;
    const uint32_t end = t.dend[v], lo = lbefore[v], hi = lbefore[end];
    const bool f = named_before(words, wpre, hi) - named_before(words, wpre, lo) == hi - lo;   // hi > lo: a leaf is below itself
    full[v] = f ? 1 : 0;
    if (f && hasleaf[v]) {   // a node of F (a leaf has no leaf child)
        atomicAdd(&diff[v], 1);
        atomicAdd(&diff[end], -1);
    }
}

// One block per segment: the node flags from the scan of the difference array.
__global__ void __launch_bounds__(kBlock) k_msk_cover(DfsView t, const uint8_t *hasleaf, const uint8_t *full, const int32_t *diff,
                                                      const int32_t *seg, uint8_t *flag) {
    __shared__ int sh[kBlock / 64];
    const uint32_t g = blockIdx.x, lo = g * kSeg, hi = min(t.n, lo + kSeg);
    int carry = seg_carry(seg, g, sh), tot;
    for (uint32_t t0 = lo; t0 < hi; t0 += kBlock) {
        const uint32_t v = t0 + threadIdx.x;
        const int A = carry + block_incl_scan(v < hi ? diff[v] : 0, sh, &tot);
        carry += tot;
        if (v >= hi) continue;
        const bool fv = full[v] != 0;
        const bool top = fv && hasleaf[v] && A == 1;
        const bool own = fv && t.leaf[v] && (v == 0 || !full[t.dpar[v]]);   // a full leaf is a named leaf
        flag[v] = (uint8_t)((A >= 1 || own ? kCover : 0) | (top || own ? kRoot : 0));
    }
}

// The key as the reference's get_string() tells keys apart: the codes 0 and 15 both print as N.
__device__ __forceinline__ size_t key_of(int32_t p, uint8_t pn) {
    const uint32_t par = pn >> 4, nuc = pn & 15u;
    return ((size_t)(uint32_t)p << 8) | ((par ? par : 15u) << 4) | (nuc ? nuc : 15u);
}

__global__ void __launch_bounds__(kBlock) k_msk_mark(DfsView t, uint32_t m, const uint8_t *mpn, const uint8_t *flag, uint8_t *table) {
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= m) return;
    const int32_t p = t.mpos[e];
    if (p >= 0 && !(flag[t.mnode[e]] & kCover)) table[key_of(p, mpn[e])] = 1;
}

// out is in the caller's CSR order (morig); every entry's byte is written.
__global__ void __launch_bounds__(kBlock) k_msk_read(DfsView t, uint32_t m, const uint8_t *mpn, const uint8_t *flag, const uint8_t *table,
                                                     uint8_t *out, u64 *n_masked) {
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    bool mk = false;
    if (e < m) {
        const int32_t p = t.mpos[e];
        mk = p >= 0 && (flag[t.mnode[e]] & kCover) && !table[key_of(p, mpn[e])];
        out[t.morig[e]] = mk ? 1 : 0;
    }
    const u64 votes = __ballot(mk);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(n_masked, (u64)__popcll(votes));
}

struct LinesView {   // a batch of lines, sorted by position and within one position by file order
    uint32_t n;
    const uint32_t *pos;          // as uint32: a negative position sorts last and equals no entry's
    const uint8_t *par, *nuc;     // 4-bit codes, 15: any
    const uint32_t *tlo, *thi;    // the target's depth-first range
    const uint32_t *idx;          // the line's number in the file
    const uint32_t *xoff, *xlo, *xhi;   // per line its exclusion ranges [xoff[k], xoff[k + 1])
};

// first (caller's CSR order) is kNil where no earlier batch took the entry; counts is indexed by file line.
__global__ void __launch_bounds__(kBlock) k_msk_mutations(DfsView t, uint32_t m, const uint8_t *mpn, const uint8_t *skip, LinesView L,
                                                          uint32_t *first, u64 *counts) {
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= m) return;
    const int32_t p = t.mpos[e];
    if (p < 0) return;
    uint32_t k = lower_bound_u32(L.pos, 0, L.n, (uint32_t)p);
    if (k >= L.n || L.pos[k] != (uint32_t)p) return;
    const uint32_t o = t.morig[e];
    if ((skip && skip[o]) || first[o] != kNil) return;
    const uint32_t v = t.mnode[e], par = mpn[e] >> 4, nuc = mpn[e] & 15u;
    for (; k < L.n && L.pos[k] == (uint32_t)p; k++) {
        if ((L.par[k] != 15u && L.par[k] != par) || (L.nuc[k] != 15u && L.nuc[k] != nuc)) continue;
        if (v < L.tlo[k] || v >= L.thi[k]) continue;
        bool out = false;
        for (uint32_t x = L.xoff[k]; x < L.xoff[k + 1] && !out; x++) out = v >= L.xlo[x] && v < L.xhi[x];
        if (out) continue;
        first[o] = L.idx[k];
        atomicAdd(&counts[L.idx[k]], 1ull);
        return;
    }
}

}  // namespace

struct MskState : QueryBase {
    uint32_t nleaf = 0, nwords = 0;               // nwords counts the zero word past the last leaf
    std::vector<uint32_t> h_lbefore, h_dend;      // [n + 1], [n]
    DBuf<uint32_t> lbefore;
    DBuf<uint8_t> hasleaf, mpn;                   // per node; per depth-first entry: stored parent allele << 4 | allele
    // restricted pass
    DBuf<uint32_t> ranks, wpre;
    DBuf<u64> words, nmasked;
    DBuf<int32_t> diff, seg;
    DBuf<uint8_t> full, flag, table, emask;
    std::vector<uint8_t> h_flag;
    // mutation pass
    DBuf<uint32_t> lpos, ltlo, lthi, lidx, lxoff, lxlo, lxhi, first;
    DBuf<uint8_t> lpar, lnuc, skip;
    DBuf<u64> counts;
};

void msk_free(MskState *s) { query_free(s); }

int msk_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, MskState **out) {
    std::vector<uint8_t> mpn;
    return query_attach(
        "ugp_mask_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out,
        [&](const DfsTables &T) { return stored_alleles(tree, dfs2bfs, T, "ugp_mask_attach", &mpn); },
        [&](MskState *S) {
            const uint32_t N = S->T->n;
            const uint64_t M = S->T->m;
            LeafRanks R;
            leaf_ranks(tree, dfs2bfs, bfs2dfs, &R);
            std::vector<uint8_t> hasleaf(N, 0);   // "has a leaf child"
            for (uint32_t i : R.leaf_dfs) if (i) hasleaf[bfs2dfs[tree->parent[dfs2bfs[i]]]] = 1;
            const uint32_t nleaf = (uint32_t)R.leaf_dfs.size();
            S->h_lbefore = std::move(R.lbefore);
            S->h_dend = std::move(R.dend);
            S->nleaf = nleaf;
            S->nwords = nleaf / 64u + 1u;
            S->h_flag.resize(N);
            const StreamDrain drain{S->stream};   // hasleaf and mpn
            hipError_t err = S->lbefore.upload(S->h_lbefore, S->stream);
            if (err == hipSuccess) err = S->hasleaf.upload(hasleaf, S->stream);
            if (err == hipSuccess) err = S->mpn.upload(mpn, S->stream);
            if (err == hipSuccess) err = S->words.alloc(S->nwords);
            if (err == hipSuccess) err = S->wpre.alloc(S->nwords);
            if (err == hipSuccess) err = S->diff.alloc((size_t)N + 1);
            if (err == hipSuccess) err = S->seg.alloc(std::max(segs_for((uint64_t)N + 1), segs_for(S->nwords)));
            if (err == hipSuccess) err = S->full.alloc(N);
            if (err == hipSuccess) err = S->flag.alloc(N);
            if (err == hipSuccess) err = S->nmasked.alloc(1);
            if (err == hipSuccess) err = S->emask.alloc(M);
            if (err == hipSuccess) err = S->first.alloc(M);
            if (err == hipSuccess) err = hipStreamSynchronize(S->stream);   // hasleaf and mpn are read until here
            return hip_rc("ugp_mask_attach", err);
        });
}

static int msk_ready(MskState *S, const char *who) { return query_ready(S, who, "mask"); }

// ---- restricted samples -------------------------------------------------------------------------------------------------

// The names as leaf ranks (duplicates stay: the bitmap takes them once).
static int msk_ranks(MskState *S, const char *who, uint64_t n, const uint32_t *leaves_bfs, std::vector<uint32_t> *ranks) {
    const uint32_t N = S->T->n;
    if (!n || !leaves_bfs) return set_error(UGP_ERR_INVALID, std::string(who) + ": no nodes given");
    if (n >= (1ull << 31)) return set_error(UGP_ERR_INVALID, std::string(who) + ": more than 2^31 nodes given");
    for (uint64_t i = 0; i < n; i++)
        if (leaves_bfs[i] >= N) return set_error(UGP_ERR_INVALID, std::string(who) + ": node " + std::to_string(i) + " is out of range");
    if ((uint64_t)S->T->tp > kMaxTablePos)
        return set_error(UGP_ERR_UNSUPPORTED, std::string(who) + ": positions reach past the direct key table; walk on the host");
    ranks->resize(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t v = S->T->bfs2dfs[leaves_bfs[i]];
        if (S->h_dend[v] != v + 1)
            return set_error(UGP_ERR_UNSUPPORTED, std::string(who) + ": node " + std::to_string(i) + " is not a leaf; walk on the host");
        (*ranks)[i] = S->h_lbefore[v];
    }
    return UGP_OK;
}

// The passes over the staged ranks: S->flag per node, S->emask per entry, S->nmasked.
static int msk_restricted_passes(MskState *S, uint32_t nn) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const uint32_t N = t.n, M = (uint32_t)S->T->m, nw = S->nwords;
    UGP_HIP_TRY(hipMemsetAsync(S->words.p, 0, (size_t)nw * sizeof(u64), st));
    UGP_HIP_TRY(hipMemsetAsync(S->diff.p, 0, ((size_t)N + 1) * sizeof(int32_t), st));
    UGP_HIP_TRY(hipMemsetAsync(S->table.p, 0, std::max<size_t>((size_t)t.tp * 256, 1), st));
    UGP_HIP_TRY(hipMemsetAsync(S->nmasked.p, 0, sizeof(u64), st));
    k_msk_names<<<blocks_for(nn), kBlock, 0, st>>>(nn, S->ranks.p, S->words.p);
    k_msk_segsum<<<segs_for(nw), kBlock, 0, st>>>(nw, WordBits{S->words.p}, S->seg.p);
    k_msk_wordscan<<<segs_for(nw), kBlock, 0, st>>>(nw, S->words.p, S->seg.p, S->wpre.p);
    k_msk_full<<<blocks_for(N), kBlock, 0, st>>>(t, S->lbefore.p, S->hasleaf.p, S->words.p, S->wpre.p, S->full.p, S->diff.p);
    k_msk_segsum<<<segs_for(N), kBlock, 0, st>>>(N, DiffAt{S->diff.p}, S->seg.p);
    k_msk_cover<<<segs_for(N), kBlock, 0, st>>>(t, S->hasleaf.p, S->full.p, S->diff.p, S->seg.p, S->flag.p);
    if (M) {
        k_msk_mark<<<blocks_for(M), kBlock, 0, st>>>(t, M, S->mpn.p, S->flag.p, S->table.p);
        k_msk_read<<<blocks_for(M), kBlock, 0, st>>>(t, M, S->mpn.p, S->flag.p, S->table.p, S->emask.p, S->nmasked.p);
    }
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

static int msk_restricted_stage(MskState *S, const std::vector<uint32_t> &ranks) {
    UGP_HIP_TRY(hipSetDevice(S->device));
    UGP_HIP_TRY(S->table.alloc((size_t)S->T->tp * 256));
    UGP_HIP_TRY(S->ranks.upload(ranks, S->stream));
    return UGP_OK;
}

int msk_restricted(MskState *S, uint64_t n, const uint32_t *leaves_bfs, uint8_t *entry_masked, uint32_t *roots_bfs, uint64_t roots_cap,
                   uint64_t *n_roots, uint64_t *n_masked) {
    if (int rc = msk_ready(S, "ugp_mask_restricted")) return rc;
    if (!n_roots || !n_masked || (roots_cap && !roots_bfs) || (S->T->m && !entry_masked)) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        std::vector<uint32_t> ranks;
        if (int rc = msk_ranks(S, "ugp_mask_restricted", n, leaves_bfs, &ranks)) return rc;
        int rc = msk_restricted_stage(S, ranks);
        if (!rc) rc = msk_restricted_passes(S, (uint32_t)n);
        if (rc) { (void)hipStreamSynchronize(S->stream); return rc; }
        hipStream_t st = S->stream;
        u64 nm = 0;
        UGP_HIP_TRY(hipMemcpyAsync(S->h_flag.data(), S->flag.p, S->T->n, hipMemcpyDeviceToHost, st));
        if (S->T->m) UGP_HIP_TRY(hipMemcpyAsync(entry_masked, S->emask.p, S->T->m, hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(&nm, S->nmasked.p, sizeof(nm), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));   // ranks is read until here
        uint64_t nr = 0;
        for (uint32_t v = 0; v < S->T->n; v++)
            if (S->h_flag[v] & kRoot) {
                if (nr < roots_cap) roots_bfs[nr] = (*S->dfs2bfs)[v];
                nr++;
            }
        *n_roots = nr;
        *n_masked = nm;
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

// ---- mutations ----------------------------------------------------------------------------------------------------------

namespace {
struct HostLines {   // every line, in file order, with its ranges in depth-first positions
    std::vector<uint32_t> tlo, thi, xoff, xlo, xhi;
};
}  // namespace

static int msk_check_lines(MskState *S, const char *who, uint64_t n_lines, const int32_t *pos, const uint8_t *par, const uint8_t *nuc,
                           const uint32_t *node_bfs, const uint64_t *excl_off, const uint32_t *excl_bfs, HostLines *H) {
    if (n_lines && (!pos || !par || !nuc || !node_bfs || !excl_off)) return set_error(UGP_ERR_INVALID, "null argument");
    if (n_lines >= (1ull << 31)) return set_error(UGP_ERR_INVALID, std::string(who) + ": more than 2^31 lines");
    const uint32_t N = S->T->n;
    for (uint64_t l = 0; l < n_lines; l++) {
        if (node_bfs[l] >= N) return set_error(UGP_ERR_INVALID, std::string(who) + ": the node of line " + std::to_string(l) + " is out of range");
        if (par[l] > 15 || nuc[l] > 15) return set_error(UGP_ERR_INVALID, std::string(who) + ": line " + std::to_string(l) + " has an allele above 15");
        if (excl_off[l + 1] < excl_off[l] || (l == 0 && excl_off[0] != 0) || excl_off[l + 1] >= (1ull << 31))
            return set_error(UGP_ERR_INVALID, std::string(who) + ": the exclusion offsets do not ascend from 0");
        if (excl_off[l + 1] > excl_off[l] && !excl_bfs) return set_error(UGP_ERR_INVALID, "null argument");
    }
    H->tlo.resize(n_lines);
    H->thi.resize(n_lines);
    H->xoff.assign(n_lines + 1, 0);
    for (uint64_t l = 0; l < n_lines; l++) {
        const uint32_t tv = S->T->bfs2dfs[node_bfs[l]];
        H->tlo[l] = tv;
        H->thi[l] = S->h_dend[tv];
        for (uint64_t x = excl_off[l]; x < excl_off[l + 1]; x++) {
            if (excl_bfs[x] >= N) continue;   // a name that is not in the tree has no effect
            const uint32_t xv = S->T->bfs2dfs[excl_bfs[x]];
            if (xv <= tv || xv >= S->h_dend[tv]) continue;   // only a strict descendant of the target stops the walk
            H->xlo.push_back(xv);
            H->xhi.push_back(S->h_dend[xv]);
        }
        H->xoff[l + 1] = (uint32_t)H->xlo.size();
    }
    return UGP_OK;
}

// Lines [l0, l1) to the device, sorted by position (a stable sort: file order within a position).
static int msk_stage_lines(MskState *S, const HostLines &H, uint64_t l0, uint64_t l1, const int32_t *pos, const uint8_t *par,
                           const uint8_t *nuc, LinesView *L) {
    const uint32_t n = (uint32_t)(l1 - l0);
    std::vector<uint32_t> ord(n);
    std::iota(ord.begin(), ord.end(), (uint32_t)l0);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return (uint32_t)pos[a] < (uint32_t)pos[b]; });
    std::vector<uint32_t> lpos(n), tlo(n), thi(n), xoff(n + 1, 0), xlo, xhi;
    std::vector<uint8_t> lpar(n), lnuc(n);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t l = ord[k];
        lpos[k] = (uint32_t)pos[l];
        lpar[k] = par[l];
        lnuc[k] = nuc[l];
        tlo[k] = H.tlo[l];
        thi[k] = H.thi[l];
        xlo.insert(xlo.end(), H.xlo.begin() + H.xoff[l], H.xlo.begin() + H.xoff[l + 1]);
        xhi.insert(xhi.end(), H.xhi.begin() + H.xoff[l], H.xhi.begin() + H.xoff[l + 1]);
        xoff[k + 1] = (uint32_t)xlo.size();
    }
    hipStream_t st = S->stream;
    UGP_HIP_TRY(S->lpos.upload(lpos, st));
    UGP_HIP_TRY(S->lpar.upload(lpar, st));
    UGP_HIP_TRY(S->lnuc.upload(lnuc, st));
    UGP_HIP_TRY(S->ltlo.upload(tlo, st));
    UGP_HIP_TRY(S->lthi.upload(thi, st));
    UGP_HIP_TRY(S->lidx.upload(ord, st));
    UGP_HIP_TRY(S->lxoff.upload(xoff, st));
    UGP_HIP_TRY(S->lxlo.upload(xlo, st));
    UGP_HIP_TRY(S->lxhi.upload(xhi, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));   // the vectors above are read until here
    *L = LinesView{n, S->lpos.p, S->lpar.p, S->lnuc.p, S->ltlo.p, S->lthi.p, S->lidx.p, S->lxoff.p, S->lxlo.p, S->lxhi.p};
    return UGP_OK;
}

static int msk_clear_mutations(MskState *S, uint64_t n_lines) {
    UGP_HIP_TRY(hipMemsetAsync(S->first.p, 0xff, std::max<size_t>(S->T->m, 1) * sizeof(uint32_t), S->stream));
    UGP_HIP_TRY(hipMemsetAsync(S->counts.p, 0, std::max<size_t>(n_lines, 1) * sizeof(u64), S->stream));
    return UGP_OK;
}

static int msk_launch_mutations(MskState *S, const LinesView &L, const uint8_t *skip) {
    const uint32_t M = (uint32_t)S->T->m;
    if (!M || !L.n) return UGP_OK;
    k_msk_mutations<<<blocks_for(M), kBlock, 0, S->stream>>>(S->T->view(), M, S->mpn.p, skip, L, S->first.p, S->counts.p);
    UGP_HIP_TRY(hipGetLastError());
    return UGP_OK;
}

int msk_mutations(MskState *S, uint64_t n_lines, const int32_t *pos, const uint8_t *par, const uint8_t *nuc, const uint32_t *node_bfs,
                  const uint64_t *excl_off, const uint32_t *excl_bfs, const uint8_t *skip, uint32_t *first_line, uint64_t *counts,
                  uint32_t chunk) {
    if (int rc = msk_ready(S, "ugp_mask_mutations")) return rc;
    const uint64_t M = S->T->m;
    if ((M && !first_line) || (n_lines && !counts)) return set_error(UGP_ERR_INVALID, "null argument");
    try {
        HostLines H;
        if (int rc = msk_check_lines(S, "ugp_mask_mutations", n_lines, pos, par, nuc, node_bfs, excl_off, excl_bfs, &H)) return rc;
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        UGP_HIP_TRY(S->counts.alloc(n_lines));
        if (skip && M) UGP_HIP_TRY(S->skip.upload(skip, M, st));
        int rc = msk_clear_mutations(S, n_lines);
        const uint64_t per = chunk ? chunk : kDefaultLines;
        for (uint64_t l0 = 0; l0 < n_lines && !rc; l0 += per) {
            LinesView L;
            rc = msk_stage_lines(S, H, l0, std::min(n_lines, l0 + per), pos, par, nuc, &L);
            if (!rc) rc = msk_launch_mutations(S, L, skip && M ? S->skip.p : nullptr);
            if (!rc) UGP_HIP_TRY(hipStreamSynchronize(st));   // the next batch replaces the staged lines
        }
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
        if (M) UGP_HIP_TRY(hipMemcpyAsync(first_line, S->first.p, M * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (n_lines) UGP_HIP_TRY(hipMemcpyAsync(counts, S->counts.p, n_lines * sizeof(u64), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));   // skip is read until here
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

// ---- the passes alone ---------------------------------------------------------------------------------------------------

int msk_time(MskState *S, uint64_t n, const uint32_t *leaves_bfs, uint64_t n_lines, const int32_t *pos, const uint8_t *par,
             const uint8_t *nuc, const uint32_t *node_bfs, const uint64_t *excl_off, const uint32_t *excl_bfs, uint32_t reps,
             double *restricted_ms, double *mutations_ms) {
    if (int rc = msk_ready(S, "ugp_mask_time")) return rc;
    if (!reps || !restricted_ms || !mutations_ms) return set_error(UGP_ERR_INVALID, "null argument");
    *restricted_ms = *mutations_ms = 0;
    try {
        if (n) {
            std::vector<uint32_t> ranks;
            if (int rc = msk_ranks(S, "ugp_mask_time", n, leaves_bfs, &ranks)) return rc;
            if (int rc = msk_restricted_stage(S, ranks)) return rc;
            UGP_HIP_TRY(hipStreamSynchronize(S->stream));   // ranks is read until here
            if (int rc = timed(S->stream, "ugp_mask_time", reps, restricted_ms, [&] { return msk_restricted_passes(S, (uint32_t)n); })) return rc;
        }
        if (n_lines) {
            if (n_lines > kDefaultLines) return set_error(UGP_ERR_INVALID, "ugp_mask_time: more lines than one batch takes");
            HostLines H;
            if (int rc = msk_check_lines(S, "ugp_mask_time", n_lines, pos, par, nuc, node_bfs, excl_off, excl_bfs, &H)) return rc;
            UGP_HIP_TRY(hipSetDevice(S->device));
            UGP_HIP_TRY(S->counts.alloc(n_lines));
            LinesView L;
            if (int rc = msk_stage_lines(S, H, 0, n_lines, pos, par, nuc, &L)) return rc;
            if (int rc = timed(S->stream, "ugp_mask_time", reps, mutations_ms, [&] {
                    const int c = msk_clear_mutations(S, n_lines);
                    return c ? c : msk_launch_mutations(S, L, nullptr);
                })) return rc;
        }
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

}  // namespace ugp
