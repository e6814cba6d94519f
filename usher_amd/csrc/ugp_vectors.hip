// ugp_vectors.hip -- node_excess_mutations and node_imputed_mutations of mapper2_body (usher_mapper.cpp:167-504 with compute_vecs)
// for (sample, node) pairs, in closed form.  One wave per pair (sample s, node j); the same code counts and fills.
//
// The ancestral state g(p) of j at position p is the allele of the NEAREST OWNER: the last owner of p at or before j in depth-first
// order (a binary search over the owners' nodes), then up the owners above (mlink) until one's subtree holds j -- and one more step
// when that owner is j's own entry and loop 1 did not keep it.
//   part 1   lanes take j's own entries, 64 at a time.  Loop 1's merge pointer in front of an entry is the largest pointer any entry
//            before it left behind, and what an entry leaves behind does not depend on where the pointer stood (merge_probe): a
//            prefix maximum over the lanes.  A row the pointer has passed is not seen (the entry is kept only if it is a
//            reference allele); own entries in position order never pass one.
//   part 2   lanes take the sample's rows, 64 at a time: g(p) against the row.
//   part 3   the nodes of j's root path 64 at a time (the parent chain itself is followed by the whole wave, one load a node), a
//            lane per node and its entries in step: an entry that owns its position, is off its reference, has no row in s and is
//            the nearest owner of its position for j is a back-mutation.  They go to a second buffer in the order found;
//            k_vec_order ranks each among its pair's (positions are distinct) and writes it to its place.
//   k_vec_count  the counts and the info of every pair      k_vec_scan   their prefix sums, 64-bit
//   k_vec_fill   the lists, part 3 unordered                k_vec_order  part 3 by position, one lane per entry
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_translate.hpp"
#include "ugp_vectors.hpp"

namespace ugp {
namespace {

constexpr uint32_t kDefaultPairs = 1u << 18;   // pairs per launch window
constexpr uint32_t kScanTile = 8;              // values a thread of the prefix sum takes at a time
typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "offsets are 64-bit");
static_assert(sizeof(ugp_vec_entry) == 8 && sizeof(ugp_vec_info) == 20, "the records of usher_amd.h");

struct VecView {
    DfsView t;
    const uint32_t *onode;     // per slot of pent the owner's node
    const uint8_t *spar;       // per depth-first entry the parent allele as stored
    const u64 *ent_off;        // the samples' rows
    const int32_t *qpos;
    const uint8_t *qref, *qnuc, *qmis;
};

struct Rows {   // one sample's
    const int32_t *pos;
    const uint8_t *ref, *nuc, *mis;
    uint32_t n;
};

struct Branch {   // what loop 1 leaves for the lookups: j's entries, the first masked one (or their end), no row was ever passed
    uint32_t e0, stop;
    bool allvis;
};

// First row at or behind position p.
__device__ __forceinline__ uint32_t row_lb(const Rows &r, int32_t p) {
    uint32_t lo = 0, hi = r.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (r.pos[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Loop 1 (usher_mapper.cpp:204-241) for an entry (p, nuc) whose row, if any, the merge pointer has not passed: the row, and where
// the pointer stands afterwards (`after`).  From a pointer beyond the row the loop leaves at once and the pointer stays.
struct Probe {
    uint32_t lb, after;
    bool here, match, miss;
};
__device__ __forceinline__ Probe merge_probe(const Rows &r, int32_t p, uint32_t nuc) {
    Probe o;
    o.lb = row_lb(r, p);
    o.here = o.lb < r.n && r.pos[o.lb] == p;
    o.miss = o.here && r.mis[o.lb] != 0;
    o.match = o.here && !o.miss && ((uint32_t)r.nuc[o.lb] & nuc) != 0;
    if (r.n == 0) o.after = 0;
    else if (o.lb == r.n) o.after = r.n - 1;                      // ran off the end: the last row visited
    else if (o.here && !o.match) o.after = min(o.lb + 1, r.n - 1);   // a missing row or another allele: one row further
    else o.after = o.lb;
    return o;
}

// Did loop 1 keep j's own entry e (non-masked)?  `here`: s has a row at its position, row lb.
__device__ __forceinline__ bool own_kept(const DfsView &t, const Rows &r, const Branch &b, uint32_t e, bool here, uint32_t lb) {
    if (e >= b.stop) return false;
    const uint32_t bits = t.mbits[e];
    if (here && !b.allvis) {   // some row was passed: the pointer in front of e, entry by entry
        uint32_t s = 0;
        for (uint32_t x = b.e0; x < e; x++) s = max(s, merge_probe(r, t.mpos[x], b_nuc(t.mbits[x])).after);
        here = lb >= s;
    }
    if (here) return !r.mis[lb] && ((uint32_t)r.nuc[lb] & b_nuc(bits)) != 0;
    return b_nuc(bits) == b_ref(bits);
}

// The entry whose allele is g(p) for node j, or kNil.
__device__ __forceinline__ uint32_t nearest_owner(const VecView &v, const Rows &r, const Branch &b, uint32_t j, int32_t p, bool here, uint32_t lb) {
    const DfsView &t = v.t;
    if ((uint32_t)p >= t.tp) return kNil;   // p < 0 too
    const uint32_t lo = t.poff[p], x = lower_bound_u32(v.onode, lo, t.poff[p + 1], j + 1);
    uint32_t cur = x > lo ? t.pent[x - 1] : kNil;
    while (cur != kNil && j >= t.dend[t.mnode[cur]]) cur = t.mlink[cur];
    if (cur != kNil && j != 0 && t.mnode[cur] == j && !own_kept(t, r, b, cur, here, lb)) cur = t.mlink[cur];
    return cur;
}

__device__ __forceinline__ void put(ugp_vec_entry *dst, uint32_t room, uint32_t at, int32_t p, uint32_t ref, uint32_t par, uint32_t nuc) {
    if (at >= room) return;
    ugp_vec_entry o;
    o.pos = p; o.ref = (uint8_t)ref; o.par = (uint8_t)par; o.nuc = (uint8_t)nuc; o.pad = 0;
    dst[at] = o;
}

// One wave, one pair.  Fill = false: *info and *n3 (the entries of part 3).  Fill = true: parts 1 and 2 to ex[0 ..), part 3 behind
// them in tmp in the order found, the imputed list to im; nothing past ex_room / im_room entries.
template <bool Fill>
__device__ __forceinline__ void vec_pair(const VecView &v, uint32_t s, uint32_t j, uint32_t lane, ugp_vec_info *info, uint32_t *n3_out,
                                         ugp_vec_entry *ex, ugp_vec_entry *tmp, uint32_t ex_room, ugp_vec_entry *im, uint32_t im_room) {
    const DfsView &t = v.t;
    const u64 r0 = v.ent_off[s];
    const Rows r{v.qpos + r0, v.qref + r0, v.qnuc + r0, v.qmis + r0, (uint32_t)(v.ent_off[s + 1] - r0)};
    const uint32_t e0 = t.moff[j], e1 = t.moff[j + 1];
    const u64 lt = (1ull << lane) - 1ull;

    // refused: a non-masked entry of j that does not own its position
    bool dup = false;
    for (uint32_t e = e0 + lane; e < e1; e += 64) dup = dup || (t.mpos[e] >= 0 && !(t.mflag[e] & kOwner));
    if (__ballot(dup)) {
        if (!Fill && lane == 0) {
            ugp_vec_info o = {};
            o.refused = 1;
            *info = o;
            *n3_out = 0;
        }
        return;
    }

    // part 1
    Branch br{e0, e1, true};
    uint32_t start = 0, nm = 0, common = 0, n1 = 0;
    bool hu = false;
    if (j != 0) {
        for (uint32_t base = e0; base < e1; base += 64) {
            const uint32_t e = base + lane;
            const bool live = e < e1;
            const int32_t p = live ? t.mpos[e] : 0;
            const uint32_t bits = live ? t.mbits[e] : 0u, nuc = b_nuc(bits), ref = b_ref(bits);
            const u64 mb = __ballot(live && p < 0);
            const uint32_t first_masked = mb ? (uint32_t)__ffsll((long long)mb) - 1u : 64u;
            const bool act = live && lane < first_masked;   // looked at and not masked
            Probe pr = {0, 0, false, false, false};
            if (act) pr = merge_probe(r, p, nuc);
            uint32_t incl = act ? pr.after : 0u;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d, 64);
                if ((int)lane >= d) incl = max(incl, o);
            }
            uint32_t before = __shfl_up(incl, 1, 64);
            before = max(start, lane ? before : 0u);
            const bool passed = act && pr.here && pr.lb < before;
            const bool seen = act && pr.here && !passed;
            const bool kept = act && (seen ? pr.match : nuc == ref);
            const bool com = kept || (seen && pr.miss);
            if (__ballot(passed)) br.allvis = false;
            if (__ballot(act && !com) || mb) hu = true;
            nm += (uint32_t)__popcll(__ballot(live && lane <= first_masked));
            common += (uint32_t)__popcll(__ballot(com));
            const u64 kb = __ballot(kept);
            if (Fill && kept) put(ex, ex_room, n1 + (uint32_t)__popcll(kb & lt), p, ref, v.spar[e], nuc);
            n1 += (uint32_t)__popcll(kb);
            start = max(start, (uint32_t)__shfl(incl, 63, 64));
            if (mb) { br.stop = base + first_masked; break; }
        }
    }

    // part 2 and the imputed list
    uint32_t n2 = 0, nim = 0;
    for (uint32_t base = 0; base < r.n; base += 64) {
        const uint32_t k = base + lane;
        bool isex = false, isim = false;
        int32_t p = 0;
        uint32_t rr = 0, anc = 0, mut = 0, imnuc = 0;
        if (k < r.n && !r.mis[k]) {
            p = r.pos[k];
            rr = r.ref[k];
            const uint32_t a = r.nuc[k];
            const uint32_t cur = nearest_owner(v, r, br, j, p, true, k);
            anc = cur != kNil ? b_nuc(t.mbits[cur]) : rr;
            const bool found = cur != kNil && (a & anc) != 0, has_ref = (a & rr) != 0;
            isim = (a & (a - 1u)) != 0;
            if (found) imnuc = anc;                            // :322-335
            else if (cur == kNil && has_ref) imnuc = rr;       // :341-351
            else {                                             // :356-387
                mut = has_ref ? rr : lowbit4(a);
                imnuc = mut;
                isex = mut != anc;
            }
        }
        const u64 xb = __ballot(isex), ib = __ballot(isim);
        if (Fill && isex) put(ex, ex_room, n1 + n2 + (uint32_t)__popcll(xb & lt), p, rr, anc, mut);
        if (Fill && isim) put(im, im_room, nim + (uint32_t)__popcll(ib & lt), p, rr, anc, imnuc);
        n2 += (uint32_t)__popcll(xb);
        nim += (uint32_t)__popcll(ib);
    }

    // part 3
    uint32_t n3 = 0;
    if (j == 0) {   // the root's own entries, masked ones included, in stored order
        for (uint32_t base = e0; base < e1; base += 64) {
            const uint32_t e = base + lane;
            bool flag = false;
            int32_t p = 0;
            uint32_t nuc = 0, ref = 0;
            if (e < e1) {
                p = t.mpos[e];
                const uint32_t bits = t.mbits[e];
                nuc = b_nuc(bits); ref = b_ref(bits);
                if (nuc != ref) {
                    if (p < 0) flag = true;
                    else {
                        const uint32_t lb = row_lb(r, p);
                        flag = !(lb < r.n && r.pos[lb] == p);
                    }
                }
            }
            const u64 fb = __ballot(flag);
            if (Fill && flag) put(tmp, ex_room, n1 + n2 + n3 + (uint32_t)__popcll(fb & lt), p, ref, nuc, ref);
            n3 += (uint32_t)__popcll(fb);
        }
    } else {
        uint32_t vtx = j;
        while (vtx != kNil) {
            uint32_t mine = kNil;
            for (uint32_t i = 0; i < 64 && vtx != kNil; i++) {
                if (lane == i) mine = vtx;
                vtx = t.dpar[vtx];
            }
            uint32_t a = 0, b = 0;
            if (mine != kNil) { a = t.moff[mine]; b = t.moff[mine + 1]; }
            for (uint32_t i = 0; __ballot(a + i < b); i++) {
                const uint32_t e = a + i;
                bool flag = false;
                int32_t p = 0;
                uint32_t nuc = 0, ref = 0;
                if (e < b) {
                    p = t.mpos[e];
                    const uint32_t bits = t.mbits[e];
                    nuc = b_nuc(bits); ref = b_ref(bits);
                    if (p >= 0 && nuc != ref && (t.mflag[e] & kOwner)) {
                        const uint32_t lb = row_lb(r, p);
                        if (!(lb < r.n && r.pos[lb] == p)) flag = nearest_owner(v, r, br, j, p, false, 0) == e;
                    }
                }
                const u64 fb = __ballot(flag);
                if (Fill && flag) put(tmp, ex_room, n1 + n2 + n3 + (uint32_t)__popcll(fb & lt), p, ref, nuc, ref);
                n3 += (uint32_t)__popcll(fb);
            }
        }
    }

    if (!Fill && lane == 0) {
        const bool lf = t.leaf[j] != 0;
        ugp_vec_info o = {};
        o.n_excess = n1 + n2 + n3;
        o.n_imputed = nim;
        o.n_branch = n1;
        o.set_difference = (int32_t)(n2 + n3);
        o.has_unique = hu ? 1 : 0;
        o.eligible = (j == 0 || (hu && !lf && common > 0 && nm != common) || (lf && common > 0) || (!hu && !lf && nm == common)) ? 1 : 0;
        *info = o;
        *n3_out = n3;
    }
}

__global__ void __launch_bounds__(kBlock) k_vec_count(VecView v, const uint32_t *ps, const uint32_t *pn, uint32_t np, ugp_vec_info *info,
                                                      uint32_t *n3) {
    const uint32_t i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (i >= np) return;
    vec_pair<false>(v, ps[i], pn[i], threadIdx.x & 63u, info + i, n3 + i, nullptr, nullptr, 0, nullptr, 0);
}

// Block 0: off_ex[i] = the excess entries of the pairs before i; block 1: off_im, the imputed ones.  64-bit, off[np] = all.
__global__ void __launch_bounds__(kBlock) k_vec_scan(const ugp_vec_info *info, uint32_t np, u64 *off_ex, u64 *off_im) {
    __shared__ u64 sh[kBlock / 64];
    const bool imp = blockIdx.x != 0;
    u64 *off = imp ? off_im : off_ex;
    u64 carry = 0;
    for (uint64_t t0 = 0; t0 < np; t0 += (uint64_t)kBlock * kScanTile) {
        const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kScanTile;
        u64 sum = 0;
        for (uint32_t k = 0; k < kScanTile; k++)
            if (i0 + k < np) sum += imp ? info[i0 + k].n_imputed : info[i0 + k].n_excess;
        u64 tot;
        u64 run = carry + block_incl_scan(sum, sh, &tot) - sum;
        for (uint32_t k = 0; k < kScanTile; k++)
            if (i0 + k < np) { off[i0 + k] = run; run += imp ? info[i0 + k].n_imputed : info[i0 + k].n_excess; }
        carry += tot;
    }
    if (threadIdx.x == 0) off[np] = carry;
}

__global__ void __launch_bounds__(kBlock) k_vec_fill(VecView v, const uint32_t *ps, const uint32_t *pn, uint32_t np, const u64 *off_ex,
                                                     const u64 *off_im, ugp_vec_entry *ex, ugp_vec_entry *tmp, ugp_vec_entry *im) {
    const uint32_t i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (i >= np) return;
    const u64 xo = off_ex[i], io = off_im[i];
    const uint32_t xr = (uint32_t)(off_ex[i + 1] - xo), ir = (uint32_t)(off_im[i + 1] - io);
    if (!xr && !ir) return;
    vec_pair<true>(v, ps[i], pn[i], threadIdx.x & 63u, nullptr, nullptr, ex + xo, tmp + xo, xr, im + io, ir);
}

// One lane per excess entry of the window: an entry of part 3 goes from tmp to its rank among its pair's -- masked entries (the
// root's) first, in the order found, then by position.
__global__ void __launch_bounds__(kBlock) k_vec_order(const ugp_vec_info *info, const uint32_t *n3, const u64 *off_ex, uint32_t np, u64 total,
                                                      const ugp_vec_entry *tmp, ugp_vec_entry *ex) {
    const u64 g = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total) return;
    uint32_t lo = 0, hi = np;   // the last pair that starts at or before g
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off_ex[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t cnt = n3[lo], first = info[lo].n_excess - cnt, at = (uint32_t)(g - off_ex[lo]);
    if (at < first || at - first >= cnt) return;
    const ugp_vec_entry *part = tmp + off_ex[lo] + first;
    const uint32_t me = at - first;
    const ugp_vec_entry mine = part[me];
    uint32_t rank = 0;
    for (uint32_t k = 0; k < cnt; k++) {
        const int32_t p = part[k].pos;
        const bool less = mine.pos < 0 ? (p < 0 && k < me) : (p < mine.pos);
        rank += less ? 1u : 0u;
    }
    ex[off_ex[lo] + first + rank] = mine;   // rank < cnt: at most cnt - 1 others are less
}

}  // namespace

struct VecState : QueryBase {
    DBuf<uint8_t> spar;
    // per call
    DBuf<u64> ent_off, off_ex, off_im;
    DBuf<uint32_t> ps, pn, n3;
    DBuf<ugp_vec_info> info;
    DBuf<ugp_vec_entry> ex, tmp, im;
};

void vec_free(VecState *s) { query_free(s); }

int vec_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, VecState **out) {
    std::vector<uint8_t> spar;
    return query_attach(
        "ugp_vectors_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out,
        [&](const DfsTables &T) {
            if (T.m && !tree->mut_par)
                return set_error(UGP_ERR_INVALID, "ugp_vectors_attach needs mut_par: the node's own entries report the parent allele as stored");
            spar.reserve(T.m);
            for (uint32_t b : dfs2bfs)
                for (uint64_t k = tree->mut_off[b]; k < tree->mut_off[b + 1]; k++) {
                    if (tree->mut_nuc[k] > 15 || tree->mut_ref[k] > 15 || tree->mut_par[k] > 15)
                        return set_error(UGP_ERR_UNSUPPORTED, "ugp_vectors_attach: an allele of entry " + std::to_string(k) + " is not a 4-bit code");
                    spar.push_back(tree->mut_par[k]);
                }
            return (int)UGP_OK;
        },
        [&](VecState *S) {
            hipError_t err = S->spar.upload(spar, S->stream);
            if (err == hipSuccess) err = hipStreamSynchronize(S->stream);   // spar is read until here
            if (int rc = hip_rc("ugp_vectors_attach", err)) return rc;
            return tr_owner_nodes(*tables, S->stream);
        });
}

int vec_check(VecState *S, const char *who, const ugp_queries *q, uint64_t n_pairs, const uint32_t *sample, const uint32_t *node) {
    if (int rc = query_ready(S, who, "vectors")) return rc;
    if (!q || (n_pairs && !node)) return set_error(UGP_ERR_INVALID, "null argument");
    if (n_pairs >= (1ull << 32)) return set_error(UGP_ERR_INVALID, std::string(who) + ": more than 2^32 pairs");
    const uint32_t N = S->T->n;
    for (uint64_t i = 0; i < n_pairs; i++) {
        if ((sample ? sample[i] : i) >= q->n_queries) return set_error(UGP_ERR_INVALID, std::string(who) + ": the sample of pair " + std::to_string(i) + " is out of range");
        if (node[i] >= N) return set_error(UGP_ERR_INVALID, std::string(who) + ": the node of pair " + std::to_string(i) + " is out of range");
    }
    return UGP_OK;
}

int vec_run(VecState *S, const ugp_queries *q, const int32_t *d_pos, const uint8_t *d_ref, const uint8_t *d_nuc, const uint8_t *d_missing,
            uint64_t n_pairs, const uint32_t *sample, const uint32_t *node, ugp_vec_info *info, uint64_t *ex_off, ugp_vec_entry *excess,
            uint64_t ex_cap, uint64_t *n_excess, uint64_t *im_off, ugp_vec_entry *imputed, uint64_t im_cap, uint64_t *n_imputed,
            uint32_t chunk_pairs, double *kernel_ms) {
    const bool timing = kernel_ms != nullptr;
    if (!timing && (!ex_off || !im_off || !n_excess || !n_imputed || (n_pairs && !info) || (ex_cap && !excess) || (im_cap && !imputed)))
        return set_error(UGP_ERR_INVALID, "null argument");
    if (timing) kernel_ms[0] = kernel_ms[1] = 0;
    uint64_t base_ex = 0, base_im = 0;
    try {
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        const uint64_t chunk = chunk_pairs ? chunk_pairs : kDefaultPairs;
        const std::vector<uint32_t> &b2d = S->T->bfs2dfs;
        EventPair ev(st);
        if (timing) UGP_HIP_TRY(ev.create());
        if (n_pairs) {
            const uint64_t most = std::min<uint64_t>(chunk, n_pairs);
            UGP_HIP_TRY(S->ent_off.upload((const u64 *)q->ent_off, q->n_queries + 1, st));   // read until the first synchronisation below
            UGP_HIP_TRY(S->ps.alloc(most)); UGP_HIP_TRY(S->pn.alloc(most)); UGP_HIP_TRY(S->n3.alloc(most)); UGP_HIP_TRY(S->info.alloc(most));
            UGP_HIP_TRY(S->off_ex.alloc(most + 1)); UGP_HIP_TRY(S->off_im.alloc(most + 1));
        }
        const VecView v{S->T->view(), S->T->onode.p, S->spar.p, S->ent_off.p, d_pos, d_ref, d_nuc, d_missing};
        std::vector<uint32_t> hs, hn;
        std::vector<u64> hox, hoi;
        for (uint64_t c0 = 0; c0 < n_pairs; c0 += chunk) {
            const uint32_t nc = (uint32_t)std::min<uint64_t>(chunk, n_pairs - c0);
            const uint32_t grid = (nc + kBlock / 64 - 1) / (kBlock / 64);
            hs.resize(nc); hn.resize(nc);
            for (uint32_t i = 0; i < nc; i++) { hs[i] = sample ? sample[c0 + i] : (uint32_t)(c0 + i); hn[i] = b2d[node[c0 + i]]; }
            UGP_HIP_TRY(S->ps.upload(hs, st));
            UGP_HIP_TRY(S->pn.upload(hn, st));
            if (timing) UGP_HIP_TRY(ev.start());
            k_vec_count<<<grid, kBlock, 0, st>>>(v, S->ps.p, S->pn.p, nc, S->info.p, S->n3.p);
            k_vec_scan<<<2, kBlock, 0, st>>>(S->info.p, nc, S->off_ex.p, S->off_im.p);
            UGP_HIP_TRY(hipGetLastError());
            if (timing) UGP_HIP_TRY(ev.lap(&kernel_ms[0]));
            const size_t firstoff = timing ? nc : 0;   // the bench hook needs the totals only
            hox.resize((size_t)nc + 1 - firstoff); hoi.resize(hox.size());
            if (!timing) UGP_HIP_TRY(hipMemcpyAsync(info + c0, S->info.p, nc * sizeof(ugp_vec_info), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(hox.data(), S->off_ex.p + firstoff, hox.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(hoi.data(), S->off_im.p + firstoff, hoi.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipStreamSynchronize(st));
            const uint64_t tx = hox.back(), ti = hoi.back();
            if (!timing) for (uint32_t i = 0; i < nc; i++) { ex_off[c0 + i] = base_ex + hox[i]; im_off[c0 + i] = base_im + hoi[i]; }
            // the window's lists; only what lies below the caps leaves the device
            const uint64_t take_ex = timing || base_ex >= ex_cap ? 0 : std::min<uint64_t>(tx, ex_cap - base_ex);
            const uint64_t take_im = timing || base_im >= im_cap ? 0 : std::min<uint64_t>(ti, im_cap - base_im);
            if ((tx || ti) && (timing || take_ex || take_im)) {
                UGP_HIP_TRY(S->ex.alloc(tx)); UGP_HIP_TRY(S->tmp.alloc(tx)); UGP_HIP_TRY(S->im.alloc(ti));
                if (timing) UGP_HIP_TRY(ev.start());
                k_vec_fill<<<grid, kBlock, 0, st>>>(v, S->ps.p, S->pn.p, nc, S->off_ex.p, S->off_im.p, S->ex.p, S->tmp.p, S->im.p);
                if (tx) k_vec_order<<<blocks_for(tx), kBlock, 0, st>>>(S->info.p, S->n3.p, S->off_ex.p, nc, tx, S->tmp.p, S->ex.p);
                UGP_HIP_TRY(hipGetLastError());
                if (timing) UGP_HIP_TRY(ev.lap(&kernel_ms[1]));
                if (take_ex) UGP_HIP_TRY(hipMemcpyAsync(excess + base_ex, S->ex.p, take_ex * sizeof(ugp_vec_entry), hipMemcpyDeviceToHost, st));
                if (take_im) UGP_HIP_TRY(hipMemcpyAsync(imputed + base_im, S->im.p, take_im * sizeof(ugp_vec_entry), hipMemcpyDeviceToHost, st));
                UGP_HIP_TRY(hipStreamSynchronize(st));
            }
            base_ex += tx;
            base_im += ti;
        }
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    if (!timing) {
        ex_off[n_pairs] = base_ex; im_off[n_pairs] = base_im;
        *n_excess = base_ex; *n_imputed = base_im;
    }
    return UGP_OK;
}

}  // namespace ugp
