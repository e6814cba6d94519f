// ugp_translate.hip -- matUtils summary --translate (matUtils/translate.cpp: translate_main, do_mutations in TSV mode) on the device.
//
// The reference walks the tree once with a mutable codon per (gene, codon number): entering a node it writes every mutation's parent
// allele and then its allele into the codons of the position, leaving a branch it writes the parent alleles back.  When every stored
// parent allele equals what the walk finds there (the CONSISTENT case, usher_amd.h), the letters of a codon before a node are, slot
// by slot, the allele of the nearest strict ancestor with a mutation at the slot's position, else the slot's initial letter: no walk.
// That lookup runs over the per-position owner lists of the depth-first tables (ugp_dense.hpp): poff / pent list the owners of a
// position in depth-first order of their node, mlink names the owner above, mbits carries its allele.
//   k_tr_onode                     attach: per owner of the lists its node, so that the search reads one array;
//   (host, per codon table)        the WORK-ITEMS: every owner at a coding position paired with every codon of the position, the
//                                  owners of a node ascending by position, the codons by index -- the order do_mutations touches them;
//   k_tr_items                     a window of the items.  The first item of an owner checks its stored parent allele against the
//                                  state before (the owner above, else the initial letter of every slot that holds the position).
//                                  Every item finds the node's owners in its codon's three slots by a scan of the node's row; the
//                                  item at the lowest of them owns the record: a mutated slot takes the state before from the owner
//                                  above its entry, an unmutated one from a binary search among the position's owners for the last
//                                  one in front of the node and the climb over the owners above until one contains the node;
//   (scan_flags, ugp_scan.hpp)     the records in front of every item of the window;
//   k_tr_emit                      the records of the window, compacted in order behind those of the windows before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_translate.hpp"

namespace ugp {
namespace {

constexpr uint64_t kDefaultItems = 1ull << 22;   // work-items per launch window
constexpr int32_t kMaxSlotPos = 1 << 28;         // as the bound of the tables on mutation positions
static_assert(sizeof(ugp_tr_record) == 28 && offsetof(ugp_tr_record, node) == 0, "k_tr_emit copies the record as seven words");

__device__ __forceinline__ uint8_t nuc_letter(uint32_t c) { return (uint8_t) "NACMGRSVTWYHKDBN"[c & 15u]; }   // get_nuc

__global__ void k_tr_onode(uint32_t npo, const uint32_t *pent, const uint32_t *mnode, uint32_t *onode) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < npo) onode[x] = mnode[pent[x]];
}

struct TrView {   // what the item kernel reads beside the depth-first tables
    const uint32_t *ient, *icod, *onode;   // per item its owner (depth-first entry) and codon << 2 | slot; per listed owner its node
    const int32_t *spos;                   // [3 n_codons]
    const uint8_t *sinit, *mpar;           // [3 n_codons]; the caller's mut_par (by CSR index)
    uint32_t nitems;
};

// The allele (0: none) in force at position p above node v, which has no owner there: the last owner of p in front of v in
// depth-first order, then up the owners above until one contains v.
__device__ __forceinline__ uint32_t allele_above(const DfsView &t, const uint32_t *onode, uint32_t v, int32_t p) {
    if ((uint32_t)p >= t.tp) return 0;
    const uint32_t lo = t.poff[p], x = lower_bound_u32(onode, lo, t.poff[p + 1], v);
    uint32_t cur = x > lo ? t.pent[x - 1] : kNil;
    while (cur != kNil && v >= t.dend[t.mnode[cur]]) cur = t.mlink[cur];
    return cur == kNil ? 0u : b_nuc(t.mbits[cur]);
}

// Items [i0, i0 + cnt): flag[j] = 1 and rec[j] (its node as a depth-first position) when item i0 + j owns a record.
// counters[0] += the inconsistent owners of the window, counters[1] = min(their depth-first entry index).
__global__ void __launch_bounds__(kBlock) k_tr_items(DfsView t, TrView s, uint32_t i0, uint32_t cnt, uint8_t *flag, ugp_tr_record *rec,
                                                     uint32_t *counters) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    uint32_t e = 0;
    if (j < cnt) {
        const uint32_t i = i0 + j, ic = s.icod[i], c = ic >> 2;
        e = s.ient[i];
        const uint32_t v = t.mnode[e], anc = b_anc(t.mbits[e]);
        const int32_t p = t.mpos[e];
        if (i == 0 || s.ient[i - 1] != e) {   // the owner's first item: is its stored parent allele the state before it?
            const uint8_t par = nuc_letter(s.mpar[t.morig[e]]);
            if (anc) bad = par != nuc_letter(anc);
            else
                for (uint32_t k = i; k < s.nitems && s.ient[k] == e && !bad; k++) {
                    const uint32_t ck = s.icod[k];
                    bad = par != s.sinit[3 * (ck >> 2) + (ck & 3u)];
                }
        }
        const int32_t p0 = s.spos[3 * c], p1 = s.spos[3 * c + 1], p2 = s.spos[3 * c + 2];
        uint32_t e0 = kNil, e1 = kNil, e2 = kNil;
        for (uint32_t k = t.moff[v], end = t.moff[v + 1]; k < end; k++) {
            if (!(t.mflag[k] & kOwner)) continue;
            const int32_t q = t.mpos[k];
            if (q == p0) e0 = k;
            if (q == p1) e1 = k;
            if (q == p2) e2 = k;
        }
        const bool lowest = !((e0 != kNil && p0 < p) || (e1 != kNil && p1 < p) || (e2 != kNil && p2 < p));
        flag[j] = lowest ? 1 : 0;
        if (lowest) {
            ugp_tr_record o;
            o.node = v;
            o.codon = c;
            o.pad[0] = o.pad[1] = 0;
            const uint32_t es[3] = {e0, e1, e2};
            const int32_t ps[3] = {p0, p1, p2};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint32_t up = es[k] != kNil ? b_anc(t.mbits[es[k]]) : allele_above(t, s.onode, v, ps[k]);
                const uint8_t before = up ? nuc_letter(up) : s.sinit[3 * c + k];
                o.before[k] = before;
                o.after[k] = es[k] != kNil ? nuc_letter(b_nuc(t.mbits[es[k]])) : before;
                o.ent[k] = es[k] != kNil ? t.morig[es[k]] : kNil;
            }
            rec[j] = o;
        }
    }
    // one atomic per wave that found any
    const unsigned long long votes = __ballot(bad);
    if (bad) {
        if ((uint32_t)__ffsll((long long)votes) - 1u == (threadIdx.x & 63u)) atomicAdd(&counters[0], (uint32_t)__popcll(votes));
        atomicMin(&counters[1], e);
    }
}

// The flagged records of a window go behind the `base` records before them, the node as a breadth-first index, while below cap.
__global__ void k_tr_emit(uint32_t cnt, const uint8_t *flag, const uint32_t *off, const ugp_tr_record *rec, const uint32_t *d2b, uint64_t base,
                          uint64_t cap, ugp_tr_record *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt || !flag[j]) return;
    const uint64_t o = base + off[j];
    if (o >= cap) return;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(rec + j);   // seven words, the node first
    uint32_t *dst = reinterpret_cast<uint32_t *>(out + o);
    dst[0] = d2b[src[0]];
#pragma unroll
    for (int k = 1; k < (int)(sizeof(ugp_tr_record) / sizeof(uint32_t)); k++) dst[k] = src[k];
}

}  // namespace

struct TrState : QueryBase {
    std::vector<uint32_t> h_moff, h_morig;        // host copies of the tables the item list is made from
    std::vector<int32_t> h_mpos;
    std::vector<uint8_t> h_mflag;
    DBuf<uint8_t> mpar;
    DBuf<uint32_t> d2b;
    // the codon table and its items
    bool have_codons = false;
    uint64_t nitems = 0, nnodes = 0, ndup = 0;
    uint32_t first_dup = kNil;                    // depth-first position
    DBuf<int32_t> spos;
    DBuf<uint8_t> sinit;
    DBuf<uint32_t> ient, icod;
    // per call
    DBuf<uint8_t> flag;
    DBuf<uint32_t> seg, off, counters;
    DBuf<ugp_tr_record> rec, rout;
    TrView view() const { return TrView{ient.p, icod.p, T->onode.p, spos.p, sinit.p, mpar.p, (uint32_t)nitems}; }
};

void tr_free(TrState *s) { query_free(s); }

int tr_owner_nodes(DfsTables *T, hipStream_t st) {
    if (!T) return set_error(UGP_ERR_INVALID, "null argument");
    if (T->have_onode) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(T->device));
    uint32_t npo = 0;
    if (T->tp) UGP_HIP_TRY(hipMemcpyAsync(&npo, T->poff.p + T->tp, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));
    UGP_HIP_TRY(T->onode.alloc(npo));
    if (npo) {
        k_tr_onode<<<blocks_for(npo), kBlock, 0, st>>>(npo, T->pent.p, T->mnode.p, T->onode.p);
        UGP_HIP_TRY(hipGetLastError());
    }
    UGP_HIP_TRY(hipStreamSynchronize(st));
    T->have_onode = true;
    return UGP_OK;
}

static int tr_build(TrState *S, DfsTables *tables, const ugp_tree_desc *tree) {
    const DfsTables &T = *S->T;
    const uint32_t N = T.n;
    const uint64_t M = T.m;
    hipStream_t st = S->stream;
    S->h_moff.resize((size_t)N + 1); S->h_morig.resize(M); S->h_mpos.resize(M); S->h_mflag.resize(M);
    UGP_HIP_TRY(hipMemcpyAsync(S->h_moff.data(), T.moff.p, ((size_t)N + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (M) {
        UGP_HIP_TRY(hipMemcpyAsync(S->h_morig.data(), T.morig.p, M * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(S->h_mpos.data(), T.mpos.p, M * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(S->h_mflag.data(), T.mflag.p, M, hipMemcpyDeviceToHost, st));
    }
    UGP_HIP_TRY(S->mpar.upload(tree->mut_par, M, st));
    UGP_HIP_TRY(S->d2b.upload(S->dfs2bfs->data(), N, st));
    UGP_HIP_TRY(hipStreamSynchronize(st));
    return tr_owner_nodes(tables, st);
}

int tr_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, TrState **out) {
    return query_attach(
        "ugp_translate_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out,
        [&](const DfsTables &T) { return coded_alleles(tree, T, "translate needs mut_par: a node's codons start from the parent allele as stored"); },
        [&](TrState *S) { return tr_build(S, *tables, tree); });
}

int tr_codons(TrState *S, uint64_t n_codons, const int32_t *slot_pos, const uint8_t *slot_init) {
    if (int rc = query_ready(S, "ugp_translate_codons", "translate")) return rc;
    if (n_codons && (!slot_pos || !slot_init)) return set_error(UGP_ERR_INVALID, "null argument");
    if (n_codons >= (1ull << 30)) return set_error(UGP_ERR_INVALID, "more than 2^30 codons");
    int32_t maxp = 0;
    for (uint64_t c = 0; c < n_codons; c++) {
        const int32_t a = slot_pos[3 * c], b = slot_pos[3 * c + 1], d = slot_pos[3 * c + 2];
        if (a < 1 || b < 1 || d < 1 || a >= kMaxSlotPos || b >= kMaxSlotPos || d >= kMaxSlotPos)
            return set_error(UGP_ERR_INVALID, "codon " + std::to_string(c) + ": slot position outside [1, 2^28)");
        if (a == b || a == d || b == d) return set_error(UGP_ERR_INVALID, "codon " + std::to_string(c) + ": slot positions are not distinct");
        maxp = std::max(maxp, std::max(a, std::max(b, d)));
    }
    try {
        // the codons of every position, ascending by index: cpoff / cpcod (codon << 2 | slot)
        std::vector<uint32_t> cpoff((size_t)maxp + 2, 0), cpcod(3 * n_codons);
        for (uint64_t k = 0; k < 3 * n_codons; k++) cpoff[(size_t)slot_pos[k] + 1]++;
        for (int32_t p = 0; p <= maxp; p++) cpoff[(size_t)p + 1] += cpoff[p];
        {
            std::vector<uint32_t> fill(cpoff.begin(), cpoff.end() - 1);
            for (uint64_t c = 0; c < n_codons; c++)
                for (uint32_t s = 0; s < 3; s++) cpcod[fill[slot_pos[3 * c + s]]++] = (uint32_t)c << 2 | s;
        }
        // the items: per node its owners at coding positions ascending by position, each with the codons of its position
        std::vector<uint32_t> ient, icod;
        std::vector<std::pair<int32_t, uint32_t>> own;
        uint64_t nnodes = 0, ndup = 0;
        uint32_t first_dup = kNil;
        const uint32_t N = S->T->n;
        for (uint32_t v = 0; v < N; v++) {
            own.clear();
            bool dup = false;
            for (uint32_t e = S->h_moff[v]; e < S->h_moff[v + 1]; e++) {
                const int32_t p = S->h_mpos[e];
                if (p < 0 || p > maxp || cpoff[p] == cpoff[(size_t)p + 1]) continue;
                if (S->h_mflag[e] & kOwner) own.emplace_back(p, e);
                else dup = true;
            }
            if (dup) { if (!ndup++) first_dup = v; }
            if (own.empty()) continue;
            nnodes++;
            std::sort(own.begin(), own.end());
            for (const auto &pe : own)
                for (uint32_t x = cpoff[pe.first]; x < cpoff[(size_t)pe.first + 1]; x++) { ient.push_back(pe.second); icod.push_back(cpcod[x]); }
        }
        if (ient.size() >= (1ull << 32)) return set_error(UGP_ERR_UNSUPPORTED, "more than 2^32 (mutation, codon) pairs");
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        S->have_codons = false;
        UGP_HIP_TRY(S->spos.upload(slot_pos, 3 * n_codons, st));
        UGP_HIP_TRY(S->sinit.upload(slot_init, 3 * n_codons, st));
        UGP_HIP_TRY(S->ient.upload(ient, st));
        UGP_HIP_TRY(S->icod.upload(icod, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));   // the host vectors are read until here
        S->nitems = ient.size();
        S->nnodes = nnodes;
        S->ndup = ndup;
        S->first_dup = first_dup;
        S->have_codons = true;
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

// Every window of the items: records into rout (room for `room`) behind each other; *total = their number.  `count` false (the
// bench hook): every window compacts to the front of rout and nothing is read back.
static int tr_windows(TrState *S, uint64_t win, uint64_t room, bool count, uint64_t *total) {
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const TrView v = S->view();
    uint64_t base = 0;
    for (uint64_t i0 = 0; i0 < S->nitems; i0 += win) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(win, S->nitems - i0);
        k_tr_items<<<blocks_for(cnt), kBlock, 0, st>>>(t, v, (uint32_t)i0, cnt, S->flag.p, S->rec.p, S->counters.p);
        UGP_HIP_TRY(scan_flags(S->seg, cnt, S->flag.p, S->off.p, st));
        k_tr_emit<<<blocks_for(cnt), kBlock, 0, st>>>(cnt, S->flag.p, S->off.p, S->rec.p, S->d2b.p, base, room, S->rout.p);
        UGP_HIP_TRY(hipGetLastError());
        if (!count) continue;
        uint32_t got = 0;
        UGP_HIP_TRY(hipMemcpyAsync(&got, S->off.p + cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        base += got;
    }
    if (total) *total = base;
    return UGP_OK;
}

static int tr_ready(TrState *S, const char *who) {
    if (int rc = query_ready(S, who, "translate")) return rc;
    if (!S->have_codons) return set_error(UGP_ERR_INVALID, std::string(who) + ": no codon table: call ugp_translate_codons first");
    return UGP_OK;
}

static int tr_workspace(TrState *S, uint64_t win, uint64_t room) {
    UGP_HIP_TRY(S->flag.alloc(win)); UGP_HIP_TRY(S->off.alloc(win + 1)); UGP_HIP_TRY(S->rec.alloc(win)); UGP_HIP_TRY(S->rout.alloc(room));
    UGP_HIP_TRY(S->seg.alloc(segs_for(win))); UGP_HIP_TRY(S->counters.alloc(2));
    const uint32_t zero[2] = {0, kNil};
    UGP_HIP_TRY(hipMemcpyAsync(S->counters.p, zero, sizeof(zero), hipMemcpyHostToDevice, S->stream));
    UGP_HIP_TRY(hipStreamSynchronize(S->stream));   // `zero` is read until here
    return UGP_OK;
}

int tr_run(TrState *S, ugp_tr_record *out, uint64_t cap, uint64_t *n_out, ugp_tr_info *info, uint64_t chunk_items) {
    if (int rc = tr_ready(S, "ugp_translate")) return rc;
    if (!n_out || (cap && !out)) return set_error(UGP_ERR_INVALID, "null argument");
    *n_out = 0;
    ugp_tr_info I{0, S->nnodes, 0, S->ndup, kNil, S->first_dup == kNil ? kNil : (*S->dfs2bfs)[S->first_dup]};
    uint32_t counters[2] = {0, kNil};
    const uint64_t room = std::min<uint64_t>(cap, S->nitems);
    if (S->nitems) {
        UGP_HIP_TRY(hipSetDevice(S->device));
        const uint64_t win = std::min<uint64_t>(std::min<uint64_t>(chunk_items ? chunk_items : kDefaultItems, 1ull << 30), S->nitems);
        if (int rc = tr_workspace(S, win, room)) return rc;
        if (int rc = tr_windows(S, win, room, true, &I.n_records)) return rc;
        UGP_HIP_TRY(hipMemcpyAsync(counters, S->counters.p, sizeof(counters), hipMemcpyDeviceToHost, S->stream));
        UGP_HIP_TRY(hipStreamSynchronize(S->stream));
    }
    I.n_inconsistent = counters[0];
    if (counters[0]) I.first_inconsistent = S->h_morig[counters[1]];
    if (info) *info = I;
    if (I.n_inconsistent || I.n_duplicate)
        return set_error(UGP_ERR_UNSUPPORTED, "ugp_translate: " + std::to_string(I.n_inconsistent) + " inconsistent entries, " +
                                                  std::to_string(I.n_duplicate) + " nodes with a coding position twice: the closed form does not hold");
    *n_out = I.n_records;
    const uint64_t fill = std::min<uint64_t>(room, I.n_records);
    if (fill) {
        UGP_HIP_TRY(hipMemcpyAsync(out, S->rout.p, fill * sizeof(ugp_tr_record), hipMemcpyDeviceToHost, S->stream));
        UGP_HIP_TRY(hipStreamSynchronize(S->stream));
    }
    return UGP_OK;
}

int tr_time(TrState *S, uint32_t reps, double *ms) {
    if (int rc = tr_ready(S, "ugp_translate_time")) return rc;
    if (!reps || !ms) return set_error(UGP_ERR_INVALID, "null argument");
    *ms = 0;
    if (!S->nitems) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(S->device));
    const uint64_t win = std::min<uint64_t>(kDefaultItems, S->nitems);
    if (int rc = tr_workspace(S, win, win)) return rc;
    return timed(S->stream, "ugp_translate_time", reps, ms, [&] { return tr_windows(S, win, win, false, nullptr); });
}

}  // namespace ugp
