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
// node in depth-first order with best = 1e9, dense: the literal score of ugp_dense.hpp (shared with ugp_uncertainty.hip) with
// the RowGroups cost -- the cost of the rows at a position against a state is the SUM over all rows at that position (loop 2 of
// usher_mapper.cpp:292-350 runs per row, loop 3 only asks whether a row exists there) -- and loop 1 over the rows in their
// stored order.  The depth-first tables (owners, mlink, morig, flags) are the handle's (ugp_dense.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_annotate.hpp"
#include "ugp_query.hpp"

namespace ugp {
namespace {

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
__global__ void k_walk(DfsView t, Alleles A, int emit) {
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
__global__ void k_count(DfsView t, Alleles A, uint32_t V) {
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

__global__ void k_desc(DfsView t, const uint32_t *xs, const uint32_t *coff, const uint32_t *pc, const uint32_t *pu, uint32_t np,
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

__device__ __forceinline__ RowGroups rows(const Search &S) { return RowGroups{S.tab, S.goff, S.grow}; }

__global__ void k_tab(Search S, int set) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < S.ng) S.tab[S.gpos[g]] = set ? g + 1 : 0;
}

// One thread per row position: every owner there adds its term over its subtree.
__global__ void k_events(DfsView t, Search S) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.ng) return;
    const int32_t p = S.gpos[g];
    for (uint32_t i = t.poff[p]; i < t.poff[p + 1]; i++) {
        const uint32_t e = t.pent[i];
        const int ev = ev_term(rows(S), g + 1, t.mbits[e]);
        if (!ev) continue;
        const uint32_t u = t.mnode[e], end = t.dend[u];
        atomicAdd(&S.diff[u], ev);
        if (end < t.n) atomicAdd(&S.diff[end], -ev);
    }
}

__global__ void k_segscan(Search S) {
    if (blockIdx.x || threadIdx.x) return;
    int run = 0;
    for (uint32_t g = 0; g < S.nseg; g++) { const int v = S.seg[g]; S.seg[g] = run; run += v; }
    S.mn[0] = kNone;
}

// The score of every node; eligible ones keep it, the rest read kNone.
__global__ void __launch_bounds__(kBlock) k_score(DfsView t, Search S) {
    score_segment(t, rows(S), Literal{S.qpos, S.qnr, S.nq, S.base, kNil}, S.diff, S.seg[blockIdx.x], blockIdx.x, S.mn);
}

__global__ void __launch_bounds__(kBlock) k_tiecount(DfsView t, Search S) {
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
__global__ void __launch_bounds__(kBlock) k_tiewrite(DfsView t, Search S) {
    const int32_t m = S.mn[0];
    if (m == kNone || !S.scnt[blockIdx.x]) return;
    write_ties(S.diff, t.n, blockIdx.x, m, S.soff[blockIdx.x], S.ties, S.cap, [](uint32_t) {});
}

}  // namespace

struct AnnState : QueryBase {
    // per call
    DBuf<uint32_t> xs, cid, coff, len, ecnt, voff, eoff, cvoff, vis, vcl, veoff, oent, pc, pu, dout;
    DBuf<int32_t> ocnt;
    DBuf<int32_t> qpos, gpos, diff, seg, mn;
    DBuf<uint16_t> qnr, grow;
    DBuf<uint32_t> goff, tab, scnt, soff, total, ties;
};

void ann_free(AnnState *s) { query_free(s); }

int ann_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
               DfsTables **tables, AnnState **out) {
    return query_attach("ugp_annotate_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out, NoCheck(), [](AnnState *S) {
        const uint32_t tp = std::max<uint32_t>(S->T->tp, 1);
        hipError_t err = S->tab.alloc(tp);
        if (err == hipSuccess) err = hipMemsetAsync(S->tab.p, 0, (size_t)tp * sizeof(uint32_t), S->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(S->stream);
        return hip_rc("ugp_annotate_attach", err);
    });
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
            if (nodes[k] >= S->T->n) return set_error(UGP_ERR_INVALID, "node index out of range");
            xs[k] = S->T->bfs2dfs[nodes[k]];
        }
        std::sort(xs.begin() + clade_off[c], xs.begin() + clade_off[c + 1]);
    }
    coff[nc] = (uint32_t)nx;
    UGP_HIP_TRY(hipSetDevice(S->device));
    UGP_HIP_TRY(S->xs.upload(xs, S->stream));
    UGP_HIP_TRY(S->coff.upload(coff, S->stream));
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
        UGP_HIP_TRY(S->cid.upload(cid, st));
        UGP_HIP_TRY(S->len.alloc(nx)); UGP_HIP_TRY(S->ecnt.alloc(nx));
        DfsView t = S->T->view();
        Alleles A{nx, S->xs.p, S->cid.p, S->coff.p, S->len.p, S->ecnt.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        const uint32_t gx = (nx + kBlock - 1) / kBlock;
        if (nx) k_walk<<<gx, kBlock, 0, st>>>(t, A, 0);
        std::vector<uint32_t> len(nx), ecnt(nx);
        if (nx) {
            UGP_HIP_TRY(hipMemcpyAsync(len.data(), S->len.p, nx * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(ecnt.data(), S->ecnt.p, nx * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        UGP_HIP_TRY(hipStreamSynchronize(st));
        std::vector<uint32_t> voff(nx + 1, 0), eoff(nx + 1, 0), cvoff(nc + 1);
        uint64_t V = 0, E = 0;
        for (uint32_t i = 0; i < nx; i++) {
            voff[i] = (uint32_t)V; eoff[i] = (uint32_t)E;
            V += len[i]; E += ecnt[i];
            if (V >= (1ull << 32) || E >= (1ull << 32)) return set_error(UGP_ERR_UNSUPPORTED, "more than 2^32 visited entries in one call");
        }
        voff[nx] = (uint32_t)V; eoff[nx] = (uint32_t)E;
        for (uint64_t c = 0; c <= nc; c++) cvoff[c] = voff[coff[c]];
        UGP_HIP_TRY(S->voff.upload(voff, st)); UGP_HIP_TRY(S->eoff.upload(eoff, st)); UGP_HIP_TRY(S->cvoff.upload(cvoff, st));
        UGP_HIP_TRY(S->vis.alloc(V)); UGP_HIP_TRY(S->vcl.alloc(V)); UGP_HIP_TRY(S->veoff.alloc(V));
        UGP_HIP_TRY(S->oent.alloc(E)); UGP_HIP_TRY(S->ocnt.alloc(E));
        if (E) UGP_HIP_TRY(hipMemsetAsync(S->ocnt.p, 0, E * sizeof(int32_t), st));
        A.voff = S->voff.p; A.eoff = S->eoff.p; A.cvoff = S->cvoff.p;
        A.vis = S->vis.p; A.vcl = S->vcl.p; A.veoff = S->veoff.p; A.oent = S->oent.p; A.ocnt = S->ocnt.p;
        if (nx) k_walk<<<gx, kBlock, 0, st>>>(t, A, 1);
        if (V) k_count<<<(uint32_t)((V + kBlock - 1) / kBlock), kBlock, 0, st>>>(t, A, (uint32_t)V);
        UGP_HIP_TRY(hipGetLastError());
        std::vector<uint32_t> oent(E);
        std::vector<int32_t> ocnt(E);
        if (E) {
            UGP_HIP_TRY(hipMemcpyAsync(oent.data(), S->oent.p, E * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(ocnt.data(), S->ocnt.p, E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        UGP_HIP_TRY(hipStreamSynchronize(st));
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
            if (pair_node[i] >= S->T->n) return set_error(UGP_ERR_INVALID, "node index out of range");
            pu[i] = S->T->bfs2dfs[pair_node[i]];
        }
        hipStream_t st = S->stream;
        UGP_HIP_TRY(S->pc.upload(pair_clade, np, st));
        UGP_HIP_TRY(S->pu.upload(pu, st));
        UGP_HIP_TRY(S->dout.alloc(np));
        k_desc<<<(uint32_t)((np + kBlock - 1) / kBlock), kBlock, 0, st>>>(S->T->view(), S->xs.p, S->coff.p, S->pc.p, S->pu.p, (uint32_t)np, S->dout.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(hipMemcpyAsync(out, S->dout.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

int ann_search(AnnState *S, const ugp_queries *q, uint32_t cap, int32_t *best, uint32_t *tie_dfs, uint32_t *tie_count) {
    if (!S) return set_error(UGP_ERR_INVALID, "no annotate tables: call ugp_annotate_attach first");
    if (!q || !best || !tie_count || (cap && !tie_dfs)) return set_error(UGP_ERR_INVALID, "null argument");
    if (!q->n_queries) return UGP_OK;
    if (!q->ent_off) return set_error(UGP_ERR_INVALID, "null argument");
    if (!S->T->literal_ok) return set_error(UGP_ERR_UNSUPPORTED, "two mutations at one position on one branch");
    const uint64_t nent = q->ent_off[q->n_queries];
    if (nent && (!q->pos || !q->ref || !q->nuc)) return set_error(UGP_ERR_INVALID, "null row arrays");
    try {
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        const uint32_t N = S->T->n, nseg = (N + kSeg - 1) / kSeg;
        UGP_HIP_TRY(S->diff.alloc(N)); UGP_HIP_TRY(S->seg.alloc(nseg)); UGP_HIP_TRY(S->mn.alloc(1));
        UGP_HIP_TRY(S->scnt.alloc(nseg)); UGP_HIP_TRY(S->soff.alloc(nseg)); UGP_HIP_TRY(S->total.alloc(1)); UGP_HIP_TRY(S->ties.alloc(std::max<uint32_t>(cap, 1)));
        const DfsView t = S->T->view();
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
                base += row_cost(a, r, r);
            }
            // rows grouped by position (the positions the tree has entries at)
            order.resize(nq);
            for (uint32_t k = 0; k < nq; k++) order[k] = k;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return qpos[a] < qpos[b]; });
            gpos.clear(); goff.assign(1, 0); grow.clear();
            for (uint32_t k : order) {
                const int32_t p = qpos[k];
                if (p < 0 || (uint32_t)p >= S->T->tp) continue;
                if (gpos.empty() || gpos.back() != p) { gpos.push_back(p); goff.push_back(goff.back()); }
                grow.push_back(qnr[k]);
                goff.back()++;
            }
            const uint32_t ng = (uint32_t)gpos.size();
            UGP_HIP_TRY(S->qpos.upload(qpos, st)); UGP_HIP_TRY(S->qnr.upload(qnr, st));
            UGP_HIP_TRY(S->gpos.upload(gpos, st)); UGP_HIP_TRY(S->goff.upload(goff, st)); UGP_HIP_TRY(S->grow.upload(grow, st));
            Search B{nq, ng, nseg, cap, S->qpos.p, S->qnr.p, S->gpos.p, S->goff.p, S->grow.p, S->tab.p, base,
                     S->diff.p, S->seg.p, S->mn.p, S->scnt.p, S->soff.p, S->total.p, S->ties.p};
            const uint32_t gg = (ng + kBlock - 1) / kBlock;
            UGP_HIP_TRY(hipMemsetAsync(S->diff.p, 0, (size_t)N * sizeof(int32_t), st));
            if (ng) k_tab<<<gg, kBlock, 0, st>>>(B, 1);
            if (ng) k_events<<<gg, kBlock, 0, st>>>(t, B);
            k_segsum<><<<nseg, kBlock, 0, st>>>(N, nseg, B.diff, B.seg);
            k_segscan<<<1, 64, 0, st>>>(B);
            k_score<<<nseg, kBlock, 0, st>>>(t, B);
            k_tiecount<<<nseg, kBlock, 0, st>>>(t, B);
            k_tiescan<<<1, 64, 0, st>>>(B);
            k_tiewrite<<<nseg, kBlock, 0, st>>>(t, B);
            if (ng) k_tab<<<gg, kBlock, 0, st>>>(B, 0);
            UGP_HIP_TRY(hipGetLastError());
            UGP_HIP_TRY(hipMemcpyAsync(best + s, S->mn.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(tie_count + s, S->total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipStreamSynchronize(st));
            const uint32_t k = std::min(cap, tie_count[s]);
            if (k) UGP_HIP_TRY(hipMemcpy(tie_dfs + (size_t)s * cap, S->ties.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

}  // namespace ugp
