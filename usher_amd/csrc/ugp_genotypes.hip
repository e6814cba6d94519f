// ugp_genotypes.hip -- make_vcf / r_add_genotypes (matUtils convert.cpp:53-292) for a selection of nodes on the device.
//
// The reference walks the tree with a stack of the non-masked mutations of the root path and, at every selected node, pushes the
// whole stack into per-position lists: the column's allele at a position is the LAST mutation of the stack there, REF is par_nuc of
// the first mutation ever inserted for the position, the alternates are the distinct alleles != REF in ascending code order (the
// std::map of make_alts), and a position without an alternate is skipped.
//
// On the depth-first tables (ugp_dense.hpp) the owners of one position -- the first non-masked entry of the position on a node --
// are a laminar family of depth-first ranges [v, dend[v]); poff / pent list them in depth-first order and mlink names the owner
// above.  With rank[] the exclusive prefix count of the selected nodes, owner e of node v spans the columns
// [rank[v], rank[dend[v]]), len(e) of them, and it is the innermost owner of len(e) - sum of len over the owners directly below it.
// Summed per allele that is  cnt[allele(e)] += len(e), cnt[allele(owner above e)] -= len(e)  (DESIGN.md 12): no walk per column.
//   k_gt_e2x / k_gt_owner          attach: per owner its node, the owner above, the allele of the LAST non-masked entry of the
//                                  position on the node, mut_par of the first;
//   k_gt_mark / k_flag_segsum / k_gt_rank   the selection flags in depth-first order, their prefix count (the flag scan of
//                                  ugp_scan.hpp with a callable of its own) and the column -> node list;
//   k_gt_count                     the closed-form counts, the covered columns and the first owner with columns (REF);
//   k_gt_flag / k_gt_compact / k_gt_table   positions with an alternate, in ascending order: the site table and a 16-byte
//                                  allele -> code map per site;
//   k_gt_rows                      a window of (sites x columns): a thread writes 16 consecutive cells with one 16-byte store.  It
//                                  finds the last owner at or before its first and last column's node (binary search over the
//                                  position's owner nodes) and climbs the owners above until one contains the node; since the
//                                  columns ascend in depth-first order the climb of one column continues that of the one before.
// Rows run in windows of bounded workspace (rows x columns, or a part of one row when a row alone is larger).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_genotypes.hpp"

namespace ugp {
namespace {

constexpr uint32_t kCellsPerThread = 16;      // one 16-byte store
constexpr uint32_t kScanTile = 16;            // positions per thread of the site scan
constexpr uint64_t kDefaultCells = 1ull << 26;
constexpr uint64_t kMaxCells = 1ull << 30;

__global__ void k_gt_e2x(uint32_t npo, const uint32_t *pent, uint32_t *e2x) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x < npo) e2x[pent[x]] = x;
}

__global__ void k_gt_owner(DfsView t, uint32_t npo, const uint32_t *e2x, const uint8_t *mpar, uint32_t *onode, uint32_t *oup, uint8_t *oal,
                           uint8_t *opar) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= npo) return;
    const uint32_t e = t.pent[x], v = t.mnode[e], end = t.moff[v + 1];
    const int32_t p = t.mpos[e];
    uint32_t al = b_nuc(t.mbits[e]);
    for (uint32_t k = e + 1; k < end; k++) if (t.mpos[k] == p) al = b_nuc(t.mbits[k]);   // convert.cpp:81-90 overwrites
    const uint32_t up = t.mlink[e];
    onode[x] = v;
    oup[x] = up == kNil ? kNil : e2x[up];
    oal[x] = (uint8_t)al;
    opar[x] = mpar[t.morig[e]];
}

__global__ void k_gt_mark(const uint32_t *pos, uint32_t nsel, uint8_t *flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nsel) flag[pos[i]] = 1;
}

// One block per segment: rank[i] = selected nodes before i (the carry: the segments before), rank[n] = all; column -> node.
__global__ void __launch_bounds__(kBlock) k_gt_rank(uint32_t n, const uint8_t *flag, const uint32_t *seg, uint32_t *rank, uint32_t *coldfs) {
    const uint32_t all = scan_flag_segment(n, flag, seg, blockIdx.x, [&](uint32_t i, uint32_t before, bool set) {
        rank[i] = before;
        if (set) coldfs[before] = i;
    });
    if (last_segment(n, blockIdx.x) && threadIdx.x == 0) rank[n] = all;
}

// One thread per owner: its columns to its allele and from the allele of the owner above (none: to the covered columns).
__global__ void k_gt_count(DfsView t, uint32_t npo, const uint32_t *rank, const uint32_t *onode, const uint32_t *oup, const uint8_t *oal,
                           const uint32_t *oj, uint32_t *cnt, uint32_t *cov, uint32_t *first) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= npo) return;
    const uint32_t v = onode[x], len = rank[t.dend[v]] - rank[v];
    if (!len) return;
    const uint32_t j = oj[x], up = oup[x];
    atomicAdd(&cnt[(size_t)j * 16 + oal[x]], len);
    if (up == kNil) atomicAdd(&cov[j], len);
    else atomicSub(&cnt[(size_t)j * 16 + oal[up]], len);
    atomicMin(&first[j], x);
}

// One thread per position that has owners: does a column carry an allele other than REF?
__global__ void k_gt_flag(uint32_t np, const uint32_t *cnt, const uint32_t *first, const uint8_t *opar, uint8_t *flag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    const uint32_t f = first[j];
    uint32_t any = 0;
    if (f != kNil) {
        const uint32_t ref = opar[f];
#pragma unroll
        for (uint32_t a = 0; a < 16; a++) any |= a != ref ? cnt[(size_t)j * 16 + a] : 0u;
    }
    flag[j] = any ? 1 : 0;
}

// One block: the flagged positions in ascending order.
__global__ void __launch_bounds__(kBlock) k_gt_compact(uint32_t np, const uint8_t *flag, uint32_t *sitej, uint32_t *nsites) {
    __shared__ int sh[kBlock / 64];
    uint32_t carry = 0;
    for (uint64_t t0 = 0; t0 < np; t0 += (uint64_t)kBlock * kScanTile) {
        const uint64_t i0 = t0 + (uint64_t)threadIdx.x * kScanTile;
        uint32_t bits = 0;
        int sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kScanTile; k++) if (i0 + k < np && flag[i0 + k]) { bits |= 1u << k; sum++; }
        int tot;
        const int incl = block_incl_scan(sum, sh, &tot);
        uint32_t run = carry + (uint32_t)(incl - sum);
#pragma unroll
        for (uint32_t k = 0; k < kScanTile; k++) if (bits & (1u << k)) sitej[run++] = (uint32_t)(i0 + k);
        carry += (uint32_t)tot;
    }
    if (threadIdx.x == 0) *nsites = carry;
}

// One thread per site: its row of the site table and its allele -> code map.
__global__ void k_gt_table(uint32_t ns, const uint32_t *sitej, const int32_t *cpos, const uint32_t *cnt, const uint32_t *cov, const uint32_t *first,
                           const uint8_t *opar, ugp_gt_site *tab, uint8_t *map) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const uint32_t j = sitej[s], ref = opar[first[j]];
    ugp_gt_site o;
    o.pos = cpos[j];
    o.ref = (uint8_t)ref;
    o.covered = cov[j];
    uint32_t na = 0;
    uint32_t mw[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 14; k++) { o.alt[k] = 0; o.ac[k] = 0; }
#pragma unroll
    for (uint32_t a = 0; a < 16; a++) {
        const uint32_t c = cnt[(size_t)j * 16 + a];
        if (a == ref || !c || na >= 14) continue;   // (alleles and REF are 1 .. 15: at most 14 alternates)
#pragma unroll
        for (uint32_t k = 0; k < 14; k++) if (k == na) { o.alt[k] = (uint8_t)a; o.ac[k] = c; }
        na++;
        mw[a >> 2] |= na << ((a & 3) * 8);
    }
    o.n_alt = (uint8_t)na;
    tab[s] = o;
    *reinterpret_cast<uint4 *>(map + (size_t)s * 16) = make_uint4(mw[0], mw[1], mw[2], mw[3]);
}

// First index in [lo, hi) of the ascending xs with xs[k] > v.
__device__ __forceinline__ uint32_t upper_bound_u32(const uint32_t *xs, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (xs[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Sites [s0, s0 + rows) x column groups [g0, g0 + gw) of 16 columns: cell (r, g) of `out` (row pitch gw * 16 bytes) holds the
// codes of columns 16 (g0 + g) .. + 15, zero past n_cols.
__global__ void __launch_bounds__(kBlock) k_gt_rows(DfsView t, uint32_t ncols, uint32_t s0, uint32_t rows, uint32_t g0, uint32_t gw,
                                                    const uint32_t *coldfs, const uint32_t *sitej, const uint32_t *coff, const uint32_t *onode,
                                                    const uint32_t *oup, const uint8_t *oal, const uint8_t *map, uint8_t *out) {
    const uint64_t tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tid >= (uint64_t)rows * gw) return;
    const uint32_t r = (uint32_t)(tid / gw), g = (uint32_t)(tid % gw);
    const uint32_t s = s0 + r, j = sitej[s], xlo = coff[j], xhi = coff[j + 1];
    const uint8_t *m = map + (size_t)s * 16;
    const uint32_t c0 = (g0 + g) * kCellsPerThread;            // < ncols: the groups cover ceil(ncols / 16)
    const uint32_t cl = min(c0 + kCellsPerThread - 1, ncols - 1);
    const uint32_t na = coldfs[c0], nb = coldfs[cl];
    const uint32_t a = upper_bound_u32(onode, xlo, xhi, na);
    const uint32_t b = nb == na ? a : upper_bound_u32(onode, a, xhi, nb);
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t lastx = kNil, cur = kNil;
#pragma unroll
    for (uint32_t k = 0; k < kCellsPerThread; k++) {
        const uint32_t c = c0 + k;
        if (c < ncols) {
            const uint32_t node = coldfs[c];
            const uint32_t x = a == b ? a : upper_bound_u32(onode, a, b, node);
            if (x != lastx) { cur = x > xlo ? x - 1 : kNil; lastx = x; }   // else: the climb of the column before goes on
            while (cur != kNil && node >= t.dend[onode[cur]]) cur = oup[cur];
            const uint32_t code = cur == kNil ? 0u : m[oal[cur]];
            w[k >> 2] |= code << ((k & 3) * 8);
        }
    }
    *reinterpret_cast<uint4 *>(out + ((size_t)r * gw + g) * kCellsPerThread) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

struct GtState : QueryBase {
    uint32_t npo = 0, np = 0;                     // owners; positions that have owners
    DBuf<uint32_t> onode, oup, oj, coff;          // per owner: node, owner above, compact position; per compact position: first owner
    DBuf<uint8_t> oal, opar;
    DBuf<int32_t> cpos;
    // the selection
    bool selected = false;
    uint32_t ncols = 0, nsites = 0;
    DBuf<uint8_t> flag, pflag, map, cells;
    DBuf<uint32_t> sel, seg, rank, coldfs, cnt, cov, first, sitej, nsites_d;
    DBuf<ugp_gt_site> tab;
};

void gt_free(GtState *s) { query_free(s); }

int gt_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, GtState **out) {
    return query_attach(
        "ugp_genotypes_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out,
        [&](const DfsTables &T) { return coded_alleles(tree, T, "genotypes need mut_par: REF is the parent allele as stored"); },
        [&](GtState *S) {
            const DfsTables &T = *S->T;
            hipStream_t st = S->stream;
            // the positions that have owners, and each owner's index among them
            std::vector<uint32_t> poff((size_t)T.tp + 1, 0), coff, oj;
            std::vector<int32_t> cpos;
            if (T.tp) UGP_HIP_TRY(hipMemcpy(poff.data(), T.poff.p, poff.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            const uint32_t npo = poff[T.tp];
            oj.resize(npo);
            for (uint32_t p = 0; p < T.tp; p++) {
                if (poff[p + 1] == poff[p]) continue;
                for (uint32_t x = poff[p]; x < poff[p + 1]; x++) oj[x] = (uint32_t)cpos.size();
                cpos.push_back((int32_t)p);
                coff.push_back(poff[p]);
            }
            coff.push_back(npo);
            S->npo = npo;
            S->np = (uint32_t)cpos.size();
            DBuf<uint32_t> e2x;
            DBuf<uint8_t> mpar;
            const StreamDrain drain{st};   // the vectors and temporaries above
            hipError_t err = S->oj.upload(oj, st);
            if (err == hipSuccess) err = S->coff.upload(coff, st);
            if (err == hipSuccess) err = S->cpos.upload(cpos, st);
            if (err == hipSuccess) err = S->onode.alloc(npo);
            if (err == hipSuccess) err = S->oup.alloc(npo);
            if (err == hipSuccess) err = S->oal.alloc(npo);
            if (err == hipSuccess) err = S->opar.alloc(npo);
            if (err == hipSuccess) err = e2x.alloc(T.m);
            if (err == hipSuccess) err = mpar.upload(tree->mut_par, T.m, st);
            if (err == hipSuccess && npo) {
                k_gt_e2x<<<blocks_for(npo), kBlock, 0, st>>>(npo, T.pent.p, e2x.p);
                k_gt_owner<<<blocks_for(npo), kBlock, 0, st>>>(T.view(), npo, e2x.p, mpar.p, S->onode.p, S->oup.p, S->oal.p, S->opar.p);
                err = hipGetLastError();
            }
            if (err == hipSuccess) err = hipStreamSynchronize(st);   // the vectors and temporaries above are read until here
            return hip_rc("ugp_genotypes_attach", err);
        });
}

int gt_select(GtState *S, const uint32_t *nodes, uint64_t nsel, uint32_t *n_cols, uint64_t *n_sites) {
    if (int rc = query_ready(S, "ugp_genotype_select", "genotypes")) return rc;
    if (!n_cols || !n_sites) return set_error(UGP_ERR_INVALID, "null argument");
    const uint32_t N = S->T->n;
    if (!nodes) nsel = 0;
    if (nsel >= (1ull << 32)) return set_error(UGP_ERR_INVALID, "more than 2^32 nodes in the selection");
    for (uint64_t i = 0; i < nsel; i++) if (nodes[i] >= N) return set_error(UGP_ERR_INVALID, "node index out of range");
    try {
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        const DfsView t = S->T->view();
        const uint32_t nseg = (N + kSeg - 1) / kSeg, np = S->np;
        S->selected = false;
        const uint8_t *flag = t.leaf;   // nothing named: all leaves
        if (nsel) {
            std::vector<uint32_t> pos(nsel);
            for (uint64_t i = 0; i < nsel; i++) pos[i] = S->T->bfs2dfs[nodes[i]];
            UGP_HIP_TRY(S->flag.alloc(N));
            UGP_HIP_TRY(hipMemsetAsync(S->flag.p, 0, N, st));
            UGP_HIP_TRY(S->sel.upload(pos, st));
            k_gt_mark<<<blocks_for(nsel), kBlock, 0, st>>>(S->sel.p, (uint32_t)nsel, S->flag.p);
            UGP_HIP_TRY(hipGetLastError());
            UGP_HIP_TRY(hipStreamSynchronize(st));   // `pos` is read until here
            flag = S->flag.p;
        }
        UGP_HIP_TRY(S->seg.alloc(nseg)); UGP_HIP_TRY(S->rank.alloc((size_t)N + 1));
        UGP_HIP_TRY(S->coldfs.alloc(nsel ? std::min<uint64_t>(nsel, N) : N));
        UGP_HIP_TRY(S->cnt.alloc((size_t)np * 16)); UGP_HIP_TRY(S->cov.alloc(np)); UGP_HIP_TRY(S->first.alloc(np));
        UGP_HIP_TRY(S->pflag.alloc(np)); UGP_HIP_TRY(S->sitej.alloc(np)); UGP_HIP_TRY(S->nsites_d.alloc(1));
        k_flag_segsum<<<nseg, kBlock, 0, st>>>(N, flag, S->seg.p);
        k_gt_rank<<<nseg, kBlock, 0, st>>>(N, flag, S->seg.p, S->rank.p, S->coldfs.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(hipMemsetAsync(S->nsites_d.p, 0, sizeof(uint32_t), st));
        if (np) {
            UGP_HIP_TRY(hipMemsetAsync(S->cnt.p, 0, (size_t)np * 16 * sizeof(uint32_t), st));
            UGP_HIP_TRY(hipMemsetAsync(S->cov.p, 0, (size_t)np * sizeof(uint32_t), st));
            UGP_HIP_TRY(hipMemsetAsync(S->first.p, 0xff, (size_t)np * sizeof(uint32_t), st));
            k_gt_count<<<blocks_for(S->npo), kBlock, 0, st>>>(t, S->npo, S->rank.p, S->onode.p, S->oup.p, S->oal.p, S->oj.p, S->cnt.p, S->cov.p,
                                                              S->first.p);
            k_gt_flag<<<blocks_for(np), kBlock, 0, st>>>(np, S->cnt.p, S->first.p, S->opar.p, S->pflag.p);
            k_gt_compact<<<1, kBlock, 0, st>>>(np, S->pflag.p, S->sitej.p, S->nsites_d.p);
            UGP_HIP_TRY(hipGetLastError());
        }
        uint32_t ncols = 0, ns = 0;
        UGP_HIP_TRY(hipMemcpyAsync(&ncols, S->rank.p + N, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipMemcpyAsync(&ns, S->nsites_d.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        UGP_HIP_TRY(S->tab.alloc(ns)); UGP_HIP_TRY(S->map.alloc((size_t)ns * 16));
        if (ns) {
            k_gt_table<<<blocks_for(ns), kBlock, 0, st>>>(ns, S->sitej.p, S->cpos.p, S->cnt.p, S->cov.p, S->first.p, S->opar.p, S->tab.p, S->map.p);
            UGP_HIP_TRY(hipGetLastError());
            UGP_HIP_TRY(hipStreamSynchronize(st));
        }
        S->ncols = ncols;
        S->nsites = ns;
        S->selected = true;
        *n_cols = ncols;
        *n_sites = ns;
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

static int gt_ready(GtState *S, const char *what, uint64_t lo, uint64_t hi) {
    if (int rc = query_ready(S, what, "genotypes")) return rc;
    if (!S->selected) return set_error(UGP_ERR_INVALID, std::string(what) + ": no selection: call ugp_genotype_select first");
    if (lo > hi || hi > S->nsites) return set_error(UGP_ERR_INVALID, std::string(what) + ": site range outside [0, n_sites]");
    return UGP_OK;
}

int gt_columns(GtState *S, uint32_t *nodes) {
    if (int rc = gt_ready(S, "ugp_genotype_columns", 0, 0)) return rc;
    if (!nodes) return set_error(UGP_ERR_INVALID, "null argument");
    UGP_HIP_TRY(hipSetDevice(S->device));
    UGP_HIP_TRY(hipMemcpyAsync(nodes, S->coldfs.p, (size_t)S->ncols * sizeof(uint32_t), hipMemcpyDeviceToHost, S->stream));
    UGP_HIP_TRY(hipStreamSynchronize(S->stream));
    for (uint32_t c = 0; c < S->ncols; c++) nodes[c] = (*S->dfs2bfs)[nodes[c]];
    return UGP_OK;
}

int gt_sites(GtState *S, uint64_t lo, uint64_t hi, ugp_gt_site *out) {
    if (int rc = gt_ready(S, "ugp_genotype_sites", lo, hi)) return rc;
    if (lo == hi) return UGP_OK;
    if (!out) return set_error(UGP_ERR_INVALID, "null argument");
    UGP_HIP_TRY(hipSetDevice(S->device));
    UGP_HIP_TRY(hipMemcpyAsync(out, S->tab.p + lo, (hi - lo) * sizeof(ugp_gt_site), hipMemcpyDeviceToHost, S->stream));
    UGP_HIP_TRY(hipStreamSynchronize(S->stream));
    return UGP_OK;
}

// The windows of sites [lo, hi): each is computed into the workspace and, with `codes`, copied to its place in the caller's matrix.
static int gt_windows(GtState *S, uint64_t lo, uint64_t hi, uint8_t *codes, uint64_t chunk_cells) {
    const uint32_t ncols = S->ncols, groups = (ncols + kCellsPerThread - 1) / kCellsPerThread;
    const uint64_t cells = std::min<uint64_t>(chunk_cells ? chunk_cells : kDefaultCells, kMaxCells);
    // a window: whole rows while one fits, else a part of one row; its workspace is rows * gw * 16 bytes <= cells + 16 * rows
    const uint32_t gw = cells >= ncols ? groups : (uint32_t)std::max<uint64_t>(1, cells / kCellsPerThread);
    const uint64_t rows_per = cells >= ncols ? std::max<uint64_t>(1, cells / ((uint64_t)groups * kCellsPerThread)) : 1;
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    UGP_HIP_TRY(S->cells.alloc(std::min<uint64_t>(rows_per, hi - lo) * gw * kCellsPerThread));
    for (uint64_t s0 = lo; s0 < hi; s0 += rows_per) {
        const uint32_t rows = (uint32_t)std::min<uint64_t>(rows_per, hi - s0);
        for (uint32_t g0 = 0; g0 < groups; g0 += gw) {
            const uint32_t w = std::min(gw, groups - g0);
            k_gt_rows<<<blocks_for((uint64_t)rows * w), kBlock, 0, st>>>(t, ncols, (uint32_t)s0, rows, g0, w, S->coldfs.p, S->sitej.p, S->coff.p,
                                                                         S->onode.p, S->oup.p, S->oal.p, S->map.p, S->cells.p);
            UGP_HIP_TRY(hipGetLastError());
            if (!codes) continue;
            const size_t c0 = (size_t)g0 * kCellsPerThread, width = std::min<size_t>((size_t)w * kCellsPerThread, ncols - c0);
            UGP_HIP_TRY(hipMemcpy2DAsync(codes + (s0 - lo) * ncols + c0, ncols, S->cells.p, (size_t)w * kCellsPerThread, width, rows,
                                         hipMemcpyDeviceToHost, st));
        }
    }
    return UGP_OK;
}

int gt_rows(GtState *S, uint64_t lo, uint64_t hi, uint8_t *codes, uint64_t chunk_cells) {
    if (int rc = gt_ready(S, "ugp_genotype_rows", lo, hi)) return rc;
    if (lo == hi) return UGP_OK;
    if (!codes) return set_error(UGP_ERR_INVALID, "null argument");
    UGP_HIP_TRY(hipSetDevice(S->device));
    if (int rc = gt_windows(S, lo, hi, codes, chunk_cells)) return rc;
    UGP_HIP_TRY(hipStreamSynchronize(S->stream));
    return UGP_OK;
}

int gt_rows_time(GtState *S, uint64_t lo, uint64_t hi, uint32_t reps, double *ms) {
    if (int rc = gt_ready(S, "ugp_genotype_rows_time", lo, hi)) return rc;
    if (!ms || !reps) return set_error(UGP_ERR_INVALID, "null argument");
    *ms = 0;
    if (lo == hi) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(S->device));
    return timed(S->stream, "ugp_genotype_rows_time", reps, ms, [&] { return gt_windows(S, lo, hi, nullptr, 0); });
}

}  // namespace ugp
