// ugp_summary.hip -- matUtils summary (matUtils/summary.cpp) on the device: write_mutation_table (:139-174), write_roho_table
// without dates (:343-506), write_clade_table (:88-137) and write_sample_clades_table (:297-341).
//
// The reference answers RoHo's questions by expanding the subtree of every child of every node and erasing string keys from a map.
// Here every mutation entry gets a KEY -- (position, stored parent allele, allele), the fields of Mutation::get_string(); every
// masked entry the one key "MASKED" -- and the entries are sorted once by (key, depth-first position of their node): the OCCURRENCE
// LIST.  The entries of the depth-first tables already follow their nodes' depth-first order, so one stable radix
// sort by key gives that order.  A run of the list is one key; within a run the nodes ascend, so "does the key occur inside the
// subtree of n" is a binary search for n's depth-first range [n + 1, dend[n]) inside the run.
//   k_sm_keys / (rocprim radix sort) / k_sm_heads / (scan_flags, ugp_scan.hpp) / k_sm_runs     the list, its run heads, run numbers and
//                                  run starts; the list position of every entry;
//   k_sm_nodes                     per node the leaves strictly below it (leaf prefix counts: scan_flags), per parent its non-leaf children, and
//                                  the sort key (parent, leaf count) of every non-leaf child with more than 5 leaves;
//   k_sm_bigseg                    after that sort: where each parent's sorted leaf counts begin, and each child's place in them;
//   k_sm_candkey                   the candidates -- the entries of non-leaf, non-root nodes -- keyed by their parent, for a stable
//                                  sort into (parent, entry) order: the order the records come out in;
//   k_sm_mutations                 a window of the list: a run head writes its key and the length of its run;
//   k_sm_roho                      a window of the candidates: duplicate on its own child, ownership (the LATER non-leaf child with the
//                                  key owns it), erasure (the key at depth >= depth(n) + 2 inside n's range), the leaf-count rules and
//                                  the median of the other children's counts with the owner's own element skipped by index;
//   k_sm_emit                      the records of a window that passed, compacted in order behind those of the windows before;
//   k_sm_gather / k_sm_clade_incl / k_sm_clade_leaf     the clade tables: per (column, leaf) the predecessor among the column's
//                                  annotated nodes in depth-first order, then the climb over the enclosing annotated nodes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "ugp_query.hpp"
#include "ugp_sort.hpp"
#include "ugp_summary.hpp"

namespace ugp {
namespace {

constexpr uint64_t kMaskedKey = 1ull << 40;     // above every (position << 8 | par << 4 | nuc), position < 2^31
constexpr unsigned kKeyBits = 41;
constexpr uint64_t kDefaultItems = 1ull << 22;  // work-items per launch window
constexpr uint32_t kMinLeaves = 5;              // summary.cpp:447, 451: counts must be > 5

__device__ __forceinline__ uint64_t entry_key(int32_t pos, uint32_t par, uint32_t nuc) {
    return pos < 0 ? kMaskedKey : ((uint64_t)(uint32_t)pos << 8) | (uint64_t)(par << 4) | nuc;
}

__global__ void k_sm_keys(DfsView t, uint32_t m, const uint8_t *mpar, uint64_t *key, uint32_t *val) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    key[e] = entry_key(t.mpos[e], mpar[t.morig[e]] & 15u, b_nuc(t.mbits[e]) & 15u);
    val[e] = e;
}

// Per list position x: is it the first of its key; its node; and where its entry went.
__global__ void k_sm_heads(DfsView t, uint32_t m, const uint64_t *skey, const uint32_t *sent, uint8_t *head, uint32_t *onode, uint32_t *inv) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= m) return;
    const uint32_t e = sent[x];
    head[x] = (x == 0 || skey[x] != skey[x - 1]) ? 1 : 0;
    onode[x] = t.mnode[e];
    inv[e] = x;
}

// hidx = heads before x.  rid[x] = the run of x; rstart[r] = its first position, rstart[runs] = m.
__global__ void k_sm_runs(uint32_t m, const uint8_t *head, const uint32_t *hidx, uint32_t *rid, uint32_t *rstart) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x > m) return;
    if (x == m) { rstart[hidx[m]] = m; return; }
    const uint32_t h = head[x], r = hidx[x] + h - 1;   // x = 0 is a head: r >= 0
    rid[x] = r;
    if (h) rstart[r] = x;
}

// Per node: the leaves strictly below it; a non-leaf child counts for its parent; one with more than 5 leaves enters the sort of
// (parent, leaf count) -- every other node sorts in front with key 0.
__global__ void k_sm_nodes(DfsView t, const uint32_t *lpre, uint32_t lbits, uint32_t *lcnt, uint32_t *ccount, uint32_t *bigcnt, uint64_t *bkey,
                           uint32_t *bval) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= t.n) return;
    const uint32_t c = lpre[t.dend[v]] - lpre[v + 1];   // dend[v] >= v + 1
    lcnt[v] = c;
    uint64_t key = 0;
    if (v != 0 && !t.leaf[v]) {
        const uint32_t p = t.dpar[v];
        atomicAdd(&ccount[p], 1u);
        if (c > kMinLeaves) {
            atomicAdd(&bigcnt[p], 1u);
            key = ((uint64_t)(p + 1) << lbits) | c;
        }
    }
    bkey[v] = key;
    bval[v] = v;
}

// Over the sorted (parent, leaf count) keys: the first of a parent's run is where its counts begin; every child learns its place.
__global__ void k_sm_bigseg(uint32_t n, uint32_t lbits, const uint64_t *skey, const uint32_t *sval, uint32_t *bstart, uint32_t *brank) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = skey[i] >> lbits;
    if (!p) return;
    brank[sval[i]] = i;
    if (i == 0 || (skey[i - 1] >> lbits) != p) bstart[(uint32_t)p - 1] = i;
}

// Candidates are the entries of non-leaf nodes other than the root; the rest sort behind them (key n).
__global__ void k_sm_candkey(DfsView t, uint32_t m, uint32_t *key, uint32_t *val) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const uint32_t c = t.mnode[e];
    key[e] = (c != 0 && !t.leaf[c]) ? t.dpar[c] : t.n;
    val[e] = e;
}

// List positions [x0, x0 + cnt): a head of a non-masked run writes record rid[x] when it is below cap.
__global__ void k_sm_mutations(uint32_t x0, uint32_t cnt, const uint64_t *skey, const uint32_t *rid, const uint32_t *rstart, uint64_t cap,
                               ugp_sm_mutation *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    const uint32_t x = x0 + j;
    const uint64_t key = skey[x];
    if (key == kMaskedKey || (x != 0 && skey[x - 1] == key)) return;
    const uint32_t r = rid[x];
    if (r >= cap) return;
    ugp_sm_mutation o;
    o.pos = (int32_t)(key >> 8);
    o.par = (uint8_t)((key >> 4) & 15u);
    o.nuc = (uint8_t)(key & 15u);
    o.pad[0] = o.pad[1] = 0;
    o.count = rstart[r + 1] - x;
    out[r] = o;
}

struct SmView {   // what the RoHo kernel reads beside the depth-first tables
    const uint32_t *cand, *inv, *rid, *rstart, *onode, *lcnt, *ccount, *bigcnt, *bstart, *brank;
    const uint64_t *bskey;
    uint64_t lmask;
};

// Candidates [i0, i0 + cnt) of the (parent, entry) order: flag[j] = 1 and rec[j] when candidate i0 + j is reported.
__global__ void __launch_bounds__(kBlock) k_sm_roho(DfsView t, SmView s, uint32_t i0, uint32_t cnt, uint8_t *flag, ugp_sm_roho *rec) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= cnt) return;
    flag[j] = 0;
    const uint32_t e = s.cand[i0 + j], c = t.mnode[e], n = t.dpar[c];
    const uint32_t x = s.inv[e], r = s.rid[x];
    for (uint32_t k = t.moff[c]; k < e; k++) if (s.rid[s.inv[k]] == r) return;   // stored twice on the child: one candidate
    const uint32_t w = s.lcnt[c], nb = s.bigcnt[n];
    if (w <= kMinLeaves || nb < 2) return;   // sum_wit == 0, or all_non empty (c is one of the nb); implies child_increment.size() >= 2
    const uint32_t re = s.rstart[r + 1], end = t.dend[n], deep = t.depth[n] + 2;
    for (uint32_t y = lower_bound_u32(s.onode, s.rstart[r], re, n + 1); y < re; y++) {   // the occurrences inside (n, dend[n])
        const uint32_t v = s.onode[y];
        if (v >= end) break;
        if (t.depth[v] >= deep) return;          // below a non-leaf child: erased
        if (v > c && !t.leaf[v]) return;         // a later non-leaf child carries the key: it owns it
    }
    // the sorted counts > 5 of n's children, without c's own element (at local index own)
    const uint32_t b0 = s.bstart[n], own = s.brank[c] - b0, others = nb - 1, h = others >> 1;
    const uint32_t hi = (uint32_t)(s.bskey[b0 + h + (h >= own ? 1 : 0)] & s.lmask);
    uint32_t med = hi;
    if (!(others & 1)) {
        const uint32_t lo = (uint32_t)(s.bskey[b0 + h - 1 + (h - 1 >= own ? 1 : 0)] & s.lmask);
        med = (uint32_t)(((uint64_t)lo + hi) / 2);   // summary.cpp:462: integer division
    }
    ugp_sm_roho o;
    o.parent = n; o.child = c; o.entry = t.morig[e];
    o.child_count = s.ccount[n]; o.offspring_with = w; o.median_without = med;
    rec[j] = o;
    flag[j] = 1;
}

// The flagged records of a window go behind the `base` records before them, nodes as breadth-first indices, while below cap.
__global__ void k_sm_emit(uint32_t cnt, const uint8_t *flag, const uint32_t *off, const ugp_sm_roho *rec, const uint32_t *d2b, uint64_t base,
                          uint64_t cap, ugp_sm_roho *out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt || !flag[j]) return;
    const uint64_t o = base + off[j];
    if (o >= cap) return;
    const ugp_sm_roho &r = rec[j];
    out[o] = ugp_sm_roho{d2b[r.parent], d2b[r.child], r.entry, r.child_count, r.offspring_with, r.median_without};
}

__global__ void k_sm_gather(uint32_t na, const uint32_t *anode, const uint32_t *src, uint32_t *dst) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < na) dst[a] = src[anode[a]];
}

// Per listed node (sorted by column, then depth-first position; aorig = its place in the caller's list): the leaves strictly below.
__global__ void k_sm_clade_incl(uint32_t na, const uint32_t *anode, const uint32_t *aorig, const uint32_t *lcnt, uint32_t *incl) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < na) incl[aorig[a]] = lcnt[anode[a]];
}

// Per (column, leaf of the breadth-first leaf list): the last listed node in front of the leaf, then up the enclosing listed nodes
// until one contains the leaf (a listed leaf is not in front of itself: rsearch(.., false) leaves the sample out).
__global__ void k_sm_clade_leaf(DfsView t, uint32_t ncols, uint32_t nleaves, const uint32_t *lbd, const uint32_t *coff, const uint32_t *anode,
                                const uint32_t *aup, const uint32_t *aorig, const uint32_t *d2b, uint32_t *excl, uint32_t *leaf_clade) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (uint64_t)ncols * nleaves) return;
    const uint32_t col = (uint32_t)(tid / nleaves), l = lbd[tid % nleaves];
    const uint32_t lo = coff[col], p = lower_bound_u32(anode, lo, coff[col + 1], l);
    uint32_t cur = p > lo ? p - 1 : kNil;
    while (cur != kNil && l >= t.dend[anode[cur]]) cur = aup[cur];
    leaf_clade[tid] = cur == kNil ? kNil : d2b[anode[cur]];
    if (cur != kNil) atomicAdd(&excl[aorig[cur]], 1u);
}

}  // namespace

struct SmState : QueryBase {
    uint32_t m = 0, nruns = 0, ncand = 0, nleaves = 0;   // entries; non-masked runs; candidates; leaves
    unsigned lbits = 1;
    DBuf<uint8_t> mpar;
    DBuf<uint64_t> skey, bskey;
    DBuf<uint32_t> onode, inv, rid, rstart, cand, lcnt, ccount, bigcnt, bstart, brank, d2b, lbd;
    // per call
    DBuf<uint8_t> flag;
    DBuf<uint32_t> seg, off, anode, aup, aorig, coff, adend, incl, excl, lclade;
    DBuf<ugp_sm_roho> rec, rout;
    DBuf<ugp_sm_mutation> mout;
    DBuf<unsigned char> tmp;
    SmView view() const {
        return SmView{cand.p, inv.p, rid.p, rstart.p, onode.p, lcnt.p, ccount.p, bigcnt.p, bstart.p, brank.p, bskey.p, (1ull << lbits) - 1};
    }
};

void sm_free(SmState *s) { query_free(s); }

static int sm_build(SmState *S, const ugp_tree_desc *tree) {
    const DfsTables &T = *S->T;
    const DfsView t = T.view();
    const uint32_t N = T.n, M = (uint32_t)T.m;
    hipStream_t st = S->stream;
    // host: the leaves in breadth-first order (Tree::get_leaves), the candidates, the masked entries
    std::vector<uint8_t> inner(N, 0);
    for (uint32_t b = 1; b < N; b++) inner[tree->parent[b]] = 1;
    std::vector<uint32_t> lbd;
    uint64_t ncand = 0, nmask = 0;
    for (uint32_t b = 0; b < N; b++) {
        if (!inner[b]) lbd.push_back(T.bfs2dfs[b]);
        else if (b) ncand += tree->mut_off[b + 1] - tree->mut_off[b];
    }
    for (uint64_t k = 0; k < M; k++) nmask += tree->mut_pos[k] < 0 ? 1 : 0;
    S->m = M;
    S->ncand = (uint32_t)ncand;
    S->nleaves = (uint32_t)lbd.size();
    S->lbits = bits_for(N);
    UGP_HIP_TRY(S->lbd.upload(lbd, st));
    UGP_HIP_TRY(S->d2b.upload(S->dfs2bfs->data(), N, st));
    UGP_HIP_TRY(S->mpar.upload(tree->mut_par, M, st));
    // ---- the occurrence list
    DBuf<uint64_t> ukey;
    DBuf<uint32_t> uval, sent, hidx, ckey, ckey2;
    DBuf<uint8_t> head;
    UGP_HIP_TRY(ukey.alloc(M)); UGP_HIP_TRY(uval.alloc(M)); UGP_HIP_TRY(sent.alloc(M)); UGP_HIP_TRY(S->skey.alloc(M));
    UGP_HIP_TRY(head.alloc(M)); UGP_HIP_TRY(hidx.alloc((size_t)M + 1));
    UGP_HIP_TRY(S->onode.alloc(M)); UGP_HIP_TRY(S->inv.alloc(M)); UGP_HIP_TRY(S->rid.alloc(M)); UGP_HIP_TRY(S->rstart.alloc((size_t)M + 1));
    uint32_t runs = 0;
    if (M) {
        k_sm_keys<<<blocks_for(M), kBlock, 0, st>>>(t, M, S->mpar.p, ukey.p, uval.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(sort_pairs(S->tmp, ukey.p, S->skey.p, uval.p, sent.p, M, kKeyBits, st));
        k_sm_heads<<<blocks_for(M), kBlock, 0, st>>>(t, M, S->skey.p, sent.p, head.p, S->onode.p, S->inv.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(scan_flags(S->seg, M, head.p, hidx.p, st));
        k_sm_runs<<<blocks_for((uint64_t)M + 1), kBlock, 0, st>>>(M, head.p, hidx.p, S->rid.p, S->rstart.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(hipMemcpyAsync(&runs, hidx.p + M, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        // ---- the candidates in (parent, entry) order
        UGP_HIP_TRY(ckey.alloc(M)); UGP_HIP_TRY(ckey2.alloc(M)); UGP_HIP_TRY(S->cand.alloc(M));
        k_sm_candkey<<<blocks_for(M), kBlock, 0, st>>>(t, M, ckey.p, uval.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(sort_pairs(S->tmp, ckey.p, ckey2.p, uval.p, S->cand.p, M, bits_for(N), st));
    }
    // ---- leaf counts, the children per parent, the sorted counts > 5 per parent
    DBuf<uint32_t> lpre, bval, bsval;
    DBuf<uint64_t> bkey;
    UGP_HIP_TRY(lpre.alloc((size_t)N + 1)); UGP_HIP_TRY(bval.alloc(N)); UGP_HIP_TRY(bsval.alloc(N)); UGP_HIP_TRY(bkey.alloc(N));
    UGP_HIP_TRY(S->bskey.alloc(N)); UGP_HIP_TRY(S->lcnt.alloc(N)); UGP_HIP_TRY(S->ccount.alloc(N)); UGP_HIP_TRY(S->bigcnt.alloc(N));
    UGP_HIP_TRY(S->bstart.alloc(N)); UGP_HIP_TRY(S->brank.alloc(N));
    UGP_HIP_TRY(hipMemsetAsync(S->ccount.p, 0, (size_t)N * sizeof(uint32_t), st));
    UGP_HIP_TRY(hipMemsetAsync(S->bigcnt.p, 0, (size_t)N * sizeof(uint32_t), st));
    UGP_HIP_TRY(hipMemsetAsync(S->bstart.p, 0, (size_t)N * sizeof(uint32_t), st));
    UGP_HIP_TRY(hipMemsetAsync(S->brank.p, 0, (size_t)N * sizeof(uint32_t), st));
    UGP_HIP_TRY(scan_flags(S->seg, N, t.leaf, lpre.p, st));
    k_sm_nodes<<<blocks_for(N), kBlock, 0, st>>>(t, lpre.p, S->lbits, S->lcnt.p, S->ccount.p, S->bigcnt.p, bkey.p, bval.p);
    UGP_HIP_TRY(hipGetLastError());
    UGP_HIP_TRY(sort_pairs(S->tmp, bkey.p, S->bskey.p, bval.p, bsval.p, N, 2 * S->lbits + 1, st));
    k_sm_bigseg<<<blocks_for(N), kBlock, 0, st>>>(N, S->lbits, S->bskey.p, bsval.p, S->bstart.p, S->brank.p);
    UGP_HIP_TRY(hipGetLastError());
    UGP_HIP_TRY(hipStreamSynchronize(st));   // the temporaries above are read until here
    S->nruns = runs - (nmask ? 1 : 0);
    return UGP_OK;
}

int sm_attach(const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs, int device,
              DfsTables **tables, SmState **out) {
    return query_attach(
        "ugp_summary_attach", tree, dfs2bfs, bfs2dfs, device, 31, tables, out,
        [&](const DfsTables &T) { return coded_alleles(tree, T, "summary needs mut_par: a mutation's name begins with the parent allele as stored"); },
        [&](SmState *S) { return sm_build(S, tree); });
}

int sm_mutations(SmState *S, ugp_sm_mutation *out, uint64_t cap, uint64_t *n_out, uint64_t chunk_items) {
    if (!S) return set_error(UGP_ERR_INVALID, "no summary tables: call ugp_summary_attach first");
    if (!n_out || (cap && !out)) return set_error(UGP_ERR_INVALID, "null argument");
    *n_out = S->nruns;
    const uint64_t fill = std::min<uint64_t>(cap, S->nruns);
    if (!fill) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(S->device));
    UGP_HIP_TRY(S->mout.alloc(fill));
    const uint64_t win = std::min<uint64_t>(chunk_items ? chunk_items : kDefaultItems, 1ull << 30);
    for (uint64_t x0 = 0; x0 < S->m; x0 += win) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(win, S->m - x0);
        k_sm_mutations<<<blocks_for(cnt), kBlock, 0, S->stream>>>((uint32_t)x0, cnt, S->skey.p, S->rid.p, S->rstart.p, fill, S->mout.p);
        UGP_HIP_TRY(hipGetLastError());
    }
    UGP_HIP_TRY(hipMemcpyAsync(out, S->mout.p, fill * sizeof(ugp_sm_mutation), hipMemcpyDeviceToHost, S->stream));
    UGP_HIP_TRY(hipStreamSynchronize(S->stream));
    return UGP_OK;
}

int sm_roho(SmState *S, ugp_sm_roho *out, uint64_t cap, uint64_t *n_out, uint64_t chunk_items) {
    if (!S) return set_error(UGP_ERR_INVALID, "no summary tables: call ugp_summary_attach first");
    if (!n_out || (cap && !out)) return set_error(UGP_ERR_INVALID, "null argument");
    *n_out = 0;
    if (!S->ncand) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(S->device));
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const SmView v = S->view();
    const uint64_t win = std::min<uint64_t>(std::min<uint64_t>(chunk_items ? chunk_items : kDefaultItems, 1ull << 30), S->ncand);
    const uint64_t room = std::min<uint64_t>(cap, S->ncand);
    UGP_HIP_TRY(S->flag.alloc(win)); UGP_HIP_TRY(S->off.alloc(win + 1)); UGP_HIP_TRY(S->rec.alloc(win)); UGP_HIP_TRY(S->rout.alloc(room));
    uint64_t base = 0;
    for (uint64_t i0 = 0; i0 < S->ncand; i0 += win) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(win, S->ncand - i0);
        k_sm_roho<<<blocks_for(cnt), kBlock, 0, st>>>(t, v, (uint32_t)i0, cnt, S->flag.p, S->rec.p);
        UGP_HIP_TRY(hipGetLastError());
        UGP_HIP_TRY(scan_flags(S->seg, cnt, S->flag.p, S->off.p, st));
        k_sm_emit<<<blocks_for(cnt), kBlock, 0, st>>>(cnt, S->flag.p, S->off.p, S->rec.p, S->d2b.p, base, room, S->rout.p);
        UGP_HIP_TRY(hipGetLastError());
        uint32_t got = 0;
        UGP_HIP_TRY(hipMemcpyAsync(&got, S->off.p + cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
        base += got;
    }
    *n_out = base;
    const uint64_t fill = std::min<uint64_t>(room, base);
    if (fill) {
        UGP_HIP_TRY(hipMemcpyAsync(out, S->rout.p, fill * sizeof(ugp_sm_roho), hipMemcpyDeviceToHost, st));
        UGP_HIP_TRY(hipStreamSynchronize(st));
    }
    return UGP_OK;
}

int sm_clades(SmState *S, const uint64_t *col_off, const uint32_t *nodes, uint64_t n_cols, uint32_t *incl, uint32_t *excl, uint32_t *leaf_clade) {
    if (!S) return set_error(UGP_ERR_INVALID, "no summary tables: call ugp_summary_attach first");
    if (!n_cols) return UGP_OK;
    if (!col_off || !leaf_clade) return set_error(UGP_ERR_INVALID, "null argument");
    const uint32_t N = S->T->n, L = S->nleaves;
    const uint64_t A = col_off[n_cols];
    if (n_cols >= (1ull << 16) || A >= (1ull << 31)) return set_error(UGP_ERR_INVALID, "too many columns or listed nodes");
    if (A && (!nodes || !incl || !excl)) return set_error(UGP_ERR_INVALID, "null argument");
    for (uint64_t c = 0; c < n_cols; c++) if (col_off[c] > col_off[c + 1]) return set_error(UGP_ERR_INVALID, "column offsets do not ascend");
    for (uint64_t a = 0; a < A; a++) if (nodes[a] >= N) return set_error(UGP_ERR_INVALID, "node index out of range");
    try {
        // per column the listed nodes by depth-first position
        std::vector<uint32_t> anode(A), aorig(A), aup(A, kNil), coff(n_cols + 1), adend(A);
        for (uint64_t c = 0; c <= n_cols; c++) coff[c] = (uint32_t)col_off[c];
        for (uint64_t a = 0; a < A; a++) aorig[a] = (uint32_t)a;
        for (uint64_t c = 0; c < n_cols; c++) {
            std::sort(aorig.begin() + coff[c], aorig.begin() + coff[c + 1],
                      [&](uint32_t x, uint32_t y) { return S->T->bfs2dfs[nodes[x]] < S->T->bfs2dfs[nodes[y]]; });
            for (uint32_t a = coff[c]; a < coff[c + 1]; a++) {
                anode[a] = S->T->bfs2dfs[nodes[aorig[a]]];
                if (a > coff[c] && anode[a] == anode[a - 1]) return set_error(UGP_ERR_INVALID, "a node is listed twice in one column");
            }
        }
        UGP_HIP_TRY(hipSetDevice(S->device));
        hipStream_t st = S->stream;
        const DfsView t = S->T->view();
        UGP_HIP_TRY(S->anode.upload(anode, st)); UGP_HIP_TRY(S->aorig.upload(aorig, st)); UGP_HIP_TRY(S->coff.upload(coff, st));
        UGP_HIP_TRY(S->adend.alloc(A)); UGP_HIP_TRY(S->incl.alloc(A)); UGP_HIP_TRY(S->excl.alloc(A)); UGP_HIP_TRY(S->aup.alloc(A));
        UGP_HIP_TRY(S->lclade.alloc(n_cols * L));
        if (A) {
            k_sm_gather<<<blocks_for(A), kBlock, 0, st>>>((uint32_t)A, S->anode.p, t.dend, S->adend.p);
            UGP_HIP_TRY(hipGetLastError());
            UGP_HIP_TRY(hipMemcpyAsync(adend.data(), S->adend.p, A * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipStreamSynchronize(st));
            // the enclosing listed node of every listed node: a stack over the depth-first order
            std::vector<uint32_t> stack;
            for (uint64_t c = 0; c < n_cols; c++) {
                stack.clear();
                for (uint32_t a = coff[c]; a < coff[c + 1]; a++) {
                    while (!stack.empty() && anode[a] >= adend[stack.back()]) stack.pop_back();
                    if (!stack.empty()) aup[a] = stack.back();
                    stack.push_back(a);
                }
            }
            UGP_HIP_TRY(S->aup.upload(aup, st));
            UGP_HIP_TRY(hipMemsetAsync(S->excl.p, 0, A * sizeof(uint32_t), st));
            k_sm_clade_incl<<<blocks_for(A), kBlock, 0, st>>>((uint32_t)A, S->anode.p, S->aorig.p, S->lcnt.p, S->incl.p);
            UGP_HIP_TRY(hipGetLastError());
        }
        if (L) {
            k_sm_clade_leaf<<<blocks_for(n_cols * L), kBlock, 0, st>>>(t, (uint32_t)n_cols, L, S->lbd.p, S->coff.p, S->anode.p, S->aup.p, S->aorig.p,
                                                                       S->d2b.p, S->excl.p, S->lclade.p);
            UGP_HIP_TRY(hipGetLastError());
            UGP_HIP_TRY(hipMemcpyAsync(leaf_clade, S->lclade.p, n_cols * L * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        if (A) {
            UGP_HIP_TRY(hipMemcpyAsync(incl, S->incl.p, A * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            UGP_HIP_TRY(hipMemcpyAsync(excl, S->excl.p, A * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        UGP_HIP_TRY(hipStreamSynchronize(st));   // the host vectors above are read until here
    } catch (const std::bad_alloc &) { return set_error(UGP_ERR_NOMEM, "out of host memory"); }
    return UGP_OK;
}

int sm_time(SmState *S, uint32_t reps, double *sort_ms, double *roho_ms) {
    if (!S) return set_error(UGP_ERR_INVALID, "no summary tables: call ugp_summary_attach first");
    if (!reps || !sort_ms || !roho_ms) return set_error(UGP_ERR_INVALID, "null argument");
    *sort_ms = *roho_ms = 0;
    if (!S->m) return UGP_OK;
    UGP_HIP_TRY(hipSetDevice(S->device));
    hipStream_t st = S->stream;
    const DfsView t = S->T->view();
    const uint32_t M = S->m;
    DBuf<uint64_t> ukey, skey;
    DBuf<uint32_t> uval, sent;
    UGP_HIP_TRY(ukey.alloc(M)); UGP_HIP_TRY(skey.alloc(M)); UGP_HIP_TRY(uval.alloc(M)); UGP_HIP_TRY(sent.alloc(M));
    const uint32_t win = (uint32_t)std::min<uint64_t>(kDefaultItems, std::max<uint32_t>(S->ncand, 1));
    UGP_HIP_TRY(S->flag.alloc(win)); UGP_HIP_TRY(S->rec.alloc(win));
    k_sm_keys<<<blocks_for(M), kBlock, 0, st>>>(t, M, S->mpar.p, ukey.p, uval.p);   // what the sort stage sorts
    UGP_HIP_TRY(hipGetLastError());
    const char *who = "ugp_summary_time";
    if (int rc = timed(st, who, reps, sort_ms, [&] { return hip_rc(who, sort_pairs(S->tmp, ukey.p, skey.p, uval.p, sent.p, M, kKeyBits, st)); }))
        return rc;
    return timed(st, who, reps, roho_ms, [&] {
        for (uint64_t i0 = 0; i0 < S->ncand; i0 += win) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(win, S->ncand - i0);
            k_sm_roho<<<blocks_for(cnt), kBlock, 0, st>>>(t, S->view(), (uint32_t)i0, cnt, S->flag.p, S->rec.p);
        }
        return hip_rc(who, hipGetLastError());
    });
}

}  // namespace ugp
