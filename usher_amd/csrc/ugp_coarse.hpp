// ugp_coarse.hpp -- the locality pre-pass of a plain batch without tiles: static tables of the coarse tree (built once per tree
// on the host) and the per-sample algorithm k_coarse_sparse runs on them (ugp_coarse.hip), restated for the host so that
// tests/test_coarse_sparse_cpu.py can hold it against oracle/closed_form.py.  No HIP and no getenv in here.
//
// Every row a sample does not have is the reference base, so with the closed form of DESIGN section 2
//     D(n,s)    = D(bottom,s) + D_ref(n) + sum over the events m on root->n of (delta(m,s) - delta_ref(m))
//     cost(n)   = cost_ref(n) + D(bottom,s) + sum over the events at strict ancestors of n (...)      n itself carries no event
//     common(n) = common_ref(n)                                                                       the same condition
// where *_ref are the values of the all-reference sample and an "event" is a mutation of the coarse tree at one of the sample's
// own positions.  An event shifts D by a constant over the strict descendants of its node -- a contiguous range of the depth-first
// order -- and changes cost and eligibility of its own node only.  Per sample: the events' range boundaries sorted, their shifts
// prefix-summed, one range-minimum look-up per stretch between two boundaries, and the event nodes evaluated on their own.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define UGP_COARSE_HD __host__ __device__ __forceinline__
#else
#define UGP_COARSE_HD inline
#endif

namespace ugp {

constexpr uint32_t kCoarseSparseMaxNodes = 65536;   // a depth-first position fits 16 bits (range-minimum keys, event words)
constexpr uint32_t kCoarseSparseMaxEvents = 512;    // per sample: two boundary records each, 6 bytes of LDS per record
constexpr uint32_t kCoarseNoKey = 0xFFFFFFFFu;      // range-minimum key of a node the all-reference sample may not take

// ---- records ---------------------------------------------------------------------------------------------------------------
// An event of the posting lists, two words:
//   w0 = depth-first position of the node | last position of its subtree << 16
//   w1 = mutation allele | previous allele << 4 | reference allele << 8 | behind the node's first masked mutation << 12 | root << 13
UGP_COARSE_HD uint32_t coarse_event_w0(uint32_t d, uint32_t last) { return d | (last << 16); }
UGP_COARSE_HD uint32_t coarse_event_w1(uint32_t mut, uint32_t prev, uint32_t ref, bool after_mask, bool root) {
    return (mut & 15u) | ((prev & 15u) << 4) | ((ref & 15u) << 8) | (after_mask ? 1u << 12 : 0u) | (root ? 1u << 13 : 0u);
}
// A node of the depth-first order, two words:
//   w0 = D_ref(parent) (the root: D_ref(root)) | common_ref << 16
//   w1 = -neg_ref
//
// A boundary record of a sample, one word that sorts by its position, ends before starts:
//   bits 31..14  position * 2 | is_start     (a start sits ON its node, an end one behind the node's subtree)
//   bits  2..0   shift of D + 2              (start: delta - delta_ref, end: the negative of it)
//   bits  4..3   (start) change of neg + 1   bits 6..5  (start) change of common + 1      bit 7  (start) the node is the root
// The stretch behind a start begins one position behind it: the event node itself is never part of a stretch.
constexpr uint32_t kCoarseKeyShift = 14;
UGP_COARSE_HD void coarse_boundaries(uint32_t w0, uint32_t w1, uint32_t S /* the sample's allele set at the position */, uint32_t &start, uint32_t &end) {
    const uint32_t mut = w1 & 15u, prev = (w1 >> 4) & 15u, ref = (w1 >> 8) & 15u;
    const int c = (S & mut) ? 1 : 0, pr = (S & prev) ? 1 : 0, c_ref = (ref & mut) ? 1 : 0, pr_ref = (ref & prev) ? 1 : 0;
    const int delta = pr - c, delta_ref = pr_ref - c_ref, shift = delta - delta_ref;
    const bool counted = !((w1 >> 12) & 1u);   // (in front of the node's first masked mutation: part of neg and common)
    const int dneg = counted ? (delta < 0 ? delta : 0) - (delta_ref < 0 ? delta_ref : 0) : 0, dcom = counted ? c - c_ref : 0;
    const uint32_t d = w0 & 0xFFFFu, last = w0 >> 16;
    start = ((d * 2u + 1u) << kCoarseKeyShift) | (uint32_t)(shift + 2) | ((uint32_t)(dneg + 1) << 3) | ((uint32_t)(dcom + 1) << 5) | (((w1 >> 13) & 1u) << 7);
    end = (((last + 1u) * 2u) << kCoarseKeyShift) | (uint32_t)(2 - shift);
}
UGP_COARSE_HD uint32_t coarse_rec_pos(uint32_t r) { return r >> (kCoarseKeyShift + 1); }
UGP_COARSE_HD bool coarse_rec_is_start(uint32_t r) { return (r >> kCoarseKeyShift) & 1u; }
UGP_COARSE_HD int coarse_rec_shift(uint32_t r) { return (int)(r & 7u) - 2; }
UGP_COARSE_HD int coarse_rec_dneg(uint32_t r) { return (int)((r >> 3) & 3u) - 1; }
UGP_COARSE_HD int coarse_rec_dcom(uint32_t r) { return (int)((r >> 5) & 3u) - 1; }
UGP_COARSE_HD bool coarse_rec_root(uint32_t r) { return (r >> 7) & 1u; }

// The candidate of the stretch [lo, hi) of the depth-first order under the shift `add` (running shift + D(bottom)):
// cost << 16 | position, or kCoarseNoKey.  rmq: [levels][n_nodes], level k holds the minimum key of [i, i + 2^k).
UGP_COARSE_HD uint32_t coarse_range_candidate(const uint32_t *rmq, uint32_t n_nodes, uint32_t lo, uint32_t hi, int add) {
    if (lo >= hi) return kCoarseNoKey;
    const uint32_t k = 31u - (uint32_t)__builtin_clz(hi - lo);
    const uint32_t a = rmq[(size_t)k * n_nodes + lo], b = rmq[(size_t)k * n_nodes + hi - (1u << k)];
    const uint32_t m = a < b ? a : b;
    if (m == kCoarseNoKey) return kCoarseNoKey;
    return ((uint32_t)((int)(m >> 16) + add) << 16) | (m & 0xFFFFu);
}
// The candidate of an event node: base / common_ref / neg from its node words, the shift in front of its own boundaries and the
// sums over its events.
UGP_COARSE_HD uint32_t coarse_node_candidate(uint32_t n0, uint32_t n1, uint32_t d, bool root, int d_bottom, int shift_before, int sum_shift, int sum_dneg, int sum_dcom) {
    const int base = (int)(n0 & 0xFFFFu), common_ref = (int)(n0 >> 16), neg_abs = (int)(n1 & 0x7FFFu);
    if (root) return ((uint32_t)(d_bottom + base + sum_shift) << 16) | d;   // cost = D(root), always eligible
    if (common_ref + sum_dcom <= 0) return kCoarseNoKey;                   // (a node with events has mutations: eligible by common only)
    return ((uint32_t)(d_bottom + base + shift_before - neg_abs + sum_dneg) << 16) | d;
}

// ---- tables ----------------------------------------------------------------------------------------------------------------
// levels of the range-minimum table: one per power of two up to the node count
inline uint32_t coarse_levels(uint32_t n_nodes) { uint32_t l = 1; while ((2ull << (l - 1)) <= n_nodes) l++; return l; }

struct CoarseTables {
    uint32_t n_nodes = 0;       // 0: no tables (tree too large, or a value does not fit its field) -- the walked pre-pass serves
    uint32_t max_per_pos = 0;   // the largest number of events at one position
    std::vector<uint32_t> node;       // [n_nodes][2], depth-first order
    std::vector<uint32_t> rmq;        // [coarse_levels(n_nodes)][n_nodes]
    std::vector<uint32_t> site_off;   // [n_sites + 1]
    std::vector<uint32_t> events;     // [n_events][2], by site
    bool usable() const { return n_nodes != 0; }
    void clear() { *this = CoarseTables(); }
};

// What a loaded file's tables have to satisfy before a kernel may index with them.
inline bool coarse_tables_consistent(const CoarseTables &t, uint64_t n_nodes, uint64_t n_sites) {
    if (!t.n_nodes) return t.node.empty() && t.rmq.empty() && t.site_off.empty() && t.events.empty();
    if (t.n_nodes != n_nodes || t.n_nodes > kCoarseSparseMaxNodes) return false;
    if (t.node.size() != (size_t)t.n_nodes * 2 || t.rmq.size() != (size_t)coarse_levels(t.n_nodes) * t.n_nodes || t.site_off.size() != n_sites + 1 || (t.events.size() & 1)) return false;
    if (t.site_off[0] != 0 || t.site_off[n_sites] != t.events.size() / 2) return false;
    for (uint64_t s = 0; s < n_sites; s++)
        if (t.site_off[s + 1] < t.site_off[s] || t.site_off[s + 1] - t.site_off[s] > t.max_per_pos) return false;
    for (size_t e = 0; e < t.events.size(); e += 2) {
        const uint32_t d = t.events[e] & 0xFFFFu, last = t.events[e] >> 16;
        if (d >= t.n_nodes || last >= t.n_nodes || last < d) return false;
    }
    for (uint32_t v : t.rmq) if (v != kCoarseNoKey && (v & 0xFFFFu) >= t.n_nodes) return false;
    return true;
}

// parent / mut_*: the coarse tree's arrays by BFS index (parent of the root ignored; mut_pos < 0 = masked); dfs2bfs: the flattener's
// depth-first order of it (the order the walk streams the nodes in: equal costs resolve to its first node).
inline void build_coarse_tables(uint64_t n_nodes, const uint32_t *parent, const uint64_t *mut_off, const int32_t *mut_pos, const uint8_t *mut_ref, const uint8_t *mut_nuc,
                                const uint32_t *dfs2bfs, const int32_t *pos2site, uint64_t max_pos, uint64_t n_sites, CoarseTables &t) {
    t.clear();
    if (n_nodes == 0 || n_nodes > kCoarseSparseMaxNodes) return;
    const uint32_t N = (uint32_t)n_nodes;
    std::vector<uint32_t> d_of(N), last(N), pd(N, 0);
    std::vector<uint8_t> has_child(N, 0);
    for (uint32_t d = 0; d < N; d++) d_of[dfs2bfs[d]] = d;
    for (uint32_t d = 0; d < N; d++) last[d] = d;
    for (uint32_t d = N - 1; d >= 1; d--) {
        pd[d] = d_of[parent[dfs2bfs[d]]];
        if (pd[d] >= d) return;   // (not a depth-first order)
        last[pd[d]] = std::max(last[pd[d]], last[d]);
        has_child[pd[d]] = 1;
    }
    struct Ev { uint32_t site, w0, w1; };
    std::vector<Ev> evs;
    std::vector<uint8_t> state(n_sites, 0);   // allele on the current root path, 0 = the reference
    struct Undo { uint32_t site; uint8_t old; };
    std::vector<Undo> undo;
    std::vector<uint32_t> open_d, open_undo;   // the root path of the node in hand and where each node's undo entries begin
    std::vector<int32_t> dref(N, 0);
    std::vector<uint32_t> key(N);
    t.node.assign((size_t)N * 2, 0);
    for (uint32_t d = 0; d < N; d++) {
        while (!open_d.empty() && d > last[open_d.back()]) {
            for (size_t u = undo.size(); u > open_undo.back(); u--) state[undo[u - 1].site] = undo[u - 1].old;
            undo.resize(open_undo.back());
            open_d.pop_back(); open_undo.pop_back();
        }
        open_d.push_back(d); open_undo.push_back((uint32_t)undo.size());
        const uint32_t j = dfs2bfs[d];
        const int d_par = d ? dref[pd[d]] : 0;
        int tsum = 0, neg = 0, common = 0;
        bool masked = false;
        for (uint64_t i = mut_off[j]; i < mut_off[j + 1]; i++) {
            const int32_t p = mut_pos[i];
            if (p < 0) { masked = true; continue; }
            if ((uint64_t)p > max_pos || pos2site[p] < 0 || (uint64_t)pos2site[p] >= n_sites) { t.clear(); return; }
            const uint32_t site = (uint32_t)pos2site[p];
            const uint8_t nuc = mut_nuc[i], ref = mut_ref[i];
            if (nuc == 0 || (nuc & (nuc - 1)) || nuc > 8 || ref == 0 || (ref & (ref - 1)) || ref > 8) { t.clear(); return; }   // (one-hot alleles only)
            const uint8_t prev = state[site] ? state[site] : ref;
            const int c = (ref & nuc) ? 1 : 0, pr = (ref & prev) ? 1 : 0, delta = pr - c;
            tsum += delta;
            if (!masked) { common += c; neg += std::min(delta, 0); }
            evs.push_back({site, coarse_event_w0(d, last[d]), coarse_event_w1(nuc, prev, ref, masked, d == 0)});
            undo.push_back({site, state[site]});
            state[site] = nuc;
        }
        dref[d] = d_par + tsum;
        const bool elig = d == 0 || common > 0 || (has_child[d] && mut_off[j + 1] == mut_off[j]);
        const int base = d ? d_par : dref[d], cost = d ? d_par + neg : dref[d];
        if (base < 0 || base > 0xFFFF || common > 0xFFFF || -neg > 0x7FFF || cost < 0 || cost > 0xFFFE) { t.clear(); return; }
        t.node[(size_t)d * 2] = (uint32_t)base | ((uint32_t)common << 16);
        t.node[(size_t)d * 2 + 1] = (uint32_t)(-neg);
        key[d] = elig ? ((uint32_t)cost << 16) | d : kCoarseNoKey;
    }
    // posting lists by site (a counting sort; the events of a site keep the depth-first order)
    t.site_off.assign(n_sites + 1, 0);
    for (const Ev &e : evs) t.site_off[e.site + 1]++;
    for (uint64_t s = 0; s < n_sites; s++) { t.max_per_pos = std::max(t.max_per_pos, t.site_off[s + 1]); t.site_off[s + 1] += t.site_off[s]; }
    t.events.resize(evs.size() * 2);
    {
        std::vector<uint32_t> at(t.site_off.begin(), t.site_off.end() - 1);
        for (const Ev &e : evs) { const uint32_t k = at[e.site]++; t.events[(size_t)k * 2] = e.w0; t.events[(size_t)k * 2 + 1] = e.w1; }
    }
    // range minima, one level per power of two (the entries whose range would pass the end repeat the last full one's operand)
    const uint32_t levels = coarse_levels(N);
    t.rmq.resize((size_t)levels * N);
    std::copy(key.begin(), key.end(), t.rmq.begin());
    for (uint32_t k = 1; k < levels; k++) {
        const uint32_t half = 1u << (k - 1);
        const uint32_t *below = &t.rmq[(size_t)(k - 1) * N];
        uint32_t *lvl = &t.rmq[(size_t)k * N];
        for (uint32_t i = 0; i < N; i++) lvl[i] = std::min(below[i], below[std::min(i + half, N - 1)]);
    }
    t.n_nodes = N;
}

// ---- one sample, on the host ----------------------------------------------------------------------------------------------
// The steps of k_coarse_sparse in the same order with the same helpers; returns cost << 16 | depth-first position.
// Rows outside [0, max_pos] or without a coarse site only count for D(bottom).
inline uint32_t coarse_sparse_host(const CoarseTables &t, const int32_t *pos2site, uint64_t max_pos, uint64_t n_rows, const int32_t *pos, const uint8_t *ref,
                                   const uint8_t *nuc, const uint8_t *is_missing) {
    int d_bottom = 0;
    std::vector<uint32_t> rec;
    for (uint64_t r = 0; r < n_rows; r++) {
        const uint32_t S = is_missing[r] ? 15u : nuc[r];
        if (!is_missing[r] && (nuc[r] & ref[r]) == 0) d_bottom++;
        const int32_t p = pos[r];
        const int32_t site = (p >= 0 && (uint64_t)p <= max_pos) ? pos2site[p] : -1;
        if (site < 0) continue;
        for (uint32_t e = t.site_off[site]; e < t.site_off[site + 1]; e++) {
            uint32_t s, en;
            coarse_boundaries(t.events[(size_t)e * 2], t.events[(size_t)e * 2 + 1], S, s, en);
            rec.push_back(s); rec.push_back(en);
        }
    }
    std::sort(rec.begin(), rec.end());
    const uint32_t n = (uint32_t)rec.size();
    std::vector<int> pre(n);
    for (uint32_t i = 0, run = 0; i < n; i++) { run += (uint32_t)coarse_rec_shift(rec[i]); pre[i] = (int)run; }
    uint32_t best = kCoarseNoKey;
    for (uint32_t i = 0; i <= n; i++) {
        const uint32_t lo = i ? coarse_rec_pos(rec[i - 1]) + (coarse_rec_is_start(rec[i - 1]) ? 1u : 0u) : 0u;
        const uint32_t hi = i < n ? coarse_rec_pos(rec[i]) : t.n_nodes;
        const int before = i ? pre[i - 1] : 0;
        best = std::min(best, coarse_range_candidate(t.rmq.data(), t.n_nodes, lo, hi, before + d_bottom));
        if (i < n && coarse_rec_is_start(rec[i]) && (i == 0 || (rec[i - 1] >> kCoarseKeyShift) != (rec[i] >> kCoarseKeyShift))) {   // the first event of a node
            int sum_shift = 0, sum_dneg = 0, sum_dcom = 0;
            for (uint32_t k = i; k < n && (rec[k] >> kCoarseKeyShift) == (rec[i] >> kCoarseKeyShift); k++) {
                sum_shift += coarse_rec_shift(rec[k]); sum_dneg += coarse_rec_dneg(rec[k]); sum_dcom += coarse_rec_dcom(rec[k]);
            }
            const uint32_t d = coarse_rec_pos(rec[i]);
            best = std::min(best, coarse_node_candidate(t.node[(size_t)d * 2], t.node[(size_t)d * 2 + 1], d, coarse_rec_root(rec[i]), d_bottom, before, sum_shift, sum_dneg, sum_dcom));
        }
    }
    return best;
}

}  // namespace ugp
