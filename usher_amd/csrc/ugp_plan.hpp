// ugp_plan.hpp -- the host decisions of a placement call (run_place, ugp_capi.cpp) as pure functions: which path, how many
// samples per sub-batch, how many groups, which tile builder and bitmap variant, whether the third bound can run, the layout
// of the zeroed buffer, the work units and the grid.  No HIP and no getenv in here: the facts arrive in small structs, the
// knobs as `const Knobs &`, and tests/test_plan_cpu.py pins every decision on the CPU (results never depend on one, so no
// oracle test can).  What has side effects -- the B3Tuner, the occupancy query -- stays with the caller; its answer is an input.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "ugp_coarse.hpp"
#include "ugp_flatten.hpp"
#include "ugp_knobs.hpp"
#include "ugp_tuner.hpp"

namespace ugp {

constexpr uint32_t kMaxTilesPerLaunch = 4096;   // 262,144 samples per sub-batch

// ---- inputs ---------------------------------------------------------------------------------------------------------------
struct PlanTree {   // the tree and its handle
    uint64_t n_nodes = 0, n_sites = 0;   // (n_sites as flattened: may be 0)
    uint32_t n_chunks = 0, max_chunk8_words = 0, max_path_muts = 0, lds_slots = 0;
    bool mask_not_first = false;
    bool coarse = false;         // the handle has a coarse tree (locality sort)
    bool b3_events = false;      // ... and the third bound's posting lists
    bool wide_descent = false;
    // the pre-pass from the samples' own rows (ugp_coarse.hpp): the coarse tree's static tables, and what rules them out
    uint64_t coarse_nodes = 0;            // nodes of the coarse tree the tables were built for (0: no tables)
    uint32_t coarse_max_per_pos = 0;      // the largest number of coarse mutations at one position
    bool coarse_excluded = false;         // ugp_mat_update has taken a node out of the candidate set
    bool coarse_masked = false;           // a node mask is in force on the streams (ugp_place_batch_ex)
};
struct PlanEx {   // which options an extended search carries (ExDev, ugp_capi.cpp)
    bool given = false, packed = false, mask = false, skip = false, skip_chunk = false, scores = false;
};
struct PlanCall {   // the query set and the call
    uint64_t Q = 0, max_rows = 0;
    int mode = 0;
    bool coarse_only = false;
    bool ties = false;           // the call wants tie lists
    bool nmask = false;          // the query set carries N masks for this tree
    bool sharing = false;        // (ugp_mat::sharing / share_sets)
    int share_sets = 2;
    PlanEx ex;
};

// ---- per call -------------------------------------------------------------------------------------------------------------
struct CallPlan {
    uint32_t n_sites = 1, active_words = 1, useful_words = 1;
    bool ex_packable = false, ex_skip = false, packed_ok = false, sorted = false, can_fork = false, fill_ahead = false;
    bool coarse_sparse = false;           // the pre-pass runs as k_coarse_sparse, not as a walk of the coarse tree
    uint32_t coarse_cap = 0;              // ... with this many boundary records of LDS per sample
    uint64_t sub_tiles = kMaxTilesPerLaunch;
};

inline CallPlan plan_call(const PlanTree &t, const Knobs &K, const PlanCall &c) {
    CallPlan p;
    // at least one table row, so that words without a row of their own (headers,
    // reference-everywhere sites) always have the valid row 0 to fetch
    p.n_sites = std::max<uint32_t>((uint32_t)t.n_sites, 1u);
    p.active_words = (p.n_sites + 31) / 32;
    p.useful_words = (p.n_sites + 7) / 8;
    // Locality sort: place every sample on the coarse top-of-the-tree MAT first; samples are then
    // assigned to 512-sample tiles in the DFS order of that coarse placement (k_sort_keys).
    // (16-bit phase 1: every D / cost must stay below 0x7F7F, the value the shared upper bounds start from;
    // a tree with a masked mutation behind an ordinary one on the same node -- never produced by the reference's
    // sorted Node::add_mutation, mutation_annotated_tree.cpp:720-752 -- needs the order-aware 32-bit walk)
    // (the extended searches take the packed path too when their options are the kind it can express: a node order / distance is a
    // tie rank of phase 2, a node mask has been turned into exclusions by the caller, a per-sample excluded node is taken out of
    // the one chunk minimum it can have set, behind phase 1 (k_fix_skip); per-node scores stay on the one-sample-per-lane kernel)
    p.ex_packable = c.ex.given && c.ex.packed && !c.ex.mask && (!c.ex.skip || c.ex.skip_chunk) && !c.ex.scores;
    p.ex_skip = p.ex_packable && c.ex.skip;
    // 16-bit packed phase 1 is exact while every D / cost stays below 0x8000 (bit 15 is the ineligible flag)
    p.packed_ok = (c.mode == 0) && (!c.ex.given || p.ex_packable) && !K.force_v1 && !t.mask_not_first && (c.max_rows + t.max_path_muts + 2 < 0x7F7Full);
    p.sorted = p.packed_ok && t.coarse && c.Q > 512 && !K.no_sort && !K.no_prune;
    // The pre-pass without tiles: a sorted call of the plain search (or of an extended one that only leaves a node out per sample --
    // the pre-pass never looks at it), on a coarse tree that is what its static tables describe -- no node excluded since, no mask on
    // the streams --, whose positions fit 16 bits, and whose samples' events fit the LDS of a lane group: a row meets at most
    // coarse_max_per_pos events, each two boundary records.  UGP_COARSE_PHASE2=1 keeps the walked pass.
    p.coarse_sparse = p.sorted && (!c.ex.given || (c.ex.packed && !c.ex.mask && !c.ex.scores)) && !K.coarse_phase2 && t.coarse_nodes != 0 &&
                      t.coarse_nodes <= kCoarseSparseMaxNodes && !t.coarse_excluded && !t.coarse_masked &&
                      c.max_rows * (uint64_t)t.coarse_max_per_pos <= kCoarseSparseMaxEvents;
    if (p.coarse_sparse) for (p.coarse_cap = 32; p.coarse_cap < 2 * c.max_rows * (uint64_t)t.coarse_max_per_pos; p.coarse_cap *= 2) {}
    // The side stream (see Work::aux): only where there is something to put on it -- the sorted main pass.
    // And only for a call that has the device to itself: measured with three calls in flight (six queues instead of three), the
    // cross-queue waits cost far more than the overlap gives -- 12.9 -> 10.4 M placements/s; a lone call gains 45 us of its 1.96 ms.
    // OPT-IN (UGP_FORK=1) since the end of round 6: a process has four hardware queues by default, a handle's three streams plus
    // their side streams oversubscribe them, and which streams then share a queue -- and serialise -- depends on what the process
    // created before: the SECOND handle of a process ran its overlapped calls one after the other (tools/probe_context.py: config 3's
    // size 7.7 -> 4.7 M/s, the headline workload 13.9 -> 9.6) for a gain of 45 us on the first.
    p.can_fork = p.sorted && !c.coarse_only && !K.no_fork && !c.sharing;
    // plain batches (fill + scatter; the other tile builders write every row themselves): the fill depends on nothing but the set
    // being free, which `s` has just waited for
    p.fill_ahead = p.can_fork && !(c.nmask && p.n_sites) && K.tile_build <= 0 && t.n_sites && std::min<uint64_t>(c.Q, (uint64_t)kMaxTilesPerLaunch * 64) == c.Q;
    // samples per sub-batch: at most 262,144, and few enough that the per-(chunk, sample) minima of phase 1
    // (2 bytes each) stay below 24 GiB (8 until round 4: 131,072 samples per launch sequence at 10M nodes; the walk does
    // 16,384 samples' worth of work in 0.55 ms at 262,144 per launch against 0.68 at 65,536 -- 1M queries per call 20.0 -> 23.1 M/s)
    if (t.n_chunks) p.sub_tiles = std::min<uint64_t>(p.sub_tiles, std::max<uint64_t>(8, ((K.lbest_gib ? (uint64_t)K.lbest_gib : 24ull) << 30) / ((uint64_t)t.n_chunks * 128) & ~7ull));
    return p;
}

// ---- per sub-batch --------------------------------------------------------------------------------------------------------
inline uint32_t pick_groups(const PlanTree &t, const Knobs &K, uint32_t n_tiles, uint32_t target_waves = 4096) {
    if (K.target_waves) target_waves = K.target_waves;
    uint32_t g = (target_waves + n_tiles - 1) / n_tiles;
    if (K.groups) g = K.groups;
    g = std::min<uint32_t>(g, t.n_chunks);
    g = std::max<uint32_t>(g, 1);
    if (g >= 8) g &= ~7u;   // XCD-aware block mapping wants a multiple of 8
    return g;
}

struct SubPlan {
    uint32_t n_tiles = 0, n_tiles512 = 0, G = 1;
    bool nmask = false;          // the tiles come from the query set's N masks
    bool lds_build = false;
    uint32_t lds_bits_plan = 0;
    bool b3_can = false, b3_tuned = false;
    bool b3_want = false;        // (b3_tuned: the caller overwrites it with the tuner's answer)
    int b3_class = 0;
    bool uniq_ok = false;
};

// nq samples with `rows` rows between them
inline SubPlan plan_sub(const PlanTree &t, const Knobs &K, const PlanCall &c, const CallPlan &cp, uint64_t nq, uint64_t rows) {
    SubPlan p;
    p.n_tiles = (uint32_t)((nq + 63) / 64);
    p.n_tiles512 = (uint32_t)((nq + 511) / 512);
    p.G = pick_groups(t, K, p.n_tiles);
    if (cp.packed_ok) {   // work units of a few chunks each, pulled from per-XCD queues by persistent waves (see k_best8)
        uint32_t unit_chunks = 16;   // (most far units end in their preamble: the replay is the cost to amortise)
        if (K.unit_chunks) unit_chunks = K.unit_chunks;
        p.G = std::max<uint32_t>(1, (t.n_chunks + unit_chunks - 1) / unit_chunks);
        // a small batch still has to fill the chip: at least ~4096 units in total
        while (p.G < t.n_chunks && (uint64_t)p.G * p.n_tiles512 < 4096) p.G = std::min<uint32_t>(t.n_chunks, p.G * 2);
        if (K.groups) p.G = std::min<uint32_t>(t.n_chunks, K.groups);
    }
    // (what the walk will be launched with is decided here, in front of the tile build: a batch whose walk keeps its active-row
    // bitmap in LDS -- lds_bits == 1 -- has no third-bound variant, and building the tables for it, or letting the tuner book
    // the batch as one "with", would be cost without effect: ADVICE r5)
    p.nmask = c.nmask && cp.packed_ok && cp.n_sites;
    // many rows per sample (high-ambiguity queries): the (tile, site block)-in-LDS builder; otherwise fill + one atomic per row
    // (only for batches in arrival order, i.e. the coarse pass: consecutive threads then read neighbouring row lists; behind
    // the locality sort the builder's uncoalesced row reads cost more than the scatter's atomics -- measured on config 5:
    // coarse pass 2.72 -> 2.33 ms, sorted build 1.77 -> 2.03 ms)
    p.lds_build = cp.packed_ok && cp.n_sites && !cp.sorted && rows >= (uint64_t)nq * 128;
    if (K.tile_build >= 0) p.lds_build = cp.packed_ok && cp.n_sites && K.tile_build != 0;
    if (cp.packed_ok) {
        const bool stats_on = K.stats;
        p.lds_bits_plan = (!stats_on && (size_t)cp.active_words * 4 <= 4096 && p.n_tiles512 >= 64 && !c.sharing) ? 1u : 0u;
        if (p.nmask && !stats_on) p.lds_bits_plan = 2u;
        if (K.lds_bits >= 0) p.lds_bits_plan = stats_on ? 0u : (K.lds_bits == 2 ? 2u : (((size_t)cp.active_words * 4 <= 4096 && K.lds_bits != 0) ? 1u : 0u));
    }
    // Third pruning bound (round 5): for the sorted main walk of batches of up to 256 tiles, when the tree carries its posting lists
    // and the tiles are built by the scatter kernels (they mark the tile's useful (site, allele) pairs)
    p.b3_can = cp.packed_ok && !c.coarse_only && cp.sorted && t.b3_events && !K.no_bound3 && K.bound3 != 0 && !K.no_prune && p.n_tiles512 <= 256 && K.tile_build <= 0 &&
               p.lds_bits_plan != 1u && !(p.lds_build && !p.nmask);
    p.b3_want = p.b3_can;
    p.b3_class = B3Tuner::class_of(rows, nq);
    // UGP_BOUND3 unset: decided from what is known of the tree and of the batch (ugp_tuner.hpp b3_static_choice) -- every call of a
    // kind runs the same way from the first one on; UGP_BOUND3=auto: the handle's run-time A/B (B3Tuner); 1 / 0: pinned
    p.b3_tuned = p.b3_can && K.bound3 == -1;
    if (!p.b3_tuned && p.b3_can && K.bound3 < -1) p.b3_want = b3_static_choice(t.wide_descent, p.b3_class, t.n_nodes);
    // phase 2 without a walk for the samples whose minimum is attained by one node (ugp_kernels.hpp Phase2Uniq): the plain search only
    p.uniq_ok = cp.packed_ok && cp.sorted && !c.coarse_only && c.mode == 0 && !c.ex.given && !c.ties && t.n_nodes < (1ull << 31) && !K.no_uniq;
    return p;
}

// every small buffer that has to start from zero lives in ONE allocation cleared by one memset:
// D(bottom) counters, active-row bitmap, work-queue heads, record lists' lengths, phase-2 item count, tie counts / keys
struct ZeroLayout {   // offsets in 32-bit words
    size_t z_dbottom = 0, z_active = 0, z_queue = 0, z_list_n = 0, z_nitems = 0, z_cnt = 0, z_key = 0, z_useful = 0, z_end = 0;
};
inline ZeroLayout zero_layout(uint32_t n_tiles512, uint32_t active_words, uint32_t useful_words, bool b3_want) {
    ZeroLayout z;
    z.z_dbottom = 0; z.z_active = z.z_dbottom + (size_t)n_tiles512 * 512; z.z_queue = z.z_active + (size_t)n_tiles512 * active_words;
    z.z_list_n = z.z_queue + 8; z.z_nitems = z.z_list_n + n_tiles512; z.z_cnt = z.z_nitems + 8; z.z_key = z.z_cnt + (size_t)n_tiles512 * 512;
    z.z_useful = z.z_key + (size_t)n_tiles512 * 512; z.z_end = z.z_useful + (b3_want ? (size_t)n_tiles512 * useful_words : 0);
    return z;
}

// (the unused slots of the last tile: far from everything, see k_seed_ub; 16-bit safe by the guard of the packed path)
inline uint32_t seed_pad_d(const PlanTree &t, const Knobs &K) {
    return K.no_pad_fix ? 0u : (uint32_t)std::min<uint64_t>(4096, 0x7F7Eu - 2u - std::min<uint64_t>(t.max_path_muts, 0x7F00u));
}

// ---- per packed walk ------------------------------------------------------------------------------------------------------
struct UnitCaps { uint32_t n_side = 0, per_tile_cap = 0; };
// how many units a tile's list can hold: the heavy units of its own region, and on either side units that grow with the distance
inline UnitCaps unit_caps(uint32_t n_chunks, uint32_t unit_chunks, uint32_t heavy_chunks, uint32_t grow_every, uint32_t unit_max) {
    auto len_of = [&](uint32_t i) -> uint64_t {
        if (!grow_every) return unit_chunks;
        return std::min<uint64_t>((uint64_t)unit_chunks << std::min<uint32_t>(i / grow_every, 16u), std::max(unit_max, unit_chunks));
    };
    UnitCaps u;
    for (uint64_t done = 0; done < n_chunks; u.n_side++) done += len_of(u.n_side);
    u.per_tile_cap = (n_chunks + heavy_chunks - 1) / heavy_chunks + 2u * u.n_side + 2u;
    return u;
}

struct WalkPlan {
    bool tile_ranges = false;    // every tile's own region is handed out first (launch_tile_ranges)
    bool bounds = false;         // the walk prunes (Best8Args::ub)
    uint32_t unit_chunks = 1, heavy_chunks = 16, light_order = 0, grow_every = 0, unit_max = 0, no_pre_records = 0;
    uint32_t n_side = 0, per_tile_cap = 0;
    uint32_t split_cycles = 0, split_heavy = 0, split_dense = 0, split_many = 0, ub_every = 128;
    uint32_t lds_bits = 0;
    size_t lds_bytes = 0;
    bool b3 = false;             // the walk runs with the third bound
    int variant = 0;             // (the kernel launch_best8 will pick)
};

inline WalkPlan plan_walk(const PlanTree &t, const Knobs &K, const PlanCall &c, const CallPlan &cp, const SubPlan &sp) {
    WalkPlan w;
    w.bounds = !K.no_prune;
    w.tile_ranges = cp.sorted && !K.no_lpt;   // hand out every tile's own region first (scheduling only)
    w.unit_chunks = std::max<uint32_t>(1, (t.n_chunks + sp.G - 1) / sp.G);
    if (K.ub_every) w.ub_every = K.ub_every;
    // (trees with large polytomies keep the tile-after-tile order: measured, 7 % apart in either direction)
    w.light_order = K.light_order >= 0 ? (uint32_t)K.light_order : (t.wide_descent ? 1u : 0u);
    if (K.heavy_chunks) w.heavy_chunks = K.heavy_chunks;
    // Units outside the tiles' own regions grow with the distance from the region (they end in their preamble or after a
    // few jumps: what they cost is the replay, not their length) -- only when there is a region to measure from and bounds
    // to prune with.
    w.grow_every = (w.tile_ranges && w.bounds) ? 8u : 0u; w.unit_max = w.unit_chunks * 16u;
    if (K.unit_grow >= 0) w.grow_every = (w.tile_ranges && w.bounds) ? (uint32_t)K.unit_grow : 0u;
    if (K.unit_max) w.unit_max = K.unit_max;
    // A preamble record says where the body goes on behind a path node's subtree in INFO_JUMP_MASK's 18 bits, the largest
    // value meaning "beyond the unit": no unit may be longer than that many words.  (Should even the basic units be --
    // chunks of thousands of words: nodes with thousands of mutations -- the replay runs without those records.)
    {
        const uint64_t reach = INFO_JUMP_MASK - 1u, cw = std::max<uint32_t>(1, t.max_chunk8_words);
        w.unit_max = (uint32_t)std::max<uint64_t>(w.unit_chunks, std::min<uint64_t>(w.unit_max, reach / cw));
        w.no_pre_records = ((uint64_t)std::max(w.unit_chunks, w.heavy_chunks) * cw > reach) ? 1u : 0u;
    }
    const UnitCaps u = unit_caps(t.n_chunks, w.unit_chunks, w.heavy_chunks, w.grow_every, w.unit_max);
    w.n_side = u.n_side; w.per_tile_cap = u.per_tile_cap;
    // units that run long are cut while they run: the shared list of split-off halves (k_best8)
    w.split_cycles = 400000; w.split_heavy = 400000;
    if (K.split_cycles >= 0) w.split_cycles = (uint32_t)K.split_cycles;
    if (K.split_heavy >= 0) w.split_heavy = (uint32_t)K.split_heavy;
    if (!w.split_heavy) w.split_heavy = 0xFFFFFFFFu;
    if (!w.split_cycles || t.n_chunks >= (1u << 20) || sp.n_tiles512 > 4096) w.split_cycles = w.split_heavy = 0xFFFFFFFFu;   // (never; the entry's fields)
    w.split_dense = K.split_dense >= 0 ? (uint32_t)K.split_dense : 0xFFFFFFFFu;
    w.split_many = K.split_many ? ((K.split_many & 0xFFFFu) | (std::max(1u, K.split_many_heavy ? K.split_many_heavy : K.split_many) << 16)) : 0u;
    // LDS holds the hot slots only (the kernel's registers allow 6 waves per SIMD, 13 KB of LDS per wave
    // would stop at 3); the colder ones, touched once per ~1,300 words, go to a small global scratch
    // (lds_slots: fixed when the tree was flattened -- headers touching colder slots are flagged there)
    // The variant with the tile's active-row bitmap in LDS (up to 4 KB of it, i.e. 32,768 sites): a restart of the walk is two
    // memory round trips instead of three, for 3 KB more LDS per wave (13 resident waves per CU instead of 17).  Measured:
    // k_best8 4.52 -> 4.09 ms at 65,536 samples, where the launch is long enough to be bound by its throughput; 1.87 -> 1.97 ms
    // at 16,384, where the tail of the launch and the number of resident waves matter more.  Hence: from 64 tiles on.
    // (not when two calls share the device: the grids are halved then, and the LDS is better spent on resident waves --
    // 65,536 samples per call, pipelined: 10.5 M/s with, 11.0 M/s without)
    w.lds_bits = sp.lds_bits_plan;   // (decided in front of the tile build, with the third bound)
    // Batches with thousands of N cells per sample (their tiles come from the N masks: nmi >= 0): every site row of every tile is
    // live, the bitmap says "fetch the row" for every word -- the variant without a bitmap saves each restart a dependent round
    // trip and each group a load (round 5; exact for any batch: a site's own row is always right, the constant row is the shortcut)
    // (nmi >= 0: lds_bits_plan == 2)
    w.lds_bytes = (size_t)t.lds_slots * 64 * 16 + (w.lds_bits == 1 ? (((size_t)cp.active_words * 4 + 15) & ~(size_t)15) : 0);
    w.b3 = sp.b3_want && w.bounds && w.lds_bits != 1;
    w.variant = c.coarse_only ? (w.lds_bits == 2 ? 4 : 2) : (w.b3 ? (w.lds_bits == 2 ? 6 : 5) : (w.lds_bits == 2 ? 3 : (w.lds_bits ? 1 : 0)));
    return w;
}

// persistent grid: as many one-wave blocks as the device keeps resident (cached per handle and LDS
// size), never more than there are units; the cold-slot scratch is sized for exactly that grid
struct GridPlan { int waves_cu = 1; uint64_t blocks = 8; };
inline GridPlan plan_grid(const PlanTree &t, const Knobs &K, const PlanCall &c, const CallPlan &cp, const SubPlan &sp, int occ_per_cu, int n_cu) {
    GridPlan g;
    g.waves_cu = std::max(occ_per_cu, 1);
    // Two calls on the device (ugp_place_device, the other set's call still running when this one is queued): each walk
    // takes half of what the device keeps resident, so that both grids ARE resident instead of one waiting for the other's
    // waves to exit -- measured at 16,384 samples per call: 2.71 -> 2.29 ms per call (6.05 -> 7.2 M placements/s), best at
    // 8 of the 17 waves per CU of that time (7: 2.32, 9: 2.39, 12: 2.51); with 16 resident since the B halves moved into registers, 8 again (6: 1.85, 8: 1.75, 10: 1.86 ms).  A call that finds the device to itself keeps the full grid.
    // (end of round 6, measured again with the smaller helpers, interleaved A/Bs in profiles/r06_ab_shared*.txt: a caller that keeps
    // THREE short calls in flight does best with 5 of the 16 slots per walk whatever the number of walks found running at the
    // moment -- 14.1-14.5 M/s against 13.6 with the share recomputed per call (5 or 8), 13.9 with 6, 13.8 with 4 or 7; the
    // SARS-CoV-2 shape 12.6 against 12.3.  Callers of long calls -- two sets: 65 536 samples, hundreds of rows per sample -- keep
    // half of the slots: 6.8 M/s against 5.8 with 5 on config 5.)
    if (c.sharing) g.waves_cu = std::max(1, K.shared_waves ? (int)K.shared_waves : (c.share_sets >= 3 ? g.waves_cu * 5 / 16 : g.waves_cu / 2));
    // (round 6) A lone call of a short, plain batch fills three quarters of the slots: with every slot taken more waves wait for
    // work at the end of the launch, every waiting wave makes a running one cut its unit, and every piece replays a preamble --
    // measured alone (profiles/r06_sweep_lone_waves.txt), 16 -> 12 waves per CU: 0.98 -> 0.89 ms at 16 384 x 10 M, 0.92 -> 0.77 at
    // 4 096, 0.76 -> 0.67 at 1 M nodes; batches of hundreds of rows per sample, 65 536 samples and the polytomy shape gain nothing or lose.
    else if (!c.coarse_only && cp.sorted && sp.b3_class == 0 && sp.n_tiles512 <= 32 && !t.wide_descent && g.waves_cu >= 16) g.waves_cu = g.waves_cu * 3 / 4;
    if (K.waves_per_cu) g.waves_cu = std::max(1, std::min(std::max(occ_per_cu, 1), (int)K.waves_per_cu));   // tuning
    g.blocks = (uint64_t)g.waves_cu * std::max(n_cu, 1);
    g.blocks = std::min<uint64_t>(g.blocks, (uint64_t)sp.n_tiles512 * sp.G);
    g.blocks = ((g.blocks + 7) / 8) * 8;
    return g;
}

// ---- the pipeline of overlapped calls -------------------------------------------------------------------------------------
constexpr int kMaxSets = 4;   // workspace sets per handle = calls of ugp_place_device_overlapped that can be on the device at a time
inline int pipeline_depth(const Knobs &K) { return std::max(2, std::min(kMaxSets, (int)K.depth)); }
// Long calls gain nothing from a third batch on the device (measured: 65,536 samples per call 17.4 M/s with two, 16.9 with three;
// thousands of N rows per sample 3.1 against 2.9), short ones do (16,384: 10.2 -> 11.3; 1,024 on a 100k-node tree 5.7 -> 6.8):
// they cycle through two of the handle's sets.  The ordering promise is the handle's (depth - 1 calls of lag) either way.
inline int sets_in_use(const Knobs &K, uint64_t n_queries, uint64_t n_rows) {
    return (n_queries > 32768 || n_rows > n_queries * 128) ? 2 : pipeline_depth(K);
}

}  // namespace ugp
