"""The host decisions of a placement call (usher_amd/csrc/ugp_plan.hpp) on the CPU.  Results never depend on which path runs, so
no oracle test can see a wrong decision: it only costs speed.  A small C++ driver fills the plan's input structs from `name=value`
arguments, calls the plan functions the way run_place does and prints every field.

Every expected value below is worked out by hand from the expressions run_place had before the split (the arithmetic stands
beside it); none was obtained by running the header."""
import functools
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "ugp_plan.hpp"
static std::map<std::string, long long> A;
static long long get(const char *k, long long d) { auto it = A.find(k); return it == A.end() ? d : it->second; }
#define P(name, v) printf("%s=%lld\n", name, (long long)(v))
int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) { const char *e = strchr(argv[i], '='); if (!e) return 2; A[std::string(argv[i], e - argv[i])] = atoll(e + 1); }
    if (get("caps", 0)) {   // unit_caps alone
        const ugp::UnitCaps u = ugp::unit_caps((uint32_t)get("n_chunks", 0), (uint32_t)get("unit_chunks", 16), (uint32_t)get("heavy_chunks", 16),
                                               (uint32_t)get("grow_every", 0), (uint32_t)get("unit_max", 256));
        P("n_side", u.n_side); P("per_tile_cap", u.per_tile_cap);
        return 0;
    }
    ugp::Knobs K;
    if (get("pipe", 0)) {   // the pipeline helpers alone
        K.depth = (uint32_t)get("K_depth", K.depth);
        P("depth", ugp::pipeline_depth(K)); P("sets", ugp::sets_in_use(K, (uint64_t)get("Q", 0), (uint64_t)get("rows", 0)));
        return 0;
    }
    ugp::PlanTree t;
    t.n_nodes = get("n_nodes", 10000000); t.n_sites = get("n_sites", 500); t.n_chunks = (uint32_t)get("n_chunks", 100);
    t.max_chunk8_words = (uint32_t)get("max_chunk8_words", 1000); t.max_path_muts = (uint32_t)get("max_path_muts", 100);
    t.lds_slots = (uint32_t)get("lds_slots", 4); t.mask_not_first = get("mask_not_first", 0); t.coarse = get("coarse", 1);
    t.b3_events = get("b3_events", 1); t.wide_descent = get("wide_descent", 0);
    ugp::PlanCall c;
    c.Q = get("Q", 16384); c.max_rows = get("max_rows", 50); c.mode = (int)get("mode", 0); c.coarse_only = get("coarse_only", 0);
    c.ties = get("ties", 0); c.nmask = get("nmask", 0); c.sharing = get("sharing", 0); c.share_sets = (int)get("share_sets", 2);
    c.ex.given = get("ex_given", 0); c.ex.packed = get("ex_packed", 0); c.ex.mask = get("ex_mask", 0); c.ex.skip = get("ex_skip", 0);
    c.ex.skip_chunk = get("ex_skip_chunk", 0); c.ex.scores = get("ex_scores", 0);
    K.force_v1 = get("K_force_v1", 0); K.no_sort = get("K_no_sort", 0); K.no_prune = get("K_no_prune", 0); K.no_lpt = get("K_no_lpt", 0);
    K.no_fork = get("K_no_fork", 1); K.no_bound3 = get("K_no_bound3", 0); K.no_uniq = get("K_no_uniq", 0); K.no_pad_fix = get("K_no_pad_fix", 0);
    K.stats = get("K_stats", 0); K.bound3 = (int)get("K_bound3", 1); K.tile_build = (int)get("K_tile_build", -1); K.lds_bits = (int)get("K_lds_bits", -1);
    K.light_order = (int)get("K_light_order", -1); K.unit_grow = (int)get("K_unit_grow", -1); K.split_cycles = (int)get("K_split_cycles", -1);
    K.split_heavy = (int)get("K_split_heavy", K.split_cycles);   // (UGP_SPLIT_CYCLES sets both, as Knobs::from_env)
    K.groups = (uint32_t)get("K_groups", 0); K.lbest_gib = (uint32_t)get("K_lbest_gib", 0); K.unit_chunks = (uint32_t)get("K_unit_chunks", 0);
    K.unit_max = (uint32_t)get("K_unit_max", 0); K.heavy_chunks = (uint32_t)get("K_heavy_chunks", 0); K.ub_every = (uint32_t)get("K_ub_every", 0);
    K.waves_per_cu = (uint32_t)get("K_waves_per_cu", 0); K.shared_waves = (uint32_t)get("K_shared_waves", 0);
    const ugp::CallPlan cp = ugp::plan_call(t, K, c);
    P("n_sites", cp.n_sites); P("active_words", cp.active_words); P("useful_words", cp.useful_words); P("ex_packable", cp.ex_packable);
    P("ex_skip_used", cp.ex_skip); P("packed_ok", cp.packed_ok); P("sorted", cp.sorted); P("can_fork", cp.can_fork); P("fill_ahead", cp.fill_ahead);
    P("sub_tiles", cp.sub_tiles);
    const uint64_t nq = (uint64_t)get("nq", (long long)std::min<uint64_t>(c.Q, cp.sub_tiles * 64));
    ugp::SubPlan sp = ugp::plan_sub(t, K, c, cp, nq, (uint64_t)get("rows", (long long)(10 * nq)));
    P("b3_static_or_pinned", sp.b3_want);
    if (sp.b3_tuned && get("tuner_says", -1) >= 0) sp.b3_want = get("tuner_says", -1) != 0;
    P("n_tiles", sp.n_tiles); P("n_tiles512", sp.n_tiles512); P("G", sp.G); P("sub_nmask", sp.nmask); P("lds_build", sp.lds_build);
    P("lds_bits_plan", sp.lds_bits_plan); P("b3_can", sp.b3_can); P("b3_tuned", sp.b3_tuned); P("b3_want", sp.b3_want); P("b3_class", sp.b3_class);
    P("uniq_ok", sp.uniq_ok);
    const ugp::ZeroLayout z = ugp::zero_layout(sp.n_tiles512, cp.active_words, cp.useful_words, sp.b3_want);
    P("z_dbottom", z.z_dbottom); P("z_active", z.z_active); P("z_queue", z.z_queue); P("z_list_n", z.z_list_n); P("z_nitems", z.z_nitems);
    P("z_cnt", z.z_cnt); P("z_key", z.z_key); P("z_useful", z.z_useful); P("z_end", z.z_end);
    P("pad_d", ugp::seed_pad_d(t, K));
    if (!cp.packed_ok) return 0;
    const ugp::WalkPlan w = ugp::plan_walk(t, K, c, cp, sp);
    P("tile_ranges", w.tile_ranges); P("bounds", w.bounds); P("unit_chunks", w.unit_chunks); P("heavy_chunks", w.heavy_chunks);
    P("light_order", w.light_order); P("grow_every", w.grow_every); P("unit_max", w.unit_max); P("no_pre_records", w.no_pre_records);
    P("n_side", w.n_side); P("per_tile_cap", w.per_tile_cap); P("split_cycles", w.split_cycles); P("split_heavy", w.split_heavy);
    P("split_dense", w.split_dense); P("split_many", w.split_many); P("ub_every", w.ub_every); P("lds_bits", w.lds_bits); P("lds_bytes", w.lds_bytes);
    P("b3", w.b3); P("variant", w.variant);
    const ugp::GridPlan g = ugp::plan_grid(t, K, c, cp, sp, (int)get("occ", 16), (int)get("n_cu", 256));
    P("waves_cu", g.waves_cu); P("blocks", g.blocks);
    return 0;
}
"""


@functools.lru_cache(None)
def _exe():
    d = tempfile.mkdtemp(prefix="ugp_plan_")
    src, exe = os.path.join(d, "plan_driver.cpp"), os.path.join(d, "plan_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "usher_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    return exe


def _plan(**kw):
    """Defaults: a 10M-node tree of 100 chunks and 500 sites with a coarse tree and posting lists; a plain call of 16,384 samples with
    10 rows each, alone on the device; UGP_BOUND3=1, no other knob."""
    r = subprocess.run([_exe()] + ["%s=%d" % (k, int(v)) for k, v in kw.items()], capture_output=True, text=True, check=True)
    return {k: int(v) for k, v in (line.split("=") for line in r.stdout.split())}


F32 = 0xFFFFFFFF


def test_groups():
    # packed: G = max(1, ceil(n_chunks / 16)), doubled while G < n_chunks and G * T < 4096 (capped at n_chunks), then UGP_GROUPS
    assert _plan(n_chunks=100, Q=512)["G"] == 100          # T=1: ceil(100/16)=7 -> 14 -> 28 -> 56 -> min(100, 112)=100; 100 is not < n_chunks
    assert _plan(n_chunks=40000, Q=16384)["G"] == 2500     # T=32: ceil(40000/16)=2500; 2500*32=80000 >= 4096
    assert _plan(n_chunks=40000, Q=512)["G"] == 5000       # T=1: 2500*1 < 4096 -> 5000; 5000 >= 4096
    assert _plan(n_chunks=100, K_groups=3)["G"] == 3                 # min(n_chunks, UGP_GROUPS)
    assert _plan(n_chunks=100, K_groups=1 << 20)["G"] == 100
    # not packed (pick_groups): ceil(4096 / n_tiles), at most n_chunks, at least 1, from 8 on a multiple of 8
    p = _plan(n_chunks=100, Q=1300, K_force_v1=1)
    assert p["packed_ok"] == 0 and p["n_tiles"] == 21      # ceil(1300/64) = 21
    assert p["G"] == 96                                    # ceil(4096/21)=196 -> min(196, 100)=100 -> 100 & ~7 = 96
    assert _plan(n_chunks=5, Q=1300, K_force_v1=1)["G"] == 5         # below 8: as it is


def test_tiles():
    p = _plan(Q=1300)
    assert (p["n_tiles"], p["n_tiles512"]) == (21, 3)      # ceil(1300/64), ceil(1300/512)
    p = _plan(Q=512)
    assert (p["n_tiles"], p["n_tiles512"]) == (8, 1)


def test_sub_tiles():
    # min(4096, max(8, ((GiB << 30) / (n_chunks * 128)) & ~7)); GiB = 24 unless UGP_LBEST_GIB; `/` binds tighter than `&`
    assert _plan(n_chunks=0)["sub_tiles"] == 4096                        # no chunks: the cap alone
    assert _plan(n_chunks=100)["sub_tiles"] == 4096                      # 24*2^30 / 12800 = 2,013,265 -> min with 4096
    assert _plan(n_chunks=1 << 20)["sub_tiles"] == 192                   # 24*2^30 / 2^27 = 192; 192 & ~7 = 192
    assert _plan(n_chunks=1 << 20, K_lbest_gib=1)["sub_tiles"] == 8      # 2^30 / 2^27 = 8
    assert _plan(n_chunks=1 << 21, K_lbest_gib=1)["sub_tiles"] == 8      # 2^30 / 2^28 = 4; 4 & ~7 = 0; max(8, 0) = 8


def test_sorted():
    assert _plan(Q=512)["sorted"] == 0           # Q > 512
    assert _plan(Q=513)["sorted"] == 1
    assert _plan(Q=513, coarse=0)["sorted"] == 0
    assert _plan(Q=513, K_no_sort=1)["sorted"] == 0
    assert _plan(Q=513, K_no_prune=1)["sorted"] == 0
    p = _plan(Q=513, K_force_v1=1)
    assert p["packed_ok"] == 0 and p["sorted"] == 0


def test_packed_ok():
    # max_rows + max_path_muts + 2 < 0x7F7F; max_path_muts = 100, so max_rows = 0x7F7E - 102 = 32536 gives 0x7F7E
    assert 32536 + 100 + 2 == 0x7F7E
    assert _plan(max_rows=32536)["packed_ok"] == 1
    assert _plan(max_rows=32537)["packed_ok"] == 0      # the sum is 0x7F7F
    assert _plan(mode=1)["packed_ok"] == 0
    assert _plan(mode=2)["packed_ok"] == 0
    assert _plan(mask_not_first=1)["packed_ok"] == 0
    assert _plan(K_force_v1=1)["packed_ok"] == 0
    # extended searches: packable = arranged by the caller, no mask left, a skip only with its chunks, no scores
    assert _plan(ex_given=1)["packed_ok"] == 0                                               # not arranged for
    assert _plan(ex_given=1, ex_packed=1)["packed_ok"] == 1
    assert _plan(ex_given=1, ex_packed=1, ex_mask=1)["packed_ok"] == 0
    assert _plan(ex_given=1, ex_packed=1, ex_skip=1)["packed_ok"] == 0
    assert _plan(ex_given=1, ex_packed=1, ex_scores=1)["packed_ok"] == 0
    p = _plan(ex_given=1, ex_packed=1, ex_skip=1, ex_skip_chunk=1)
    assert (p["ex_packable"], p["packed_ok"], p["ex_skip_used"]) == (1, 1, 1)
    assert _plan(ex_given=1, ex_packed=1)["ex_skip_used"] == 0


def test_fork_and_fill_ahead():
    # can_fork = sorted && !coarse_only && !no_fork && !sharing; the fork is opt-in (no_fork is true unless UGP_FORK)
    assert _plan()["can_fork"] == 0
    p = _plan(K_no_fork=0)
    assert (p["can_fork"], p["fill_ahead"]) == (1, 1)
    assert _plan(K_no_fork=0, sharing=1)["can_fork"] == 0
    assert _plan(K_no_fork=0, coarse_only=1)["can_fork"] == 0
    assert _plan(K_no_fork=0, Q=512)["can_fork"] == 0                    # not sorted
    # fill_ahead: no N masks, UGP_TILE_BUILD <= 0, the tree has sites, and the call is one sub-batch of at most 4096 * 64 samples
    assert _plan(K_no_fork=0, nmask=1)["fill_ahead"] == 0
    assert _plan(K_no_fork=0, K_tile_build=1)["fill_ahead"] == 0
    assert _plan(K_no_fork=0, K_tile_build=0)["fill_ahead"] == 1
    assert _plan(K_no_fork=0, n_sites=0)["fill_ahead"] == 0
    assert _plan(K_no_fork=0, Q=262144)["fill_ahead"] == 1
    assert _plan(K_no_fork=0, Q=262145)["fill_ahead"] == 0


def test_sites():
    p = _plan(n_sites=0)
    assert (p["n_sites"], p["active_words"], p["useful_words"]) == (1, 1, 1)      # at least one row
    p = _plan(n_sites=500)
    assert (p["n_sites"], p["active_words"], p["useful_words"]) == (500, 16, 63)  # ceil(500/32), ceil(500/8)


def test_lds_bits_plan():
    # 1 when: no stats, the bitmap (active_words * 4 bytes) fits 4096, T >= 64, not sharing; 2 with N masks; UGP_LDS_BITS pins
    assert _plan(Q=63 * 512)["lds_bits_plan"] == 0
    assert _plan(Q=64 * 512)["lds_bits_plan"] == 1
    assert _plan(Q=64 * 512, sharing=1)["lds_bits_plan"] == 0
    assert _plan(Q=64 * 512, n_sites=32768)["lds_bits_plan"] == 1      # 1024 words = 4096 bytes
    assert _plan(Q=64 * 512, n_sites=32769)["lds_bits_plan"] == 0      # 1025 words = 4100 bytes
    assert _plan(nmask=1)["lds_bits_plan"] == 2
    assert _plan(Q=64 * 512, K_lds_bits=0)["lds_bits_plan"] == 0
    assert _plan(K_lds_bits=1)["lds_bits_plan"] == 1                   # (whatever T)
    assert _plan(K_lds_bits=1, n_sites=32769)["lds_bits_plan"] == 0    # ... but only a bitmap that fits
    assert _plan(K_lds_bits=2)["lds_bits_plan"] == 2
    assert _plan(Q=64 * 512, K_stats=1)["lds_bits_plan"] == 0
    assert _plan(nmask=1, K_stats=1)["lds_bits_plan"] == 0
    assert _plan(K_lds_bits=2, K_stats=1)["lds_bits_plan"] == 0
    assert _plan(Q=64 * 512, K_force_v1=1)["lds_bits_plan"] == 0       # not packed


def test_b3_can():
    # 40,000 sites: the bitmap does not fit LDS, so lds_bits_plan stays 0 at any T
    assert _plan(Q=256 * 512, n_sites=40000)["b3_can"] == 1
    assert _plan(Q=256 * 512 + 1, n_sites=40000)["b3_can"] == 0        # T = 257
    p = _plan(Q=64 * 512)                                              # 500 sites, T = 64: lds_bits_plan == 1
    assert (p["lds_bits_plan"], p["b3_can"]) == (1, 0)
    assert _plan(Q=64 * 512, n_sites=40000)["b3_can"] == 1
    # (on a sorted batch lds_build is true only through UGP_TILE_BUILD=1, which rules the third bound out by itself: the term
    # `!(lds_build && !nmask)` cannot be reached alone through plan_sub's inputs, and this one case covers both)
    p = _plan(K_tile_build=1)
    assert (p["lds_build"], p["b3_can"]) == (1, 0)
    assert _plan(K_tile_build=0)["b3_can"] == 1
    assert _plan(Q=512)["b3_can"] == 0                                 # not sorted
    assert _plan(coarse_only=1)["b3_can"] == 0
    assert _plan(b3_events=0)["b3_can"] == 0
    assert _plan(K_no_bound3=1)["b3_can"] == 0
    assert _plan(K_bound3=0)["b3_can"] == 0
    assert _plan(nmask=1)["b3_can"] == 1                               # lds_bits_plan == 2 has a third-bound variant


def test_b3_mode():
    # pinned (1): want = can; unset (-2): b3_static_choice(wide_descent, class, n_nodes); auto (-1): the tuner's answer
    p = _plan(K_bound3=1)
    assert (p["b3_tuned"], p["b3_want"]) == (0, 1)
    assert _plan(K_bound3=-2, n_nodes=10000000)["b3_want"] == 1        # class 0, no polytomies: n_nodes >= 3,000,000
    assert _plan(K_bound3=-2, n_nodes=1000000)["b3_want"] == 0
    assert _plan(K_bound3=-2, n_nodes=10000000, wide_descent=1)["b3_want"] == 0
    p = _plan(K_bound3=-2, n_nodes=1000000, rows=256 * 16384)          # 256 rows per sample: class 2
    assert (p["b3_class"], p["b3_want"]) == (2, 1)
    assert _plan(rows=31 * 16384)["b3_class"] == 0 and _plan(rows=32 * 16384)["b3_class"] == 1
    p = _plan(K_bound3=-1, tuner_says=0)
    assert (p["b3_can"], p["b3_tuned"], p["b3_want"], p["z_end"] - p["z_useful"]) == (1, 1, 0, 0)
    p = _plan(K_bound3=-1, tuner_says=1)
    assert (p["b3_tuned"], p["b3_want"]) == (1, 1)
    assert _plan(K_bound3=-1, Q=512)["b3_tuned"] == 0                  # nothing to tune where it cannot run


def test_lds_build():
    # unsorted batches of at least 128 rows per sample; UGP_TILE_BUILD pins
    assert _plan(Q=512, rows=128 * 512)["lds_build"] == 1
    assert _plan(Q=512, rows=128 * 512 - 1)["lds_build"] == 0
    assert _plan(Q=513, rows=128 * 513)["lds_build"] == 0              # sorted
    assert _plan(Q=513, rows=10, K_tile_build=1)["lds_build"] == 1
    assert _plan(Q=512, rows=128 * 512, K_tile_build=0)["lds_build"] == 0
    assert _plan(Q=512, rows=128 * 512, K_force_v1=1)["lds_build"] == 0   # not packed


def test_uniq_ok():
    assert _plan()["uniq_ok"] == 1
    assert _plan(Q=512)["uniq_ok"] == 0              # not sorted
    assert _plan(ties=1)["uniq_ok"] == 0
    assert _plan(ex_given=1, ex_packed=1)["uniq_ok"] == 0
    assert _plan(coarse_only=1)["uniq_ok"] == 0
    assert _plan(n_nodes=(1 << 31) - 1)["uniq_ok"] == 1
    assert _plan(n_nodes=1 << 31)["uniq_ok"] == 0
    assert _plan(K_no_uniq=1)["uniq_ok"] == 0


def test_zero_layout():
    # T=3, 500 sites: active_words=16, useful_words=63
    want = dict(z_dbottom=0,
                z_active=1536,       # 3 * 512
                z_queue=1584,        # + 3 * 16
                z_list_n=1592,       # + 8
                z_nitems=1595,       # + 3
                z_cnt=1603,          # + 8
                z_key=3139,          # + 3 * 512
                z_useful=4675)       # + 3 * 512
    p = _plan(Q=1300, K_bound3=0)
    assert {k: p[k] for k in want} == want and p["z_end"] == 4675
    p = _plan(Q=1300, K_bound3=1)
    assert {k: p[k] for k in want} == want and p["z_end"] == 4864      # + 3 * 63


def test_pad_d():
    assert _plan(max_path_muts=100)["pad_d"] == 4096                   # min(4096, 0x7F7E - 2 - 100)
    assert _plan(max_path_muts=0x7F00, max_rows=0)["pad_d"] == 124     # 0x7F7C - 0x7F00
    assert _plan(max_path_muts=0x7F70, max_rows=0)["pad_d"] == 124     # (the path length is capped at 0x7F00)
    assert _plan(K_no_pad_fix=1)["pad_d"] == 0


def _caps(**kw):
    return _plan(caps=1, **kw)


def test_unit_counts():
    # n_side: units of len_of(i) chunks until n_chunks are covered; per_tile_cap = ceil(n_chunks / heavy_chunks) + 2 * n_side + 2
    p = _caps(n_chunks=100, unit_chunks=16, heavy_chunks=16, grow_every=0)
    assert (p["n_side"], p["per_tile_cap"]) == (7, 23)                 # ceil(100/16)=7; 7 + 14 + 2
    # growth every 8 up to 256: 8 x 16, 8 x 32, 8 x 64, 8 x 128 = 1920 chunks in 32 units, then ceil(38080 / 256) = 149 more
    p = _caps(n_chunks=40000, unit_chunks=16, heavy_chunks=16, grow_every=8, unit_max=256)
    assert (p["n_side"], p["per_tile_cap"]) == (181, 2864)             # 2500 + 362 + 2
    # the same through the walk's plan: 16,384 sorted samples (T=32) of a 40,000-chunk tree
    p = _plan(n_chunks=40000)
    assert (p["G"], p["tile_ranges"], p["unit_chunks"], p["grow_every"], p["unit_max"]) == (2500, 1, 16, 8, 256)
    assert (p["n_side"], p["per_tile_cap"]) == (181, 2864)
    p = _plan(n_chunks=40000, K_no_lpt=1)                              # no regions: no growth
    assert (p["tile_ranges"], p["grow_every"], p["n_side"]) == (0, 0, 2500)
    p = _plan(n_chunks=40000, Q=512)                                   # unsorted: G=5000, units of 8
    assert (p["tile_ranges"], p["unit_chunks"], p["grow_every"], p["unit_max"]) == (0, 8, 0, 128)
    assert _plan(n_chunks=40000, K_unit_grow=3)["grow_every"] == 3
    assert _plan(n_chunks=40000, K_no_prune=1)["grow_every"] == 0      # (unsorted, and no bounds)
    # a unit stays below the reach of a preamble's jump field: INFO_JUMP_MASK - 1 = 2^18 - 2 words
    p = _plan(n_chunks=40000, max_chunk8_words=2000)
    assert (p["unit_max"], p["no_pre_records"]) == (131, 0)            # 262142 / 2000 = 131; 16 * 2000 <= 262142
    p = _plan(n_chunks=40000, max_chunk8_words=20000)
    assert (p["unit_max"], p["no_pre_records"]) == (16, 1)             # 262142 / 20000 = 13 -> not below unit_chunks; 16 * 20000 > 262142
    assert _plan(n_chunks=40000, K_unit_max=64)["unit_max"] == 64


def test_splits_and_small_walk_fields():
    p = _plan()
    assert (p["split_cycles"], p["split_heavy"], p["split_dense"]) == (400000, 400000, F32)
    assert p["split_many"] == (4 | (2 << 16))                          # UGP_SPLIT_MANY=4, UGP_SPLIT_MANY_HEAVY=2
    assert (p["ub_every"], p["heavy_chunks"], p["light_order"], p["bounds"]) == (128, 16, 0, 1)
    p = _plan(n_chunks=1 << 20)
    assert (p["split_cycles"], p["split_heavy"]) == (F32, F32)
    p = _plan(nq=4097 * 512)                                           # T > 4096
    assert p["n_tiles512"] == 4097 and (p["split_cycles"], p["split_heavy"]) == (F32, F32)
    assert _plan(nq=4096 * 512)["split_cycles"] == 400000
    p = _plan(K_split_cycles=0)
    assert (p["split_cycles"], p["split_heavy"]) == (F32, F32)
    p = _plan(K_split_cycles=7, K_split_heavy=0)                       # heavy 0 alone: never for the heavy units
    assert (p["split_cycles"], p["split_heavy"]) == (7, F32)
    assert _plan(K_ub_every=5)["ub_every"] == 5
    assert _plan(K_heavy_chunks=3)["heavy_chunks"] == 3
    assert _plan(wide_descent=1)["light_order"] == 1
    assert _plan(wide_descent=1, K_light_order=0)["light_order"] == 0
    assert _plan(K_no_prune=1)["bounds"] == 0


def test_variant_and_lds_bytes():
    # (coarse_only, third bound on, lds_bits) -> the kernel
    assert _plan(K_bound3=0)["variant"] == 0
    p = _plan(K_bound3=0, Q=64 * 512)
    assert (p["lds_bits"], p["variant"]) == (1, 1)
    assert p["lds_bytes"] == 4 * 1024 + 64                             # 4 slots x 64 lanes x 16 bytes + 16 words of bitmap
    assert _plan(coarse_only=1)["variant"] == 2
    assert _plan(K_bound3=0, nmask=1)["variant"] == 3
    assert _plan(coarse_only=1, nmask=1)["variant"] == 4
    p = _plan(K_bound3=1)
    assert (p["b3"], p["variant"], p["lds_bytes"]) == (1, 5, 4096)
    assert _plan(K_bound3=1, nmask=1)["variant"] == 6
    p = _plan(K_bound3=1, K_no_prune=1)                                # no bounds (and no sort): no third bound
    assert (p["b3"], p["variant"]) == (0, 0)
    assert _plan(coarse_only=1, Q=64 * 512)["variant"] == 2            # (the coarse pass has no variant with the bitmap in LDS)


def test_grid():
    # sharing: 5/16 of the resident waves for callers cycling through 3 sets, half for 2
    assert _plan(occ=16, sharing=1, share_sets=3)["waves_cu"] == 5     # 16 * 5 / 16
    assert _plan(occ=16, sharing=1, share_sets=2)["waves_cu"] == 8
    assert _plan(occ=17, sharing=1, share_sets=3)["waves_cu"] == 5     # 85 / 16
    assert _plan(occ=16, sharing=1, share_sets=3, K_shared_waves=7)["waves_cu"] == 7
    # a lone, sorted, plain (class 0) call of at most 32 tiles on a tree without large polytomies, 16 or more resident: 3/4
    assert _plan(occ=16, Q=32 * 512)["waves_cu"] == 12
    assert _plan(occ=16, Q=32 * 512 + 1)["waves_cu"] == 16             # T = 33
    assert _plan(occ=15, Q=32 * 512)["waves_cu"] == 15
    assert _plan(occ=16, Q=32 * 512, wide_descent=1)["waves_cu"] == 16
    assert _plan(occ=16, Q=32 * 512, rows=32 * 32 * 512)["waves_cu"] == 16   # class 1
    assert _plan(occ=16, Q=32 * 512, coarse_only=1)["waves_cu"] == 16
    assert _plan(occ=16, Q=512)["waves_cu"] == 16                      # not sorted
    assert _plan(occ=16, K_waves_per_cu=2)["waves_cu"] == 2
    assert _plan(occ=16, K_waves_per_cu=40)["waves_cu"] == 16          # never above the occupancy
    assert _plan(occ=0)["waves_cu"] == 1
    # blocks = min(waves * CUs, T * G), rounded up to a multiple of 8
    assert _plan(occ=16, n_cu=256, Q=32 * 512, n_chunks=40000)["blocks"] == 3072   # 12 * 256 = 3072 <= 32 * 2500
    assert _plan(occ=16, n_cu=256, Q=512, n_chunks=100)["blocks"] == 104           # min(16 * 256, 1 * 100) = 100 -> 104


def test_pipeline_depth_and_sets():
    # depth = UGP_PIPELINE_DEPTH within 2..4 (default 3); more than 32,768 samples or more than 128 rows per sample: 2 sets
    assert _plan(pipe=1)["depth"] == 3
    assert _plan(pipe=1, K_depth=1)["depth"] == 2 and _plan(pipe=1, K_depth=9)["depth"] == 4
    assert _plan(pipe=1, Q=32768, rows=32768 * 128)["sets"] == 3
    assert _plan(pipe=1, Q=32769, rows=10)["sets"] == 2
    assert _plan(pipe=1, Q=100, rows=100 * 128 + 1)["sets"] == 2
    assert _plan(pipe=1, Q=100, rows=100, K_depth=4)["sets"] == 4
