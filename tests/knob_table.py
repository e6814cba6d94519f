"""Every UGP_* environment variable the library reads, with how the suite covers it (plain data; imports nothing).

KNOBS[name] = (class, reason):
- "grid": tests/test_knobs_gpu.py runs it against the oracle, with the values the reason names;
- "tested:<file>": the test file of that name (under tests/) runs it;
- "diagnostic": it only prints, or writes a side file; results do not pass through it.

FLATTEN[name]: the knob is read while a tree is flattened (a flat file of ugp_flat_save carries its effect).  The value is
"signature" when flat_signature() (ugp_capi.cpp) hashes it, so that a file written under another value is refused; otherwise
it says why a file written without the knob stays correct.

tests/test_knob_inventory.py checks this table against the sources and the test files.
"""

KNOBS = {
    # ---- seeds: the descent from the coarse winner and the bounds it hands to the walk
    "UGP_DESCENT_LANES": ("grid", "k_descend<16> / k_descend<64>: 16 and 64 on a deep random tree (A) and on a tree of polytomies (B)"),
    "UGP_DESCENT_MAX": ("grid", "expansions of the seed descent: 1, 2, 4096"),
    "UGP_DESCENT_SLACK": ("grid", "widening of the seed descent: 0, 1, 40"),
    "UGP_LIGHT_ORDER": ("grid", "k_build_units light-unit order: 0 and 1 on A and B"),
    "UGP_NO_PAD_FIX": ("grid", "no D(bottom) padding of the last tile: batches of 1, 513 and 1,300 samples"),
    "UGP_NO_SEED": ("tested:test_gpu_parity.py", "walk without seeded upper bounds"),
    "UGP_NO_DESCENT": ("tested:test_gpu_parity.py", "seeds from the coarse pass only"),
    "UGP_SEED_PREV": ("grid", "experiments build: bounds from the previous call's answers, one query set placed twice"),
    "UGP_SEED_CHECK": ("grid", "experiments build, with UGP_STATS: seeds checked against the previous call's answers"),
    # ---- tiles of the batch
    "UGP_TILE_BUILD": ("grid", "LDS tile builder on or off: 0 and 1 x sorted / unsorted x A / high-ambiguity D x UGP_NMASK x UGP_BOUND3"),
    "UGP_NMASK": ("grid", "tiles from per-sample N bit masks: unset and 1 in the tile-build grid"),
    "UGP_NO_SORT": ("grid", "no locality sort (and no coarse tree): in the tile-build grid"),
    "UGP_NO_PRUNE": ("tested:test_gpu_parity.py", "walk without pruning"),
    "UGP_FORCE_V1": ("tested:test_gpu_parity.py", "the 32-bit one-sample-per-lane kernel"),
    "UGP_RADIX_SORT": ("tested:test_gpu_parity.py", "the device radix sort instead of the counting sort over the coarse nodes"),
    "UGP_LDS_BITS": ("tested:test_gpu_parity.py", "active-row bitmaps of the tiles in LDS"),
    # ---- pruning bounds
    "UGP_BOUND3": ("tested:test_bound3_gpu.py", "third pruning bound: pinned 0 / 1 or tuned at run time"),
    "UGP_NO_BOUND3": ("tested:test_bound3_gpu.py", "a tree flattened without the third bound's posting lists"),
    "UGP_NO_BOUND2": ("tested:test_gpu_parity.py", "first lower bound only"),
    "UGP_PRUNE_MIN_WORDS": ("tested:test_gpu_parity.py", "smallest chunk that carries pruning records"),
    "UGP_PRE_WEIGHT": ("tested:test_gpu_parity.py", "weight of the pre-pass in the unit order"),
    # ---- walk scheduling and units
    "UGP_GROUPS": ("grid", "chunk groups of the walk: 1, 3, 1<<20 (n_groups asserted)"),
    "UGP_TARGET_WAVES": ("grid", "waves the group count aims at: 1, 7"),
    "UGP_WAVES_PER_CU": ("grid", "resident waves per CU of the persistent walk: 1, 2"),
    "UGP_HEAVY_PRIO": ("grid", "heavy units first: 1"),
    "UGP_SPLIT_HEAVY": ("grid", "cut threshold of heavy units: 0, 1 (with UGP_SPLIT_CYCLES=1)"),
    "UGP_SPLIT_DENSE": ("grid", "cut threshold of dense units: 0, 1, 100000 (with UGP_SPLIT_CYCLES=1)"),
    "UGP_REFILL_ALL": ("grid", "every row refilled at a unit's start"),
    "UGP_FORK": ("grid", "side stream of a lone call: on, and on with UGP_NO_FORK"),
    "UGP_NO_FORK": ("grid", "side stream off although UGP_FORK is set"),
    "UGP_SPLIT_CYCLES": ("tested:test_gpu_parity.py", "when a running unit is cut"),
    "UGP_SPLIT_MANY": ("tested:test_gpu_parity.py", "pieces a cut unit is split into"),
    "UGP_SPLIT_MANY_HEAVY": ("tested:test_gpu_parity.py", "pieces a cut unit of the tile's own region is split into"),
    "UGP_UNIT_CHUNKS": ("tested:test_gpu_parity.py", "chunks per work unit"),
    "UGP_HEAVY_CHUNKS": ("tested:test_gpu_parity.py", "chunks per unit of the tile's own region"),
    "UGP_UNIT_GROW": ("tested:test_gpu_parity.py", "unit growth with the distance from the tile's region"),
    "UGP_UNIT_MAX": ("tested:test_gpu_parity.py", "largest unit"),
    "UGP_UB_EVERY": ("tested:test_gpu_parity.py", "period of the upper-bound exchange"),
    "UGP_NO_LPT": ("tested:test_gpu_parity.py", "no longest-first scheduling"),
    "UGP_KBEST_EXCLUSIVE": ("grid", "experiments build: exclusive k-best merge"),
    "UGP_STATS": ("grid", "experiments build: walk counters (and lds_bits forced to 0)"),
    # ---- phase 2, ties, scores
    "UGP_NO_UNIQ": ("tested:test_phase2_uniq_gpu.py", "phase 2 without the unique-sample shortcut"),
    "UGP_PHASE2_PACKED": ("tested:test_gpu_parity.py", "experiments build: phase 2 as a mode of the packed walk"),
    "UGP_TIES_DFS": ("tested:test_gpu_parity.py", "tie lists from the full one-sample-per-lane walk"),
    "UGP_SCORES_DFS": ("tested:test_gpu_parity.py", "per-node scores by the depth-first walk"),
    "UGP_SCORES_BLOCK": ("grid", "k_scores_level block size: 10, 64, 100, 128, 1000, 1024, 5000"),
    "UGP_EX_SLOW": ("tested:test_other_callers.py", "extended searches on the one-sample-per-lane kernel"),
    # ---- sub-batches and the pipeline of overlapped calls
    "UGP_LBEST_GIB": ("grid", "sub-batch cap: 1 on a 1M-node tree of many chunks (three sub-batches and more)"),
    "UGP_PIPELINE_DEPTH": ("grid", "workspace sets of overlapped calls: 2 and 4, and 1 / 9 clamped"),
    "UGP_SHARED_WAVES": ("grid", "wave budget while sets share the device: 1, 3"),
    # ---- coarse tree of the locality sort
    "UGP_COARSE_MIN_NODES": ("tested:test_gpu_parity.py", "smallest tree with a coarse tree"),
    "UGP_COARSE_DIV": ("grid", "coarse tree size divisor: 2, 1000"),
    "UGP_COARSE_FLOOR": ("grid", "coarse tree size floor: 16, 100000"),
    "UGP_COARSE_CHUNK_NODES": ("grid", "chunk size of the coarse tree: 1, 7"),
    "UGP_COARSE_PHASE2": ("tested:test_gpu_parity.py", "the coarse pass with its full phase 2"),
    # ---- flattening
    "UGP_CHUNK_NODES": ("tested:test_multi_gpu.py", "nodes per chunk"),
    "UGP_LDS_SLOTS": ("tested:test_gpu_parity.py", "hot slots kept in LDS"),
    "UGP_NO_SIB": ("grid", "flattening without sibling records: place, ties and per-node scores on A and B"),
    "UGP_NO_UPDATE_MAPS": ("grid", "a handle without the add-mode maps: exact placements, update() fails with UGP_ERR_UNSUPPORTED"),
    "UGP_FLATTEN_THREADS": ("tested:test_flatten_cpu.py", "host threads of the flattening"),
    "UGP_FLATTEN_GRAIN": ("tested:test_flatten_cpu.py", "work grain of the flattening's host threads"),
    "UGP_FLATTEN_VERBOSE": ("diagnostic", "prints the flattening's timings to stderr"),
    # ---- add mode, Fitch, RIPPLES
    "UGP_TOUCHED_RECS": ("grid", "records per block of the touched-node kernel: 1, 64 (one child process each)"),
    "UGP_FITCH_BYTES": ("tested:test_fitch.py", "device budget of the Fitch-Sankoff pass"),
    "UGP_FITCH_PIECES": ("tested:test_fitch.py", "pieces of a Fitch-Sankoff launch"),
    "UGP_FITCH_EMIT_CAP": ("tested:test_fitch.py", "segment capacity of the emitted mutations"),
    "UGP_FITCH_VERBOSE": ("diagnostic", "prints the Fitch-Sankoff pass's plan to stderr"),
    "UGP_RIPPLES_LIMITS": ("tested:test_ripples_at_size_gpu.py", "lowered workspace limits of the RIPPLES search"),
    # ---- diagnostics
    "UGP_BOUND3_VERBOSE": ("diagnostic", "prints the third bound's per-call decision to stderr"),
    "UGP_DEBUG_SHARING": ("diagnostic", "prints which workspace set a call took and whether it shared the device"),
    "UGP_TRACE": ("diagnostic", "experiments build, with UGP_STATS: writes per-unit walk records to the named file"),
}

FLATTEN = {
    "UGP_CHUNK_NODES": "signature",
    "UGP_PRUNE_MIN_WORDS": "signature",
    "UGP_NO_SIB": "signature",
    "UGP_NO_BOUND2": "signature",
    "UGP_NO_BOUND3": "signature",
    "UGP_LDS_SLOTS": "signature",
    "UGP_PRE_WEIGHT": "signature",
    "UGP_NO_UPDATE_MAPS": "signature",
    "UGP_COARSE_MIN_NODES": "signature",
    "UGP_NO_SORT": "signature",
    "UGP_COARSE_DIV": "signature",
    "UGP_COARSE_FLOOR": "signature",
    "UGP_COARSE_CHUNK_NODES": "signature",
    "UGP_PHASE2_PACKED": "adds the node_pos8 / rank_dfs tables only; a handle without them runs phase 2 as k_ties (the packed "
                         "phase 2 is taken only when both tables are on the device), so a file written without the knob places exactly",
    "UGP_FLATTEN_THREADS": "splits the host work only; the flattening is the same for every thread count (test_flatten_cpu.py)",
    "UGP_FLATTEN_GRAIN": "splits the host work only; the flattening is the same for every grain (test_flatten_cpu.py)",
    "UGP_FLATTEN_VERBOSE": "prints timings only",
}
