"""The three table kernels of the third pruning bound (ugp_bound3.hip) on nibbles the test chooses, through the hook
ugp_debug_bound3_build, against the restatement in tests/stream_interp.py (b3_tables) block by block, and the three levels of
maxima against the device's own `over`.  A tile's useful nibbles never hold the reference bit, so handing them to b3_tables as
one "sample" restates the tile.  Tile counts at the edges of the write-out's row passes and of a slice of 8 tiles (7, 8, 9), at
the pairmask-word edge (31, 32, 33) and with a partly filled second pairmask row (33, 40); every position of the random case
holds a tile of its own, so a wrong tile index or mask shift cannot pass by returning a neighbour's table."""
import functools

import numpy as np
import pytest

from tests import stream_interp, synth
from usher_amd import FlatTreeView, Placer, UgpError

pytestmark = pytest.mark.gpu

LONG = dict(n_leaves=6000, genome_len=4000, n_sites=900, n_ambig=(0, 0, 2), mut_counts=(0, 1, 1, 1, 2, 3) * 8 + (300, 420))
TREES = {"mid": dict(seed=11, n_leaves=3000, n_sites=400, n_ambig=(0, 0, 2, 6), p_masked=0.01),
         "one_group": dict(seed=12, n_leaves=50, n_sites=400, n_ambig=(0, 0, 0, 0), p_masked=0.01),
         "long81": dict(seed=81, **LONG), "long83": dict(seed=83, **LONG)}
TILE_COUNTS = (1, 7, 8, 9, 31, 32, 33, 40)
_open = {}


@pytest.fixture(scope="module")
def trees():
    def get(name):
        if name not in _open:
            kw = dict(TREES[name])
            arrays, _ = synth.make_case(kw.pop("seed"), n_queries=1, **kw)
            _open[name] = (FlatTreeView(arrays), Placer(arrays))
        return _open[name]
    yield get
    for _, placer in _open.values():
        placer.close()
    _open.clear()


def _nibbles(flat, kind, tile):
    """One tile's nibble per site, never with the site's reference bit."""
    ref = flat.site_ref.astype(np.int64)
    if kind == "zero":
        return np.zeros(len(ref), np.int64)
    if kind == "full":                                   # every non-reference allele of every site
        return 15 & ~ref
    rng = np.random.default_rng(7000 + tile)             # about 4 % of the pairs, another draw per tile
    bits = (rng.random((len(ref), 4)) < 0.04).astype(np.int64)
    return (bits[:, 0] | bits[:, 1] << 1 | bits[:, 2] << 2 | bits[:, 3] << 3) & ~ref


def _pack(nibs):
    n_sites = nibs.shape[1]
    w = np.zeros((nibs.shape[0], (n_sites + 7) // 8 * 8), np.uint64)
    w[:, :n_sites] = nibs
    w = w.reshape(nibs.shape[0], -1, 8) << (4 * np.arange(8, dtype=np.uint64))
    return np.bitwise_or.reduce(w, axis=2).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _want(name, kind, tile):
    """The restatement of one tile, computed once: the random tile of position `tile` is the same at every tile count."""
    flat = _open[name][0]
    b3 = stream_interp.b3_tables(flat, [_nibbles(flat, kind, tile)])
    return b3["over"], b3["under"]


def _maxima(a):
    n = (a.shape[1] + 63) // 64
    p = np.zeros((a.shape[0], n * 64), a.dtype)
    p[:, :a.shape[1]] = a
    return p.reshape(a.shape[0], n, 64).max(axis=2)


@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
@pytest.mark.parametrize("kind", ["zero", "random", "full"])
@pytest.mark.parametrize("name", list(TREES))
def test_tables_of_chosen_nibbles(trees, name, kind, n_tiles):
    flat, placer = trees(name)
    nibs = np.stack([_nibbles(flat, kind, t) for t in range(n_tiles)])
    got = placer.bound3_build(_pack(nibs))
    nb = got["over"].shape[1]
    assert nb % 256 == 0 and got["l1"].shape[1] == (nb + 63) // 64
    for t in range(n_tiles):
        over, under = _want(name, kind, t if kind == "random" else 0)
        assert len(over) == nb
        np.testing.assert_array_equal(got["over"][t], np.minimum(over, 255), err_msg="over, tile %d" % t)     # (one byte per block: 255 = "255 or more")
        np.testing.assert_array_equal(got["under"][t], np.minimum(under, 255), err_msg="under, tile %d" % t)
    assert (got["under"] <= got["over"]).all()
    np.testing.assert_array_equal(got["l1"], _maxima(got["over"]))
    np.testing.assert_array_equal(got["l2"], _maxima(got["l1"]))
    np.testing.assert_array_equal(got["l3"], _maxima(got["l2"]))
    if kind == "zero":
        assert not got["over"].any()
    if kind == "full" and name.startswith("long"):
        over, _ = _want(name, kind, 0)
        assert over.max() >= 256 and got["over"].max() == 255, "the long branches do not saturate the byte"


def test_random_tiles_differ(trees):
    """What the test above relies on: neighbouring positions hold different tables."""
    trees("mid")
    tabs = [_want("mid", "random", t)[0] for t in range(40)]
    assert all((tabs[i] != tabs[j]).any() for i in range(40) for j in range(i))


def test_a_handle_without_event_lists_is_refused(monkeypatch):
    monkeypatch.setenv("UGP_NO_BOUND3", "1")
    arrays, _ = synth.make_case(12, n_leaves=50, n_queries=1, n_sites=400)
    placer = Placer(arrays)
    try:
        with pytest.raises(UgpError) as e:
            placer.bound3_build(np.zeros((1, (placer.info()["n_sites"] + 7) // 8), np.uint32))
        assert e.value.code == -2   # UGP_ERR_UNSUPPORTED
    finally:
        placer.close()
