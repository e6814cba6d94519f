"""Hand-shaped trees for the nearest-k tests, as the breadth-first arrays of tests/synth.py.  A spec is an int (a leaf with that
many mutation entries) or a pair (entries, [child specs]); only the entry COUNTS matter to get_nearby, so a node with m entries
mutates positions 1 .. m."""
import numpy as np

SEG = 16384   # depth-first positions per segment of the dense kernels


def from_spec(spec):
    nmut, parent = [], []
    queue, head = [(spec, -1)], 0
    while head < len(queue):   # breadth-first numbering, children in their listed order
        s, p = queue[head]
        m, kids = (s, ()) if isinstance(s, int) else s
        nmut.append(m); parent.append(p)
        for c in kids:
            queue.append((c, head))
        head += 1
    n = len(parent)
    nmut = np.asarray(nmut, np.int64)
    off = np.concatenate([[0], np.cumsum(nmut)]).astype(np.int64)
    pos = (np.arange(off[-1]) - np.repeat(off[:-1], nmut) + 1).astype(np.int32)
    m = len(pos)
    return {"n": n, "parent": np.asarray(parent, np.int64), "mut_off": off, "mut_pos": pos, "mut_ref": np.full(m, 1, np.int8),
            "mut_par": np.full(m, 1, np.int8), "mut_nuc": np.full(m, 2, np.int8), "names": ["n%d" % j for j in range(n)]}


def leaves(k, m=1):
    return [m] * k


def segment_tree():
    """~40,000 nodes.  Depth-first: root 0, w 1, c1 [2, 16000), v [16000, 33000) = 383 leaves, c2 [16384, 32768) -- one whole
    segment --, 232 leaves; c3 [33000, 39001); 5 more leaves of the root.  w starts inside segment 0 and ends inside segment 2;
    v straddles both segment edges.  Returns (arrays, breadth-first ids by name)."""
    rng = np.random.default_rng(5)
    def some(k):
        return [int(x) for x in rng.integers(0, 4, k)]
    c1 = (1, some(15997))
    c2 = (2, some(SEG - 1))
    v = (1, some(383) + [c2] + some(232))
    c3 = (0, some(6000))
    arrays = from_spec((0, [(1, [c1, v, c3])] + some(5)))
    # breadth-first ids: root 0; level 1: w 1, five leaves; level 2: c1 7, v 8, c3 9
    ids = {"w": 1, "c1": 7, "v": 8, "c3": 9}
    kids_v = np.flatnonzero(arrays["parent"] == ids["v"])
    ids["c2"] = int(kids_v[383])
    return arrays, ids


def digit_tree():
    """A polytomy P whose leaves sit at 1 (the query), 5, 5, 5, 2047, 2048, 2048, 2049 entries and three (7, 8, 9 entries) at the
    end of a chain of 2,100 branches of 2,000 entries (beyond 2^22); the root has three more leaves.  Returns (arrays, query leaf,
    leaves of P)."""
    far = (2000, [7, 8, 9])
    for _ in range(2099):
        far = (2000, [far])
    arrays = from_spec((0, [(3, [1, 5, 5, 5, 2047, 2048, 2048, 2049, far]), 1, 2, 3]))
    return arrays, 5, 11   # breadth-first: root 0, P 1, three leaves 2-4, P's children from 5


def tie_tree():
    """P with a child S of 20 leaves and 480 leaves of its own, every leaf one entry from P; the root has 30 more leaves.
    Returns (arrays, a leaf of S)."""
    arrays = from_spec((0, [(2, leaves(200) + [(0, leaves(20))] + leaves(280))] + leaves(30, 3)))
    s = int(np.flatnonzero(arrays["parent"] == 1)[200])
    return arrays, int(np.flatnonzero(arrays["parent"] == s)[7])


SORT_LDS = 4096   # pairs the sort of one query's candidates takes in LDS; more go through a global scratch


def sort_tree(L=8300, spare=4):
    """A root with a polytomy P of L leaves and `spare` more leaves.  Leaf i of P has (L - i) % 64 + 1 entries, so in depth-first
    order the keys fall and wrap: the compaction hands the sort an unsorted list with long runs of ties, and a sort that passed its
    input through would fail.  About 32.5 * L entries.  Returns (arrays, the first leaf of P, P): from that leaf every k < L has
    last_anc = the leaf itself, one leaf held, and need = k - 1 candidates to order -- the leaf among them (is_ancestor starts at the
    parent)."""
    arrays = from_spec((0, [(2, [(L - i) % 64 + 1 for i in range(L)])] + leaves(spare, 3)))
    return arrays, spare + 2, 1   # breadth-first: root 0, P 1, the spare leaves, P's children from spare + 2
