"""Hand-shaped trees for the relatives calls (test helper).  A tree is written as nested (nm, [children]) tuples -- nm mutation
entries on the branch -- and numbered breadth-first, children in the order written."""
import numpy as np


def build(spec):
    order, head = [(spec, -1)], 0
    while head < len(order):
        (nm, kids), _ = order[head]
        for k in kids:
            order.append((k, head))
        head += 1
    n = len(order)
    parent = np.array([p for _, p in order], np.int64)
    nmut = np.array([s[0] for s, _ in order], np.int64)
    mut_off = np.concatenate([[0], np.cumsum(nmut)]).astype(np.int64)
    m = int(mut_off[-1])
    return {"n": n, "parent": parent, "mut_off": mut_off, "mut_pos": np.arange(1, m + 1, dtype=np.int32),   # every position once
            "mut_ref": np.full(m, 1, np.int8), "mut_par": np.full(m, 1, np.int8), "mut_nuc": np.full(m, 2, np.int8),
            "names": ["n%d" % j for j in range(n)]}


def leaf(nm):
    return (nm, [])


def two_nodes():
    return build((0, [leaf(1)]))


def chain():   # a single chain ending in one leaf: no relatives anywhere
    return build((1, [(2, [(0, [(1, [leaf(3)])])])]))


def star(n_leaves=300, seed=1):
    rng = np.random.default_rng(seed)
    return build((0, [leaf(int(x)) for x in rng.integers(0, 3, n_leaves)]))


def all_zero():   # every leaf ties at distance 0 and no level ever stops the climb
    return build((0, [(0, [leaf(0), leaf(0), leaf(0)]), (0, [leaf(0), (0, [leaf(0), leaf(0)])]), leaf(0)]))


def caterpillar(depth=120, seed=2):   # chain nodes without entries: L_j = 0, so the bottom leaf climbs every level
    rng = np.random.default_rng(seed)
    spec = (0, [leaf(1), leaf(2)])
    for _ in range(depth - 1):
        spec = (0, [leaf(int(rng.integers(1, 4))), spec])
    return build(spec)


def no_leaf_sibling():   # node 3 (a leaf) has one sibling, internal: min_of_sibling_leaves stays SIZE_MAX, max_path too
    return build((0, [(1, [leaf(1), (1, [leaf(2), leaf(1), (0, [leaf(0), leaf(4)])])]), leaf(5)]))


def append_across_levels():
    """t = the leaf without entries under p0: s is 2 away at level 0 (L_0 = 1: no stop), u is 4 away at level 1 (L_1 = 1), w is
    2 away again at level 2: the list is [s, w]."""
    arrays = build((0, [(0, [(1, [leaf(0), leaf(2)]), leaf(3)]), leaf(1)]))
    # breadth-first: 0 root, 1 p1, 2 w, 3 p0, 4 u, 5 t, 6 s
    return arrays, 5, [6, 2]


def replace_at_deeper_level():
    """t under p0 without entries: s is 3 away at level 0 (L_0 = 0: no stop), u is 1 away at level 1: [u] replaces [s]."""
    arrays = build((0, [(0, [leaf(0), leaf(3)]), leaf(1)]))
    # breadth-first: 0 root, 1 p0, 2 u, 3 t, 4 s
    return arrays, 3, [2]


def rmq_tree(n_leaves, seed=3):
    """n_leaves leaves in one depth-first row under a few nested parents, so that ring ranges start and end at every offset of the
    range-minimum blocks: a comb whose teeth hold 1, 2, 3, ... leaves, then a polytomy with the rest."""
    rng = np.random.default_rng(seed)
    left = n_leaves
    teeth = []
    k = 1
    while left > 2 * k + 8:
        teeth.append((int(rng.integers(0, 2)), [leaf(int(x)) for x in rng.integers(0, 4, k)]))
        left -= k
        k += 1
    rest = [leaf(int(x)) for x in rng.integers(0, 4, left)]
    return build((0, teeth[:len(teeth) // 2] + rest + teeth[len(teeth) // 2:]))


def hand_cases():
    return {"two_nodes": two_nodes(), "chain": chain(), "star": star(), "all_zero": all_zero(), "caterpillar": caterpillar(),
            "no_leaf_sibling": no_leaf_sibling(), "append": append_across_levels()[0], "replace": replace_at_deeper_level()[0]}
