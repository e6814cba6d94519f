"""Inputs for tests/test_fitch_counts.py: trees stated as degree profiles and sites at which ONE child decides what a node gets.

ugp_fitch.hip counts, per node, site and base, the children that lack the base -- in 3, 5 or 8 bit-sliced planes by the widest
node of a group of eight, eight rows per batch with the `stored` windows fetched ahead, and, above FS_WIDE children, in chunks
of FS_CHUNK rows that are added in K = 32 - clz(children) planes.  With random variants under a wide node the argmin is decided
by margins of dozens and a miscounted child never shows.  Here every "target" (a child of the root with c children) gets, at
every site, one of five kinds of cells in which an error of one, or a counter that wraps, changes the result:

  balanced     half of the children X, half Y (both not the reference); an odd one N or X|Y in turn      -> {X, Y}
  half_absent  c // 2 children X (an odd one X|ref), the others no cell                                   -> {X, ref}
  saturated    every child X, the target's own cell X|Z: the counter of Z reaches exactly c               -> {X}
  near_tie     half + 1 against half - 1 (an odd one N)                                                   -> {X}
  internal     balanced, with children that are internal nodes over two leaves: one with a cell of its own,
               one handing up the two-base set {X, Y}, one handing up {Z, ref}                              -> {X, Y}

Which child plays which part is a fresh random permutation at every site.  The root's own cell goes through three modes (none;
the higher base of the tied pair; a base outside it), so the backward sweep meets a parent state inside the tied set that is not
its lowest base, and one outside it, at the targets and at their internal children.

Rows that are never stored.  A leaf has a row only where it has a cell among the 512 sites of a tile, so "no cell at this site"
alone would never reach that path: per (target, tile) a quarter of the leaf children ("ghosts", from c = 8 on) get no cell at all
and are read from the reference row.  The parts above are dealt among the other children, the ghosts add the same to X and Y, and
half_absent still gives X to c // 2 of ALL children; in `saturated` the target's cell is X|Z rather than X|ref, because every
child, ghosts included, lacks Z.  Tile 0 keeps the children at the positions of `edge_positions` out of the ghosts (so that a
fault at them shows there), the other tiles make the first and the last child ghosts (from c = 12 on).

A site holds one kind per target, kind = (site + index of the target) % 5, so every word of eight sites holds every kind: "a site
of each kind on each edge" is asserted as "in each WORD that holds one of the listed edge sites" (tests/test_fitch_counts.py).

The model below is the set formulation of tests/test_fitch.py, vectorised over sites, with an injectable counting fault; the CPU
tests prove it equal to the oracle on these inputs and prove that every fault changes the mutation list of every case."""
import functools
import zlib

import numpy as np

# FS_WIDE / FS_CHUNK of usher_amd/csrc/ugp_fitch.hip (test_constants_follow_the_source fails when they change there)
FS_WIDE = 255
FS_CHUNK = 64

KINDS = ("balanced", "half_absent", "saturated", "near_tie", "internal")
TIE_OF = {"balanced": "XY", "half_absent": "XR", "saturated": "X", "near_tie": "X", "internal": "XY"}
EDGE_SITES = (0, 7, 8, 63, 64, 511, 512, 513)

# child counts of the single target: the plane choices 7|8 and 31|32, the last streamed width and the first polytomy (K: 8 -> 9),
# 5 chunks + 1 row (the odd tail of the two-chunks-in-flight loop), and K going up at 512, 4096 and 65536
SINGLE_DEGREES = (2, 7, 8, 9, 15, 16, 31, 32, 33, 63, 64, 65, 127, 128, 254, 255, 256, 257, 319, 320, 321, 511, 512, 513, 4095,
                  4096, 4097, 65535, 65536, 65537)
# one level of internal nodes: polytomies first, in the middle, last and side by side within a group of eight, every plane choice
# by the widest node of the open prefix; 8k+1 and 8k+7 nodes, so the last group reads the next level's entries
MIXED_A = (2, 7, 8, 3, 31, 32, 255, 256, 300, 1, 1, 5, 64, 65, 257, 9, 256, 256, 2, 4, 255, 13, 320, 6, 33)
MIXED_B = (256, 2, 7, 300, 8, 31, 3, 32, 5, 255, 1, 64, 257, 65, 1, 9, 2, 256, 256, 321, 6, 15, 128)
# many small targets: their internal children fill several eight-node waves of k_fs_backward with tied sets
BACKWARD = (9, 2, 8, 3, 7, 16, 4, 5, 15, 2, 9, 33, 6, 8, 7, 3, 10)


def tree_from_degrees(levels):
    """levels[L] = the child counts of the nodes of level L, in order (0 = a leaf); levels[0] = [the root's].  The children of the
    last level given are leaves.  Returns the breadth-first parent array (parent[0] = -1)."""
    if len(levels[0]) != 1:
        raise ValueError("level 0 is the root alone")
    parent, start = [-1], 0
    for L, degs in enumerate(levels):
        if L and len(degs) != sum(levels[L - 1]):
            raise ValueError("level %d has %d nodes, level %d has %d children" % (L, len(degs), L - 1, sum(levels[L - 1])))
        for k, d in enumerate(degs):
            parent.extend([start + k] * int(d))
        start += len(degs)
    return np.asarray(parent, np.int64)


def topology(parent):
    """(child counts, first child -- valid for internal nodes --, level offsets) of a breadth-first parent array."""
    n = len(parent)
    nch = np.bincount(parent[1:], minlength=n) if n > 1 else np.zeros(1, np.int64)
    first = np.searchsorted(parent[1:], np.arange(n)) + 1
    lvl = [0, 1]
    while lvl[-1] < n:
        lvl.append(int(np.searchsorted(parent[1:], lvl[-1])) + 1)
    return nch, first, lvl


def edge_positions(c):
    """The child positions the faults are injected at: first, last, and the last k with k % 8 in {0, 7}, k % 64 in {0, 63}."""
    out = {"first": 0, "last": c - 1}
    for m, r in ((8, 0), (8, 7), (64, 0), (64, 63)):
        if c - 1 >= r:
            out["k%%%d==%d" % (m, r)] = (c - 1 - r) // m * m + r
    return out


def internal_positions(c):
    """Which children of a target with c children are internal nodes (over two leaves each): away from edge_positions if possible."""
    if c < 2:
        return ()
    want = 1 if c < 4 else 2 if c < 7 else 3
    edges = set(edge_positions(c).values())
    out = []
    for p in [1, c // 2, c - 2] + list(range(2, min(c, 12))):
        if 0 < p < c and p not in edges and p not in out:
            out.append(p)
        if len(out) == want:
            break
    return tuple(sorted(out)) if out else (1,)


def profile_levels(degrees):
    """Root -> one internal node per entry of `degrees` -> their children, of which internal_positions() are internal -> leaves."""
    lvl2 = []
    for c in degrees:
        d = [0] * c
        for p in internal_positions(c):
            d[p] = 2
        lvl2.extend(d)
    return [[len(degrees)], list(degrees), lvl2]


class Case:
    pass


def kind_at(site, ti):
    return KINDS[(site + ti) % len(KINDS)]


def build_case(name, degrees, n_sites, seed=None):
    """The tree of profile_levels(degrees) with the five kinds of sites at every target (a child of the root with >= 2 children)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) if seed is None else seed)
    k = Case()
    k.name, k.degrees, k.n_sites = name, tuple(degrees), n_sites
    k.parent = tree_from_degrees(profile_levels(degrees))
    nch, first, lvl = topology(k.parent)
    n_tiles = (n_sites + 511) // 512
    k.targets = []
    for i, c in enumerate(degrees):
        if c < 2:
            continue
        t = 1 + i
        t_ = {"index": len(k.targets), "node": t, "c": c, "first": int(first[t]), "internal": internal_positions(c)}
        leafpos = np.setdiff1d(np.arange(c), t_["internal"])
        edges = np.asarray(sorted(set(edge_positions(c).values())))
        ghosts = []
        for y in range(n_tiles):
            g = np.zeros(c, bool)
            ng = (c - 4) // 4 if c >= 8 else 0
            if ng:
                if y == 0:
                    pool = np.setdiff1d(leafpos, edges)
                    g[rng.choice(pool, min(ng, len(pool)), replace=False)] = True
                else:
                    forced = np.intersect1d(leafpos, [0, c - 1]) if ng >= 2 else np.zeros(0, np.int64)
                    pool = np.setdiff1d(leafpos, forced)
                    g[forced] = True
                    g[rng.choice(pool, max(ng - len(forced), 0), replace=False)] = True
            ghosts.append(g)
        t_["ghosts"] = ghosts
        k.targets.append(t_)
    ref = np.zeros(n_sites, np.uint8)
    k.bases = np.zeros((n_sites, 3), np.uint8)   # X, Y, Z of the site: the three bases that are not the reference, shuffled
    k.root_mode = np.zeros(n_sites, np.int64)
    off, nodes, nucs = [0], [], []
    n_cells = 0
    for s in range(n_sites):
        r = 1 << int(rng.integers(0, 4))
        X, Y, Z = (int(b) for b in rng.permutation([b for b in (1, 2, 4, 8) if b != r]))
        ref[s], k.bases[s] = r, (X, Y, Z)
        alt = (s // len(KINDS)) % 2          # the odd child: N, or X|Y
        mode = (s // len(KINDS)) % 3         # the root's own cell: none, the higher base of the tied pair, a base outside it
        k.root_mode[s] = mode
        if mode and k.targets:
            pair = {"XY": (X, Y), "XR": (X, r), "X": (X, Y)}[TIE_OF[kind_at(s, 0)]]
            nodes.append(np.asarray([0])); nucs.append(np.asarray([max(pair) if mode == 1 else Z], np.uint8))
        tcell_nodes, tcell_nucs, ch_nodes, ch_nucs, gc_nodes, gc_nucs = [], [], [], [], [], []
        for t_ in k.targets:
            c, kind = t_["c"], kind_at(s, t_["index"])
            ghost = t_["ghosts"][s // 512]
            cell = np.zeros(c, np.uint8)
            part = np.ones(c, bool) & ~ghost   # the children the parts are dealt among
            if kind == "internal":
                for q, p in enumerate(t_["internal"]):
                    role = (q + s) % 3
                    if role == 2 and c < 7:
                        role = 1
                    if role == 0:
                        continue
                    part[p] = False
                    g0 = int(first[t_["first"] + p])   # the internal child's two leaves
                    if role == 1:
                        gc_nodes += [g0, g0 + 1]; gc_nucs += [X, Y]
                    else:
                        gc_nodes += [g0]; gc_nucs += [Z]   # (the other leaf has no cell: the reference)
            perm = rng.permutation(np.flatnonzero(part))
            m = len(perm)

            def odd_one_is_a_leaf(at):   # (an internal node would settle a cell of several bases by its own children)
                j = int(np.flatnonzero(~np.isin(perm, t_["internal"]))[0])
                perm[[at, j]] = perm[[j, at]]
            if kind in ("balanced", "internal"):
                h = m // 2
                if m % 2:
                    odd_one_is_a_leaf(2 * h)
                    cell[perm[2 * h]] = (X | Y) if alt else 15
                cell[perm[:h]], cell[perm[h:2 * h]] = X, Y
            elif kind == "half_absent":
                h = c // 2
                if c % 2:
                    odd_one_is_a_leaf(h)
                    cell[perm[h]] = X | r
                cell[perm[:h]] = X
            elif kind == "saturated":
                cell[perm] = X
                tcell_nodes.append(t_["node"]); tcell_nucs.append(X | (Z if ghost.any() else r))
            else:
                h = m // 2
                a, b = h + 1, max(h - 1, 0)
                if m > a + b:
                    odd_one_is_a_leaf(a + b)
                    cell[perm[a + b]] = 15
                cell[perm[:a]], cell[perm[a:a + b]] = X, Y
            at = np.flatnonzero(cell)
            ch_nodes.append(t_["first"] + at); ch_nucs.append(cell[at])
        # cells ascend by node within a site: root, targets (level 1), their children (level 2), the internal children's leaves
        nodes += [np.asarray(tcell_nodes, np.int64)] + ch_nodes + [np.asarray(gc_nodes, np.int64)]
        nucs += [np.asarray(tcell_nucs, np.uint8)] + ch_nucs + [np.asarray(gc_nucs, np.uint8)]
        n_cells += (1 if mode and k.targets else 0) + len(tcell_nodes) + sum(len(a) for a in ch_nodes) + len(gc_nodes)
        off.append(n_cells)
    k.ref = ref
    k.off = np.asarray(off, np.uint64)
    k.nodes = (np.concatenate(nodes) if nodes else np.zeros(0)).astype(np.uint32)
    k.nucs = (np.concatenate(nucs) if nucs else np.zeros(0)).astype(np.uint8)
    k.max_children = int(nch.max())
    return k


def _single_sites(i, c):
    return (40, 46, 520, 1030)[i % 4] if c <= 513 else (40, 46)[i % 2]


CASES = {"single-%d" % c: ((c,), _single_sites(i, c)) for i, c in enumerate(SINGLE_DEGREES)}
CASES["mixed-8k+1"] = (MIXED_A, 520)
CASES["mixed-8k+7"] = (MIXED_B, 1030)
CASES["backward"] = (BACKWARD, 46)
CASE_NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    degrees, n_sites = CASES[name]
    return build_case(name, degrees, n_sites)


@functools.lru_cache(maxsize=None)
def oracle_list(name):
    """The literal oracle's mutation list of a case (computed once per process, shared by the tests, never changed)."""
    from oracle import capi
    k = case(name)
    out = []
    nodes, nucs = k.nodes.astype(np.int64), k.nucs.astype(np.int8)
    for s in range(k.n_sites):
        a, b = int(k.off[s]), int(k.off[s + 1])
        _, mpar, mnuc = capi.fitch_site(k.parent, int(k.ref[s]), nodes[a:b], nucs[a:b])
        j = np.flatnonzero(mnuc)
        out += zip([s] * len(j), j.tolist(), mpar[j].tolist(), mnuc[j].tolist())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the set formulation, vectorised over sites, with an injectable counting fault

def _lack(F):
    """(..., 4): 1 where the base is NOT in the set."""
    return ((F[..., None] >> np.arange(4)) & 1) ^ 1


def _argmin_sets(allowed, cnt):
    cost = np.where((allowed[..., None] >> np.arange(4)) & 1, cnt, np.iinfo(np.int64).max)
    return (((cost == cost.min(axis=-1, keepdims=True)) << np.arange(4)).sum(axis=-1)).astype(np.int16)


def _pick(F, sp):
    """the backward rule: the parent's state if it is in the set, else the set's lowest base"""
    return np.where(F & sp, sp, F & -F)


def fault_positions(c):
    """(label, position) of edge_positions, one label per position"""
    seen, out = set(), []
    for label, p in edge_positions(c).items():
        if p not in seen:
            seen.add(p)
            out.append((label, p))
    return out


def wrap_moduli(c):
    """mod 8, 32, 256 and 2^(K-1), K = the planes of a node with c children: those that are <= c (others change nothing)"""
    return sorted({m for m in (8, 32, 256, 1 << (int(c).bit_length() - 1)) if 2 <= m <= c})


def faults_for(c, internal=()):
    """Every fault of the list that applies to a node with c children: (name, kind, argument)."""
    out = []
    for label, p in fault_positions(c):
        out.append(("drop %s" % label, "drop", p))
        out.append(("twice %s" % label, "twice", p))
        if p not in internal:
            out.append(("as-reference %s" % label, "asref", p))
    out += [("wrap mod %d" % m, "wrap", m) for m in wrap_moduli(c)]
    return out


def apply_fault(cnt, kind, arg, child_sets, refs):
    """cnt (S, 4): the counters of one node; child_sets (S, c): its children's sets; refs (S,): the reference base."""
    if kind == "wrap":
        return cnt % arg
    mine = _lack(child_sets[:, arg])
    if kind == "drop":
        return cnt - mine
    if kind == "twice":
        return cnt + mine
    assert kind == "asref"
    return cnt - mine + _lack(refs)


def initial_sets(parent, ref, off, nodes, nucs, nch):
    S = len(ref)
    F = np.where(nch[None, :] > 0, 15, np.asarray(ref, np.int16)[:, None]).astype(np.int16)
    site_of = np.repeat(np.arange(S), np.diff(np.asarray(off).astype(np.int64)))
    F[site_of, np.asarray(nodes, np.int64)] = np.asarray(nucs, np.int16)
    return F


def forward_sets(parent, ref, off, nodes, nucs, fault=None, keep=None):
    """Fitch sets of every (site, node) after the bottom-up sweep.  fault = (node, kind, argument) miscounts that node's children;
    keep: a dict that receives the counters {node: (S, 4)} of the nodes it already has as keys."""
    nch, first, lvl = topology(parent)
    F = initial_sets(parent, ref, off, nodes, nucs, nch)
    refs = np.asarray(ref, np.int16)
    for L in range(len(lvl) - 2, -1, -1):
        inner = lvl[L] + np.flatnonzero(nch[lvl[L]:lvl[L + 1]] > 0)
        if not len(inner):
            continue
        ca, ce = int(first[inner[0]]), int(first[inner[-1]] + nch[inner[-1]])
        cnt = np.add.reduceat(_lack(F[:, ca:ce]).astype(np.int64), first[inner] - ca, axis=1)   # (S, inner, 4)
        for at, j in enumerate(inner):
            if fault is not None and fault[0] == j:
                cnt[:, at] = apply_fault(cnt[:, at], fault[1], fault[2], F[:, first[j]:first[j] + nch[j]], refs)
            if keep is not None and int(j) in keep:
                keep[int(j)] = cnt[:, at].copy()
        F[:, inner] = _argmin_sets(F[:, inner], cnt)
    return F


def backward_states(parent, ref, F):
    _, _, lvl = topology(parent)
    st = np.zeros_like(F)
    st[:, 0] = _pick(F[:, 0], np.asarray(ref, np.int16))
    for L in range(1, len(lvl) - 1):
        a, e = lvl[L], lvl[L + 1]
        st[:, a:e] = _pick(F[:, a:e], st[:, parent[a:e]])
    return st


def mutation_list(parent, ref, st):
    sp = np.empty_like(st)
    sp[:, 0] = np.asarray(ref, np.int16)
    sp[:, 1:] = st[:, parent[1:]]
    s, j = np.nonzero(st != sp)
    return list(zip(s.tolist(), j.tolist(), sp[s, j].tolist(), st[s, j].tolist()))


def set_model(parent, ref, off, nodes, nucs, fault=None):
    """The mutation list by the set formulation (what ugp_fitch.hip computes), optionally with a counting fault at one node."""
    F = forward_sets(parent, ref, off, nodes, nucs, fault)
    return mutation_list(parent, ref, backward_states(parent, ref, F))


class Sensitivity:
    """Whether a fault at a target changes the mutation list of a case, without running the whole model per fault: the fault
    changes the target's set, through it the root's, and states only at the root, the root's children and below the target.  (The
    list changes exactly when some state does: the topmost node whose state differs has the same parent state in both runs, so its
    entry differs.)  test_quick_sensitivity_equals_the_full_model holds this against set_model(fault=...)."""

    def __init__(self, k):
        self.k = k
        self.nch, self.first, self.lvl = topology(k.parent)
        self.F_init = initial_sets(k.parent, k.ref, k.off, k.nodes, k.nucs, self.nch)
        self.cnt = {t_["node"]: None for t_ in k.targets}
        self.F = forward_sets(k.parent, k.ref, k.off, k.nodes, k.nucs, keep=self.cnt)
        self.st = backward_states(k.parent, k.ref, self.F)
        self.refs = np.asarray(k.ref, np.int16)

    def target_sets(self, t_):
        return self.F[:, t_["node"]]

    def changes(self, t_, kind, arg):
        t, c, f0 = t_["node"], t_["c"], t_["first"]
        kids = self.F[:, f0:f0 + c]
        Ft = _argmin_sets(self.F_init[:, t], apply_fault(self.cnt[t], kind, arg, kids, self.refs))
        if np.array_equal(Ft, self.F[:, t]):
            return False
        a, e = self.lvl[1], self.lvl[2]
        F1 = self.F[:, a:e].copy()
        F1[:, t - a] = Ft
        root = _pick(_argmin_sets(self.F_init[:, 0], _lack(F1).astype(np.int64).sum(axis=1)), self.refs)
        st1 = _pick(F1, root[:, None])
        if not (np.array_equal(root, self.st[:, 0]) and np.array_equal(st1, self.st[:, a:e])):
            return True
        return False   # (the same states at the target and above: nothing below it changes either)


def width_class(c):
    return "<=7" if c <= 7 else "<=31" if c <= 31 else "<=255" if c <= FS_WIDE else "polytomy"
