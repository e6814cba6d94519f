"""Hand-shaped record trees and sample batches for the record scoring of the add mode (ugp_mat_update / ugp_touched_*).  A case is
a small tree R, the nodes of R whose records are handed to the device -- in groups, one group per ugp_mat_update call; record ids
count through the groups -- and a batch of samples.  The records all have flat_j = None: the handle under test is built on BASE,
a small unrelated tree whose largest position (BASE_MAX_POS) lies below the positions >= FAR of R, where no sample has a row
either, so that such a record position is beyond the dense table (p >= n_pos, read as "no row").  The reference is the oracle's
literal mapper2_body over the live record nodes of R (oracle()); none of this needs the device library.  mapper2_body walks a
node's mutations and the sample's rows side by side, so every node lists its mutations by ascending position (a masked one apart)."""
import numpy as np

from oracle import capi, refio
from tests.genotypes_cases import hand

A, C, G, T = 1, 2, 4, 8
INT_MAX = 2 ** 31 - 1
ORACLE_NONE = 10 ** 9          # place_list's initial best: what it still reports when no node of the list was eligible
FAR = 200                      # record positions from here on are beyond the dense table of every batch below
BASE_MAX_POS = 25


def tree_from_arrays(arrays):
    """refio.Tree with the nodes of `arrays` (names n<j>), children in index order."""
    T = refio.Tree()
    nodes = []
    for j in range(int(arrays["n"])):
        p = int(arrays["parent"][j])
        nd = T.create_node("n%d" % j, nodes[p] if p >= 0 else None)
        for i in range(int(arrays["mut_off"][j]), int(arrays["mut_off"][j + 1])):
            m = refio.Mutation(int(arrays["mut_pos"][i]), int(arrays["mut_ref"][i]), int(arrays["mut_par"][i]), int(arrays["mut_nuc"][i]))
            nd.mutations.append(m)           # (already in the stored order)
        nodes.append(nd)
    return T, nodes


def record_of(node, flat_index):
    """What the driver reports for a touched node: the parent's state wherever it is not the reference base, the own mutations in
    front of the first masked one with their true parent state."""
    state, ref = {}, {}
    a = node.parent
    chain = []
    while a is not None:
        chain.append(a)
        a = a.parent
    for a in reversed(chain):                       # root first: later mutations overwrite
        for m in a.mutations:
            if m.is_masked():
                continue
            state[m.position] = m.mut_nuc
            ref[m.position] = m.ref_nuc
    path = [(p, s, ref[p]) for p, s in state.items() if s != ref[p]]
    own, masked = [], False
    for m in node.mutations:
        if m.is_masked():
            masked = True
            break
        own.append((m.position, m.mut_nuc, state.get(m.position, m.ref_nuc), m.ref_nuc))
    return {"flat_j": flat_index, "leaf": node.is_leaf(), "masked": masked, "path": path, "own": own}


def REF(p):
    return (A, C, G, T)[p % 4]


def alt(p, k=0):
    """The k-th base that is not the reference base at p."""
    return [b for b in (A, C, G, T) if b != REF(p)][k % 3]


def mut(p, nuc, par=None):
    return (p, REF(p), REF(p) if par is None else par, nuc)


MASK = (-1, 0, 0, 0)           # a masked mutation (negative position)


def base_arrays():
    """The tree the handle under test is built on: positions 3 .. BASE_MAX_POS, unrelated to every R."""
    return hand([-1, 0, 0, 1, 1, 2], {1: [mut(3, alt(3))], 2: [mut(11, alt(11, 1))], 3: [mut(17, alt(17))], 4: [mut(BASE_MAX_POS, alt(BASE_MAX_POS))],
                                      5: [mut(3, alt(3, 2)), mut(19, alt(19))]})


def sample(rows, name="s"):
    """rows = {position: allele mask, None: a missing call}"""
    ps = sorted(rows)
    assert all(0 < p < FAR for p in ps)
    return {"name": name, "pos": np.asarray(ps, np.int32), "ref": np.asarray([REF(p) for p in ps], np.int8),
            "nuc": np.asarray([15 if rows[p] is None else rows[p] for p in ps], np.int8),
            "is_missing": np.asarray([rows[p] is None for p in ps], np.int8)}


def random_samples(rng, n, positions, p_row=0.55):
    """Rows that hit (the first alternative base: what most records below mutate to), miss, are ambiguous or are missing."""
    out = []
    for i in range(n):
        rows = {}
        for p in positions:
            if rng.random() >= p_row:
                continue
            kind = rng.random()
            if kind < 0.45:
                rows[p] = alt(p, 0)
            elif kind < 0.6:
                rows[p] = alt(p, int(rng.integers(1, 3)))
            elif kind < 0.85:
                m = int(rng.integers(1, 16))
                while bin(m).count("1") < 2:
                    m = int(rng.integers(1, 16))
                rows[p] = m
            else:
                rows[p] = None
        out.append(sample(rows, "r%d" % i))
    return out


class Builder:
    def __init__(self, root_muts=()):
        self.parent, self.muts = [-1], {0: list(root_muts)}

    def add(self, parent, muts=()):
        self.parent.append(parent)
        self.muts[len(self.parent) - 1] = list(muts)
        return len(self.parent) - 1


class Case:
    def __init__(self, name, builder, groups, samples):
        self.name = name
        self.arrays = hand(builder.parent, builder.muts)
        self.T, self.nodes = tree_from_arrays(self.arrays)
        self.bfs_of = {id(n): j for j, n in enumerate(self.T.breadth_first_expansion())}
        self.groups = [list(g) for g in groups]
        self.rec_nodes = [v for g in self.groups for v in g]            # record id -> node of R (ids in the order handed over)
        assert 0 not in self.rec_nodes and len(self.rec_nodes) <= len(self.nodes)
        self.samples = samples
        self._ot = None

    @property
    def n_rec(self):
        return len(self.rec_nodes)

    def first_id(self, g):
        return sum(len(x) for x in self.groups[:g])

    def ids(self, g):
        return list(range(self.first_id(g), self.first_id(g + 1)))

    def record(self, rid):
        return record_of(self.nodes[self.rec_nodes[rid]], None)

    def records(self, g):
        return [self.record(r) for r in self.ids(g)]

    def n_pos(self, samples=None):
        """Rows of the dense table the device builds for the batch: every position from here on is beyond it."""
        samples = self.samples if samples is None else samples
        return max([BASE_MAX_POS] + [int(p) for s in samples for p in s["pos"]]) + 1

    def beyond(self, rid, samples=None):
        """The record's positions beyond the dense table, path entries and own mutations apart."""
        r, n = self.record(rid), self.n_pos(samples)
        return [e[0] for e in r["path"] if e[0] >= n], [e[0] for e in r["own"] if e[0] >= n]

    def oracle(self, smp, live):
        """(best, num_best, {record id: has_unique}) of mapper2_body over the nodes of the live records; (INT_MAX, 0, {}) where
        place_list still holds what it started from (best 10^9, the one placeholder entry 0): no record was eligible."""
        if self._ot is None:
            self._ot = capi.OracleTree(refio.tree_to_bfs_arrays(self.T))
        live = sorted(live)
        nodes = [self.bfs_of[id(self.nodes[self.rec_nodes[r]])] for r in live]
        w = self._ot.place_list(smp, nodes, jidx=live, init_best=ORACLE_NONE, tie_cap=max(1, len(live)))
        if w["best"] == ORACLE_NONE:
            assert w["num_best"] == 1 and w["ties"].tolist() == [0] and not w["ties_has_unique"][0]
            return INT_MAX, 0, {}
        assert w["num_best"] == len(w["ties"])
        return w["best"], w["num_best"], {int(r): bool(h) for r, h in zip(w["ties"], w["ties_has_unique"])}


# ---- the eight-entry batches: one record per (n_path, n_own), one of 40 entries ---------------------------------------------------

ENTRY_PATH, ENTRY_OWN = (0, 1, 7, 8, 9, 16), (0, 1, 7, 8, 9)
ENTRY_N_ALL = (0, 1, 7, 8, 9, 16, 17, 40)
ENTRY_POOL = list(range(1, 48)) + [50, 51]       # positions of the samples' rows; 50 and 51 are named by no record


def entry_case():
    """Parents P(n_path) under the root mutate positions 1 .. n_path (P(9): 1 .. 8 and FAR + 10, beyond the table); a child with
    n_own mutations takes position 1 from the parent's state to another base (n_own odd) or back to the reference base (n_own even),
    position 2 the other way round when the parent has it, then fresh positions 30 ..; from eight own mutations on the last one is
    beyond the table (FAR + k).  Children with 0 or 9 own mutations are internal (a child of their own that is no record).  The
    batch: the genotype of every record's node (without the positions beyond the table), then 34 random samples."""
    b = Builder()
    recs, cells = [], {}
    for n_path in ENTRY_PATH + (23,):
        ps = list(range(1, n_path + 1))
        if n_path == 9:
            ps[-1] = FAR + 10
        par = 0 if n_path == 0 else b.add(0, [mut(p, alt(p)) for p in ps])
        for n_own in (ENTRY_OWN if n_path != 23 else (17,)):
            own = []
            for k in range(n_own):
                if k < 2 and n_path > 6 * k:                  # at a position of the parent's state: prev is that state, not REF
                    p = k + 1
                    own.append(mut(p, alt(p, 1) if (n_own + k) % 2 else REF(p), par=alt(p)))
                elif n_own >= 8 and k == n_own - 1:
                    own.append(mut(FAR + k, alt(FAR + k)))
                else:
                    own.append(mut(30 + k, alt(30 + k, 1 if k % 5 == 4 else 0)))
            v = b.add(par, own)
            if n_own in (0, 9):
                b.add(v, [mut(47, alt(47))])
            recs.append(v)
            cells[(n_path, n_own)] = len(recs) - 1
    case = Case("entry_batches", b, [recs], [])
    smp = []
    for rid in range(case.n_rec):
        r = case.record(rid)
        state = {p: s for p, s, _ in r["path"]}
        state.update({p: m for p, m, _, _ in r["own"]})
        smp.append(sample({p: s for p, s in state.items() if s != REF(p) and p < FAR}, "g%d" % rid))
    case.samples = smp + random_samples(np.random.default_rng(11), 65 - len(smp), ENTRY_POOL)
    case.cells = cells
    return case


# ---- lists: polytomies of identical leaves ----------------------------------------------------------------------------------------

def ties_case(k):
    """k identical leaves under the root (position 5 to its first alternative base); one leaf with the second alternative base
    there, under an internal node that mutates position 7 (one step worse wherever the identical leaves are eligible); one leaf
    with a mutation at position 6.  Samples: the first base (k ties), the second (one), both (k), a missing call at 5 (k), no
    rows at all (no record eligible), a row nobody names (none either)."""
    b = Builder()
    recs = [b.add(0, [mut(5, alt(5))]) for _ in range(k)]
    recs.append(b.add(b.add(0, [mut(7, alt(7))]), [mut(5, alt(5, 1))]))
    recs.append(b.add(0, [mut(6, alt(6))]))
    smp = [sample({5: alt(5)}), sample({5: alt(5, 1)}), sample({5: alt(5) | alt(5, 1)}), sample({5: None}), sample({}), sample({9: alt(9)})]
    case = Case("ties%d" % k, b, [recs], smp)
    case.want_num_best = [k, 1, k, k, 0, 0]
    return case


# ---- values -----------------------------------------------------------------------------------------------------------------------

VALUES_POOL = [2, 3, 5, 7, 9, 11, 13, 20, 21]      # 20 and 21 are named by no record: D(bottom) from rows outside every record


def values_case():
    """The records of the issue's value list, by node (record id = node - 1):
      1  internal under a root that mutates position 2; mutates 3 and 5
      2  leaf of 1: position 3 from 1's state to a third base (prev = a parent state among the path entries), and position 7
      3  leaf of 1: position 5 back to the reference base
      4  leaf of 1 without mutations (never eligible)        5  internal of 1 without mutations (always eligible)
      6  leaf of 5: position 9
      7  internal of the root: position 11, then a masked mutation, then 13 (own = [11], masked)
      8  leaf of the root: a masked mutation first (own = [], masked: never eligible)
      9  leaf of the root: positions 7 and FAR (beyond the table)
      10 internal of the root: positions 9 and FAR + 1;  11 leaf of 10: position 5 and FAR + 1 back to the reference base (a path entry
         and an own mutation beyond the table)
      12 leaf of 7 (a masked mutation among the ancestors'): position 13
      13 leaf of the root: position 3"""
    b = Builder([mut(2, alt(2))])
    n1 = b.add(0, [mut(3, alt(3)), mut(5, alt(5, 1))])
    b.add(n1, [mut(3, alt(3, 2), par=alt(3)), mut(7, alt(7))])
    b.add(n1, [mut(5, REF(5), par=alt(5, 1))])
    b.add(n1)
    n5 = b.add(n1)
    b.add(n5, [mut(9, alt(9))])
    n7 = b.add(0, [mut(11, alt(11)), MASK, mut(13, alt(13))])
    b.add(0, [MASK, mut(11, alt(11))])
    b.add(0, [mut(7, alt(7)), mut(FAR, alt(FAR))])
    n10 = b.add(0, [mut(9, alt(9)), mut(FAR + 1, alt(FAR + 1))])
    b.add(n10, [mut(5, alt(5)), mut(FAR + 1, REF(FAR + 1), par=alt(FAR + 1))])
    b.add(n7, [mut(13, alt(13))])
    b.add(0, [mut(3, alt(3))])
    hand_made = [sample({}), sample({p: None for p in VALUES_POOL}), sample({20: alt(20), 21: alt(21, 1)}), sample({20: None, 21: alt(21)}),
                 sample({2: alt(2), 3: alt(3), 5: alt(5, 1)}),                    # the genotype of node 1 = of 4 and 5
                 sample({2: alt(2), 3: alt(3)}),                                  # ... of node 3: no row where it went back to REF
                 sample({2: alt(2), 3: alt(3, 2), 5: alt(5, 1), 7: alt(7)}),      # ... of node 2
                 sample({2: alt(2), 3: alt(3) | alt(3, 2), 5: None, 7: 15 ^ alt(7)}),
                 sample({2: alt(2), 11: alt(11)}), sample({2: alt(2), 11: alt(11), 13: alt(13)}), sample({2: alt(2), 7: alt(7)}),
                 sample({2: alt(2), 5: alt(5)}), sample({5: alt(5), 20: alt(20)}), sample({2: alt(2), 9: alt(9)})]
    smp = hand_made + random_samples(np.random.default_rng(3), 70 - len(hand_made), VALUES_POOL, p_row=0.6)
    return Case("values", b, [list(range(1, 14))], smp)


# ---- the running list -------------------------------------------------------------------------------------------------------------

RUNNING_POOL = [1, 2, 3, 4, 5, 6, 7, 30]


def running_case(n_samples=129, seed=2):
    """Four groups of three records: leaves of the root or of an internal node that mutates position 7, with 1 + g .. own mutations
    at positions 1 .. 6 in group g, so that later groups lower the minimum of some samples, equal it for others and stay above it
    for the rest.  The samples' rows name position 30 too (beyond BASE's, named by no record)."""
    rng = np.random.default_rng(seed)
    b = Builder()
    inner = b.add(0, [mut(7, alt(7))])
    groups = []
    for g in range(4):
        grp = []
        for _ in range(3):
            ps = sorted(rng.choice(6, size=min(6, 1 + g + int(rng.integers(0, 2))), replace=False) + 1)
            grp.append(b.add(inner if rng.random() < 0.4 else 0, [mut(int(p), alt(int(p), 0 if rng.random() < 0.8 else 1)) for p in ps]))
        groups.append(grp)
    return Case("running", b, groups, random_samples(np.random.default_rng(seed + 100), n_samples, RUNNING_POOL, p_row=0.5))


def branch_of_call(case, smp, g):
    """What group g does to the sample's running list: 'falls', 'equals', 'above' (an eligible record, at a higher cost) or
    'none' (no record of the group eligible); from the oracle's answers over the earlier groups and over group g alone."""
    old = case.oracle(smp, range(case.first_id(g)))[0]
    new = case.oracle(smp, case.ids(g))[0]
    if new == INT_MAX:
        return "none"
    return "falls" if new < old else "equals" if new == old else "above"
