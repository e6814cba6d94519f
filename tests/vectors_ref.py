"""The closed form of ugp_vectors (usher_amd/csrc/ugp_vectors.hip) written down in Python over the per-position owner lists, step by
step as the kernels compute it: the refusal, loop 1 with its merge pointer as a prefix maximum, the nearest owner g(p) of every row,
the back-mutations of the root path ordered by position.  tests/test_vectors_cpu.py holds it against the literal mapper2_body of the
oracle (OracleTree.node_vecs_split); the device is held against the oracle too, so this file only says WHY the kernel is right --
and, through the trace and the faults of vectors(), WHERE a pair puts the kernel's steps of 64 and what a kernel that lost one piece
of their bookkeeping would answer.
"""
from bisect import bisect_left, bisect_right

import numpy as np

NIL = -1


def lowbit4(a):
    for b in range(4):
        if a & (1 << b):
            return 1 << b
    return 0


class Tables:
    """The depth-first tables the kernel reads (ugp_dense.hpp), as Python lists indexed by depth-first position / entry."""

    def __init__(self, arrays):
        n = self.n = int(arrays["n"])
        par = [int(p) for p in arrays["parent"]]
        off = [int(o) for o in arrays["mut_off"]]
        kids = [[] for _ in range(n)]
        for j in range(1, n):
            kids[par[j]].append(j)
        order, stack = [], [0]
        while stack:   # preorder, children in increasing index
            v = stack.pop()
            order.append(v)
            stack.extend(reversed(kids[v]))
        self.dfs2bfs = order
        self.bfs2dfs = [0] * n
        for i, b in enumerate(order):
            self.bfs2dfs[b] = i
        self.dpar = [NIL if par[b] < 0 else self.bfs2dfs[par[b]] for b in order]
        size = [1] * n
        for i in range(n - 1, 0, -1):
            size[self.dpar[i]] += size[i]
        self.dend = [i + size[i] for i in range(n)]
        self.leaf = [not kids[b] for b in order]
        self.moff, self.mpos, self.mref, self.mpar, self.mnuc, self.mnode, self.owner = [0], [], [], [], [], [], []
        for i, b in enumerate(order):
            seen = set()
            for k in range(off[b], off[b + 1]):
                p = int(arrays["mut_pos"][k])
                self.mpos.append(p)
                self.mref.append(int(arrays["mut_ref"][k]) & 255)
                self.mpar.append(int(arrays["mut_par"][k]) & 255)
                self.mnuc.append(int(arrays["mut_nuc"][k]) & 255)
                self.mnode.append(i)
                self.owner.append(p >= 0 and p not in seen)   # the first non-masked entry of its position on its node
                seen.add(p)
            self.moff.append(len(self.mpos))
        # owners by position in depth-first order of their node, and each owner's nearest owner above
        self.pent, self.onode = {}, {}
        for e, p in enumerate(self.mpos):
            if self.owner[e]:
                self.pent.setdefault(p, []).append(e)
                self.onode.setdefault(p, []).append(self.mnode[e])
        self.mlink = [NIL] * len(self.mpos)
        for p, ents in self.pent.items():
            st = []
            for e in ents:
                while st and self.dend[self.mnode[st[-1]]] <= self.mnode[e]:
                    st.pop()
                if st:
                    self.mlink[e] = st[-1]
                st.append(e)


class _Rows:
    def __init__(self, sample):
        self.pos = [int(p) for p in sample["pos"]]
        self.ref = [int(x) & 255 for x in sample["ref"]]
        self.nuc = [int(x) & 255 for x in sample["nuc"]]
        self.mis = [bool(x) for x in sample["is_missing"]]
        self.n = len(self.pos)


def _probe(r, p, nuc):
    """merge_probe: the row at p, and where loop 1's pointer stands after an entry (p, nuc) whose row it has not passed."""
    lb = bisect_left(r.pos, p)
    here = lb < r.n and r.pos[lb] == p
    miss = here and r.mis[lb]
    match = here and not miss and (r.nuc[lb] & nuc) != 0
    if r.n == 0:
        after = 0
    elif lb == r.n:
        after = r.n - 1
    elif here and not match:
        after = min(lb + 1, r.n - 1)
    else:
        after = lb
    return lb, after, here, match, miss


FAULTS = ("carry", "stop", "nm")   # the kernel's wave bookkeeping undone, one piece at a time: see vectors()


def vectors(T, sample, j_bfs, trace=None, fault=None):
    """What ugp_vectors answers for one pair: a dict with the fields of ugp_vec_info and the two lists of (pos, ref, par, nuc).
    trace: a dict that receives what the kernel's 64-entry steps meet on this pair -- stop (br.stop - e0), nm, allvis, passed (per
    passed entry its index, the index of the first entry that left the pointer behind its row, and whether only the pointer carried
    in from an earlier step hides the row), own_asks (index, here) of every own_kept question, part3 (node, index within the node,
    masked) of every entry of part 3 in the order found.  fault: the answer of a kernel that lost one piece of that bookkeeping --
    "carry": start is not carried from one step of 64 to the next; "stop": br.stop = base instead of base + first_masked; "nm": the
    masked entry is not counted.  Only tests/test_vectors_cpu.py passes one, to show that the cases would notice."""
    assert fault is None or fault in FAULTS
    r = _Rows(sample)
    j = T.bfs2dfs[j_bfs]
    e0, e1 = T.moff[j], T.moff[j + 1]
    if any(T.mpos[e] >= 0 and not T.owner[e] for e in range(e0, e1)):
        return {"refused": 1, "excess": [], "imputed": [], "n_branch": 0, "set_difference": 0, "has_unique": 0, "eligible": 0}
    # part 1
    kept_e, start, stop, nm, common, hu, part1 = set(), 0, e1, 0, 0, False, []
    afters, local, passed = [], 0, []
    if j != 0:
        for e in range(e0, e1):
            if (e - e0) % 64 == 0:               # a new step of 64 lanes
                local = 0
                if fault == "carry":
                    start = 0
            nm += 1
            if T.mpos[e] < 0:
                hu, stop = True, e
                if fault == "stop":
                    stop = e - (e - e0) % 64
                if fault == "nm":
                    nm -= 1
                break
            lb, after, here, match, miss = _probe(r, T.mpos[e], T.mnuc[e])
            if here and lb < start:
                passed.append((e - e0, next(x for x, a in enumerate(afters) if a > lb), lb >= local))
            afters.append(after)
            local = max(local, after)
            seen = here and lb >= start          # a row the pointer has passed is not seen
            kept = match if seen else T.mnuc[e] == T.mref[e]
            if kept:
                kept_e.add(e)
                part1.append((T.mpos[e], T.mref[e], T.mpar[e], T.mnuc[e]))
            if kept or (seen and miss):
                common += 1
            else:
                hu = True
            start = max(start, after)
        kept_e = {e for e in kept_e if e < stop}
    own_asks, found3 = [], []

    def nearest_owner(p, here):
        on = T.onode.get(p)
        if not on:
            return NIL
        x = bisect_right(on, j)
        cur = T.pent[p][x - 1] if x else NIL
        while cur != NIL and j >= T.dend[T.mnode[cur]]:
            cur = T.mlink[cur]
        if cur != NIL and j != 0 and T.mnode[cur] == j:
            own_asks.append((cur - e0, here))
            if cur not in kept_e:
                cur = T.mlink[cur]
        return cur

    # part 2 and the imputed list
    part2, imputed = [], []
    for k in range(r.n):
        if r.mis[k]:
            continue
        p, rr, a = r.pos[k], r.ref[k], r.nuc[k]
        cur = nearest_owner(p, True)
        anc = T.mnuc[cur] if cur != NIL else rr
        found, has_ref, amb = cur != NIL and (a & anc) != 0, (a & rr) != 0, (a & (a - 1)) != 0
        if found:
            im = anc
        elif cur == NIL and has_ref:
            im = rr
        else:
            im = rr if has_ref else lowbit4(a)
            if im != anc:
                part2.append((p, rr, anc, im))
        if amb:
            imputed.append((p, rr, anc, im))
    # part 3
    masked, back = [], []
    rowpos = set(r.pos)
    if j == 0:
        for e in range(e0, e1):
            if T.mnuc[e] == T.mref[e]:
                continue
            if T.mpos[e] < 0:
                masked.append((T.mpos[e], T.mref[e], T.mnuc[e], T.mref[e]))
                found3.append((0, e - e0, True))
            elif T.mpos[e] not in rowpos:
                back.append((T.mpos[e], T.mref[e], T.mnuc[e], T.mref[e]))
                found3.append((0, e - e0, False))
    else:
        v = j
        while v != NIL:
            for e in range(T.moff[v], T.moff[v + 1]):
                p = T.mpos[e]
                if p >= 0 and T.owner[e] and T.mnuc[e] != T.mref[e] and p not in rowpos and nearest_owner(p, False) == e:
                    back.append((p, T.mref[e], T.mnuc[e], T.mref[e]))
                    found3.append((v, e - T.moff[v], False))
            v = T.dpar[v]
    part3 = masked + sorted(back)
    if trace is not None:
        trace.update(stop=stop - e0, nm=nm, allvis=not passed, passed=passed, own_asks=own_asks, part3=found3)
    lf = T.leaf[j]
    eligible = j == 0 or (hu and not lf and common > 0 and nm != common) or (lf and common > 0) or (not hu and not lf and nm == common)
    return {"refused": 0, "excess": part1 + part2 + part3, "imputed": imputed, "n_branch": len(part1), "set_difference": len(part2) + len(part3),
            "has_unique": int(hu), "eligible": int(bool(eligible))}


def oracle_answer(ot, sample, j_bfs):
    """OracleTree.node_vecs as lists of unsigned codes, for a comparison with vectors() and with the device."""
    o = ot.node_vecs(sample, int(j_bfs))
    u = lambda l: [(p, a & 255, b & 255, c & 255) for p, a, b, c in l]
    return {"excess": u(o["excess"]), "imputed": u(o["imputed"]), "set_difference": o["set_difference"], "has_unique": int(o["has_unique"])}


def oracle_answer_split(ot, sample, j_bfs):
    """oracle_answer with the two fields the score folds together: n_branch and eligible, from OracleTree.node_vecs_split."""
    o = ot.node_vecs_split(sample, int(j_bfs))
    u = lambda l: [(p, a & 255, b & 255, c & 255) for p, a, b, c in l]
    return {"excess": u(o["excess"]), "imputed": u(o["imputed"]), "set_difference": o["set_difference"], "has_unique": int(o["has_unique"]),
            "n_branch": o["n_branch"], "eligible": o["eligible"]}


def agrees_split(mine, orc):
    """agrees, and n_branch, eligible and set_difference (the score before the +1) each on its own, exactly: orc is an
    oracle_answer_split."""
    return (agrees(mine, orc) and mine["n_branch"] == orc["n_branch"] and mine["eligible"] == orc["eligible"]
            and mine["set_difference"] == orc["set_difference"] - (0 if orc["eligible"] else 1))


def agrees(mine, orc):
    """The closed form, or the device, against the oracle: the lists, has_unique, and the score with its +1 of an ineligible node."""
    return (mine["excess"] == orc["excess"] and mine["imputed"] == orc["imputed"] and mine["has_unique"] == orc["has_unique"]
            and mine["set_difference"] + (0 if mine["eligible"] else 1) == orc["set_difference"])


def device_answers(info, ex_off, ex, im_off, im):
    """Placer.vectors' result as one dict per pair, in the shape of vectors()."""
    rec = lambda a: [(int(x["pos"]), int(x["ref"]), int(x["par"]), int(x["nuc"])) for x in a]
    out = []
    for i in range(len(info)):
        f = info[i]
        assert int(f["n_excess"]) == int(ex_off[i + 1]) - int(ex_off[i]) and int(f["n_imputed"]) == int(im_off[i + 1]) - int(im_off[i])
        out.append({"refused": int(f["refused"]), "excess": rec(ex[int(ex_off[i]):int(ex_off[i + 1])]),
                    "imputed": rec(im[int(im_off[i]):int(im_off[i + 1])]), "n_branch": int(f["n_branch"]),
                    "set_difference": int(f["set_difference"]), "has_unique": int(f["has_unique"]), "eligible": int(f["eligible"])})
    return out
