"""Restatements of RIPPLES' recombination search (ripples/main.cpp:280-680) for the tests of ugp_ripples / Placer.ripples:
the literal search -- pass 1 through the oracle's literal mapper2_body (orc_place_sample_list / orc_node_vecs), the literal
unmatched-mutation filter, the pair loops with a full sort and the 1000-truncation -- and the closed form the device runs
(bucket counts from the parent's genotype plus per-own-mutation corrections, top-3 per list, the top-2 selection).
Also a generator of trees with a planted recombinant branch.

A raw event is a dict: branch (index in the branch list), i, j, donor, acceptor (BFS), donor_count, acceptor_count,
donor_score, acceptor_score (node_set_difference), donor_sibling, acceptor_sibling."""
from bisect import bisect_left

import numpy as np

from oracle import capi
from tests import synth

KEYS = ("branch", "i", "j", "donor", "acceptor", "donor_count", "acceptor_count", "donor_score", "acceptor_score",
        "donor_sibling", "acceptor_sibling")


def _muts(arrays, v):
    o = arrays["mut_off"]
    return [(int(arrays["mut_pos"][i]), int(arrays["mut_ref"][i]), int(arrays["mut_nuc"][i])) for i in range(int(o[v]), int(o[v + 1]))]


def subtree_sizes(arrays):
    """tree_num_leaves of main.cpp:280-289: subtree NODES, self included."""
    par = np.asarray(arrays["parent"])
    sz = np.ones(len(par), np.int64)
    for j in range(len(par) - 1, 0, -1):
        sz[par[j]] += sz[j]
    return sz


def name_ranks(arrays):
    """Rank of every node's name in std::string (byte-wise) order."""
    names = [s.encode() for s in arrays["names"]]
    order = sorted(range(len(names)), key=lambda k: names[k])
    rank = np.empty(len(names), np.uint32)
    rank[order] = np.arange(len(names), dtype=np.uint32)
    return rank


def is_strict_desc(par, anc, k):
    """T.is_ancestor(anc, k): anc is a strict ancestor of k."""
    while par[k] >= 0:
        k = par[k]
        if k == anc:
            return True
    return False


def pruned_sample(arrays, nid):
    """Pruned_Sample (main.cpp:68-90) of nid's root path: lowest occurrence per position wins, reversions to the reference
    are dropped but take their position, par := ref; sorted by position.  Rows (pos, ref, nuc)."""
    par = np.asarray(arrays["parent"])
    rows, seen = [], set()
    v = int(nid)
    while v >= 0:
        for (p, r, m) in _muts(arrays, v):
            if r != m and p not in seen:
                rows.insert(bisect_left([x[0] for x in rows], p), (p, r, m))
            seen.add(p)
        v = int(par[v])
    return rows


def as_sample(rows):
    return {"pos": np.asarray([r[0] for r in rows], np.int32), "ref": np.asarray([r[1] for r in rows], np.int8),
            "nuc": np.asarray([r[2] for r in rows], np.int8), "is_missing": np.zeros(len(rows), np.int8)}


def valid_pairs(pos, l, r, R):
    """main.cpp:383-413: (i, j) with donor rows [i, j), j < M."""
    M = len(pos)
    out = []
    for i in range(M):
        for j in range(i, M):
            el = pos[j - 1] if j >= 1 else 0
            if (j - i) < l or (M - (j - i)) < l or el - pos[i] < r or el - pos[i] > R:
                continue
            out.append((i, j))
    return out


# ---- the literal search ---------------------------------------------------------------------------------------------

def literal_branch(arrays, ot, nid, bidx, l=3, r=1000, R=10 ** 7, p=3, n_desc=10, sz=None):
    """Raw events of one branch, as main.cpp:300-680 finds them (serial; node_has_unique of the final ties only)."""
    par = np.asarray(arrays["parent"])
    n = len(par)
    sz = subtree_sizes(arrays) if sz is None else sz
    names = [s.encode() for s in arrays["names"]]
    leaf = np.ones(n, bool); leaf[par[1:]] = False
    rows = pruned_sample(arrays, nid)
    pos = [x[0] for x in rows]
    orig = int(arrays["mut_off"][nid + 1] - arrays["mut_off"][nid])
    pairs = valid_pairs(pos, l, r, R)
    if not pairs or orig < p:
        return []
    cand = [k for k in range(n) if sz[k] >= n_desc]
    if not cand:
        return []
    sample = as_sample(rows)
    w = ot.place_list(sample, cand, jidx=cand, compute_scores=True, tie_cap=n + 1)
    score = dict(zip(cand, w["scores"].tolist()))
    tie_hu = dict(zip(w["ties"].tolist(), w["ties_has_unique"].tolist()))
    U = {}
    for k in cand:
        if is_strict_desc(par, nid, k):
            continue
        own = _muts(arrays, k)
        u = []
        for (ep, er, epar, em) in ot.node_vecs(sample, k)["excess"]:
            found = ep >= 0 and any(op == ep and om == em for (op, _, om) in own)
            if not found:
                u.append(ep)
        U[k] = u
    events = []
    for (i, j) in pairs:
        sh, el = pos[i], pos[j - 1]
        acc, don = [], []
        for k, u in U.items():
            nin = sum(1 for x in u if sh <= x <= el)
            nout = len(u) - nin
            if nout + p <= orig:
                acc.append((nout, names[k], k))
            if nin + p <= orig:
                don.append((nin, names[k], k))
        acc.sort(); don.sort()
        acc, don = acc[:1000], don[:1000]
        hit = None
        for d in don:
            for a in acc:
                if d[2] != a[2] and d[2] != nid and a[2] != nid and orig >= d[0] + a[0] + p:
                    hit = (d, a)
                    break
            if hit:
                break
        if hit:
            d, a = hit
            sib = lambda k: bool(leaf[k] or tie_hu.get(k, False))
            events.append({"branch": bidx, "i": i, "j": j, "donor": d[2], "acceptor": a[2], "donor_count": d[0],
                           "acceptor_count": a[0], "donor_score": score[d[2]], "acceptor_score": score[a[2]],
                           "donor_sibling": sib(d[2]), "acceptor_sibling": sib(a[2])})
    return events


def literal(arrays, branches, ot=None, **opts):
    ot = ot or capi.OracleTree(arrays)
    sz = subtree_sizes(arrays)
    out = []
    for b, nid in enumerate(branches):
        out.extend(literal_branch(arrays, ot, int(nid), b, sz=sz, **opts))
    return out


# ---- the closed form (what ugp_ripples.hip computes) -----------------------------------------------------------------

def _lowbit(a):
    for b in range(4):
        if a & (1 << b):
            return 1 << b
    return 0


def closed_branch(arrays, nid, bidx, l=3, r=1000, R=10 ** 7, p=3, n_desc=10, sz=None, rank=None, anc=None, detail=None):
    """Per candidate k: the bucket counts of U_k (2M + 1 buckets: below / at / between the sample positions) from the
    parent's genotype, corrected at k's own mutations by a literal loop 1; pass-1 score and flags from the same terms;
    then top-3 donors / acceptors per pair by (count << 32 | name rank) and the top-2 selection.
    detail: a dict that receives what the search held -- rows, pairs, B, cand, under (the candidates below nid), best (the
    smallest eligible set difference) and, per candidate, S (bucket prefix sums), score, elig, has_unique, nm, common."""
    par = np.asarray(arrays["parent"])
    n = len(par)
    sz = subtree_sizes(arrays) if sz is None else sz
    rank = name_ranks(arrays) if rank is None else rank
    anc = parent_states(arrays) if anc is None else anc
    leaf = np.ones(n, bool); leaf[par[1:]] = False
    rows = pruned_sample(arrays, nid)
    pos = [x[0] for x in rows]
    M = len(rows)
    orig = int(arrays["mut_off"][nid + 1] - arrays["mut_off"][nid])
    B = orig - p
    pairs = valid_pairs(pos, l, r, R)
    cand = [k for k in range(n) if sz[k] >= n_desc]
    if detail is not None:
        detail.update(rows=rows, pairs=pairs, B=B, cand=cand)
    if not pairs or B < 0 or not cand:
        return []
    srow = {x[0]: (x[2], x[1]) for x in rows if x[0] >= 0}
    nb = 2 * M + 1

    def bucket(q):
        lb = bisect_left(pos, q)
        return 2 * lb + (1 if lb < M and pos[lb] == q else 0)

    def term(q, rf, st):   # is there an unmatched entry at q when the ancestral state there is st (0: none)?
        if q in srow:
            s, sr = srow[q]
            return int((s & (st if st else sr)) == 0)
        return int(st != 0 and st != rf)

    base0 = [0] * nb
    for (q, rf, s) in rows:
        if (s & rf) == 0:
            base0[bucket(q)] += 1
    S, score, elig, hu_of, nm_of, common_of = {}, {}, {}, {}, {}, {}
    off = arrays["mut_off"]
    for k in cand:
        cnt = list(base0)
        E = sum(base0)
        v = int(par[k])
        while v >= 0:   # every mutation strictly above k: its term against the state it replaced
            for e in range(int(off[v]), int(off[v + 1])):
                q, rf, m = int(arrays["mut_pos"][e]), int(arrays["mut_ref"][e]), int(arrays["mut_nuc"][e])
                if q < 0:
                    continue
                d = term(q, rf, m) - term(q, rf, anc[e])
                cnt[bucket(q)] += d; E += d
            v = int(par[v])
        own = [(int(arrays["mut_pos"][e]), int(arrays["mut_ref"][e]), int(arrays["mut_nuc"][e]), anc[e]) for e in range(int(off[k]), int(off[k + 1]))]
        kept = [k == 0] * len(own)
        nm = common = 0
        hu = False
        if k != 0:   # loop 1 literally (usher_mapper.cpp:190-264) against the sorted sample
            start = 0
            for x, (q, rf, m, _) in enumerate(own):
                nm += 1
                if q < 0:
                    hu = True
                    break
                found = found_pos = False
                for t in range(start, M):
                    start = t
                    if q == pos[t]:
                        found_pos = True
                        if rows[t][2] & m:
                            found = True
                            break
                    if q < pos[t]:
                        break
                if found or (not found_pos and m == rf):
                    kept[x] = True; common += 1
                else:
                    hu = True
        for x, (q, rf, m, a) in enumerate(own):
            if q < 0:
                if k == 0 and m != rf:   # the root's masked mutations reach loop 3 (usher_mapper.cpp:266-269, 446-470)
                    cnt[bucket(q)] += 1; E += 1
                continue
            st = m if kept[x] else (a if k != 0 else 0)
            ent_k, ent_b = term(q, rf, st), term(q, rf, a if k != 0 else 0)
            if q in srow:
                s, sr = srow[q]
                bq = sr if (s & sr) else _lowbit(s)
            else:
                bq = rf
            u_k = int(ent_k and m != bq)   # an own mutation equal to the entry hides it from U_k (main.cpp:436-449)
            cnt[bucket(q)] += u_k - ent_b
            E += ent_k - ent_b
        el = k == 0 or (hu and not leaf[k] and common > 0 and nm != common) or (leaf[k] and common > 0) or \
            (not hu and not leaf[k] and nm == common)
        score[k] = E + (0 if el else 1)
        elig[k] = el; hu_of[k] = hu and k != 0
        nm_of[k] = nm; common_of[k] = common
        pre = [0]
        for c in cnt:
            pre.append(pre[-1] + c)
        S[k] = pre
    best = min(score[k] for k in cand if elig[k])
    sib = lambda k: bool(leaf[k] or (elig[k] and score[k] == best and hu_of[k]))
    events = []
    keep = [k for k in cand if not is_strict_desc(par, nid, k)]
    if detail is not None:
        kept_set = set(keep)
        detail.update(S=S, score=score, elig=elig, has_unique=hu_of, nm=nm_of, common=common_of, best=best,
                      under=[k for k in cand if k not in kept_set])
    for (i, j) in pairs:
        don, acc = [], []
        for k in keep:
            pre = S[k]
            nin = pre[2 * j] - pre[2 * i + 1]
            nout = pre[nb] - nin
            if nin <= B:
                don.append((nin << 32) | int(rank[k]))
            if nout <= B:
                acc.append((nout << 32) | int(rank[k]))
        don = sorted(don)[:3]; acc = sorted(acc)[:3]
        ev = select(don, acc, int(rank[nid]), B)
        if ev:
            inv = {int(rank[k]): k for k in cand}
            d, a = inv[ev[0] & 0xffffffff], inv[ev[1] & 0xffffffff]
            events.append({"branch": bidx, "i": i, "j": j, "donor": d, "acceptor": a, "donor_count": ev[0] >> 32,
                           "acceptor_count": ev[1] >> 32, "donor_score": score[d], "acceptor_score": score[a],
                           "donor_sibling": sib(d), "acceptor_sibling": sib(a)})
    return events


def select(don, acc, nid_rank, B):
    """main.cpp:594-680 on the top-3 lists (keys count << 32 | rank, ascending): nid removed, the first two of each decide."""
    don = [x for x in don if (x & 0xffffffff) != nid_rank][:2]
    acc = [x for x in acc if (x & 0xffffffff) != nid_rank][:2]
    for d in don:
        for a in acc:
            if (d & 0xffffffff) != (a & 0xffffffff) and (d >> 32) + (a >> 32) <= B:
                return d, a
    return None


def parent_states(arrays):
    """anc[e]: the allele of the nearest non-masked entry above mutation e at its position (0: none)."""
    par = np.asarray(arrays["parent"])
    n = len(par)
    off = arrays["mut_off"]
    geno = [None] * n
    anc = [0] * int(off[n])
    for v in range(n):
        g = dict(geno[par[v]]) if v else {}
        for e in range(int(off[v]), int(off[v + 1])):
            q = int(arrays["mut_pos"][e])
            if q < 0:
                continue
            anc[e] = g.get(q, 0)
        for e in range(int(off[v]), int(off[v + 1])):
            q = int(arrays["mut_pos"][e])
            if q >= 0:
                g[q] = int(arrays["mut_nuc"][e])
        geno[v] = g
    return anc


def closed(arrays, branches, **opts):
    sz, rank, anc = subtree_sizes(arrays), name_ranks(arrays), parent_states(arrays)
    out = []
    for b, nid in enumerate(branches):
        out.extend(closed_branch(arrays, int(nid), b, sz=sz, rank=rank, anc=anc, **opts))
    return out


def default_branches(arrays, l=3, n_desc=10):
    """main.cpp:228-251 without -s: non-root nodes with >= l mutations and >= n_desc true leaves, names sorted (the
    shuffle of :249 is the caller's business; tests take the sorted order)."""
    par = np.asarray(arrays["parent"])
    n = len(par)
    leaf = np.ones(n, bool); leaf[par[1:]] = False
    nl = leaf.astype(np.int64)
    for j in range(n - 1, 0, -1):
        nl[par[j]] += nl[j]
    off = np.asarray(arrays["mut_off"])
    ks = [k for k in range(1, n) if off[k + 1] - off[k] >= l and nl[k] >= n_desc]
    return sorted(ks, key=lambda k: arrays["names"][k].encode())


# ---- fixtures --------------------------------------------------------------------------------------------------------

def planted(seed, n_leaves=300, genome_len=29903, n_sites=600, p_masked=0.0, masked_rows=False, iupac=False):
    """A random tree plus a recombinant branch X under the root: X carries clade A's path mutations inside [x, y] and clade
    B's outside, and gets 12 leaf children (so >= 10 descendants).  X is named "recomb_<seed>"."""
    rng = np.random.default_rng(seed)
    arrays, ref, sites, state = synth.random_tree(rng, n_leaves, genome_len, n_sites, mut_counts=(0, 1, 1, 2, 3, 4),
                                                  p_masked=p_masked, root_muts=int(rng.integers(0, 3)))
    sz = subtree_sizes(arrays)
    n = arrays["n"]
    big = [k for k in range(1, n) if sz[k] >= 12 and len(state[k]) >= 6]
    a, b = rng.choice(big, 2, replace=False) if len(big) >= 2 else (1, 2)
    ga = {p: s for p, s in state[int(a)].items() if s != int(ref[p])}
    gb = {p: s for p, s in state[int(b)].items() if s != int(ref[p])}
    x, y = genome_len // 3, 2 * genome_len // 3
    geno = {p: s for p, s in gb.items() if not (x <= p <= y)}
    geno.update({p: s for p, s in ga.items() if x <= p <= y})
    root_state = dict(state[0])
    muts = []
    for p in sorted(set(geno) | set(root_state)):
        cur = root_state.get(p, int(ref[p]))
        want = geno.get(p, int(ref[p]))
        if want != cur:
            if iupac and rng.random() < 0.1:
                want = want | (1 if want != 1 else 2)
            muts.append((p, int(ref[p]), cur, want))
    if masked_rows:
        muts.insert(0, (-1, 1, 1, 4))
    # rebuild BFS arrays with X (and its leaves) appended: X is a child of the root, so it sorts after the root's other
    # children in the root's child list; renumber breadth-first
    par = list(np.asarray(arrays["parent"]).tolist())
    off = np.asarray(arrays["mut_off"])
    node_muts = [[(int(arrays["mut_pos"][e]), int(arrays["mut_ref"][e]), int(arrays["mut_par"][e]), int(arrays["mut_nuc"][e]))
                  for e in range(int(off[v]), int(off[v + 1]))] for v in range(n)]
    names = list(arrays["names"])
    X = n
    par.append(0); node_muts.append(muts); names.append("recomb_%d" % seed)
    for t in range(12):
        par.append(X); node_muts.append([]); names.append("rleaf_%d_%d" % (seed, t))
        if t % 3 == 0:   # a private mutation on some leaves
            p = int(rng.choice(sites))
            cur = geno.get(p, int(ref[p]))
            node_muts[-1].append((p, int(ref[p]), cur, int(rng.choice([q for q in synth.ONEHOT if q != cur]))))
    return _bfs_arrays(par, node_muts, names)


def _bfs_arrays(par, node_muts, names):
    n = len(par)
    kids = [[] for _ in range(n)]
    for v in range(1, n):
        kids[par[v]].append(v)
    order, h = [0], 0
    while h < len(order):
        order.extend(kids[order[h]]); h += 1
    new = {o: i for i, o in enumerate(order)}
    parent = np.array([-1] + [new[par[o]] for o in order[1:]], np.int64)
    pos, rf, pa, nu, off = [], [], [], [], [0]
    for o in order:
        for (p, r, a, m) in node_muts[o]:
            pos.append(p); rf.append(r); pa.append(a); nu.append(m)
        off.append(len(pos))
    return {"n": n, "parent": parent, "mut_off": np.asarray(off, np.int64), "mut_pos": np.asarray(pos, np.int32),
            "mut_ref": np.asarray(rf, np.int8), "mut_par": np.asarray(pa, np.int8), "mut_nuc": np.asarray(nu, np.int8),
            "names": [names[o] for o in order]}


def node_named(arrays, name):
    return arrays["names"].index(name)


# ---- the host side of ripples/main.cpp: branch order, refinement, combine_intervals, the two files ---------------------

def load_uncondensed(path):
    """load_mutation_annotated_tree + uncondense_leaves (mutation_annotated_tree.cpp:1334-1382), condensed nodes in file order,
    as BFS arrays with names."""
    from oracle import refio
    T = refio.load_mutation_annotated_tree(path)
    for name, leaves in list(T.condensed_nodes.items()):
        n = T.get_node(name)
        par = n.parent if n.parent is not None else n
        if len(leaves) > 1 and n.mutations:
            del T.all_nodes[n.identifier]
            n.identifier = T.new_internal_node_id()
            T.all_nodes[n.identifier] = n
            for s in leaves:
                c = refio.Node(s, n, -1.0)
                T.all_nodes[s] = c
                n.children.append(c)
        elif len(leaves) > 1:
            del T.all_nodes[n.identifier]
            n.identifier = leaves[0]
            T.all_nodes[n.identifier] = n
            for s in leaves[1:]:
                c = refio.Node(s, par, n.branch_length)
                T.all_nodes[s] = c
                par.children.append(c)
        elif len(leaves) == 1:
            del T.all_nodes[n.identifier]
            n.identifier = leaves[0]
            T.all_nodes[n.identifier] = n
    T.condensed_nodes = {}
    return refio.tree_to_bfs_arrays(T)


def branch_order(arrays, so, l=3, n_desc=10, samples=None):
    """main.cpp:196-251: the branch names (default list, or every node on the root paths of `samples`), std::sort, then
    std::shuffle with default_random_engine(0); BFS indices."""
    names = arrays["names"]
    par = np.asarray(arrays["parent"])
    if samples is None:
        chosen = set(default_branches(arrays, l, n_desc))
    else:
        idx = {s: k for k, s in enumerate(names)}
        chosen = set()
        for s in samples:
            v = idx[s]
            while v >= 0:
                chosen.add(v)
                v = int(par[v])
    srt = sorted(chosen, key=lambda k: names[k].encode())
    return so.shuffle(srt)


def leaves_bfs(arrays, v):
    par = np.asarray(arrays["parent"])
    kids = {}
    for j in range(1, len(par)):
        kids.setdefault(int(par[j]), []).append(j)
    out, q, h = [], [v], 0
    while h < len(q):
        x = q[h]; h += 1
        if x not in kids:
            out.append(x)
        q.extend(kids.get(x, []))
    return out


def combine_intervals(pairs, so):
    """main.cpp:133-164, with this library's std::sort orders.  An interval: dict d, a (name, node_parsimony, parsimony,
    is_sibling), sl, sh, el, eh."""
    pairs = so.sort(list(pairs), key=lambda x: x["el"])
    i = 0
    while i < len(pairs):
        j = i + 1
        while j < len(pairs):
            x, y = pairs[i], pairs[j]
            if (x["d"][0] == y["d"][0] and x["a"][0] == y["a"][0] and x["sl"] == y["sl"] and x["sh"] == y["sh"] and x["eh"] == y["el"]
                    and x["d"][2] + x["a"][2] == y["d"][2] + y["a"][2]):
                x["eh"] = y["eh"]
                del pairs[j]
            else:
                j += 1
        i += 1
    pairs = so.sort(pairs, key=lambda x: x["sl"])
    i = 0
    while i < len(pairs):
        j = i + 1
        while j < len(pairs):
            x, y = pairs[i], pairs[j]
            if (x["d"][0] == y["d"][0] and x["a"][0] == y["a"][0] and x["el"] == y["el"] and x["eh"] == y["eh"] and x["sh"] == y["sl"]
                    and x["d"][2] + x["a"][2] == y["d"][2] + y["a"][2]):
                x["sh"] = y["sh"]
                del pairs[j]
            else:
                j += 1
        i += 1
    return pairs


def render(arrays, order, so, l=3, r=1000, R=10 ** 7, p=3, n_desc=10, S=-1, E=-1, ot=None):
    """descendants.tsv and recombination.tsv of main.cpp:255-702 for the branch order `order`, events from the literal search."""
    ot = ot or capi.OracleTree(arrays)
    names = arrays["names"]
    sz = subtree_sizes(arrays)
    desc = "#node_id\tdescendants\n"
    rec = ("#recomb_node_id\tbreakpoint-1_interval\tbreakpoint-2_interval\tdonor_node_id\tdonor_is_sibling\tdonor_parsimony\t"
           "acceptor_node_id\tacceptor_is_sibling\tacceptor_parsimony\toriginal_parsimony\tmin_starting_parsimony\trecomb_parsimony\n")
    s, e = 0, len(order)
    if S >= 0 and E >= 0:
        s = S
        e = min(e, E)
    for idx in range(s, e):
        nid = order[idx]
        orig = int(arrays["mut_off"][nid + 1] - arrays["mut_off"][nid])
        ps = pruned_sample(arrays, nid)
        ppos = [x[0] for x in ps]
        valid = []
        for ev in literal_branch(arrays, ot, nid, 0, l=l, r=r, R=R, p=p, n_desc=n_desc, sz=sz):
            i, j = ev["i"], ev["j"]
            sh, sl = ppos[i], ppos[i - 1] if i >= 1 else 0
            el, eh = ppos[j - 1] if j >= 1 else 0, 10 ** 9
            dpos = [x[0] for x in pruned_sample(arrays, ev["donor"])]
            for mp in dpos:
                if sl < mp <= sh and mp not in ppos:
                    sl = mp
                if el < mp <= eh and mp not in ppos:
                    eh = mp
            for mp in ppos:
                if sl < mp <= sh and mp not in dpos:
                    sl = mp
                if el < mp <= eh and mp not in dpos:
                    eh = mp
            sib = lambda b: "y" if b else "n"
            valid.append({"d": (names[ev["donor"]], ev["donor_score"], ev["donor_count"], sib(ev["donor_sibling"])),
                          "a": (names[ev["acceptor"]], ev["acceptor_score"], ev["acceptor_count"], sib(ev["acceptor_sibling"])),
                          "sl": sl, "sh": sh, "el": el, "eh": eh})
        for x in combine_intervals(valid, so):
            ehs = "GENOME_SIZE" if x["eh"] == 10 ** 9 else str(x["eh"])
            rec += "%s\t(%d,%d)\t(%d,%s)\t%s\t%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\n" % (
                names[nid], x["sl"], x["sh"], x["el"], ehs, x["d"][0], x["d"][3], x["d"][1], x["a"][0], x["a"][3], x["a"][1], orig,
                min(orig, x["d"][1], x["a"][1]), x["d"][2] + x["a"][2])
        if valid:
            desc += names[nid] + "\t" + "".join(names[v] + "," for v in leaves_bfs(arrays, nid)) + "\n"
    return desc, rec
