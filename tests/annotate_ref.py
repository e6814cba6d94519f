"""Restatements of matUtils annotate (annotate.cpp) for the tests of ugp_clade_alleles / ugp_clade_descendants /
ugp_annotate_search: the exemplar walk of parse_clade_names (:355-390) literally and in closed form, the clade rows it builds
(:395-419), is_ancestor counting (get_freq_overlap, :466-481), and annotate's search (:611-638) through the oracle's literal
mapper2_body in depth-first order with best = 1e9.  Trees are the BFS flat arrays of oracle/refio.tree_to_bfs_arrays."""
import numpy as np

from tests import uncertainty_ref as U

N_NUC = 15   # MAT::get_nuc_id('N')


def _entries(arrays, v):
    return range(int(arrays["mut_off"][v]), int(arrays["mut_off"][v + 1]))


def walk_entries(arrays, x):
    """The entries :361-372 adds for exemplar x (rsearch(x, true)), in walk order: the first non-masked entry of a position wins,
    masked entries are always taken."""
    out, seen = [], set()
    v = int(x)
    while v >= 0:
        for i in _entries(arrays, v):
            p = int(arrays["mut_pos"][i])
            if p < 0 or p not in seen:
                out.append(i)
                if p >= 0:
                    seen.add(p)
        v = int(arrays["parent"][v])
    return out


def alleles_literal(arrays, clade):
    """{entry: count} over the clade's exemplars (repeats count); entries with ref == mut count nothing (:374)."""
    cnt = {}
    for x in clade:
        for i in walk_entries(arrays, x):
            if int(arrays["mut_ref"][i]) != int(arrays["mut_nuc"][i]):
                cnt[i] = cnt.get(i, 0) + 1
    return cnt


def alleles_closed(arrays, clade):
    """The closed form of DESIGN.md 11: count(e) = cnt(u) - sum of cnt(v) over the owners f at v whose nearest owning ancestor
    entry is e; masked entries count cnt(u)."""
    par = np.asarray(arrays["parent"], np.int64)
    n = len(par)
    below = np.zeros(n, np.int64)
    for x in clade:
        below[int(x)] += 1
    for v in range(n - 1, 0, -1):   # BFS order: children after parents
        below[par[v]] += below[v]
    owner = {}
    for v in range(n):
        seen = set()
        for i in _entries(arrays, v):
            p = int(arrays["mut_pos"][i])
            if p >= 0 and p not in seen:
                seen.add(p)
                owner[(v, p)] = i
    cnt = {}
    for (v, p), i in owner.items():
        cnt[i] = cnt.get(i, 0) + int(below[v])
        a = int(par[v])
        while a >= 0 and (a, p) not in owner:
            a = int(par[a])
        if a >= 0:
            e = owner[(a, p)]
            cnt[e] = cnt.get(e, 0) - int(below[v])
    for v in range(n):
        for i in _entries(arrays, v):
            if int(arrays["mut_pos"][i]) < 0:
                cnt[i] = cnt.get(i, 0) + int(below[v])
    return {i: c for i, c in cnt.items() if c > 0 and int(arrays["mut_ref"][i]) != int(arrays["mut_nuc"][i])}


def is_ancestor(arrays, anc, v):
    """Tree::is_ancestor (mutation_annotated_tree.cpp:920-929): starts at v's parent."""
    a = int(arrays["parent"][int(v)])
    while a >= 0:
        if a == int(anc):
            return True
        a = int(arrays["parent"][a])
    return False


def descendants(arrays, clade, node):
    return sum(1 for x in clade if is_ancestor(arrays, node, x))


def clade_rows(arrays, clade, so, min_freq=0.8, mask_freq=0.2, chrom="NC_045512v2"):
    """:392-419 for one clade: rows (key order of the std::map<std::string, int>) then the std::sort by position of :586 --
    replayed with libstdc++'s introsort by `so` (a tests/stdorder.StdOrder), since rows can share a position."""
    counts = {}
    for x in clade:
        for i in walk_entries(arrays, x):
            r, m = int(arrays["mut_ref"][i]), int(arrays["mut_nuc"][i])
            if r != m:
                key = "%s\t%d\t%d\t%d" % (chrom, r, int(arrays["mut_pos"][i]), m)
                counts[key] = counts.get(key, 0) + 1
    rows = []
    k = len(clade)
    for key in sorted(counts, key=lambda s: s.encode()):
        w = key.split("\t")
        f = np.float32(counts[key]) / np.float32(k)
        if f >= np.float32(min_freq):
            rows.append((int(w[2]), int(w[1]), int(w[3])))
        elif f >= np.float32(mask_freq):
            rows.append((int(w[2]), int(w[1]), N_NUC))
    rows = so.sort(rows, key=lambda r: r[0])
    return {"pos": np.asarray([r[0] for r in rows], np.int32), "ref": np.asarray([r[1] for r in rows], np.int8),
            "nuc": np.asarray([r[2] for r in rows], np.int8), "is_missing": np.zeros(len(rows), np.int8)}


def awkward(rows):
    """Rows the packed search refuses: a repeated or a masked (negative) position."""
    p = np.asarray(rows["pos"])
    return bool(len(p) and ((p < 0).any() or len(np.unique(p)) != len(p)))


def search(ot, arrays, rows, dfs=None):
    """annotate's search (:611-638) as a serial run: (best score, tied depth-first positions ascending)."""
    if dfs is None:
        dfs = U.dfs_order(arrays)
    n = len(dfs)
    w = ot.place_list(rows, dfs, jidx=np.arange(n), init_best=10 ** 9, tie_cap=n + 1)
    return w["best"], sorted(int(t) for t in w["ties"])


# ---- annotate_main (:94-156) and assignLineages (both overloads), assignLineagesFromPaths, on refio trees ------------------

def _mut_from_string(s):
    """mutation_from_string (mutation_annotated_tree.cpp:358-380); None when the string does not parse."""
    import re
    from oracle import refio
    m = re.fullmatch(r"([A-Z])(-?\d+)([A-Z])", s)
    if not m:
        return None
    r = refio.get_nuc_id(m.group(1))
    mut = refio.Mutation(int(m.group(2)), r, r, refio.get_nuc_id(m.group(3)))
    return mut if mut.get_string() == s else None


def _split_tab(line):
    """string_split(line, '\\t'): a trailing empty piece is dropped."""
    w = line.split("\t")
    return w[:-1] if w and w[-1] == "" else w


def path_to_node(n):
    """:437-455."""
    parts = []
    while n is not None:
        parts.append(n.identifier + ":" + ",".join(m.get_string() for m in n.mutations))
        n = n.parent
    return " > ".join(reversed(parts))


def _write_mutations(muts, unmasked, masked):
    out = [m.get_string() for m in muts]
    return ", ".join(s for s in out if (unmasked and s[-1] != "N") or (masked and s[-1] == "N"))


def _init(T, clear):
    """init_annotations, :158-168."""
    for n in T.depth_first_expansion():
        if clear:
            n.clade_annotations = []
        n.clade_annotations.append("")
    if len({len(n.clade_annotations) for n in T.depth_first_expansion()}) > 1:
        raise ValueError("ragged annotations")   # the tool exits: the reference would read out of bounds


def assign_from_nids(T, lines, clear):
    """assignLineages(T, clade_to_nid, clear), :170-206.  Returns an error message or None."""
    _init(T, clear)
    for line in lines:
        w = _split_tab(line)
        if len(w) > 2 or len(w) == 1:
            return "ERROR: Incorrect format for clade to node id assignment file"
        n = T.get_node(w[1])
        if n is None:
            return "ERROR: Node id %s not found!" % w[1]
        if n.clade_annotations[-1] == "":
            n.clade_annotations[-1] = w[0]
    return None


def assign_from_paths(T, lines, done):
    """assignLineagesFromPaths, :832-913: the terminal node of each path gets the clade, unless it has one."""
    for line in lines:
        w = _split_tab(line)
        if len(w) == 1 and line.endswith("\t"):
            w.append("")
        assert len(w) == 2, line
        clade = w[0]
        if clade in done:
            continue
        node, ok = T.root, True
        for el in w[1].split():
            if el == ">":
                continue
            muts = _split_tab(el.replace(",", "\t"))
            kid = next((c for c in node.children if len(c.mutations) == len(muts) and
                        all(m.get_string() in muts for m in c.mutations)), None)
            if kid is None:
                ok = False
                break
            node = kid
        if ok:
            if node.clade_annotations[-1] == "":
                node.clade_annotations[-1] = clade
            done.add(clade)


def parse_clade_mutations(lines, done):
    """:208-299 -> ({clade: rows}, error): a first word naming an earlier clade inherits its set; add_mutation merges."""
    from oracle import refio
    allm, err = {}, False
    for line in lines:
        if line.startswith("#"):
            continue
        w = _split_tab(line)
        if len(w) == 1 and line.endswith("\t"):
            w.append("")
        if len(w) != 2 or w[0] in allm:
            err = True
            continue
        node = refio.Node("x", None)
        mw = w[1].split()
        if mw and mw[0] in allm:
            node.mutations = [m.copy() for m in allm[mw[0]]]
            mw = mw[1:]
        for el in mw:
            if el == ">":
                continue
            for s in el.split(","):
                if s == "":
                    continue
                m = _mut_from_string(s)
                if m is None:
                    err = True
                else:
                    node.add_mutation(m)
        allm[w[0]] = node.mutations
    return {c: v for c, v in allm.items() if c not in done}, err


def assign_lineages(T, so, names_lines=None, muts_lines=None, paths_lines=None, min_freq=0.8, mask_freq=0.2, set_overlap=0.6,
                    clip=0.1, clear=False):
    """assignLineages(T, names, mutations, paths, ...), :483-806, with the search run serially through the oracle (depth-first
    order, best = 1e9; ties ascending, the order a serial run gives).  `so`: a tests/stdorder.StdOrder (std::sort replays).
    Returns the -u and -D texts."""
    from oracle import capi, refio
    from tests import usher_model as UM
    f32 = np.float32
    dfs = T.depth_first_expansion()
    dfs_idx = {id(n): k for k, n in enumerate(dfs)}
    _init(T, clear)
    done = set()
    if paths_lines is not None:
        assign_from_paths(T, paths_lines, done)
    clade_muts, clade_map = {}, {}
    if muts_lines is not None:
        clade_muts, err = parse_clade_mutations(muts_lines, done)
        assert not err
    arrays = refio.tree_to_bfs_arrays(T)
    bfs = T.breadth_first_expansion()
    bfs_idx = {id(n): j for j, n in enumerate(bfs)}
    entries = [m for n in bfs for m in n.mutations]
    if names_lines is not None:
        C = UM.copy_tree(T)
        UM.uncondense_leaves(C)
        cdfs = {id(n): k for k, n in enumerate(C.depth_first_expansion())}
        names = {}
        for line in names_lines:
            w = _split_tab(line)
            assert len(w) in (0, 2)
            if len(w) != 2 or w[0] in clade_muts or w[0] in done:
                continue
            n = C.get_node(w[1])
            if n is not None:
                names.setdefault(w[0], []).append(n)
        for clade in sorted(names, key=lambda s: s.encode()):
            counts = {}
            for n in names[clade]:
                for i in walk_entries(arrays, bfs_idx[id(dfs[cdfs[id(n)]])]):
                    m = entries[i]
                    if m.ref_nuc != m.mut_nuc:
                        key = "%s\t%d\t%d\t%d" % (m.chrom, m.ref_nuc, m.position, m.mut_nuc)
                        counts[key] = counts.get(key, 0) + 1
            rows = []
            for key in sorted(counts, key=lambda s: s.encode()):
                w = key.split("\t")
                f = f32(counts[key]) / f32(len(names[clade]))
                if f >= f32(min_freq):
                    rows.append(refio.Mutation(int(w[2]), int(w[1]), int(w[1]), int(w[3]), False, w[0]))
                elif f >= f32(mask_freq):
                    rows.append(refio.Mutation(int(w[2]), int(w[1]), int(w[1]), N_NUC, False, w[0]))
            clade_muts[clade] = rows
            samples = [T.get_node(n.identifier) for n in names[clade]]
            if any(s is None for s in samples):
                raise LookupError(clade)   # get_freq_overlap would dereference a null node
            clade_map[clade] = samples
    ot = capi.OracleTree(arrays)
    dorder = U.dfs_order(arrays)
    u_out = ["clade\tmutations\n"]
    cas = []
    for clade in sorted(clade_muts, key=lambda s: s.encode()):
        rows = so.sort(clade_muts[clade], key=lambda m: m.position)
        u_out.append("%s\t%s\n" % (clade, _write_mutations(rows, True, False)))
        sample = {"pos": np.asarray([m.position for m in rows], np.int32), "ref": np.asarray([m.ref_nuc for m in rows], np.int8),
                  "nuc": np.asarray([m.mut_nuc for m in rows], np.int8), "is_missing": np.zeros(len(rows), np.int8)}
        best, ties = search(ot, arrays, sample, dorder)
        if clade in clade_map:
            samples = clade_map[clade]
            bnf, best_freq = [], f32(-1.0)
            for j in sorted(ties):
                a = dfs[j]
                while a is not None:
                    nd = sum(1 for s in samples if UM._is_ancestor(a, s))
                    freq = f32(nd) / f32(T.get_num_leaves(a))
                    ov = f32(nd) / f32(len(samples))
                    if not (freq >= best_freq and ov >= f32(set_overlap)):
                        break
                    fc = f32(clip) if freq > f32(clip) else freq
                    bnf.append((dfs_idx[id(a)], freq, ov, fc))
                    best_freq = freq
                    a = a.parent
            bnf.sort(key=lambda b: -(b[3] * b[2] * b[2]))   # stable: Node_freq::operator< is > on the product
            cas.append([clade, len(samples), bnf, rows])
        else:
            bnf = []
            if best == 0:   # the first node with the most leaves (:701-712)
                bj, most = 0, 0
                for j in ties:
                    nl = T.get_num_leaves(dfs[j])
                    if nl > most:
                        bj, most = j, nl
                bnf.append((bj, f32(1), f32(1), min(f32(1), f32(clip))))
            cas.append([clade, 0, bnf, rows])
    cas = so.sort(cas, key=lambda c: (int(c[1] > 0) << 62) | (len(c[2]) << 40) | ((1 << 40) - 1 - c[1]))
    d_out = ["clade\tmutations\tmasked_mutations\tnode:freq:overlap\talready_assigned\tfinal_overlap\texemplar_count\tbest_node_path\n"]
    for clade, size, bnf, rows in cas:
        assigned, already = None, []
        for b in bnf:
            n = dfs[b[0]]
            if n.clade_annotations[-1] == "":
                n.clade_annotations[-1] = clade
                assigned = b
                break
            already.append(n.identifier + ":" + n.clade_annotations[-1])
        cand = ", ".join("%s:%f:%f" % (dfs[b[0]].identifier, b[1], b[2]) for b in bnf) or "n/a"
        path = "n/a"
        if assigned is not None:
            path = path_to_node(dfs[assigned[0]])
        elif bnf:
            path = path_to_node(dfs[bnf[0][0]])
        d_out.append("%s\t%s\t%s\t%s\t%s\t%f\t%d\t%s\n" % (clade, _write_mutations(rows, True, False), _write_mutations(rows, False, True),
                     cand, ", ".join(already) or "n/a", assigned[2] if assigned is not None else 0.0, size, path))
    return "".join(u_out), "".join(d_out)
