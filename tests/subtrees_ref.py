"""get_minimum_subtrees (matUtils convert.cpp:665-798) for -t, restated over breadth-first arrays: the cover loop statement by
statement on tests/nearest_ref.literal (get_nearby), every neighbourhood's subtree from tests/subtree_ref.literal (get_subtree),
write_newick_string (mutation_annotated_tree.cpp:215-346, print_internal and print_branch_len set, the branch length forced to the
number of mutations) and the assignment table.

`cover` returns the sample sets in the order they are made and samples_we_have_seen; `files` the bytes of every file the
reference writes, by path."""
from tests import nearest_ref as NR
from tests import subtree_ref as SR


def cover(T, samples, n, sorter=None):
    """:681-711.  samples: BFS indices in the order given (names twice stay); sorter: tests/stdorder.StdOrder for the reference's tie
    order, None for the canonical one."""
    seen, sets = {}, []
    for s in samples:
        if s in seen:
            continue
        keep = NR.literal(T, int(s), n, sorter)["nodes"]
        if not keep:
            seen[s] = -1
            continue
        for l in keep:
            seen.setdefault(l, len(sets))   # insert: the first subtree that holds a sample owns it
        sets.append([int(l) for l in keep])
    return sets, seen


def _float(x):
    return "%g" % float(x)   # operator<<(float): six significant digits


def newick(names, parent, nmut):
    """write_newick_string(ss, T, T.root, true, true, false) for a tree given as its nodes in depth-first order: names, the index
    of each node's parent (NIL: the root, which is node 0) and each node's number of mutations."""
    n = len(names)
    kids, level = [[] for _ in range(n)], [1] * n
    for k in range(1, n):
        kids[parent[k]].append(k)
        level[k] = level[parent[k]] + 1
    traversal, stack = [], [0]
    while stack:   # depth_first_expansion
        v = stack.pop()
        traversal.append(v)
        stack.extend(reversed(kids[v]))
    out, curr, prev_open, node_stack, len_stack = [], 0, True, [], []
    level_offset = level[0] - 1
    for v in traversal:
        lv, bl, leaf = level[v] - level_offset, float(nmut[v]), not kids[v]
        if curr < lv:
            if not prev_open:
                out.append(",")
            l = lv - 1
            if curr > 1:
                l = lv - curr
            for _ in range(l):
                out.append("(")
                prev_open = True
            if leaf:
                out.append(names[v])
                if bl >= 0:
                    out.append(":" + _float(bl))
                prev_open = False
            else:
                node_stack.append(names[v])
                len_stack.append(bl)
        elif curr > lv:
            prev_open = False
            for _ in range(lv, curr):
                out.append(")" + node_stack.pop())
                top = len_stack.pop()
                if top >= 0:
                    out.append(":" + _float(top))
            if leaf:
                out.append("," + names[v])
                if bl >= 0:
                    out.append(":" + _float(bl))
            else:
                node_stack.append(names[v])
                len_stack.append(bl)
        else:
            prev_open = False
            if leaf:
                out.append("," + names[v])
                if bl >= 0:
                    out.append(":" + _float(bl))
            else:
                node_stack.append(names[v])
                len_stack.append(bl)
        curr = lv
    while node_stack:
        out.append(")" + node_stack.pop())
        top = len_stack.pop()
        if top >= 0:
            out.append(":" + _float(top))
    out.append(";")
    return "".join(out)


def subtree_newick(arrays, names, sel):
    res = SR.literal(arrays, sel)
    nmut = [int(res["ent_off"][k + 1]) - int(res["ent_off"][k]) for k in range(len(res["kept"]))]
    return newick([names[int(v)] for v in res["kept"]], [int(p) for p in res["parent"]], nmut)


def files(arrays, names, samples, n, prefix, tree_name, sorter=None):
    """{path: bytes} of <prefix><tree_name>-subtree-<i>.nw (:724-731: the stream as it is, no newline) and
    <prefix>subtree-assignments.tsv (:748-797, no metadata), with the sets and samples_we_have_seen."""
    T = NR.Tree(arrays)
    sets, seen = cover(T, [int(s) for s in samples], n, sorter)
    newick_n = prefix + tree_name
    out = {"%s-subtree-%d.nw" % (newick_n, i): subtree_newick(arrays, names, s).encode() for i, s in enumerate(sets)}
    rows = ["samples\tnewick_file\n"]
    for s in samples:
        v = seen.get(int(s), 0)   # operator[] of the map: a sample that no subtree holds and nothing marked reads 0
        if v == -1:
            continue
        rows.append("%s\t%s-subtree-%d.nw\n" % (names[int(s)], newick_n, v))
    out[prefix + "subtree-assignments.tsv"] = "".join(rows).encode()
    return out, sets, seen
