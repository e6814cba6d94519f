"""make_vcf (matUtils convert.cpp:14-320) restated over the breadth-first arrays of tests/synth.py, two ways.

`literal(arrays, nodes)` is r_add_genotypes + VCF_Line_Writer line by line: the stack of the root path's non-masked mutations, pushed
whole at every selected node into per-position lists (REF from the first insertion, the overwrite of leaf_genotypes.back()), then
count_alleles / make_alts (a std::map: ascending allele code) / make_allele_codes per position in ascending position.
`fast(arrays, nodes)` (class Fast, for several selections of one tree) is the closed form with numpy: the owners of a position are
nested depth-first ranges, an owner's columns are rank[dend] - rank[start], and it is the innermost owner of its columns minus
those of the owners directly below it; rows are painted outermost first.

Both return Result(sites, codes, text, columns): sites a list of dicts (pos, ref, alt, ac, covered), codes a uint8 array
[sites, columns], text the VCF file, columns the selected nodes in depth-first order.  nodes: breadth-first indices, None or empty:
all leaves."""
from collections import namedtuple

import numpy as np

NUC = "NACMGRSVTWYHKDBN"   # MAT::get_nuc, mutation_annotated_tree.cpp:88-139
CHROM = "NC_045512v2"
Result = namedtuple("Result", "sites codes text columns")


def _kids(par):
    kids = [[] for _ in range(len(par))]
    for j in range(1, len(par)):
        kids[par[j]].append(j)
    return kids


def _selection(arrays, kids, nodes):
    if nodes is None or len(nodes) == 0:
        return {j for j in range(arrays["n"]) if not kids[j]}
    return {int(v) for v in nodes}


def _header(names, columns, genotypes):
    h = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    if genotypes:
        h += "\tFORMAT" + "".join("\t" + names[v] for v in columns)
    return h + "\n"


def literal(arrays, nodes=None, genotypes=True, chrom=CHROM):
    par = np.asarray(arrays["parent"]).astype(np.int64)
    off = np.asarray(arrays["mut_off"]).astype(np.int64)
    pos, mpar, nuc = (np.asarray(arrays[k]).astype(np.int64) for k in ("mut_pos", "mut_par", "mut_nuc"))
    names = arrays.get("names") or ["n%d" % j for j in range(len(par))]
    kids = _kids(par)
    use = _selection(arrays, kids, nodes)
    leaf_count = len(use)
    info = {}       # pos -> [ref, [[leaf_ix, genotype], ...]]
    columns = []
    mut_stack = []
    leaf_ix = 0
    work = [(0, False)]
    while work:     # r_add_genotypes; (node, True) is the pop_back loop after the children
        v, leaving = work.pop()
        own = [k for k in range(off[v], off[v + 1]) if pos[k] >= 0]
        if leaving:
            del mut_stack[len(mut_stack) - len(own):]
            continue
        mut_stack.extend(own)
        if v in use:
            for k in mut_stack:
                p = int(pos[k])
                if p not in info:
                    info[p] = [int(mpar[k]), []]
                gts = info[p][1]
                if not gts or gts[-1][0] < leaf_ix:
                    gts.append([leaf_ix, int(nuc[k])])
                else:
                    gts[-1][1] = int(nuc[k])
            columns.append(v)
            leaf_ix += 1
        work.append((v, True))
        work.extend((c, False) for c in reversed(kids[v]))
    sites, rows = [], []
    text = [_header(names, columns, genotypes)]
    for p in sorted(info):   # VCF_Line_Writer
        ref, gts = info[p]
        counts = {}
        for _, a in gts:
            counts[a] = counts.get(a, 0) + 1
        alts = dict(sorted((a, c) for a, c in counts.items() if a != ref))   # the std::map of make_alts
        if not alts:
            continue         # "no-alternative site encountered in vcf output; skipping"
        ident = ",".join(NUC[ref] + str(p) + NUC[a] for a in alts)
        line = "%s\t%d\t%s\t%s\t%s\t.\t.\tAC=%s;AN=%d" % (chrom, p, ident, NUC[ref], ",".join(NUC[a] for a in alts),
                                                           ",".join(str(c) for c in alts.values()), leaf_count)
        codes = {a: 1 + i for i, a in enumerate(alts)}
        row = np.zeros(leaf_count, np.uint8)
        for ix, a in gts:
            row[ix] = codes.get(a, 0)
        if genotypes:
            line += "\tGT" + "".join("\t%d" % c for c in row)
        text.append(line + "\n")
        sites.append({"pos": p, "ref": ref, "alt": list(alts), "ac": list(alts.values()), "covered": len(gts)})
        rows.append(row)
    codes = np.array(rows, np.uint8).reshape(len(rows), leaf_count)
    return Result(sites, codes, "".join(text), np.array(columns, np.int64))


class Fast:
    def __init__(self, arrays):
        self.arrays = arrays
        par = np.asarray(arrays["parent"]).astype(np.int64)
        n = self.n = len(par)
        self.kids = kids = _kids(par)
        order, st = [], [0]
        while st:
            v = st.pop()
            order.append(v)
            st.extend(reversed(kids[v]))
        self.dfs = np.array(order, np.int64)
        self.pre = np.empty(n, np.int64)
        self.pre[self.dfs] = np.arange(n)
        size = np.ones(n, np.int64)
        for v in reversed(order[1:]):
            size[par[v]] += size[v]
        self.leaf = np.array([not k for k in kids])
        off = np.asarray(arrays["mut_off"]).astype(np.int64)
        pos, mpar, nuc = (np.asarray(arrays[k]).astype(np.int64) for k in ("mut_pos", "mut_par", "mut_nuc"))
        node = np.repeat(np.arange(n), np.diff(off))
        keep = np.flatnonzero(pos >= 0)
        # owners: the first kept entry of each (node, position); its allele from the last one
        key = node[keep] * (int(pos.max(initial=0)) + 2) + pos[keep]
        srt = np.argsort(key, kind="stable")
        ks = key[srt]
        first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if len(ks) else np.zeros(0, np.int64)
        last = np.r_[first[1:] - 1, len(ks) - 1] if len(ks) else first
        e_first, e_last = keep[srt[first]], keep[srt[last]]
        o = np.lexsort((self.pre[node[e_first]], pos[e_first]))
        self.opos = pos[e_first][o]
        self.ostart = self.pre[node[e_first]][o]
        self.oend = self.ostart + size[node[e_first]][o]
        self.opar = mpar[e_first][o]
        self.oal = nuc[e_last][o]
        # the owner above: a stack per position
        up = np.full(len(o), -1, np.int64)
        stack, cur = [], None
        ostart, oend, opos = self.ostart.tolist(), self.oend.tolist(), self.opos.tolist()
        for x in range(len(o)):
            if opos[x] != cur:
                cur, stack = opos[x], []
            while stack and oend[stack[-1]] <= ostart[x]:
                stack.pop()
            if stack:
                up[x] = stack[-1]
            stack.append(x)
        self.up = up

    def run(self, nodes=None, rows=True, genotypes=True, chrom=CHROM, text=True):
        a = self.arrays
        flag = np.zeros(self.n + 1, np.int64)
        if nodes is None or len(nodes) == 0:
            flag[:self.n][self.pre[np.flatnonzero(self.leaf)]] = 1
        else:
            flag[self.pre[np.asarray(nodes, np.int64)]] = 1
        rank = np.r_[0, np.cumsum(flag[:self.n])]
        n_cols = int(rank[-1])
        columns = self.dfs[np.flatnonzero(flag[:self.n])]
        ln = rank[self.oend] - rank[self.ostart]
        plist, pidx = np.unique(self.opos, return_inverse=True)
        cnt = np.zeros((len(plist), 16), np.int64)
        np.add.at(cnt, (pidx, self.oal), ln)
        has = self.up >= 0
        np.subtract.at(cnt, (pidx[has], self.oal[self.up[has]]), ln[has])
        cov = np.zeros(len(plist), np.int64)
        np.add.at(cov, pidx[~has], ln[~has])
        live = np.flatnonzero(ln > 0)
        jj, fi = np.unique(pidx[live], return_index=True)   # the first owner with columns, per position
        sites, site_of = [], {}
        for j, x in zip(jj.tolist(), live[fi].tolist()):
            ref = int(self.opar[x])
            alts = [(al, int(cnt[j, al])) for al in range(16) if al != ref and cnt[j, al]]
            if alts:
                site_of[j] = len(sites)
                sites.append({"pos": int(plist[j]), "ref": ref, "alt": [al for al, _ in alts], "ac": [c for _, c in alts], "covered": int(cov[j])})
        codes = None
        if rows:
            codes = np.zeros((len(sites), n_cols), np.uint8)
            maps = np.zeros((len(sites), 16), np.uint8)
            for s, site in enumerate(sites):
                maps[s, site["alt"]] = 1 + np.arange(len(site["alt"]))
            lo, hi = rank[self.ostart], rank[self.oend]
            for x in live.tolist():   # ascending start within a position: outer ranges first, inner ones paint over them
                s = site_of.get(int(pidx[x]))
                if s is not None:
                    codes[s, lo[x]:hi[x]] = maps[s, self.oal[x]]
        out = None
        if text and (rows or not genotypes):
            names = a.get("names") or ["n%d" % j for j in range(self.n)]
            parts = [_header(names, columns, genotypes)]
            for s, site in enumerate(sites):
                r = NUC[site["ref"]]
                line = "%s\t%d\t%s\t%s\t%s\t.\t.\tAC=%s;AN=%d" % (chrom, site["pos"], ",".join(r + str(site["pos"]) + NUC[al] for al in site["alt"]), r,
                                                                   ",".join(NUC[al] for al in site["alt"]), ",".join(map(str, site["ac"])), n_cols)
                if genotypes:
                    line += "\tGT\t" + "\t".join(map(str, codes[s].tolist())) if n_cols else "\tGT"
                parts.append(line + "\n")
            out = "".join(parts)
        return Result(sites, codes, out, columns)


def fast(arrays, nodes=None, genotypes=True, chrom=CHROM):
    return Fast(arrays).run(nodes, genotypes=genotypes, chrom=chrom)


def site_rows(sites):
    """The site dicts as tuples, for comparisons."""
    return [(s["pos"], s["ref"], tuple(s["alt"]), tuple(s["ac"]), s["covered"]) for s in sites]


def device_sites(tab):
    """A Placer.GT_SITE array as the tuples of site_rows."""
    return [(int(t["pos"]), int(t["ref"]), tuple(int(x) for x in t["alt"][:t["n_alt"]]), tuple(int(x) for x in t["ac"][:t["n_alt"]]),
             int(t["covered"])) for t in tab]


def sites_from_device(tab):
    """A Placer.GT_SITE array as site dicts."""
    return [{"pos": p, "ref": r, "alt": list(a), "ac": list(c), "covered": v} for p, r, a, c, v in device_sites(tab)]


def compare_with_vcf(path, result, names):
    """A VCF of the same samples against `result`, at every cell whose VCF allele is one unambiguous base (a position that is no
    site of `result` carries the VCF's REF everywhere).  Returns (cells compared, cells that disagree)."""
    import gzip
    col = {names[v]: i for i, v in enumerate(result.columns)}
    site = {s["pos"]: k for k, s in enumerate(result.sites)}
    cells = bad = 0
    for line in gzip.open(path, "rt"):
        if line.startswith("##"):
            continue
        f = line.rstrip("\n").split("\t")
        if line.startswith("#"):
            samples = f[9:]
            assert all(s in col for s in samples)
            continue
        alleles = [f[3]] + f[4].split(",")
        k = site.get(int(f[1]))
        for s, g in zip(samples, f[9:]):
            g = g.split(":")[0]
            if g == "." or alleles[int(g)] not in "ACGT":
                continue
            cells += 1
            mine = f[3]
            if k is not None:
                c = int(result.codes[k, col[s]])
                mine = NUC[result.sites[k]["ref"] if c == 0 else result.sites[k]["alt"][c - 1]]
            bad += mine != alleles[int(g)]
    return cells, bad
