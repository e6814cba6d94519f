"""matUtils summary --translate restated for the tests (the reference cannot be built here).

LITERAL functions follow matUtils/translate.cpp statement by statement on the breadth-first arrays of tests/synth.py: build_reference,
build_codon_map (with its two strand loops and the codon numbering that continues over a gene's further CDS lines), translate_main's
depth-first walk with undo_mutations at every branch jump, and do_mutations in TSV mode with its string-keyed maps.  render() returns
the text the reference writes.  records() / info() give the answers in the shape of the C ABI (include/usher_amd.h): the records are
what the literal walk saw, the counts come from the definition (the nearest strict ancestor, found by climbing parents).

class Fast gives the ABI-shaped answers for trees too big for the literal walk: one pass in depth-first order over a state array per
position with an undo log of what was really there; the CPU tests hold it against the literal walk on every small case.
"""
import numpy as np

from tests import summary_ref as SR

NUC = SR.NUC
NIL = 0xFFFFFFFF
HEADER = "node_id\taa_mutations\tnt_mutations\tcodon_changes\tleaves_sharing_mutations\n"

# translate.hpp:20-42: the standard code plus the ambiguous codons that still name one amino acid
_TABLE = {
    "A": "GCT GCC GCA GCG GCN", "C": "TGT TGC TGY", "D": "GAT GAC GAY", "E": "GAA GAG GAR", "F": "TTT TTC TTY",
    "G": "GGT GGC GGA GGG GGN", "H": "CAT CAC CAY", "I": "ATT ATC ATA ATH", "K": "AAA AAG AAR",
    "L": "TTA TTG CTT CTC CTA CTG YTR CTN", "M": "ATG", "N": "AAT AAC AAY", "P": "CCT CCC CCA CCG CCN", "Q": "CAA CAG CAR",
    "R": "CGT CGC CGA CGG AGA AGG CGN MGR", "S": "TCT TCC TCA TCG AGT AGC TCN AGY", "T": "ACT ACC ACA ACG ACN",
    "V": "GTT GTC GTA GTG GTN", "W": "TGG", "Y": "TAT TAC TAY", "*": "TAG TAA TGA"}
TRANSLATION = {codon: aa for aa, codons in _TABLE.items() for codon in codons.split()}
COMPLEMENT = dict(zip("ACGTMRWSYKVHDBN", "TGCAKYWSRMBDHVN"))   # translate.hpp:44-49


def translate_codon(nt):
    return TRANSLATION.get(nt, "X")


def complement(c):
    return COMPLEMENT.get(c, "N")


class BadInput(Exception):
    """Where the reference exits with a message, or would read out of bounds (the front end exits 1 with one line instead)."""


def build_reference(text):
    """build_reference (:13-30): header lines dropped, upper-cased, one trailing CR stripped per line."""
    out = []
    for line in text.split("\n")[:-1] if text.endswith("\n") else text.split("\n"):
        if line[:1] == ">" or line == "":
            continue
        line = line.upper()
        if line.endswith("\r"):
            line = line[:-1]
        out.append(line)
    return "".join(out)


class Codon:
    def __init__(self, gene, number, start, nt):
        self.gene, self.number, self.start, self.init = gene, number, start, "".join(nt)
        self.reset()

    def reset(self):
        self.nt = list(self.init)
        self.protein = translate_codon(self.init)

    def mutate(self, pos, letter):
        self.nt[abs(pos - self.start)] = letter
        self.protein = translate_codon("".join(self.nt))

    @property
    def codon_id(self):
        return "%s:%d" % (self.gene, self.number + 1)


def _lines(text):
    return text.split("\n")[:-1] if text.endswith("\n") else text.split("\n")


def _split(s, delim):
    """split (:3-11): getline over a stringstream, so a trailing empty field does not exist."""
    parts = s.split(delim)
    if parts and parts[-1] == "":
        parts.pop()
    return parts


def _gene(field):
    parts = _split(field, '"')
    if len(parts) < 2:
        raise BadInput("gene_id without a quoted name")
    return parts[1]


def build_codon_map(gtf_text, reference):
    """build_codon_map (:42-238).  Returns the codons in creation order; slot k of a codon is position start + k ('+') or start - k
    ('-'), 0-based.  The sign of a codon is recorded for that alone."""
    lines = _lines(gtf_text)
    codons, done = [], []

    def plus(gene, counter, start, stop):
        for pos in range(start - 1, stop, 3):
            if pos < 0 or pos + 2 >= len(reference):
                raise BadInput("CDS past the end of the reference")
            c = Codon(gene, counter, pos, reference[pos:pos + 3])
            c.sign = 1
            codons.append(c)
            counter += 1
        return counter

    def minus(gene, counter, start, stop):
        pos = stop - 1
        while pos > start:     # (a 0-based pos against the 1-based start, as the reference has it)
            if pos >= len(reference) or pos - 2 < 0:
                raise BadInput("CDS past the end of the reference")
            c = Codon(gene, counter, pos, [complement(reference[pos]), complement(reference[pos - 1]), complement(reference[pos - 2])])
            c.sign = -1
            codons.append(c)
            counter += 1
            pos -= 3
        return counter

    def fields(line):
        f = _split(line, "\t")
        if len(f) < 9:
            raise BadInput("fewer than 9 columns")
        return f

    for outer in lines:
        if outer[:1] == "#" or outer == "":
            continue
        f = _split(outer, "\t")
        if len(f) <= 1:
            continue
        f = fields(outer)
        if f[8][:7] != "gene_id":
            raise BadInput("ERROR: GTF file formatted incorrectly. Please see the wiki for details.")
        gene, strand = _gene(f[8]), f[6][:1]
        if f[2] != "CDS":
            continue
        if gene in done:
            continue
        done.append(gene)
        first_start, first_stop = int(f[3]), int(f[4])
        counter = (plus if strand == "+" else minus)(gene, 0, first_start, first_stop)
        for inner in lines:
            if inner[:1] == "#" or inner == "":
                continue
            g = fields(inner)
            if g[2] == "CDS" and _gene(g[8]) == gene:
                start, stop, s2 = int(g[3]), int(g[4]), g[6][:1]
                if start != first_start or strand != s2:
                    counter = (plus if s2 == "+" else minus)(gene, counter, start, stop)
    return codons


def slot_tables(codons):
    """(slot_pos [n, 3] int32, 1-based as mut_pos; slot_init [n, 3] uint8 letters): what ugp_translate_codons takes."""
    pos = np.zeros((len(codons), 3), np.int32)
    init = np.zeros((len(codons), 3), np.uint8)
    for i, c in enumerate(codons):
        for k in range(3):
            pos[i, k] = c.start + c.sign * k + 1
            init[i, k] = ord(c.init[k])
    return pos, init


def codon_map(codons):
    m = {}
    for c in codons:
        for k in range(3):
            m.setdefault(c.start + c.sign * k, []).append(c)
    return m


# ---- literal: the walk -------------------------------------------------------------------------------------------------------

class Mut:
    def __init__(self, arrays, k):
        self.k, self.position = k, int(arrays["mut_pos"][k])
        self.par, self.nuc = SR.nuc(arrays["mut_par"][k]), SR.nuc(arrays["mut_nuc"][k])
        self.string = SR.mut_string(arrays, k)


def _stable(items, key):
    return sorted(items, key=key)


def do_mutations(muts, cmap, sort=_stable):
    """do_mutations (:498-588), taxodium_format == false.  `muts` is sorted in place.  Returns (text or "", touched) where touched
    lists (codon, letters before, letters after, [the mutations of its set]) in the order of affected_codons."""
    muts[:] = sort(muts, lambda m: m.position)
    to_nt, latest, orig_protein, orig_codon, affected = {}, {}, {}, {}, []
    for m in muts:
        pos = m.position - 1
        if pos not in cmap:
            continue
        for c in cmap[pos]:
            cid = c.codon_id
            c.mutate(pos, m.par)
            orig_protein.setdefault(cid, c.protein)
            if not any(c is a for a in affected):
                affected.append(c)
            orig_codon.setdefault(cid, "".join(c.nt))
            c.mutate(pos, m.nuc)
            latest[cid] = "".join(c.nt)
            s = to_nt.setdefault(cid, [])
            if all(x.position != m.position for x in s):      # std::set<Mutation>: operator< looks at the position alone
                s.append(m)
    prot = nuc = cch = ""
    touched = []
    for c in affected:
        cid = c.codon_id
        gene, num = _split(cid, ":")[0], _split(cid, ":")[1]
        prot += gene + ":" + orig_protein[cid] + num + c.protein + ";"
        ms = sorted(to_nt[cid], key=lambda m: m.position)
        for m in ms:
            nuc += m.string + ","
        if nuc and nuc[-1] == ",":
            nuc = nuc[:-1] + ";"
        cch += orig_codon[cid] + ">" + latest[cid] + ";"
        touched.append((c, orig_codon[cid], latest[cid], ms))
    nuc, prot, cch = (s[:-1] if s.endswith(";") else s for s in (nuc, prot, cch))
    if not nuc or not prot or not cch:
        return "", touched
    return prot + "\t" + nuc + "\t" + cch, touched


def undo_mutations(muts, cmap):
    for m in muts:
        pos = m.position - 1
        for c in cmap.get(pos, ()):
            c.mutate(pos, m.par)


def walk(T, codons, sort=_stable):
    """translate_main's loop (:270-291): per node of the depth-first expansion (node, text, touched)."""
    for c in codons:
        c.reset()
    cmap = codon_map(codons)
    muts = [[Mut(T.arrays, k) for k in T.muts(v)] for v in range(T.n)]
    out, last = [], None
    for node in T.dfs():
        par = T.par[node] if node else None
        if last != par:
            anc = set(T.rsearch(node, True))
            trace = last
            while trace not in anc:          # up to the last common ancestor
                undo_mutations(muts[trace], cmap)
                trace = T.par[trace]
        text, touched = do_mutations(muts[node], cmap, sort)
        out.append((node, text, touched))
        last = node
    return out


def n_leaves(T):
    """get_leaves(node).size(): a leaf counts itself."""
    cnt = [0] * T.n
    for v in reversed(T.dfs()):
        if T.is_leaf(v):
            cnt[v] = 1
        if v:
            cnt[T.par[v]] += cnt[v]
    return cnt


def render(T, codons, sort=_stable):
    cnt = n_leaves(T)
    return HEADER + "".join("%s\t%s\t%d\n" % (T.names[v], text, cnt[v]) for v, text, _ in walk(T, codons, sort) if text != "")


# ---- the C ABI's shape -------------------------------------------------------------------------------------------------------

def records(T, codons):
    """[(node, codon index, before, after, (ent0, ent1, ent2))] as ugp_translate writes them on a consistent tree: what the literal
    walk saw, in the order it saw it."""
    index = {id(c): i for i, c in enumerate(codons)}
    out = []
    for node, _, touched in walk(T, codons):
        for c, before, after, ms in touched:
            ent = [NIL, NIL, NIL]
            for m in ms:
                ent[abs(m.position - 1 - c.start)] = m.k
            out.append((node, index[id(c)], before, after, tuple(ent)))
    return out


def info(T, codons):
    """The counts of ugp_tr_info by the definition in include/usher_amd.h:
    {n_records, n_nodes, n_inconsistent, n_duplicate, first_inconsistent, first_duplicate}."""
    cmap = codon_map(codons)
    pos, par_c, nuc_c = T.arrays["mut_pos"], T.arrays["mut_par"], T.arrays["mut_nuc"]

    def owners(v):
        seen = {}
        for k in T.muts(v):
            p = int(pos[k])
            if p >= 0 and p not in seen:
                seen[p] = k
        return seen

    own = [owners(v) for v in range(T.n)]
    n_rec = n_nodes = n_inc = n_dup = 0
    first_inc = first_dup = NIL
    for v in T.dfs():
        coding = [int(pos[k]) for k in T.muts(v) if int(pos[k]) >= 0 and int(pos[k]) - 1 in cmap]
        if len(coding) != len(set(coding)):
            n_dup += 1
            if first_dup == NIL:
                first_dup = v
        touched = set()
        for k in T.muts(v):
            p = int(pos[k])
            if p < 0 or p - 1 not in cmap or own[v][p] != k:
                continue
            a, above = v, None
            while a != 0 and above is None:
                a = T.par[a]
                if p in own[a]:
                    above = SR.nuc(nuc_c[own[a][p]])
            bad = False
            for c in cmap[p - 1]:
                touched.add(id(c))
                before = above if above is not None else c.init[abs(p - 1 - c.start)]
                bad = bad or SR.nuc(par_c[k]) != before
            if bad:
                n_inc += 1
                if first_inc == NIL:
                    first_inc = k
        n_rec += len(touched)
        n_nodes += 1 if touched else 0
    return {"n_records": n_rec, "n_nodes": n_nodes, "n_inconsistent": n_inc, "n_duplicate": n_dup, "first_inconsistent": first_inc,
            "first_duplicate": first_dup}


def consistent(T, codons):
    i = info(T, codons)
    return i["n_inconsistent"] == 0 and i["n_duplicate"] == 0


def device_records(recs):
    """A TR_RECORD array in the shape of records()."""
    return [(int(r["node"]), int(r["codon"]), bytes(r["before"]).decode(), bytes(r["after"]).decode(), tuple(int(e) for e in r["ent"]))
            for r in recs]


# ---- fast --------------------------------------------------------------------------------------------------------------------

class Fast:
    """records() and info() for big trees: a depth-first pass over state[position] with a log of what it overwrote."""

    def __init__(self, arrays, slot_pos, slot_init):
        self.n = n = int(arrays["n"])
        self.parent = np.asarray(arrays["parent"]).astype(np.int64)
        self.off = np.asarray(arrays["mut_off"]).astype(np.int64)
        self.pos = np.asarray(arrays["mut_pos"]).astype(np.int64)
        self.par = np.asarray(arrays["mut_par"]).astype(np.int64)
        self.nuc = np.asarray(arrays["mut_nuc"]).astype(np.int64)
        self.slot_pos = np.asarray(slot_pos).astype(np.int64).reshape(-1, 3)
        self.slot_init = np.asarray(slot_init).astype(np.uint8).reshape(-1, 3)
        kids = [[] for _ in range(n)]
        for j in range(1, n):
            kids[int(self.parent[j])].append(j)
        self.kids = kids
        top = int(max(self.slot_pos.max(initial=0), self.pos.max(initial=0))) + 1
        self.at = [[] for _ in range(top)]          # position -> [(codon, slot)] by codon index
        for c in range(len(self.slot_pos)):
            for k in range(3):
                self.at[int(self.slot_pos[c, k])].append((c, k))
        self._run(top)

    def _run(self, top):
        state = [0] * top            # the allele in force, 0: none
        recs, n_nodes, n_inc, n_dup = [], 0, 0, 0
        first_inc = first_dup = NIL
        stack = [(0, False)]
        logs = {}
        pos, par, nuc, off, at = self.pos, self.par, self.nuc, self.off, self.at
        while stack:
            v, leaving = stack.pop()
            if leaving:
                for p, old in reversed(logs.pop(v)):
                    state[p] = old
                continue
            own, dup = {}, False
            for k in range(int(off[v]), int(off[v + 1])):
                p = int(pos[k])
                if p < 0:
                    continue
                if p in own:
                    dup = dup or bool(at[p])
                else:
                    own[p] = k
            if dup:
                n_dup += 1
                if first_dup == NIL:
                    first_dup = v
            touched = {}
            for p in sorted(own):
                k = own[p]
                if not at[p]:
                    continue
                bad = False
                for c, s in at[p]:
                    before = NUC[state[p]] if state[p] else chr(self.slot_init[c, s])
                    bad = bad or NUC[int(par[k])] != before
                    touched.setdefault(c, (p, c))
                if bad:
                    n_inc += 1
                    if first_inc == NIL:
                        first_inc = k
            for c in sorted(touched, key=touched.get):
                before, after, ent = [], [], []
                for s in range(3):
                    q = int(self.slot_pos[c, s])
                    b = NUC[state[q]] if state[q] else chr(self.slot_init[c, s])
                    before.append(b)
                    after.append(NUC[int(nuc[own[q]])] if q in own else b)
                    ent.append(own[q] if q in own else NIL)
                recs.append((v, c, "".join(before), "".join(after), tuple(ent)))
            n_nodes += 1 if touched else 0
            log = []
            for p, k in own.items():
                log.append((p, state[p]))
                state[p] = int(nuc[k])
            logs[v] = log
            stack.append((v, True))
            stack.extend((c, False) for c in reversed(self.kids[v]))
        self.records = recs
        self.info = {"n_records": len(recs), "n_nodes": n_nodes, "n_inconsistent": n_inc, "n_duplicate": n_dup,
                     "first_inconsistent": first_inc, "first_duplicate": first_dup}
