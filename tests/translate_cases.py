"""Hand-shaped trees, FASTA and GTF texts for matUtils summary --translate (tests/translate_ref.py).

Trees are written as the nested N(mutations, children) of tests/summary_cases.py; a mutation is the reference's string ("A1C": stored
parent allele, 1-based position, allele).  Every Case says which rule it pins, whether the device answers it (`device`: every coding
entry consistent and no coding position twice on a node) or refuses and leaves it to the serial walk, and -- where the answer is
short enough to work out by hand -- the very lines the reference writes (`lines`, without the header).  tests/test_translate_cpu.py
checks those against the literal restatement, so the device tests compare against a yardstick that is known to exercise the rule.

The default genome (75 bases, 1-based):
   1-30  gene A  +   ATG GCT TGT GAT GAA TTT GGT CAT ATT TAA           M A C D E F G H I *
  31-42  gene B  +   AAA CTT ATG AAT   (first CDS)                      K L M N
  43-45              CCC
  46-54  gene B  +   CAA CGT TCT       (second CDS: codons 5-7)         Q R S
  55-59              ACGTA
  60-71  gene M  -   GGG TTT CCC AAA   (four codons, read downwards from 71 on the complement: TTT GGG AAA CCC)
  72                 G
  73-75  gene E  +   TGG               (ends at the last base)          W
   5-19  gene C  +   a second frame over gene A: CTT GTG ATG AAT TTG    (created after B, so its codons have the larger indices)
Codon indices in creation order: A 0-9, B 10-16, M 17-20, E 21, C 22-26.
"""
import numpy as np

from tests import summary_cases as SC
from tests import summary_ref as SR
from tests import translate_ref as R

N, F = SC.N, SC.F

GENOME = "ATGGCTTGTGATGAATTTGGTCATATTTAA" "AAACTTATGAAT" "CCC" "CAACGTTCT" "ACGTA" "GGGTTTCCCAAA" "G" "TGG"
assert len(GENOME) == 75
# a header, lower case, a CR at line ends, an empty line
FASTA = ">ref some description\n" + GENOME[:20].lower() + "\r\n" + GENOME[20:50] + "\n\n" + GENOME[50:] + "\r\n"


def gtf_line(gene, start, stop, strand="+", feature="CDS"):
    return "ref\tsrc\t%s\t%d\t%d\t.\t%s\t0\tgene_id \"%s\"; transcript_id \"%s.1\";" % (feature, start, stop, strand, gene, gene)


GTF = "\n".join(["# comment", gtf_line("A", 1, 30, feature="gene"), gtf_line("A", 1, 30), gtf_line("B", 31, 42), "", gtf_line("B", 46, 54),
                 gtf_line("M", 60, 71, "-"), gtf_line("E", 73, 75), gtf_line("C", 5, 19) + "\r"]) + "\n"


class Case:
    def __init__(self, name, root, rule, device=True, lines=None, fasta=FASTA, gtf=GTF, counts=None):
        self.name, self.rule, self.device, self.lines, self.fasta, self.gtf = name, rule, device, lines, fasta, gtf
        self.arrays, self.tags, _ = SC.build(root)
        self.counts = counts or {}     # the fields of ugp_tr_info a refused case pins (tags for nodes, (tag, i) for entries)

    def __repr__(self):
        return self.name

    def codons(self):
        return R.build_codon_map(self.gtf, R.build_reference(self.fasta))

    def tree(self):
        return SR.Tree(self.arrays)

    def entry(self, tag, i):
        """CSR index of the i-th stored mutation of the tagged node."""
        return int(self.arrays["mut_off"][self.tags[tag]]) + i


def hand_cases():
    c = []
    c.append(Case("single_slots", N((), [N(["A1C"]), N(["T2C"]), N(["G3A"])]), "one mutation in each of slots 0, 1 and 2; leaves print 1",
                  lines=["n1\tA:M1L\tA1C\tATG>CTG\t1", "n2\tA:M1T\tT2C\tATG>ACG\t1", "n3\tA:M1I\tG3A\tATG>ATA\t1"]))
    c.append(Case("two_in_codon", N((), [F(2, ["G3A", "A1C"])]), "two mutations of a node in one codon, stored downwards: ',' joins them in position order",
                  lines=["n1\tA:M1L\tA1C,G3A\tATG>CTA\t2"]))
    c.append(Case("three_in_codon", N((), [F(3, ["G3A", "T2C", "A1C"])]), "three mutations of a node in one codon",
                  lines=["n1\tA:M1P\tA1C,T2C,G3A\tATG>CCA\t3"]))
    c.append(Case("two_codons", N((), [F(2, ["G4A", "G3A", "A1C"])]), "two codons of one node: ';' joins the codons, first touch by position",
                  lines=["n1\tA:M1L;A:A2T\tA1C,G3A;G4A\tATG>CTA;GCT>ACT\t2"]))
    c.append(Case("ancestor_neighbour_slot", N((), [N(["A1C"], [N(["T2C"]), N()])]), "an ancestor mutated the neighbouring slot",
                  lines=["n1\tA:M1L\tA1C\tATG>CTG\t2", "n2\tA:L1P\tT2C\tCTG>CCG\t1"]))
    c.append(Case("ancestor_same_slot", N((), [N(["A1C"], [N(["C1G"]), N()])]), "an ancestor mutated the same slot",
                  lines=["n1\tA:M1L\tA1C\tATG>CTG\t2", "n2\tA:L1V\tC1G\tCTG>GTG\t1"]))
    c.append(Case("back_mutation", N((), [N(["A1C"], [N(["C1A"]), N(["T2C"])])]), "a back-mutation to the reference letter",
                  lines=["n1\tA:M1L\tA1C\tATG>CTG\t2", "n2\tA:L1M\tC1A\tCTG>ATG\t1", "n3\tA:L1P\tT2C\tCTG>CCG\t1"]))
    c.append(Case("predecessor_not_ancestor_enclosed", N((), [N(["A1C"], [F(2, ["C1G"], tag="inner"), N(["T2C"], tag="L")], tag="outer"), N()]),
                  "the owner of position 1 in front of L is not its ancestor; the enclosing one further up is",
                  lines=["n1\tA:M1L\tA1C\tATG>CTG\t3", "n3\tA:L1V\tC1G\tCTG>GTG\t2", "n4\tA:L1P\tT2C\tCTG>CCG\t1"]))
    c.append(Case("predecessor_not_ancestor_none", N((), [F(2, ["A1C"], tag="inner"), N(["T2C"], tag="L"), F(1)]),
                  "the owner of position 1 in front of L is not its ancestor and nothing encloses it: the initial letter",
                  lines=["n1\tA:M1L\tA1C\tATG>CTG\t2", "n2\tA:M1T\tT2C\tATG>ACG\t1"]))
    c.append(Case("two_frames", N((), [F(2, ["T7A", "T6C", "G4A"])]),
                  "position 6 lies in A:2 and C:1, position 7 in A:3 and C:1: order is lowest mutated position first (A:2 at 4, C:1 at 6, "
                  "A:3 at 7), so codon 22 comes before codon 2",
                  lines=["n1\tA:A2T;C:L1P;A:C3S\tG4A,T6C;T6C,T7A;T7A\tGCT>ACC;CTT>CCA;TGT>AGT\t2"]))
    c.append(Case("two_frames_by_index", N((), [F(2, ["T6C"])]), "one position, two codons: by codon index",
                  lines=["n1\tA:A2A;C:L1P\tT6C;T6C\tGCT>GCC;CTT>CCT\t2"]))
    c.append(Case("two_cds", N((), [N(["C46A"]), N(["T42G", "A31G"])]), "the codon numbers of gene B continue across its CDS lines",
                  lines=["n1\tB:Q5K\tC46A\tCAA>AAA\t1", "n2\tB:K1E;B:N4K\tA31G;T42G\tAAA>GAA;AAT>AAG\t1"]))
    c.append(Case("minus_consistent", N((), [N(["T71C"]), N(["T70G"], [N(["T69A", "G70T"]), N()])]),
                  "a - strand gene whose stored parent alleles are the complemented letters the walk holds: descending slots on the device",
                  lines=["n1\tM:F1L\tT71C\tTTT>CTT\t1", "n2\tM:F1C\tT70G\tTTT>TGT\t2", "n3\tM:C1L\tT69A,G70T\tTGT>TTA\t1"]))
    c.append(Case("minus_ordinary", N((), [N(["A71C"], tag="x"), N(["A1C"])]),
                  "an ordinary - strand mutation: the stored parent allele A is not the complemented T the codon starts from", device=False,
                  counts={"n_inconsistent": 1, "first_inconsistent": ("x", 0), "n_duplicate": 0}))
    c.append(Case("masked_and_noncoding", N((), [N(["MASKED", "A1C", "MASKED:-7"]), N(["C44T"]), N(["MASKED"])]),
                  "masked entries are skipped; a node with only non-coding mutations prints no line", lines=["n1\tA:M1L\tA1C\tATG>CTG\t1"]))
    c.append(Case("ambiguous", N((), [N(["A1R"]), N(["T6N"]), N(["T9Y"]), N(["C34Y", "T36R"]), N(["C49M", "T51R"])]),
                  "ambiguous alleles: X when the table has no row, the table's own ambiguous rows otherwise",
                  lines=["n1\tA:M1X\tA1R\tATG>RTG\t1", "n2\tA:A2A;C:L1X\tT6N;T6N\tGCT>GCN;CTT>CNT\t1", "n3\tA:C3C;C:V2X\tT9Y;T9Y\tTGT>TGY;GTG>GYG\t1",
                         "n4\tB:L2L\tC34Y,T36R\tCTT>YTR\t1", "n5\tB:R6R\tC49M,T51R\tCGT>MGR\t1"]))
    c.append(Case("stop_codon", N((), [N(["A33G"]), N(["A31T"]), N(["C46T"])]), "a synonymous change is printed; changes to a stop codon",
                  lines=["n1\tB:K1K\tA33G\tAAA>AAG\t1", "n2\tB:K1*\tA31T\tAAA>TAA\t1", "n3\tB:Q5*\tC46T\tCAA>TAA\t1"]))
    c.append(Case("last_base", N((), [N(["G75A"]), N(["G74A", "T73C"])]), "a codon that ends at the last base of the FASTA",
                  lines=["n1\tE:W1*\tG75A\tTGG>TGA\t1", "n2\tE:W1Q\tT73C,G74A\tTGG>CAG\t1"]))
    c.append(Case("no_coding_mutation", N(["C44T"], [N(["A56C"]), N(["MASKED"]), N()]), "no coding mutation anywhere: the header alone", lines=[]))
    c.append(Case("inconsistent_par", N((), [N(["A1C"], [N(["G1T"], tag="x"), N()]), N(["C2G"], tag="y")]),
                  "stored parent alleles that are not what is above them: G over C, C over the initial T", device=False,
                  counts={"n_inconsistent": 2, "first_inconsistent": ("x", 0), "n_duplicate": 0}))
    c.append(Case("duplicate_coding", N((), [N(["G4C"]), N(["A1C", "T2C", "C1G"], [N()], tag="d"), N(["G3A", "A3G"], tag="d2")]),
                  "a coding position twice on one node (two such nodes; their first entries are consistent)", device=False,
                  counts={"n_inconsistent": 0, "n_duplicate": 2, "first_duplicate": "d"}))
    c.append(Case("duplicate_noncoding", N((), [N(["C44T", "A1C", "T44G"]), N(["C44A"], [N(["A44C", "A44G", "T2C"])])]),
                  "a non-coding position twice on one node is nobody's business",
                  lines=["n1\tA:M1L\tA1C\tATG>CTG\t1", "n3\tA:M1T\tT2C\tATG>ACG\t1"]))
    return c


def _other(letter, k=1):
    return "ACGT"[("ACGT".index(letter) + k) % 4]


def wide65():
    rng = np.random.default_rng(65)
    genome = "".join(rng.choice(list("ACGT"), 210))

    def new(p):
        return _other(genome[p - 1], 1 + p % 3)

    muts = ["%s%d%s" % (genome[p - 1], p, new(p)) for p in range(1, 131, 2)]
    assert len(muts) == 65
    child = ["%s1%s" % (new(1), genome[0]), "%s2%s" % (genome[1], _other(genome[1])), "%s5%s" % (new(5), _other(new(5))),
             "%s129%s" % (new(129), genome[128]), "%s130%s" % (genome[129], _other(genome[129]))]
    return Case("wide65", N((), [N([muts[i] for i in rng.permutation(65)], [N(child[::-1]), N()]), N()]),
                "a node with 65 coding mutations in stored disorder over 43 codons: its row is longer than a wave",
                fasta=">g\n" + genome + "\n", gtf=gtf_line("G", 1, 210) + "\n")


def star600():
    kids = []
    for i in range(600):
        p = 1 + i % 3
        kids.append(N(["%s%d%s" % (GENOME[p - 1], p, _other(GENOME[p - 1], 1 + (i // 3) % 3))]))
    return Case("star600", N((), kids), "a star of 600 leaves that all mutate codon A:1: more records than two blocks cover")


def caterpillar(depth=320):
    """v0 - v1 - ...: v_i flips position 1 between A and C and has a side leaf; every 37th level also flips position 2; side leaves
    mutate position 3 (reading slots 0 and 1 from far above) or position 2."""
    node = N(["G3T"])
    a, b = "AC", "TG"
    for i in range(depth, 0, -1):
        # state of position 1 above v_i: A when i is odd
        muts = ["%s1%s" % (a[(i + 1) % 2], a[i % 2])]
        flips_before = (i - 1) // 37
        if i % 37 == 0:
            muts.insert(0, "%s2%s" % (b[flips_before % 2], b[(flips_before + 1) % 2]))
        flips = i // 37
        side = N(["G3A"]) if i % 3 else N(["%s2%s" % (b[flips % 2], "A")])
        node = N(muts, [node, side], tag="v%d" % i)
    return Case("caterpillar", N((), [node, N(["T2C"])]), "a caterpillar of depth 320 flipping position 1 at every level, position 2 at every 37th")


def all_cases():
    return hand_cases() + [wide65(), star600(), caterpillar()]


def by_name():
    return {c.name: c for c in all_cases()}


WINDOW_CASES = ["wide65", "star600", "caterpillar", "two_frames"]


def n_items(case):
    """ugp_translate's work-items: (owner at a coding position, codon of that position) pairs."""
    T, cmap = case.tree(), R.codon_map(case.codons())
    n = 0
    for v in range(T.n):
        seen = set()
        for k in T.muts(v):
            p = int(case.arrays["mut_pos"][k])
            if p >= 0 and p not in seen:
                seen.add(p)
                n += len(cmap.get(p - 1, ()))
    return n
