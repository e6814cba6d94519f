"""The closed form of the record scoring (usher_amd/csrc/ugp_update.hip, the comment above k_touched) restated in plain Python,
from the record dicts of Placer.update and the sample rows:
  D(bottom) = rows (missing calls apart) whose set excludes the reference base
  D(parent) = D(bottom) + sum over the path entries of ([state not in S] - [ref not in S])
  cost      = D(parent) + sum over the own mutations of min([prev in S] - [allele in S], 0)
  eligible  = common > 0 or (internal and no mutations);   has_unique = masked or common != #mutations
with S = the sample's row at the position (all four bases for a missing call), the reference base where it has none."""
INT_MAX = 2 ** 31 - 1


def rows_of(sample):
    return {int(p): (15 if m else int(n) & 15) for p, n, m in zip(sample["pos"], sample["nuc"], sample["is_missing"])}


def d_bottom(sample):
    return sum(1 for r, n, m in zip(sample["ref"], sample["nuc"], sample["is_missing"]) if not m and (int(n) & int(r)) == 0)


def score_record(rec, sample):
    """dict(dbot, d_parent, neg, common, cost, elig, has_unique) of one record for one sample."""
    rows = rows_of(sample)
    dbot = d_bottom(sample)
    d_parent = dbot
    for p, state, ref in rec["path"]:
        s = rows.get(p, ref)
        d_parent += int((s & state) == 0) - int((s & ref) == 0)
    neg = common = 0
    for p, allele, prev, ref in rec["own"]:
        s = rows.get(p, ref)
        c, pr = int((s & allele) != 0), int((s & prev) != 0)
        common += c
        neg += min(pr - c, 0)
    num_mut = len(rec["own"]) + (1 if rec["masked"] else 0)
    return {"dbot": dbot, "d_parent": d_parent, "neg": neg, "common": common, "cost": d_parent + neg,
            "elig": common > 0 or (not rec["leaf"] and num_mut == 0), "has_unique": bool(rec["masked"]) or common != num_mut}


def place(records, samples, live):
    """Per sample (best, {record id: has_unique}) over the live ids; records = {id: record dict} or a list.  (INT_MAX, {}) where
    no live record is eligible."""
    out = []
    for s in samples:
        sc = {r: score_record(records[r], s) for r in live}
        costs = [v["cost"] for v in sc.values() if v["elig"]]
        best = min(costs) if costs else INT_MAX
        out.append((best, {r: v["has_unique"] for r, v in sc.items() if v["elig"] and v["cost"] == best}))
    return out
