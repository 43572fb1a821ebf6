"""Shared by the range-level coding tests (test_ranges_host.py, test_gpu_ranges.py): the formulas
of tests/golden/range_cases.json restated (tools/gen_golden_ranges.py), triples of table fixtures,
the three-entry rows a triple stands for, a decoder in Python integers, and the census of the
existing fixtures whose every row total is at most 2^(prec-1)."""
import numpy as np

from conftest import load_golden

RANGE_CASES = load_golden("range_cases.json")
GEN_NAMES = ("lu1000_p48", "peak1000_p61", "lu32000_p48", "peak32000_p48", "lu5000_p61", "u32s_lu1000_p48",
             "u32s_lu32000_p40")


# ------------------------------------------------------------------ the formulas
def cdf_at(case, i):
    """c_i of a formula case; c_{-1} = 0."""
    if i < 0:
        return 0
    return (i + 1) * (i + 1 + case["par"]) if case["kind"] == "quad" else (i + 1) * case["par"]


def total_of(case):
    return cdf_at(case, case["V"] - 1)


def case_triples(case, syms=None):
    syms = case["syms"] if syms is None else syms
    T = total_of(case)
    return [cdf_at(case, s - 1) for s in syms], [cdf_at(case, s) for s in syms], [T] * len(syms)


def symbol_of(case, tgt):
    """bisect_right(cdf, tgt) in Python integers."""
    if case["kind"] != "quad":
        return tgt // case["par"]
    lo, hi = 0, case["V"]                                  # the count of i with c_i <= tgt
    while lo < hi:
        mid = (lo + hi) // 2
        if cdf_at(case, mid) <= tgt:
            lo = mid + 1
        else:
            hi = mid
    return lo


class FormulaModel:
    """decode_loop's model of a formula case, on the device (torch int64)."""

    def __init__(self, case, streams, device):
        import torch
        self.torch, self.case, self.B, self.dev = torch, case, streams, device
        self.T = total_of(case)

    def total(self, t):
        return self.T

    def cdf(self, i):                                      # c_i for a tensor of indices >= -1
        m = i + 1
        return m * (m + self.case["par"]) if self.case["kind"] == "quad" else m * self.case["par"]

    def lookup(self, t, targets):
        torch, V = self.torch, self.case["V"]
        tg = targets.clamp(min=0)
        if self.case["kind"] == "quad":                    # the largest m with m (m + K) <= tgt, m <= V
            K = self.case["par"]
            m = ((torch.sqrt((K * K + 4 * tg).to(torch.float64)) - K) / 2).to(torch.int64).clamp(0, V)
            for _ in range(2):                             # the float estimate is within one
                m = torch.where((m + 1) * (m + 1 + K) <= tg, m + 1, m)
                m = torch.where((m > 0) & (m * (m + K) > tg), m - 1, m)
            s = m.clamp(max=V - 1)
        else:
            s = (tg // self.case["par"]).clamp(max=V - 1)
        return s, self.cdf(s - 1), self.cdf(s)


# ------------------------------------------------------------------ tables
def three_rows(lo, hi, T):
    """[n, 3] uint64: the table [lo, hi - lo, T - hi] of every triple (its symbol 1 is the triple's)."""
    return np.array([[a, b - a, t - b] for a, b, t in zip(lo, hi, T)], dtype=np.uint64).reshape(-1, 3)


def four_rows(lo, hi, T):
    """The same padded to V = 4 (16-byte rows): what the parent commit can code on the device."""
    r = three_rows(lo, hi, T)
    return np.concatenate([r, np.zeros((len(r), 1), dtype=np.uint64)], axis=1)


def table_triples(rows, syms):
    """Python-integer triples of a table job: rows [n or 1][V], syms [n]."""
    out = ([], [], [])
    for t, s in enumerate(syms):
        row = [int(x) for x in rows[t if len(rows) > 1 else 0]]
        out[0].append(sum(row[:s]))
        out[1].append(sum(row[:s + 1]))
        out[2].append(sum(row))
    return out


def qualifies(rows, prec):
    return all(0 < sum(int(x) for x in r) <= 1 << (prec - 1) for r in rows)


def small_qualifying():
    """{'static': [...], 'perstep': [...]}: the cases of small_cases.json with symbols and every row
    total <= 2^(prec-1)."""
    small = load_golden("small_cases.json")
    return {kind: [c for c in small[kind] if c["syms"] and qualifies(c["rows"], c["prec"])]
            for kind in ("static", "perstep")}


def gen_qualifying():
    """The generated fixtures named in GEN_NAMES with their rows (lac_amd.synth)."""
    from lac_amd import synth
    by = {c["name"]: c for c in load_golden("gen_cases.json") + load_golden("straight_cases.json")}
    out = []
    for name in GEN_NAMES:
        c = by[name]
        rows = np.stack([synth.pmf_row(c["seed"], t, 0, c["V"], c["kind"], c["exp_range"]) for t in range(c["steps"])])
        out.append((c, rows))
    return out


# ------------------------------------------------------------------ a decoder in Python integers
def bits_of(data, nbits):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(nbits)]


def py_decode(lo, hi, T, prec, data, nbits):
    """The value-form decoder on triples: -> (targets, ndet, states) with states[t] =
    (l, h, x, pos) before step t (and the final one last).  Bits past the end read as 0."""
    bits = bits_of(data, nbits)
    get = lambda p: bits[p] if p < nbits else 0  # noqa: E731
    l, h, pos = 0, (1 << prec) - 1, prec
    x = 0
    for i in range(prec):
        x = 2 * x + get(i)
    targets, states, ndet, det_all = [], [], 0, True
    for a_, b_, t_ in zip(lo, hi, T):
        states.append((l, h, x, pos))
        w, v = h - l + 1, x - l
        tgt = (v * t_) // w
        targets.append(tgt)
        assert a_ <= tgt < b_
        u = min(max(pos - nbits, 0), prec)
        vhi = v + (1 << u) - 1
        det = vhi < w and (vhi * t_) // w < b_
        det_all = det_all and det
        ndet += det_all
        a, b = -(-(a_ * w) // t_), -(-(b_ * w) // t_)
        h, l = l + b - 1, l + a
        while h - l < 1 << (prec - 1):
            d = l >> (prec - 1)
            l, h = 2 * l - (d << prec), 2 * h + 1 - (d << prec)
            x = 2 * x + get(pos) - (d << prec)
            pos += 1
    states.append((l, h, x, pos))
    return targets, ndet, states
