"""Rows that pin the sampler's truncation threshold to the key (kr_sample_threshold), its filter (kr_gumbel_argmax_processed)
and the partition reduction (kr_sample_greedy): shared by tests/test_select_cases_cpu.py, which proves every case on the
reference alone, and tests/test_gpu_sampling_select.py, which runs them on the device.

A threshold is a uint32 key (sampling_ref.fkey: order preserving, -0 below +0).  `radix_select` (kr_sample.hip) finds it in
three histogram levels of 11 / 11 / 10 key bits, lane l of wave 0 owning nb / 64 bins of a level, highest first.  The rows
here are built from the KEYS they should hold (`unkey`), so that the cut falls where that code can go wrong:

count mode (top_k)   `landmark_keys`: the product of level-0 digits {lowest and highest finite bin, both sides of the sign
                     border, both sides of lane borders} with level-1 and level-2 digits {0, 1, last / first bin of a lane,
                     top}, without the NaN, inf and subnormal patterns: of bins 1023 / 1024 / 1025 only -0 and +0 remain.  (With
                     lanes owning 32 bins from the top, the level-0 lane borders are 31 | 32, 1055 | 1056 and 2015 | 2016; 35 | 36
                     and 2011 | 2012 lie four bins inside a lane, as bin 4 is the lowest finite one.)  639 keys,
                     each on 1..3 tokens at shuffled positions, one row per k = 1 .. tokens + 2, the rest of the row
                     -inf or -3e38 (a finite fill: k above the landmark count lands on the fill's key, in the lowest finite
                     bin).  Expected: the key of the k-th largest finite score, from a sort; no excusals.
mass mode (top_p)    groups of equal score: +-2^e for e = -126 .. -10 with +0 and -0 (weights ~ 1, cuts on both sides of the
                     sign border and between the zeros), the 40 adjacent floats around 2^e (the level-0 digit changes between
                     two neighbours), 8 - j / 4 (weights e^(-j/4)).  For the cut at group j, top_p = f32 of the midpoint of
                     the group's mass interval; a case exists only if that f32 value keeps MARGIN = 2^-10 of the total from
                     both ends of the interval.  The device moves a cumulative mass by at most V * 2^-32 of the total for the
                     32.32 truncation (2^-14.8 at V = 151936) and about 2^-18 for __expf at |x| <= 22: MARGIN is 16 times
                     their sum.  It is a condition on the case, not a measurement.  Expected: the key of group j.
combined             top_k then top_p (the total runs over what top_k kept), min_p with its f32 cut 8 keys from the nearest
                     score and the sum m + ln(min_p) far from a rounding tie (so the cut is one key whatever the last bits
                     of logf), top_k above what min_p left (lo comes back), every family behind penalties (rep 2, freq 0.5,
                     pres 0.25: dyadic, the landmarks are built on the penalised scores) and behind a guide mask that removes
                     every second token of the cut group.
filter               kept tokens exactly at the threshold, ten times as many one key below it, a seed (searched on the CPU)
                     under which a dropped token has the row's largest noise: the token must be the kept one with the
                     largest noise.
partitions           n_part 1 .. 1100 at the three vocabularies, the winner in the first, the last non-empty (ragged)
                     partition and on the last token; hand-written partials for kr_sample_greedy's eight-wide read.

Every row runs at T = 1 (v = l * (1 / T) is the logit itself) and every score is a finite normal f32, a zero or -inf.

`threshold_model` restates sample_threshold_kernel / radix_select in numpy with integer histograms and the same three levels;
`BUGS` names mistakes it can be told to make (the CPU module shows each of them returning a wrong key on these rows)."""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

from oracle import qwen2vl_oracle as O
from tests import sampling_ref as R

VS = (4099, 4100, 4101)              # one pass of radix_select's 4 * 1024 stride plus a ragged tail; not multiples of 4
V_PROD = 151936
NEG_INF_KEY = 0x007FFFFF             # fkey(-inf)
LO0 = NEG_INF_KEY + 1                # every finite score: the select's floor without min_p (= fkey(-FLT_MAX))
MARGIN = 2.0 ** -10
FILL_FINITE = np.float32(-3e38)
PEN = (2.0, 0.5, 0.25)               # repetition, frequency, presence
TINY = np.float32(2.0 ** -126)
L0_DIGITS = (4, 5, 31, 32, 35, 36, 1023, 1024, 1025, 1055, 1056, 2011, 2012, 2015, 2016, 2043)
L1_DIGITS = (0, 1, 31, 32, 2015, 2016, 2047)
L2_DIGITS = (0, 1, 15, 16, 1007, 1008, 1023)
BUGS = ("gt", "lanes_low_first", "lvl2_2048", "no_invert", "no_reduce", "no_hi_mask", "total_all")
FILTER_BUG = "filter_le"


# ----------------------------------------------------------------------------- keys
def unkey(k) -> np.ndarray:
    """fp32 values of uint32 keys: the inverse of sampling_ref.fkey."""
    k = np.asarray(k, np.uint64)
    u = np.where((k & 0x80000000) != 0, k & 0x7FFFFFFF, (~k) & 0xFFFFFFFF).astype(np.uint32)
    return u.view(np.float32)


def digits(k):
    k = int(k)
    return (k >> 21) & 2047, (k >> 10) & 2047, k & 1023


def describe(family, want, got):
    return (f"{family}: expected key {int(want):#010x} (digits {digits(want)}, score {float(unkey(want)):.9g}), "
            f"returned {int(got):#010x} (digits {digits(got)}, score {float(unkey(got)):.9g})")


def is_score(v):
    """finite normal f32, a zero, or -inf"""
    v = np.asarray(v, np.float32)
    return bool((np.isneginf(v) | (np.isfinite(v) & ((np.abs(v) >= TINY) | (v == 0)))).all())


@lru_cache(maxsize=None)
def landmark_keys() -> np.ndarray:
    ks = np.asarray([(a << 21) | (b << 10) | c for a in L0_DIGITS for b in L1_DIGITS for c in L2_DIGITS], np.uint64)
    v = unkey(ks)
    ok = np.isfinite(v) & ((np.abs(v) >= TINY) | (v == 0))          # drops NaN, inf and subnormal patterns; +0 and -0 stay
    return ks[ok]


# ----------------------------------------------------------------------------- rows and cases
@dataclass
class Row:
    """One vocabulary row.  logits: what the device reads; scores: what its work row must hold at T = 1 (penalised, -inf
    where the mask forbids), which is what every expectation is computed from."""
    logits: np.ndarray
    scores: np.ndarray
    prompt: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    outs: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    allow: Optional[np.ndarray] = None
    pen: bool = False

    @property
    def V(self):
        return self.logits.shape[0]


@dataclass
class Case:
    family: str
    row: Row
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    expect: int = 0
    note: str = ""
    cut_score: Optional[float] = None        # mass mode: the score of the cut group

    def params(self):
        rep, fq, pr = PEN if self.row.pen else (1.0, 0.0, 0.0)
        return [self.top_k, self.top_p, self.min_p, rep, fq, pr, 0, 0]


def make_row(scores, counts=None, prompt=None, allow=None) -> Row:
    """Row whose penalised, masked scores are `scores`.  counts [V] / prompt: requested output counts and prompt members; a
    token keeps them only where the penalty can be inverted exactly (l' = s + sub and the doubling / halving are exact in
    f32 and stay normal): sampling_ref.penalise of the returned logits is asserted to give `scores` back bit for bit."""
    s = np.asarray(scores, np.float32)
    V = s.shape[0]
    if counts is None and prompt is None:
        logits, outs, pr, pen = s.copy(), np.zeros(0, np.int64), np.zeros(0, np.int64), False
    else:
        c = np.zeros(V, np.int64) if counts is None else np.asarray(counts, np.int64).copy()
        inp = np.zeros(V, bool)
        if prompt is not None:
            inp[np.asarray(prompt, np.int64)] = True
        hit = (c > 0) | inp
        sub = (0.5 * c + 0.25 * (c > 0)).astype(np.float32)
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            lp = (s + sub).astype(np.float32)
            raw = np.where(lp > 0, lp * np.float32(2), lp / np.float32(2)).astype(np.float32)
            fwd = (np.where(raw > 0, raw / np.float32(2), raw * np.float32(2)).astype(np.float32) - sub).astype(np.float32)
        ok = hit & np.isfinite(raw) & ((np.abs(raw) >= TINY) | (raw == 0)) & (fwd.view(np.uint32) == s.view(np.uint32))
        c[~ok] = 0
        inp &= ok
        logits = np.where(ok, raw, s).astype(np.float32)
        outs, pr, pen = np.repeat(np.arange(V), c), np.flatnonzero(inp), True
        got = R.penalise(logits, pr, outs, V, *PEN)
        assert (got.view(np.uint32) == s.view(np.uint32)).all(), "the penalties are not inverted exactly"
    if allow is not None:
        allow = np.asarray(allow, bool)
        # forbidden tokens keep their finite logit (a token of the cut group): only the mask takes them out
        s = np.where(allow, s, -np.inf).astype(np.float32)
    return Row(logits=logits, scores=s, prompt=pr, outs=outs, allow=allow, pen=pen)


# ----------------------------------------------------------------------------- the sort-based reference
def kth_key(scores, lo, k):
    """key of the k-th largest score among the keys >= lo; lo itself when fewer than k are left"""
    ks = R.fkey(scores)
    ks = np.sort(ks[ks >= lo])[::-1]
    return int(ks[k - 1]) if k <= ks.size else int(lo)


def min_p_cut(scores, min_p):
    """(f32 cut, float64 cut) of min_p: v_max + ln(min_p), the f32 one in the kernel's operation order"""
    m = np.float32(np.asarray(scores, np.float32).max())
    mp = np.float32(min_p)
    return np.float32(m + np.float32(np.log(mp))), float(m) + float(np.log(np.float64(mp)))


def mass_groups(scores, lo):
    """(keys, mass above, mass through) per group of equal key >= lo, descending; float64 masses relative to the row maximum"""
    ks = R.fkey(scores)
    sel = ks >= lo
    vmax = float(np.asarray(scores, np.float32).max())
    uk, inv = np.unique(ks[sel], return_inverse=True)
    w = np.bincount(inv, weights=np.exp(np.asarray(scores, np.float64)[sel] - vmax))
    uk, w = uk[::-1], w[::-1]
    through = np.cumsum(w)
    return uk, through - w, through


def pre_lo(scores, top_k, min_p):
    """the select's floor before top_p: LO0, then min_p, then top_k (sample_threshold_kernel's order)"""
    lo = LO0
    if min_p > 0:
        lo = max(lo, int(R.fkey(min_p_cut(scores, min_p)[0])))
    if 0 < top_k < len(scores):
        lo = max(lo, kth_key(scores, lo, top_k))
    return lo


def expected_threshold(scores, top_k=0, top_p=1.0, min_p=0.0):
    """(key, margin): the threshold from sorts and float64 masses; margin = distance of top_p * total from the two ends of the cut
    group's mass interval, as a fraction of the total (inf without top_p)."""
    lo = pre_lo(scores, top_k, min_p)
    if not top_p < 1.0:
        return lo, np.inf
    uk, above, through = mass_groups(scores, lo)
    total = through[-1]
    want = float(np.float32(top_p)) * total
    j = int(np.searchsorted(through, want))                    # first group whose inclusive mass reaches want
    j = min(j, len(uk) - 1)
    return max(lo, int(uk[j])), min(want - above[j], through[j] - want) / total


# ----------------------------------------------------------------------------- numpy restatement of the kernels
def model_keys(scores, bug=None):
    v = np.asarray(scores, np.float32)
    if bug == "no_invert":                                      # negative floats keep their magnitude order
        u = v.view(np.uint32).astype(np.uint64)
        return np.where((u & 0x80000000) != 0, u & 0x7FFFFFFF, u | 0x80000000).astype(np.uint64)
    return R.fkey(v)


def select_model(keys, wts, lo, mass, want, bug=None, all_wts_total=None):
    """radix_select: keys uint64 [V], wts int64 [V] (1, or the 32.32 masses); returns the key."""
    prefix, hi_mask, target = 0, 0, 0
    hist = np.zeros(2048, np.int64)
    for lvl in range(3):
        shift = (21, 10, 0)[lvl]
        nb = 2048 if lvl < 2 else 1024
        sel = (keys >= lo) & (wts != 0)
        if bug != "no_hi_mask":
            sel &= (keys & np.uint64(hi_mask)) == np.uint64(prefix)
        dig = ((keys[sel] >> np.uint64(shift)) & np.uint64(nb - 1)).astype(np.int64)
        # float64 sums of integers below 2^53 (V * 2^32 < 2^45): exact, as the kernel's integer atomics are
        prev, hist = hist, np.bincount(dig, weights=wts[sel].astype(np.float64), minlength=nb).astype(np.int64)
        if lvl == 2 and bug == "lvl2_2048":
            # 2048 bins scanned over a level-2 histogram of 1024.  The kernel clears all 2048 bins at every level, so on its own
            # this scan is harmless: the upper half is zero and the same bin is found.  It returns a wrong key only together
            # with a second mistake, a clearing loop that stops at nb = 1024 like the histogram's own index range; then bins
            # 1024..2047 still hold level 1's counts.  That pair is what is restated here.
            nb, hist = 2048, np.r_[hist, prev[1024:]]
        per = nb // 64
        lanes = hist.reshape(64, per) if bug == "lanes_low_first" else hist[::-1].reshape(64, per)
        sl = lanes.sum(1)
        incl = np.cumsum(sl)
        if lvl == 0:
            total = int(incl[63]) if all_wts_total is None else int(all_wts_total)
            if mass:
                t = float(np.ceil(float(want) * float(total)))
                target = 1 if t < 1.0 else (total if t > float(total) else int(t))
            else:
                target = int(want)
        hit = (incl > target) if bug == "gt" else (incl >= target)
        if not hit.any():
            return int(lo)
        L = int(np.argmax(hit))
        inc2 = np.cumsum(lanes[L]) + (incl[L] - sl[L])
        hit2 = (inc2 > target) if bug == "gt" else (inc2 >= target)
        Q = int(np.argmax(hit2))
        b = L * per + Q if bug == "lanes_low_first" else nb - 1 - L * per - Q
        before2 = int(inc2[Q] - lanes[L][Q])
        prefix |= b << shift
        hi_mask |= (nb - 1) << shift
        if bug != "no_reduce":
            target -= before2
    return int(prefix) & 0xFFFFFFFF


def threshold_model(scores, top_k=0, top_p=1.0, min_p=0.0, bug=None, vmax_shift=0.0):
    """sample_threshold_kernel on a work row (T > 0); vmax_shift moves the maximum the masses are taken against (the device's
    __expf stands behind a shift of that size)."""
    v = np.asarray(scores, np.float32)
    V = v.shape[0]
    keys = model_keys(v, bug)
    lo = int(model_keys(np.float32(-np.inf), bug)) + 1
    use_k, use_p, use_m = 0 < top_k < V, top_p < 1.0, min_p > 0.0
    if not (use_k or use_p or use_m):
        return 0
    if use_m:
        lo = max(lo, int(model_keys(min_p_cut(v, min_p)[0], bug)))
    if use_k:
        lo = max(lo, select_model(keys, np.ones(V, np.int64), lo, False, float(top_k), bug))
    if use_p:
        with np.errstate(under="ignore"):
            w = np.floor(np.exp(v.astype(np.float64) - (float(v.max()) + vmax_shift)) * 4294967296.0)
        w = np.where(np.isfinite(w), w, 0).astype(np.int64)
        tot_all = int(w[keys >= (int(model_keys(np.float32(-np.inf), bug)) + 1)].sum()) if bug == "total_all" else None
        lo = max(lo, select_model(keys, w, lo, True, float(np.float32(top_p)), bug, tot_all))
    return lo


def argmax_model(scores, thr, seed, n, bug=None):
    """gumbel_argmax_body<PROC> + kr_sample_greedy on a work row at T = 1: the token."""
    v = np.asarray(scores, np.float32)
    k = R.fkey(v)
    drop = np.isneginf(v) | ((k <= thr) if bug == FILTER_BUG else (k < thr)) & (thr != 0)
    sc = np.where(drop, -np.inf, (v + O.gumbel_noise(seed, n, v.shape[0])).astype(np.float32))
    return int(np.argmax(sc))


# ----------------------------------------------------------------------------- count mode
@lru_cache(maxsize=None)
def landmark_row(V, fill, pen=False, seed=0):
    """(Row, number of landmark tokens): every landmark key on 1..3 tokens at shuffled positions of a row of V."""
    rng = np.random.default_rng(1000 * V + seed + (17 if np.isfinite(fill) else 0) + (5 if pen else 0))
    ks = landmark_keys()
    toks = np.repeat(ks, rng.integers(1, 4, ks.size))
    rng.shuffle(toks)
    pos = rng.permutation(V)[:toks.size]
    s = np.full(V, fill, np.float32)
    s[pos] = unkey(toks)
    if not pen:
        return make_row(s), toks.size
    counts = np.zeros(V, np.int64)
    counts[pos] = rng.integers(0, 4, pos.size)
    prompt = pos[rng.random(pos.size) < 0.5]
    return make_row(s, counts, prompt), toks.size


def count_cases(V, fill, pen=False):
    """one case per k = 1 .. landmark tokens + 2"""
    row, n = landmark_row(V, float(fill), pen)
    srt = np.sort(R.fkey(row.scores))[::-1]
    srt = srt[srt >= LO0]
    fam = f"count/V{V}/{'ninf' if np.isneginf(fill) else 'm3e38'}{'/pen' if pen else ''}"
    return [Case(fam, row, top_k=k, expect=int(srt[k - 1]) if k <= srt.size else LO0, note=f"k={k}") for k in range(1, n + 3)]


def prod_landmark_cases():
    """32 rows of V_PROD: the landmarks scattered over the whole row, -inf elsewhere; k spread over the landmark tokens."""
    row, n = landmark_row(V_PROD, float(-np.inf))
    srt = np.sort(R.fkey(row.scores))[::-1]
    srt = srt[srt >= LO0]
    ks = sorted(set(np.linspace(1, n, 30).astype(int).tolist()) | {n + 1, n + 2})
    cases = [Case("count/Vprod", row, top_k=k, expect=int(srt[k - 1]) if k <= srt.size else LO0, note=f"k={k}") for k in ks]
    for c in cases:
        check_case(c)
    return cases


# ----------------------------------------------------------------------------- mass mode
MASS_FAMILIES = ("zero",) + tuple(f"pow2_e{e}" for e in (-3, 0, 4, 10, 20)) + ("geom",)


def family_scores(name):
    """the group scores of a mass family, any order"""
    if name == "zero":
        e = np.arange(-126, -9).astype(np.float64)
        return np.r_[2.0 ** e, -(2.0 ** e), 0.0, -0.0].astype(np.float32)
    if name.startswith("pow2_e"):
        x = np.float32(2.0 ** int(name[6:]))
        up, dn = [x], []
        for _ in range(19):
            up.append(np.nextafter(up[-1], np.float32(np.inf)))
        for _ in range(20):
            dn.append(np.nextafter(dn[-1] if dn else x, np.float32(-np.inf)))
        return np.asarray(up + dn, np.float32)
    assert name == "geom"
    return (8.0 - 0.25 * np.arange(25)).astype(np.float32)


@lru_cache(maxsize=None)
def mass_row(name, pen=False, mask_group=None):
    """The family's row: every group on 1 or 2 tokens (2 for the group a mask halves), -inf elsewhere.  mask_group: index (in
    descending order) of the group whose every second token a guide mask removes."""
    i = MASS_FAMILIES.index(name)
    V = VS[i % 3]
    rng = np.random.default_rng(77 + i)
    g = family_scores(name)
    g = g[np.argsort(R.fkey(g))[::-1]]
    mult = rng.integers(1, 3, g.size)
    if mask_group is not None:
        mult[mask_group] = 2
    vals = np.repeat(g, mult)
    pos = rng.permutation(V)[:vals.size]
    s = np.full(V, -np.inf, np.float32)
    s[pos] = vals
    allow = None
    if mask_group is not None:
        allow = np.ones(V, bool)
        first = int(mult[:mask_group].sum())
        allow[pos[first + 1:first + int(mult[mask_group]):2]] = False
        allow[rng.permutation(np.flatnonzero(np.isneginf(s)))[:V // 3]] = False     # and a third of the empty tokens
    if not pen:
        return make_row(s, allow=allow)
    counts = np.zeros(V, np.int64)
    counts[pos] = rng.integers(0, 4, pos.size)
    return make_row(s, counts, pos[rng.random(pos.size) < 0.5], allow=allow)


def mass_cases(family, row, top_k=0, min_p=0.0, only_group=None):
    """(cases, groups): one case per group of the keys that min_p / top_k leave whose f32 top_p keeps MARGIN from both ends of
    the group's mass interval."""
    lo = pre_lo(row.scores, top_k, min_p)
    uk, above, through = mass_groups(row.scores, lo)
    total = through[-1]
    out = []
    for j in (range(len(uk)) if only_group is None else [only_group]):
        p = np.float32((above[j] + through[j]) / 2 / total)
        want = float(p) * total
        if p < 1.0 and min(want - above[j], through[j] - want) >= MARGIN * total:
            out.append(Case(family, row, top_k=top_k, top_p=float(p), min_p=min_p, expect=max(lo, int(uk[j])), note=f"group {j}",
                            cut_score=float(unkey(uk[j]))))
    return out, len(uk)


def top_k_for(row, frac=0.5):
    """a top_k that keeps the upper `frac` of the row's groups (and so moves the mass total by far more than MARGIN)"""
    uk, _, _ = mass_groups(row.scores, LO0)
    cut = int(uk[max(1, int(len(uk) * frac)) - 1])
    return int((R.fkey(row.scores) >= cut).sum())


@lru_cache(maxsize=None)
def mass_suite():
    """{family: (cases, groups)} for every mass family: plain, behind top_k, behind penalties; plus one masked case each."""
    out = {}
    for name in MASS_FAMILIES:
        row = mass_row(name)
        out[f"mass/{name}"] = mass_cases(f"mass/{name}", row)
        out[f"mass/{name}/top_k"] = mass_cases(f"mass/{name}/top_k", row, top_k=top_k_for(row))
        out[f"mass/{name}/pen"] = mass_cases(f"mass/{name}/pen", mass_row(name, pen=True))
        ng = out[f"mass/{name}"][1]
        out[f"mass/{name}/mask"] = mass_cases(f"mass/{name}/mask", mass_row(name, mask_group=ng // 3), only_group=ng // 3)
    return out


# ----------------------------------------------------------------------------- min_p
MINP_SPECS = ((1024.0, 0.1), (-1000.0, 0.05), (2.0 ** 20, 1e-4))     # the f32 sum m + ln(min_p) absorbs logf's last bits


@lru_cache(maxsize=None)
def min_p_row(m, min_p, V):
    """Scores around the cut of min_p: the nearest ones 8 keys above and 8 keys below it."""
    rng = np.random.default_rng(int(abs(m)) + V)
    ck = int(R.fkey(min_p_cut(np.asarray([m], np.float32), min_p)[0]))      # the cut is computed from the maximum alone
    keys = np.asarray([ck + 8] * 2 + [ck + 9, ck + 40, ck + 100, ck + 101] + [ck - 8] * 3 + [ck - 9, ck - 100, ck - 4000], np.uint64)
    pos = rng.permutation(V)[:keys.size + 1]
    s = np.full(V, -np.inf, np.float32)
    s[pos[0]] = m
    s[pos[1:]] = unkey(keys)
    assert s.max() == np.float32(m)
    return make_row(s), ck


def min_p_suite():
    cases = []
    for i, (m, mp) in enumerate(MINP_SPECS):
        row, ck = min_p_row(m, mp, VS[i % 3])
        fam = f"min_p/m{m:g}"
        kept = int((R.fkey(row.scores) >= ck).sum())
        cases.append(Case(fam, row, min_p=mp, expect=ck, note="alone"))
        cases.append(Case(fam, row, min_p=mp, top_k=kept + 5, expect=ck, note="top_k above what min_p left"))
        cases.append(Case(fam, row, min_p=mp, top_k=kept, expect=ck + 8, note="top_k = what min_p left"))
        cases.append(Case(fam, row, min_p=mp, top_k=2, expect=kth_key(row.scores, ck, 2), note="top_k=2"))
        cases += mass_cases(fam + "/top_p", row, min_p=mp)[0]
    return cases


# ----------------------------------------------------------------------------- everything that has one expected threshold
@lru_cache(maxsize=None)
def threshold_cases():
    """Every threshold case at V ~ 4100, in the order the device test batches them."""
    cases = []
    for V in VS:
        for fill in (-np.inf, FILL_FINITE):
            cases += count_cases(V, fill)
    cases += count_cases(VS[1], -np.inf, pen=True)
    # one landmark row behind a mask that removes every second token of the cut key (the first key held by three tokens)
    row, n = landmark_row(VS[2], float(-np.inf))
    ks = R.fkey(row.scores)
    uk, cnt = np.unique(ks[ks >= LO0], return_counts=True)
    for key in uk[cnt == 3][[0, len(uk[cnt == 3]) // 2, -1]]:
        allow = np.ones(row.V, bool)
        allow[np.flatnonzero(ks == key)[1::2]] = False
        mrow = make_row(row.scores, allow=allow)
        k = int((R.fkey(mrow.scores) >= key).sum())            # the cut key's last surviving token
        cases.append(Case("count/mask", mrow, top_k=k, expect=int(key), note=f"k={k}"))
        cases.append(Case("count/mask", mrow, top_k=k + 1, expect=kth_key(mrow.scores, LO0, k + 1), note=f"k={k + 1}"))
    for fam, (cs, _) in mass_suite().items():
        cases += cs
    cases += min_p_suite()
    for c in cases:
        check_case(c)
    check_coverage()
    return cases


def check_case(c: Case):
    """Every precondition of a threshold case, on the reference alone."""
    row = c.row
    assert is_score(row.scores) and np.isfinite(row.logits[np.isfinite(row.scores)]).all(), c.family
    if row.allow is not None:
        assert np.isneginf(row.scores[~row.allow]).all()
    lp = R.penalise(row.logits, row.prompt, row.outs, row.V, *(PEN if row.pen else (1.0, 0.0, 0.0)))
    masked = lp if row.allow is None else np.where(row.allow, lp, np.float32(-np.inf))
    assert (masked.view(np.uint32) == row.scores.view(np.uint32)).all(), f"{c.family}: scores are not the penalised logits"
    assert c.top_k > 0 or c.top_p < 1.0 or c.min_p > 0
    key, margin = expected_threshold(row.scores, c.top_k, c.top_p, c.min_p)
    assert key == c.expect, describe(f"{c.family} {c.note} (sort reference against the builder)", c.expect, key)
    assert margin >= MARGIN, f"{c.family} {c.note}: top_p within {margin} of a group edge"
    if c.min_p > 0:
        # the f32 cut: 8 keys from the nearest score on either side, and the exact sum >= 8 ulp of ln(min_p) away from the two
        # rounding ties around it, so that logf's last bits cannot move it
        c32, c64 = min_p_cut(row.scores, c.min_p)
        ck = int(R.fkey(c32))
        ks = R.fkey(row.scores).astype(np.int64)
        assert np.abs(ks[ks >= LO0] - ck).min() == 8, c.family
        half = float(np.spacing(np.abs(c32))) / 2
        slack = 8 * float(np.spacing(np.float32(abs(np.log(c.min_p)))))
        assert abs(c64 - float(c32)) <= half - slack, f"{c.family}: m + ln(min_p) rounds within logf's error of a tie"


def check_coverage():
    """Family coverage of the mass suite: >= 60 % of the groups of every family survive MARGIN; +0 and -0 are both cut points."""
    stats = {}
    for fam, (cs, groups) in mass_suite().items():
        if fam.endswith("/mask"):
            assert len(cs) == 1, f"{fam}: the masked case lost its margin"
        else:
            assert len(cs) >= 0.6 * groups, f"{fam}: {len(cs)} of {groups} groups keep the margin"
        stats[fam] = (len(cs), groups)
    cuts = [c.expect for c in mass_suite()["mass/zero"][0]]
    assert 0x80000000 in cuts and 0x7FFFFFFF in cuts, "+0 and -0 must both be cut points"
    ks = landmark_keys()
    assert 0x80000000 in ks and 0x7FFFFFFF in ks and len(ks) == 13 * 49 + 2    # 13 finite normal level-0 bins x 49, and the zeros
    return stats


# ----------------------------------------------------------------------------- filter rows
FILTER_KINDS = {"positive": (1.5, None), "negative": (-1.5, None), "zero": (0.0, -0.0)}
N_KEPT, N_STEP = 8, 3


@dataclass
class FilterCase:
    kind: str
    row: Row
    seed: int
    kept: np.ndarray
    dropped: np.ndarray
    thr: int
    expect: int


@lru_cache(maxsize=None)
def filter_cases(per_kind=6):
    """Kept tokens at the threshold score, ten times as many one key below, -inf elsewhere; top_k = N_KEPT makes the threshold.
    The seed is the first (from a drawn start) under which a dropped token has the row's largest noise, by more than 1e-3
    over the best kept one, and the kept tokens' top-2 noise gap exceeds 1e-3 (fp32 sums and the device's logf move a noisy
    score by ~1e-6)."""
    out = []
    rng = np.random.default_rng(4242)
    for kind, (s_keep, s_drop) in FILTER_KINDS.items():
        for r in range(per_kind):
            V = VS[r % 3]
            thr = int(R.fkey(np.float32(s_keep)))
            lo = unkey(thr - 1) if s_drop is None else np.float32(s_drop)
            pos = rng.permutation(V)[:11 * N_KEPT]
            kept, dropped = np.sort(pos[:N_KEPT]), np.sort(pos[N_KEPT:])
            s = np.full(V, -np.inf, np.float32)
            s[kept], s[dropped] = s_keep, lo
            seed = int(rng.integers(0, 2 ** 31))
            while True:
                g = O.gumbel_noise(seed, N_STEP, V)
                gk = np.sort(g[kept])
                if g[dropped].max() - gk[-1] > 1e-3 and gk[-1] - gk[-2] > 1e-3:
                    break
                seed += 1
            out.append(FilterCase(kind, make_row(s), seed, kept, dropped, thr, int(kept[np.argmax(g[kept])])))
            check_filter_case(out[-1])
    return out


def check_filter_case(c: FilterCase):
    s, g = c.row.scores, O.gumbel_noise(c.seed, N_STEP, c.row.V)
    assert is_score(s) and (R.fkey(s[c.kept]) == c.thr).all() and (R.fkey(s[c.dropped]) == c.thr - 1).all()
    assert len(c.dropped) == 10 * len(c.kept) and np.isneginf(np.delete(s, np.r_[c.kept, c.dropped])).all()
    assert int(np.argmax(np.where(np.isneginf(s), -np.inf, g))) in c.dropped, "a dropped token must have the largest noise"
    gk = np.sort(g[c.kept])
    assert gk[-1] - gk[-2] > 1e-3 and g[c.dropped].max() - gk[-1] > 1e-3
    assert expected_threshold(s, top_k=N_KEPT)[0] == c.thr
    assert c.expect == int(c.kept[np.argmax(g[c.kept])])


# ----------------------------------------------------------------------------- partitions
N_PARTS = (1, 7, 64, 1025, 1100)
IDX_NONE = 0x7FFFFFFF


def part_span(V, n_part):
    """(per, non-empty partitions) of gumbel_argmax_body: per is rounded up to 4, so trailing partitions can be empty"""
    per = (((V + n_part - 1) // n_part) + 3) & ~3
    return per, (V + per - 1) // per


def partition_rows(V, n_part):
    """(logits [6, V], temps [6], winners [6]): N(0, 1) rows whose winner (+50: above any noise) is in the first partition, at
    the start of the last non-empty one, and on the last token; greedy rows (T = 0) carry an equal value on a later token."""
    rng = np.random.default_rng(V * 7 + n_part)
    per, ne = part_span(V, n_part)
    spots = [min(2, V - 1), (ne - 1) * per, V - 1]
    logits = rng.standard_normal((6, V)).astype(np.float32)
    temps = np.asarray([0, 0, 0, 1, 1, 1], np.float32)
    for r in range(6):
        w = spots[r % 3]
        logits[r, w] = 50.0
        if r < 3 and w < V - 1:
            logits[r, V - 1] = 50.0                            # a tie in the last partition: the lower id wins
    return logits, temps, np.asarray(spots * 2)


def partials_ref(logits_row, V, n_part):
    """(values, ids) of a greedy row's partials: the maximum and its lowest index per partition, (-inf, IDX_NONE) where empty"""
    per, ne = part_span(V, n_part)
    val = np.full(n_part, -np.inf, np.float32)
    idx = np.full(n_part, IDX_NONE, np.int64)
    for p in range(ne):
        seg = logits_row[p * per:min(V, (p + 1) * per)]
        val[p], idx[p] = seg.max(), p * per + int(np.argmax(seg))
    return val, idx


GREEDY_N_PARTS = (1, 255, 256, 257, 2047, 2048, 2049, 4100)


def greedy_partials(n_part):
    """(values [R, n_part], ids [R, n_part], expected token [R]): the maximum at partial 0, 255, 256, n_part - 1 and on both
    sides of every u * 256 border of the eight-wide read, an equal value at a LATER partial with a LOWER token id (which must
    win) wherever a later partial exists."""
    rng = np.random.default_rng(n_part)
    spots = sorted({p for p in [0, 255, 256, n_part - 1] + [u * 256 + o for u in range(1, 17) for o in (-1, 0)] if 0 <= p < n_part})
    R_ = len(spots)
    val = rng.uniform(-1, 0, (R_, n_part)).astype(np.float32)
    ids = np.stack([rng.permutation(100000)[:n_part] + 1000 for _ in range(R_)]).astype(np.int64)
    want = np.zeros(R_, np.int64)
    for r, p in enumerate(spots):
        val[r, p], ids[r, p] = 5.0, 900 - r
        want[r] = ids[r, p]
        if p < n_part - 1:
            q = int(rng.integers(p + 1, n_part))
            val[r, q], ids[r, q] = 5.0, 400 - r
            want[r] = ids[r, q]
    return val, ids, want, spots


def pick(av, ai):
    """kr_sample_greedy's reduction of the partials: largest value, lowest index on ties."""
    return np.asarray([int(i[np.flatnonzero(v == v.max())].min()) for v, i in zip(av, ai)])
