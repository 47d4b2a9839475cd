"""The sampler cases of tests/select_cases.py, proven without a GPU: every case meets its preconditions on the sort-based float64
reference (representable scores, penalties inverted bit for bit, the top_p margin, the min_p cut 8 keys from any score and
away from rounding ties), the mass families keep >= 60 % of their groups with +0 and -0 both among the cut points, the numpy
restatement of radix_select returns the expected key on every case (mass mode also with the maximum moved by +-1e-5), and each
restated mistake returns a wrong key on some case.  Run with -s for the counts that DESIGN.md quotes."""
import numpy as np
import pytest

from tests import sampling_ref as R
from tests import select_cases as S
from tests.sampling_rows import prod_batch


def test_unkey_inverts_fkey_and_orders_the_zeros():
    ks = np.r_[S.landmark_keys(), np.asarray([S.LO0, S.NEG_INF_KEY, 0xFF7FFFFF, 0x80800000, 0x7F7FFFFF], np.uint64)]
    np.testing.assert_array_equal(R.fkey(S.unkey(ks)), ks)
    v = np.asarray([-np.inf, -3e38, -1.5, -2.0 ** -126, -0.0, 0.0, 2.0 ** -126, 1.5, 3e38], np.float32)
    assert (np.diff(R.fkey(v).astype(np.int64)) > 0).all(), "keys ascend with the values, -0 below +0"
    np.testing.assert_array_equal(S.unkey(R.fkey(v)).view(np.uint32), v.view(np.uint32))
    assert int(R.fkey(np.float32(-np.inf))) == S.NEG_INF_KEY and float(S.unkey(S.LO0)) == -float(np.finfo(np.float32).max)
    assert S.digits(int(R.fkey(S.FILL_FINITE)))[0] == 4, "the finite fill lies in the lowest finite level-0 bin"


def test_landmarks_cover_the_borders_of_every_level():
    ks = S.landmark_keys()
    assert S.is_score(S.unkey(ks)) and np.isfinite(S.unkey(ks)).all()
    d0, d1, d2 = (ks >> np.uint64(21)) & np.uint64(2047), (ks >> np.uint64(10)) & np.uint64(2047), ks & np.uint64(1023)
    # the all-subnormal bins 1023 / 1024 / 1025 keep only the zeros (1025 nothing): nine level-0 digits carry all 49 low parts
    assert sorted(set(d0.tolist())) == sorted(set(S.L0_DIGITS) - {1025}) and len(ks) == (len(S.L0_DIGITS) - 3) * 49 + 2
    assert set(d1.tolist()) == set(S.L1_DIGITS) and set(d2.tolist()) == set(S.L2_DIGITS)
    for nb, ds in ((2048, d0), (2048, d1), (1024, d2)):
        per = nb // 64
        lane, place = (nb - 1 - ds.astype(np.int64)) // per, (nb - 1 - ds.astype(np.int64)) % per
        assert {0, per - 1} <= set(place.tolist()), "the first and the last bin of a lane"
        assert {0, 1, 62, 63} <= set(lane.tolist()), "the first and last lane, and the lanes next to them"
    assert 4 == d0.min() and 2043 == d0.max(), "the extreme finite bins of level 0"


def test_every_threshold_case_meets_its_preconditions():
    cases = S.threshold_cases()
    for c in cases:
        S.check_case(c)
    fams = {}
    for c in cases:
        fams[c.family] = fams.get(c.family, 0) + 1
    print("\ncases per family:", fams, "total", len(cases))
    for c in S.prod_landmark_cases():
        S.check_case(c)
    # the rows that the count families share hold every landmark key, 1..3 times
    for V in S.VS:
        row, n = S.landmark_row(V, float(-np.inf))
        uk, cnt = np.unique(R.fkey(row.scores)[np.isfinite(row.scores)], return_counts=True)
        np.testing.assert_array_equal(uk, np.sort(S.landmark_keys()))
        assert cnt.min() >= 1 and cnt.max() == 3 and cnt.sum() == n


def test_mass_families_keep_their_groups_and_both_zeros_are_cut_points():
    stats = S.check_coverage()
    print("\n(cases, groups) per mass family:", stats)
    # top_k moves the mass total by far more than the margin: the total over all keys would put most cuts on another key
    for name in S.MASS_FAMILIES:
        cs = S.mass_suite()[f"mass/{name}/top_k"][0]
        moved = sum(S.threshold_model(c.row.scores, c.top_k, c.top_p, bug="total_all") != c.expect for c in cs)
        assert moved >= len(cs) // 2, name


def test_penalised_rows_carry_counts_around_the_cuts():
    row, n = S.landmark_row(S.VS[1], float(-np.inf), True)
    hit = np.zeros(row.V, bool)
    hit[row.prompt] = True
    hit[row.outs] = True
    assert hit.sum() >= n // 4 and len(row.outs) >= n // 4, "tiny scores cannot absorb a penalty exactly; the large ones do"
    geom = S.mass_row("geom", pen=True)
    assert len(set(geom.outs.tolist()) | set(geom.prompt.tolist())) >= np.isfinite(geom.scores).sum() // 2
    assert not np.array_equal(geom.logits, geom.scores)


def test_the_restated_select_returns_the_expected_key_on_every_case():
    for c in S.threshold_cases() + S.prod_landmark_cases():
        got = S.threshold_model(c.row.scores, c.top_k, c.top_p, c.min_p)
        assert got == c.expect, S.describe(f"{c.family} {c.note}", c.expect, got)
        if c.top_p < 1.0:
            for sh in (-1e-5, 1e-5):
                got = S.threshold_model(c.row.scores, c.top_k, c.top_p, c.min_p, vmax_shift=sh)
                assert got == c.expect, S.describe(f"{c.family} {c.note} (maximum moved by {sh})", c.expect, got)


def sweep():
    """the cases the mistakes are run on: every family, the count rows of one vocabulary in full and a third of the others"""
    cs = S.threshold_cases()
    return [c for i, c in enumerate(cs) if not c.family.startswith("count/V") or c.family.startswith(f"count/V{S.VS[1]}") or i % 3 == 0]


@pytest.mark.parametrize("bug", S.BUGS)
def test_each_restated_mistake_returns_a_wrong_key(bug):
    broken = {}
    cs = sweep()
    for c in cs:
        if S.threshold_model(c.row.scores, c.top_k, c.top_p, c.min_p, bug=bug) != c.expect:
            fam = c.family.split("/")[0]
            broken[fam] = broken.get(fam, 0) + 1
    print(f"\n{bug}: breaks {sum(broken.values())} of {len(cs)} cases {broken}")
    assert sum(broken.values()) > 0, f"no case notices the mistake {bug}"


def test_filter_cases_and_the_filter_mistake():
    cs = S.filter_cases()
    assert {c.kind for c in cs} == set(S.FILTER_KINDS)
    wrong = 0
    for c in cs:
        S.check_filter_case(c)
        assert S.threshold_model(c.row.scores, top_k=S.N_KEPT) == c.thr
        assert S.argmax_model(c.row.scores, c.thr, c.seed, S.N_STEP) == c.expect
        assert S.argmax_model(c.row.scores, 0, c.seed, S.N_STEP) in c.dropped, "without the filter a dropped token wins"
        wrong += S.argmax_model(c.row.scores, c.thr, c.seed, S.N_STEP, bug=S.FILTER_BUG) != c.expect
    print(f"\n{S.FILTER_BUG}: breaks {wrong} of {len(cs)} filter rows")
    assert wrong == len(cs)
    z = [c for c in cs if c.kind == "zero"][0]
    assert z.thr == 0x80000000 and (z.row.scores[z.dropped].view(np.uint32) == 0x80000000).all(), "+0 kept, -0 dropped"


def test_partition_rows_and_partials():
    empties = 0
    for V in S.VS:
        for n_part in S.N_PARTS:
            per, ne = S.part_span(V, n_part)
            assert per % 4 == 0 and (ne - 1) * per < V <= ne * per and ne <= n_part
            empties += ne < n_part
            logits, temps, win = S.partition_rows(V, n_part)
            for r in range(3):
                val, idx = S.partials_ref(logits[r], V, n_part)
                assert (idx[ne:] == S.IDX_NONE).all() and np.isneginf(val[ne:]).all() and np.isfinite(val[:ne]).all()
                assert S.pick(val[None], idx[None])[0] == win[r] == int(np.argmax(logits[r]))
            assert win[1] // per == ne - 1 and win[2] == V - 1 and win[0] // per == 0
    assert empties >= 3, "some (V, n_part) must leave trailing partitions empty"
    assert S.part_span(4101, 1025) == (8, 513) and S.part_span(4099, 1100) == (4, 1025)
    for n_part in S.GREEDY_N_PARTS:
        val, ids, want, spots = S.greedy_partials(n_part)
        np.testing.assert_array_equal(S.pick(val, ids), want)
        assert spots[0] == 0 and spots[-1] == n_part - 1
        later_lower = sum(1 for r, p in enumerate(spots) if p < n_part - 1 and want[r] < ids[r, p])
        assert later_lower == sum(p < n_part - 1 for p in spots)
    assert {255, 256, 2047, 2048, 3840, 4095, 4096, 4099} <= set(S.greedy_partials(4100)[3])


def test_what_the_gaussian_production_rows_notice():
    """Not an assertion about the kernels: how many of prod_batch's 32 N(0, 3) rows (tests/test_gpu_sampling_kernels.py) each
    restated mistake moves the threshold of.  Printed for DESIGN.md (those rows do notice most of the mistakes, as moved
    kept sets; what they leave open is WHERE the cuts fall: in a handful of level-0 bins, none at a zero or at a lane border of
    level 0, which is asserted here)."""
    logits, temps, params, prompts, outs, counts, pbits, spec = prod_batch(np.random.default_rng(5))
    rows = []
    for b, (T, k, p, m, rep, fq, pr) in enumerate(spec):
        if T > 0 and (0 < k < logits.shape[1] or p < 1 or m > 0):
            rows.append((R.tempered(R.penalise(logits[b], prompts[b], outs[b], logits.shape[1], rep, fq, pr), T), int(k), float(p), float(m)))
    good = [S.threshold_model(*r) for r in rows]
    below = sum(g < 0x80000000 for g in good)
    bins = sorted({S.digits(g)[0] for g in good})
    seen = {bug: sum(S.threshold_model(*r, bug=bug) != g for r, g in zip(rows, good)) for bug in S.BUGS}
    print(f"\nprod_batch: {len(rows)} truncated rows, {below} with a cut below zero, level-0 bins of the cuts {bins}; "
          f"rows whose threshold each mistake moves: {seen}")
    assert not any(g in (0x80000000, 0x7FFFFFFF) for g in good) and len(bins) < 24, "no cut at a zero; a handful of the 2048 bins"
    assert not any((2047 - b) % 32 in (0, 31) for b in bins), "no cut in the first or last level-0 bin of a lane"
