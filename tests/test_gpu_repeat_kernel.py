"""kr_repeat_detect through the C-ABI on crafted histories, against tests/repeat_ref.py: rep_at from the definition (block
comparison), seen and every run counter from the state machine.  Every comparison is an integer equality, and every launch sequence
is run twice from the same state and must leave the same bits.  (Fails on a tree without the feature: the symbol does not exist.)"""
import ctypes as C
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from karanta_ocr_amd._lib import KarantaHipError, lib, ptr  # noqa: E402
from tests import repeat_ref as R  # noqa: E402

GUARD = 3            # slots' worth of sentinel entries behind every per-slot array
PAD = -7             # history rows a slot has not reached yet


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return lib()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def block(p, base=100):
    return (np.arange(p) + base).tolist()          # p distinct tokens: no shorter period inside


def loop_case(p, c, m=0, junk=5, extra=4, a=None, b=None):
    return [1, 2, 3, 4, 5][:junk] + block(p) * (c + 1) + block(extra, 9000), (p if a is None else a, p if b is None else b, c, m)


def cases():
    """(tokens, (a, b, c, m)) per slot kind; what each must give is stated in test_one_launch_over_whole_histories."""
    out = {}
    for p in (1, 2, 3, 7, 64):
        out[f"p{p}"] = loop_case(p, 3)
    for p in (1023, 1024):
        out[f"p{p}"] = loop_case(p, 2, extra=2)
    for key in list(out):                                   # one token short of the trigger: nothing
        y, (a, b, c, m) = out[key]
        out[key + "-short"] = (y[:5 + c * a - 1], (a, b, c, m))
    out["span"] = loop_case(3, 2, m=20, extra=0)
    out["span"] = (out["span"][0] + block(3) * 6, out["span"][1])
    out["below-a"] = loop_case(4, 3, a=5, b=7)              # periods a - 1 and (its double) b + 1: nothing
    out["above-b"] = loop_case(8, 3, a=5, b=7)
    out["p2-as-4"] = ([9, 8, 7] + [1, 2] * 10, (3, 5, 2, 0))
    y = [1, 2, 3, 4, 5] + block(3) * 2 + [100, 101, 0] + block(3) * 5
    out["mismatch"] = (y, (3, 3, 3, 0))
    out["wide"] = ([5, 6] + block(7) * 6, (1, 1024, 4, 0))   # every period watched at once
    out["none"] = (block(60, 500), (1, 32, 2, 0))
    return out


CASES = cases()
WANT = {"p1": 7, "p2": 10, "p3": 13, "p7": 25, "p64": 196, "p1023": 5 + 2046 - 1, "p1024": 5 + 2048 - 1, "span": 5 + 20 - 1,
        "below-a": None, "above-b": None, "p2-as-4": 3 + 8 - 1, "mismatch": 5 + 9 + 9 - 1, "wide": 2 + 28 - 1, "none": None}


def test_the_reference_gives_the_hand_worked_indices():
    for key, (y, params) in CASES.items():
        want = None if key.endswith("-short") else WANT[key]
        assert R.first_repeat(y, *params) == want, key
    assert R.first_repeat(CASES["p2-as-4"][0], 3, 5, 2) == R.first_repeat(CASES["p2-as-4"][0], 4, 4, 2)     # through p = 4


class Slots:
    """B slots on the device with sentinels behind every array; `tokens[b]` is the whole sequence slot b will ever generate."""

    def __init__(self, tokens, params, stride_extra=3, prompt=(7, 0, 31), seed=0):
        B = self.B = len(tokens)
        self.tokens, self.params = [list(map(int, y)) for y in tokens], list(params)
        self.stride = B + stride_extra
        self.rows = max(len(y) for y in tokens) + 2
        hist = np.full((self.rows, self.stride), PAD, np.int32)
        for b, y in enumerate(self.tokens):
            hist[:len(y), b] = y
        rng = np.random.default_rng(seed)
        self.h = {"hist": hist, "plen": np.asarray([prompt[b % len(prompt)] for b in range(B)] + [0] * GUARD, np.int32),
                  "ctx": np.zeros(B + GUARD, np.int32), "fin": np.zeros(B + GUARD, np.int32),
                  "cfg": np.asarray([list(p) for p in params] + [[1, 4, 2, 0]] * GUARD, np.int32),
                  # no clearing is needed: fresh slots start from garbage counters
                  "run": rng.integers(0, 1 << 20, (B + GUARD, R.MAX_PERIOD)).astype(np.int32),
                  "seen": np.asarray([0] * B + [5] * GUARD, np.int32), "rep_at": np.full(B + GUARD, -1, np.int32)}
        self.set_gen([0] * B)
        self.d = {k: t_(v) for k, v in self.h.items()}
        self.ref = [R.Incremental(*p, run=self.h["run"][b]) if p[1] else None for b, p in enumerate(params)]

    def set_gen(self, gen):
        self.gen = [int(g) for g in gen]
        self.h["ctx"][:self.B] = self.h["plen"][:self.B] - 1 + np.asarray(self.gen, np.int32)
        if hasattr(self, "d"):
            self.d["ctx"] = t_(self.h["ctx"])

    def args(self, flags=0, first=0, n=None):
        from karanta_ocr_amd._lib import Repeat
        d, n = self.d, self.B - first if n is None else n
        return Repeat(n, ptr(d["hist"][:, first:]), self.stride, self.rows, ptr(d["ctx"][first:]), ptr(d["plen"][first:]),
                      ptr(d["fin"][first:]), ptr(d["cfg"][first:]), ptr(d["run"][first:]), ptr(d["seen"][first:]),
                      ptr(d["rep_at"][first:]), flags)

    def launch(self, L, flags=0):
        a = self.args(flags)
        assert L.kr_repeat_detect(C.byref(a), 0) == 0

    def read(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.d.items()}

    def step(self, L, gen, flags=0):
        """The slots now hold gen[b] tokens; one launch; the reference is fed the same tokens."""
        old = self.gen
        self.set_gen(gen)
        self.launch(L, flags)
        for b, r in enumerate(self.ref):
            if r is not None and not self.h["fin"][b] and r.rep_at < 0:
                r.feed(self.tokens[b][old[b]:self.gen[b]])
                if r.rep_at >= 0:
                    self.h["fin"][b] = 1

    def check(self, what=""):
        got = self.read()
        for k in ("hist", "plen", "ctx", "cfg"):
            np.testing.assert_array_equal(got[k], self.h[k], err_msg=f"{what}: {k} is an input")
        for k in ("fin", "run", "seen", "rep_at"):
            np.testing.assert_array_equal(got[k][self.B:], self.h[k][self.B:], err_msg=f"{what}: {k} written past the slots")
        for b, r in enumerate(self.ref):
            if r is None:
                want = (self.h["rep_at"][b], self.h["seen"][b], self.h["fin"][b], self.h["run"][b])
            else:
                want = (r.rep_at, r.seen, self.h["fin"][b], r.run)
            assert (int(got["rep_at"][b]), int(got["seen"][b]), int(got["fin"][b])) == tuple(int(x) for x in want[:3]), \
                f"{what}: slot {b} (rep_at, seen, finished)"
            np.testing.assert_array_equal(got["run"][b], want[3], err_msg=f"{what}: slot {b} run counters")
        return got


def twice(make, drive):
    """Runs `drive` on two fresh copies of the same state: equal bits."""
    outs = []
    for _ in range(2):
        s = make()
        drive(s)
        outs.append(s.check())
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=f"{k} differs between two runs of the same launches")
    return outs[0]


@pytest.mark.parametrize("B", [1, 5, 32])
def test_one_launch_over_whole_histories(L, B):
    keys = sorted(CASES)
    keys = keys[3 * B % len(keys):] + keys[:3 * B % len(keys)]
    for at in range(0, len(keys), B):
        use = [keys[(at + b) % len(keys)] for b in range(B)]
        toks, params = [CASES[k][0] for k in use], [CASES[k][1] for k in use]
        got = twice(lambda: Slots(toks, params), lambda s: s.step(L, [len(y) for y in toks]))
        for b, k in enumerate(use):
            want = None if k.endswith("-short") else WANT[k]
            assert int(got["rep_at"][b]) == (-1 if want is None else want), k
            assert int(got["fin"][b]) == (want is not None) and int(got["seen"][b]) == (len(toks[b]) if want is None else want + 1)


SHORT = ["p1", "p2", "p3", "p7", "p3-short", "span", "p2-as-4", "mismatch", "wide", "none", "below-a"]


@pytest.mark.parametrize("chunks", [[1], [2], [3], [4], [1, 4, 2, 3]])
def test_any_chunking_leaves_the_same_bits(L, chunks):
    toks, params = [CASES[k][0] for k in SHORT], [CASES[k][1] for k in SHORT]
    T = max(len(y) for y in toks)

    def drive(s, chunks):
        at = 0
        for n in itertools.cycle(chunks):
            if at >= T:
                break
            at += n
            # a slot the pass finished stays where it is, as a frozen slot does
            s.step(L, [g if s.h["fin"][b] else min(at, len(y)) for b, (g, y) in enumerate(zip(s.gen, toks))], flags=2)
            s.check(f"{chunks} at {at}")

    one = twice(lambda: Slots(toks, params), lambda s: drive(s, [1]))
    many = twice(lambda: Slots(toks, params), lambda s: drive(s, chunks))
    for k in ("rep_at", "seen", "run", "fin"):
        np.testing.assert_array_equal(many[k], one[k], err_msg=k)
    for b, k in enumerate(SHORT):
        want = None if k.endswith("-short") else WANT[k]
        assert int(one["rep_at"][b]) == (-1 if want is None else want), k


def test_off_finished_and_decided_slots_are_untouched(L):
    y, params = CASES["p3"]
    toks = [y] * 5
    cfgs = [params, (0, 0, 0, 0), params, params, (3, 2, 3, 0)]      # live, off, finished, already decided, a row out of bounds

    def make():
        s = Slots(toks, cfgs)
        s.h["fin"][2], s.h["seen"][2] = 1, len(y)           # finished earlier: unfrozen its news are pads, frozen it has none
        s.h["rep_at"][3], s.h["seen"][3] = 4, 5
        for k in ("fin", "rep_at", "seen"):
            s.d[k] = t_(s.h[k])
        s.ref[2] = s.ref[3] = s.ref[4] = None               # what they hold must stay
        return s

    got = twice(make, lambda s: [s.step(L, [len(y)] * 5, flags=f) for f in (0, 2)])
    assert got["rep_at"].tolist()[:5] == [WANT["p3"], -1, -1, 4, -1] and got["fin"].tolist()[:5] == [1, 0, 1, 0, 0]


def test_rep_at_is_written_once(L):
    y = [1, 2] + [6] * 30
    s = Slots([y], [(1, 1, 3, 0)])
    s.step(L, [10])
    got = s.check("first")
    assert int(got["rep_at"][0]) == 4 and int(got["seen"][0]) == 5
    s.d["fin"].zero_()                                      # even a slot someone revived keeps its verdict
    s.h["fin"][:] = 0
    s.ref[0] = None
    s.h["rep_at"][0], s.h["seen"][0], s.h["run"][0] = got["rep_at"][0], got["seen"][0], got["run"][0]
    s.step(L, [30])
    s.check("second")


def test_readmission_starts_from_the_new_tokens_alone(L):
    first, second = [1, 2, 3] * 4 + [1, 2], [3, 1, 2] + [4, 5] * 6

    def drive(s):
        s.step(L, [len(first)], flags=2)
        got = s.check("one short of the trigger")
        assert int(got["rep_at"][0]) == -1 and int(got["run"][0][2]) == 11
        # the admission: new tokens in the slot's history, seen = 0, rep_at = -1; run is left as it is
        s.tokens[0] = second
        s.h["hist"][:, 0] = PAD
        s.h["hist"][:len(second), 0] = second
        s.d["hist"] = t_(s.h["hist"])
        s.d["seen"][:1].zero_()
        s.ref[0].admit(1, 8, 5)
        s.set_gen([0])
        s.step(L, [4], flags=2)
        s.step(L, [len(second)], flags=2)

    got = twice(lambda: Slots([first + [0] * 8], [(1, 8, 5, 0)]), drive)
    assert int(got["rep_at"][0]) == R.first_repeat(second, 1, 8, 5) == 12


def test_a_step_that_ends_on_an_eos_still_finds_the_repeat_before_it(L):
    """A speculative step may emit several tokens and finish the slot on the last of them (the EOS): under the freeze bit the tokens
    before it are walked and only rep_at is written.  Without the freeze bit a finished slot's new tokens are pads."""
    y = [1, 2] + [6] * 4 + [99]

    def make():
        s = Slots([y, y, y], [(1, 1, 4, 0), (1, 1, 5, 0), (1, 1, 4, 0)])
        s.step(L, [4, 4, 4], flags=2)
        s.h["fin"][:3] = 1                                  # the verification emitted 6, 6, EOS and finished the slots
        s.d["fin"] = t_(s.h["fin"])
        s.ref = [None] * 3
        kept = s.read()
        assert kept["seen"].tolist()[:3] == [4, 4, 4] and kept["rep_at"].tolist()[:3] == [-1, -1, -1]
        for k in ("seen", "run", "rep_at"):
            s.h[k] = kept[k].copy()
        s.h["rep_at"][0] = s.h["rep_at"][2] = 5             # four 6s end at index 5, before the EOS at 6; five never come
        return s

    got = twice(make, lambda s: [s.set_gen([7, 7, 7]), s.launch(L, flags=2), s.launch(L, flags=2)])
    assert got["rep_at"].tolist()[:3] == [5, -1, 5]
    s = make()
    s.h["rep_at"][0] = s.h["rep_at"][2] = -1
    s.set_gen([7, 7, 7])
    s.launch(L, flags=0)
    s.check("no freeze bit: untouched")


def test_flags_bit_0_records_nothing(L):
    y, params = CASES["p3"]
    for flags in (1, 3):
        s = Slots([y, y], [params, params])
        s.ref = [None, None]
        s.set_gen([len(y)] * 2)
        s.launch(L, flags)
        s.check(f"flags {flags}")


def test_history_rows_bound_the_walk(L):
    y, params = CASES["p3"]
    s = Slots([y], [params])
    s.rows = 10                                             # the caller says the history ends here, whatever ctx_len claims
    s.set_gen([len(y)])
    s.launch(L)
    s.ref[0].feed(y[:10])
    got = s.check("capped")
    assert int(got["seen"][0]) == 10 and int(got["rep_at"][0]) == -1


def test_bad_arguments_are_rejected_on_the_host(L):
    from karanta_ocr_amd._lib import Repeat
    s = Slots([CASES["p3"][0]] * 2, [CASES["p3"][1]] * 2)
    good = s.args()
    fields = [f for f, _ in Repeat._fields_]
    with pytest.raises(KarantaHipError, match="null args"):
        L.kr_repeat_detect(None, 0)
    for name in ("history", "ctx_len", "prompt_len", "finished", "cfg", "run", "seen", "rep_at"):
        bad = Repeat(*[None if f == name else getattr(good, f) for f in fields])
        with pytest.raises(KarantaHipError, match="null pointer"):
            L.kr_repeat_detect(C.byref(bad), 0)
    for name, v, msg in (("slots", 0, "slots"), ("slots", 33, "slots"), ("hist_stride", 1, "hist_stride"), ("hist_rows", 0, "hist_rows"),
                         ("flags", 4, "flags"), ("flags", -1, "flags")):
        bad = Repeat(*[v if f == name else getattr(good, f) for f in fields])
        with pytest.raises(KarantaHipError, match=msg):
            L.kr_repeat_detect(C.byref(bad), 0)
    s.check("nothing was launched")
