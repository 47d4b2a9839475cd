"""numpy restatement of kr_logits_adjust and the seeded cases that tests/test_gpu_logit_adjust.py runs through the sampler
kernels; tests/test_adjust_cpu.py checks on the CPU that every case is decisive in the numpy reference alone (no near-tie, no
truncation-boundary token), so the GPU comparison excuses nothing."""
import numpy as np

from tests import sampling_ref as R

CAP = 320
V_SMALL = 1000       # the non-multiple-of-64 width of the sampling-kernel tests
V_PROD = 151936      # their production width
MARGIN = 1e-4        # the excuse rule of tests/test_gpu_sampling_kernels.py: a step counts when its top-2 gap exceeds this
#                      and neither of the two is a truncation-boundary token


def adjust_ref(row, ids, vals, flags, n_entries, min_tokens, n_b):
    """One row after kr_logits_adjust: l + v in fp32, -inf on the stop entries while n_b < min_tokens."""
    out = np.asarray(row, np.float32).copy()
    for e in range(int(n_entries)):
        i = int(ids[e])
        if (int(flags[e]) & 1) and n_b < min_tokens:
            out[i] = -np.inf
        else:
            out[i] = np.float32(out[i]) + np.float32(vals[e])
    return out


def tables(B, rows):
    """Device-shaped tables from per-row lists of (id, value, flag) and min_tokens: ids, vals, flags [B, CAP], meta [B, 4]."""
    ids = np.zeros((B, CAP), np.int32)
    vals = np.zeros((B, CAP), np.float32)
    flags = np.zeros((B, CAP), np.int32)
    meta = np.zeros((B, 4), np.int32)
    for b, (entries, m) in enumerate(rows):
        assert len(entries) <= CAP and len({e[0] for e in entries}) == len(entries)
        for e, (i, v, f) in enumerate(entries):
            ids[b, e], vals[b, e], flags[b, e] = i, v, f
        meta[b, :2] = len(entries), m
    return ids, vals, flags, meta


# (T, top_k, top_p, min_p, repetition, frequency, presence) per row
PLAIN = [(0.0, 0, 1, 0, 1, 0, 0), (1.0, 0, 1, 0, 1, 0, 0), (0.8, 0, 1, 0, 1, 0, 0), (0.0, 0, 1, 0, 1, 0, 0), (1.3, 0, 1, 0, 1, 0, 0),
         (1.0, 0, 1, 0, 1, 0, 0)]
PROCESSED = [(1.0, 5, 1, 0, 1, 0, 0), (0.9, 0, 0.8, 0, 1, 0, 0), (1.0, 20, 0.9, 0.02, 1.2, 0.3, 0), (0.0, 5, 0.5, 0, 1, 0, 0),
             (0.7, 3, 1, 0, 1, 0, 0.5), (1.0, 0, 0.5, 0.05, 1, 0, 0)]
SEEDS = {("plain", V_SMALL): 1, ("plain", V_PROD): 1, ("processed", V_SMALL): 1, ("processed", V_PROD): 1}


def integration_case(kind, V, seed=None):
    """Six rows: the three best tokens of every row are banned (a -100 bias, a stop entry masked by min_tokens, and an entry with
    bias AND stop flag), a token from the bulk gets +8 and joins the top, row 5 has no table; rows 3 and 4 sit at n == min_tokens
    - 1 and n == min_tokens.  Returns a dict with the logits, sampler state, the tables and the numpy tokens / margins."""
    spec = PLAIN if kind == "plain" else PROCESSED
    rng = np.random.default_rng(SEEDS[(kind, V)] if seed is None else seed)
    B = len(spec)
    logits = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    n_b = np.asarray([0, 2, 1, 3, 4, 2], np.int32)
    mins = [5, 3, 2, 4, 4, 0]          # row 3: n = m - 1 (masked); row 4: n = m (the stop entries get their bias only)
    plen = np.full(B, 7, np.int32)
    ctx = (plen + n_b - 1).astype(np.int32)
    rows = []
    for b in range(B):
        if b == 5:
            rows.append(([], 0))
            continue
        top = np.argsort(-logits[b])
        low = int(top[V // 2 + b])
        rows.append(([(int(top[0]), -100.0, 0), (int(top[1]), 0.0, 1), (int(top[2]), 2.0, 1), (low, 8.0, 0)], mins[b]))
    ids, vals, flags, meta = tables(B, rows)
    temps = np.asarray([s[0] for s in spec], np.float32)
    params = np.zeros((B, 8), np.float32)
    params[:, :6] = [s[1:] for s in spec]
    seeds = rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
    W = (V + 31) // 32
    counts = np.zeros((B, V), np.int32)
    pbits = np.zeros((B, W), np.uint32)
    prompts, outs = [], []
    for b in range(B):
        order = np.argsort(-logits[b])
        pr = np.r_[rng.integers(0, V, 20), order[3:6]]
        out = np.r_[rng.integers(0, V, 10), order[4:7], order[4:5]]
        prompts.append(pr)
        outs.append(out)
        np.bitwise_or.at(pbits[b], pr >> 5, (np.uint32(1) << (pr & 31).astype(np.uint32)))
        counts[b] = np.bincount(out, minlength=V)
    adjusted = np.stack([adjust_ref(logits[b], ids[b], vals[b], flags[b], meta[b, 0], meta[b, 1], int(n_b[b])) for b in range(B)])
    ref = [R.sample_step(adjusted[b], float(s[0]), int(seeds[b]), int(n_b[b]), prompts[b], outs[b], V, None, int(s[1]), float(s[2]),
                         float(s[3]), s[4], s[5], s[6]) for b, s in enumerate(spec)]
    return dict(B=B, V=V, spec=spec, logits=logits, adjusted=adjusted, temps=temps, params=params, seeds=seeds, counts=counts,
                pbits=pbits, ctx=ctx, plen=plen, ids=ids, vals=vals, flags=flags, meta=meta, ref=ref)


def decisive(case):
    """Per row: the numpy step is decided (the excuse rule does not apply)."""
    return [margin > MARGIN and not excused for _, margin, excused in case["ref"]]
