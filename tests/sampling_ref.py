"""numpy restatement of the sampling controls (kr_sample_threshold / kr_gumbel_argmax_processed).

Penalties and temperature in fp32, in the kernels' operation order (bit for bit); the truncation sets in float64, with the
tokens whose min_p / top_p boundary lies within `rel` of the cut reported as excused (fp32 exp / log differ there)."""
import numpy as np

from oracle import qwen2vl_oracle as O


def fkey(v: np.ndarray) -> np.ndarray:
    """Order-preserving uint32 key of fp32 values (the kernels' threshold keys)."""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    neg = (u & 0x80000000) != 0
    return np.where(neg, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def penalise(logits, prompt_ids, out_tokens, vocab, rep=1.0, freq=0.0, pres=0.0):
    """l' of one row: repetition on the prompt set or output tokens, then l' -= f * c + p * (c > 0); fp32."""
    l = np.asarray(logits, np.float32).copy()
    if rep == 1.0 and freq == 0.0 and pres == 0.0:
        return l
    c = np.bincount(np.asarray(out_tokens, np.int64), minlength=vocab)[:vocab]
    hit = c > 0
    if len(prompt_ids):
        hit[np.asarray(prompt_ids, np.int64)] = True
    r = np.float32(rep)
    with np.errstate(over="ignore"):      # np.where computes both branches: l * r may overflow where it is not taken
        l = np.where(hit, np.where(l > 0, l / r, l * r), l).astype(np.float32)
    sub = (np.float32(freq) * c.astype(np.float32)).astype(np.float32) + \
          (np.float32(pres) * (c > 0).astype(np.float32)).astype(np.float32)
    return (l - sub.astype(np.float32)).astype(np.float32)


def tempered(lp, T):
    return (np.asarray(lp, np.float32) * (np.float32(1.0) / np.float32(T))).astype(np.float32) if T > 0 else lp


def kept_set(v, allowed, top_k=0, top_p=1.0, min_p=0.0, rel=1e-4):
    """(kept, excused) boolean arrays over the vocabulary for the scores v (fp32) of the allowed tokens.
    The `>=` here compares VALUES, so -0 and +0 are one score; the device compares keys (fkey / kr_fkey), in which -0
    ranks below +0: a cut at +0 drops the tokens at -0 there.  tests/select_cases.py pins that case to the key."""
    v = np.asarray(v, np.float32)
    keep = np.asarray(allowed, bool).copy()
    exc = np.zeros_like(keep)
    vmax = float(v[keep].max())
    if min_p > 0:
        cut32 = np.float32(np.float32(vmax) + np.float32(np.log(np.float32(min_p))))
        cut = float(np.log(min_p)) + vmax
        exc |= keep & (np.abs(v.astype(np.float64) - cut) <= rel * max(1.0, abs(cut)))
        keep &= v >= cut32
    if top_k > 0 and top_k < int(keep.sum()):
        kth = np.sort(v[keep])[::-1][top_k - 1]
        keep &= v >= kth
    if top_p < 1.0:
        idx = np.flatnonzero(keep)
        vs = v[idx].astype(np.float64)
        pr = np.exp(vs - vmax)
        pr /= pr.sum()
        order = np.argsort(-vs, kind="stable")
        # mass strictly above each token's value (ties share it): kept <=> that mass < top_p
        sv, sp = vs[order], pr[order]
        cum_incl = np.cumsum(sp)
        uniq, first = np.unique(-sv, return_index=True)          # groups of equal value, descending v
        last = np.r_[first[1:], len(sv)] - 1
        above_g = np.r_[0.0, cum_incl[last][:-1]]
        grp = np.searchsorted(uniq, -sv)
        above = np.empty(len(idx))
        above[order] = above_g[grp]
        k2 = above < top_p
        k2[np.argmax(vs)] = True
        e2 = np.abs(above - top_p) <= rel * top_p
        keep[idx[~k2]] = False
        exc[idx[e2]] = True
    return keep, exc


def sample_step(logits, T, seed, n, prompt_ids, out_tokens, vocab, allowed=None, top_k=0, top_p=1.0, min_p=0.0, rep=1.0,
                freq=0.0, pres=0.0):
    """(token, margin, excused_token) of one sampling step: the argmax over the kept tokens of v + G(seed, n, i) (T > 0)
    or of l' (T == 0); margin = top-2 gap of what the argmax runs over; excused = the winner or runner-up is a boundary token."""
    allowed = np.ones(vocab, bool) if allowed is None else np.asarray(allowed, bool)
    lp = penalise(logits, prompt_ids, out_tokens, vocab, rep, freq, pres)
    if T > 0:
        v = tempered(lp, T)
        keep, exc = kept_set(v, allowed, top_k, top_p, min_p)
        sc = (v + O.gumbel_noise(seed, n, vocab)).astype(np.float32)
    else:
        keep, exc, sc = allowed, np.zeros(vocab, bool), lp
    sc = np.where(keep | exc, sc, -np.inf)
    top = np.argsort(-sc, kind="stable")[:2]
    tok = int(np.argmax(np.where(keep, sc, -np.inf)))
    return tok, float(sc[top[0]] - sc[top[1]]), bool(exc[top[0]] or exc[top[1]])
