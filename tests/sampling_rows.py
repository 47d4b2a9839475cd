"""Device state of a batch of sampler rows (kr_sample_threshold, kr_gumbel_argmax_processed) and the 32 Gaussian rows at the
production vocabulary: shared by tests/test_gpu_sampling_kernels.py, tests/test_gpu_sampling_select.py and (prod_batch, which
needs no device) tests/test_select_cases_cpu.py."""
import numpy as np
import torch

from karanta_ocr_amd._lib import ptr
from tests.select_cases import V_PROD, pick  # noqa: F401  (pick: re-exported for the GPU modules)

DEV = "cuda:0"


def d(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


class Rows:
    """Device state of a batch of rows for the three entry points."""

    def __init__(self, logits, temps, seeds, params, counts, pbits, ctx, plen, masks=None, gstate=None, finished=None):
        B, V = logits.shape
        self.B, self.V = B, V
        self.logits, self.temps, self.seeds = d(logits, np.float32), d(temps, np.float32), d(np.asarray(seeds, np.uint32).view(np.int32))
        self.params, self.counts, self.pbits = d(params, np.float32), d(counts, np.int32), d(np.asarray(pbits, np.uint32).view(np.int32))
        self.ctx, self.plen = d(ctx, np.int32), d(plen, np.int32)
        self.fin = d(np.zeros(B, np.int32) if finished is None else finished, np.int32)
        self.masks = masks
        self.gstate = d(np.zeros(B, np.int32) if gstate is None else gstate, np.int32)
        self.work = torch.zeros(B, V, device=DEV)
        self.thr = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.live = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.mask_words = 2 * ((V + 63) // 64)

    def gm(self):
        return None if self.masks is None else ptr(self.masks[0])

    def threshold(self, L, ignore_eos=0):
        assert L.kr_sample_threshold(ptr(self.logits), self.V, self.V, ptr(self.temps), ptr(self.params), ptr(self.counts), self.V,
                                     ptr(self.pbits), self.pbits.shape[1], self.gm(), ptr(self.gstate), self.mask_words,
                                     ptr(self.fin), ignore_eos, ptr(self.work), self.V, ptr(self.thr), ptr(self.live), self.B, 0) == 0
        torch.cuda.synchronize()
        return self.thr.cpu().numpy().view(np.uint32).astype(np.uint64)

    def argmax(self, L, n_part):
        av = torch.zeros(self.B, n_part, device=DEV)
        ai = torch.zeros(self.B, n_part, dtype=torch.int32, device=DEV)
        assert L.kr_gumbel_argmax_processed(ptr(self.logits), self.V, self.V, ptr(self.temps), ptr(self.seeds), ptr(self.ctx),
                                            ptr(self.plen), ptr(av), ptr(ai), n_part, self.B, self.gm(), ptr(self.gstate),
                                            self.mask_words, 0, ptr(self.params), ptr(self.counts), self.V, ptr(self.pbits),
                                            self.pbits.shape[1], ptr(self.thr), 0) == 0
        torch.cuda.synchronize()
        return av.cpu().numpy(), ai.cpu().numpy()


# ----------------------------------------------------------------------------- the Gaussian production rows (numpy only)
def prod_batch(rng):
    """32 rows at the production vocabulary: logits with ties built in, every control alone and combined, penalties, a guided
    row, greedy rows."""
    B, V = 32, V_PROD
    logits = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    for b in range(B):     # exact ties around the top and in the bulk
        top = np.argsort(-logits[b])[:40]
        logits[b, top[5:9]] = logits[b, top[5]]
        logits[b, top[20:25]] = logits[b, top[20]]
        logits[b, rng.integers(0, V, 500)] = logits[b, top[30]]
    spec = [  # (T, top_k, top_p, min_p, rep, freq, pres)
        (1.0, 1, 1, 0, 1, 0, 0), (1.0, 5, 1, 0, 1, 0, 0), (0.7, 7, 1, 0, 1, 0, 0), (1.0, 50, 1, 0, 1, 0, 0),
        (1.3, 1000, 1, 0, 1, 0, 0), (1.0, V + 5, 1, 0, 1, 0, 0), (1.0, 0, 0.1, 0, 1, 0, 0), (1.0, 0, 0.5, 0, 1, 0, 0),
        (0.8, 0, 0.9, 0, 1, 0, 0), (2.0, 0, 0.99, 0, 1, 0, 0), (1.0, 0, 1e-6, 0, 1, 0, 0), (1.0, 0, 1, 0.01, 1, 0, 0),
        (1.0, 0, 1, 0.1, 1, 0, 0), (0.5, 0, 1, 0.5, 1, 0, 0), (1.0, 0, 1, 1.0, 1, 0, 0), (1.0, 40, 0.9, 0.05, 1, 0, 0),
        (1.0, 10, 0.5, 0, 1, 0, 0), (3.0, 0, 0.95, 0.001, 1, 0, 0), (1.0, 0, 0.9, 0, 1.3, 0, 0), (1.0, 20, 1, 0, 1.1, 0.5, 0.3),
        (0.9, 0, 0.8, 0.02, 1.05, -0.4, 1.2), (1.0, 0, 1, 0, 1, 0, 0), (0.0, 0, 1, 0, 1, 0, 0), (0.0, 5, 0.5, 0.1, 1, 0, 0),
        (0.0, 0, 1, 0, 1.2, 0.3, 0), (1.0, 0, 0.9, 0, 1, 0, 0), (1.0, 3, 1, 0, 1, 0, 0), (0.6, 0, 0.7, 0, 1, 0, 0),
        (1.0, 0, 1, 0, 1, 0, 0), (1.0, 100, 0.99, 0, 1, 0, 0), (1.5, 0, 0.3, 0.2, 2.0, 1.0, 1.0), (1.0, 2, 1, 0, 1, 0, 0),
    ]
    temps = np.asarray([s[0] for s in spec], np.float32)
    params = np.zeros((B, 8), np.float32)
    params[:, :6] = [[s[1], s[2], s[3], s[4], s[5], s[6]] for s in spec]
    W = (V + 31) // 32
    prompts, outs = [], []
    counts = np.zeros((B, V), np.int32)
    pbits = np.zeros((B, W), np.uint32)
    for b in range(B):
        pr = rng.integers(0, V, 60)
        pr = np.r_[pr, np.argsort(-logits[b])[:6]]        # penalties hit the top of the row
        out = np.r_[rng.integers(0, V, 30), np.argsort(-logits[b])[2:5], np.argsort(-logits[b])[2:4]]
        prompts.append(pr)
        outs.append(out)
        np.bitwise_or.at(pbits[b], pr >> 5, (np.uint32(1) << (pr & 31).astype(np.uint32)))
        counts[b] = np.bincount(out, minlength=V)
    return logits, temps, params, prompts, outs, counts, pbits, spec
