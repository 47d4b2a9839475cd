// Runaway repetition, seen on the device inside the decode step (include/karanta_hip.h, kr_repeat).
//   repeat_detect_kernel   one workgroup per slot, its threads over the periods a..b of the slot's cfg row.  The tokens the slot
//                          gained since the last launch are walked in order; per token every period updates its run counter
//                          run[p] = (g >= p && y[g] == y[g - p]) ? run[p] + 1 : 0 and tests it against max((c - 1) p, m - p); one
//                          block-wide "any" per token decides whether the sequence repeats there.
// The kernel keeps its own place (seen), so it does not know or care whether a plain step (one new token), a speculative step (up to
// k + 1) or nothing (a frozen slot) came before it.  Integer work only: plain loads and stores, no atomics.
#include "kr_decode_common.h"

namespace {

constexpr int REP_THREADS = 256, REP_PER_THREAD = KR_REP_MAX_PERIOD / REP_THREADS;

__global__ void __launch_bounds__(REP_THREADS) repeat_detect_kernel(const kr_repeat a) {
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int32_t* cfg = a.cfg + (int64_t)slot * 4;
    const int pa = cfg[0], pb = cfg[1], cnt = cfg[2], span = max(cfg[3], 0);
    // every return below is uniform over the workgroup
    if (pb == 0 || pa < 1 || pb > KR_REP_MAX_PERIOD || pa > pb || cnt < 2) return;      // off (or a row the host would have refused)
    if (a.rep_at[slot] >= 0) return;                                                    // written once
    const int fin = a.finished[slot];
    // a finished slot has no new token where it is frozen, and pads where it is not: untouched.  The one finished slot with news is
    // the one THIS step finished, under the freeze bit: a speculative step that emitted several tokens, the last of them the EOS.
    // The tokens before the EOS are still looked at, so the cut is where one-token steps would have made it.
    if (fin && !(a.flags & 2)) return;
    const int gen = min(max(a.ctx_len[slot] - a.prompt_len[slot] + 1, 0), a.hist_rows);
    const int end = fin ? gen - 1 : gen;
    const int s0 = max(a.seen[slot], 0);
    if (s0 >= end) return;
    const int32_t* y = a.history + slot;
    const int64_t ld = a.hist_stride;
    int32_t* run = a.run + (int64_t)slot * KR_REP_MAX_PERIOD;
    int r[REP_PER_THREAD];
    long long thr[REP_PER_THREAD];
#pragma unroll
    for (int k = 0; k < REP_PER_THREAD; ++k) {
        const int p = pa + tid + k * REP_THREADS;
        r[k] = p <= pb ? run[p - 1] : 0;
        thr[k] = max((long long)(cnt - 1) * p, (long long)span - p);
    }
    int found = -1;
    for (int g = s0; g < end; ++g) {
        const int yg = y[g * ld];
        int hit = 0;
#pragma unroll
        for (int k = 0; k < REP_PER_THREAD; ++k) {
            const int p = pa + tid + k * REP_THREADS;
            if (p > pb) continue;
            r[k] = (g >= p && y[(g - p) * ld] == yg) ? r[k] + 1 : 0;      // g = 0 clears every period: no reset at admission
            hit |= (long long)r[k] >= thr[k];
        }
        if (__syncthreads_or(hit)) {
            found = g;
            break;
        }
    }
    if (fin) {          // the slot is over either way; only the cause is recorded
        if (found >= 0 && tid == 0) a.rep_at[slot] = found;
        return;
    }
#pragma unroll
    for (int k = 0; k < REP_PER_THREAD; ++k) {
        const int p = pa + tid + k * REP_THREADS;
        if (p <= pb) run[p - 1] = r[k];
    }
    if (tid == 0) {
        a.seen[slot] = found >= 0 ? found + 1 : gen;      // the state is that of the last token looked at
        if (found >= 0) {
            a.rep_at[slot] = found;
            a.finished[slot] = 1;
        }
    }
}

}  // namespace

extern "C" int kr_repeat_detect(const kr_repeat* a, kr_stream s) {
    KR_CHECK_ARG(a, "kr_repeat_detect: null args");
    KR_CHECK_ARG(a->slots >= 1 && a->slots <= 32, "kr_repeat_detect: slots=%d (1..32)", a->slots);
    KR_CHECK_ARG(a->history && a->ctx_len && a->prompt_len && a->finished && a->cfg && a->run && a->seen && a->rep_at,
                 "kr_repeat_detect: null pointer");
    KR_CHECK_ARG(a->hist_stride >= a->slots && a->hist_rows >= 1, "kr_repeat_detect: hist_stride=%d hist_rows=%d (stride >= slots, rows >= 1)",
                 a->hist_stride, a->hist_rows);
    KR_CHECK_ARG((a->flags & ~3) == 0, "kr_repeat_detect: flags=%d (bits 0 and 1)", a->flags);
    if (a->flags & 1) return KR_OK;               // fixed-length runs: nothing finishes, nothing is recorded
    repeat_detect_kernel<<<a->slots, REP_THREADS, 0, kr_hs(s)>>>(*a);
    KR_CHECK_LAUNCH();
    return KR_OK;
}
