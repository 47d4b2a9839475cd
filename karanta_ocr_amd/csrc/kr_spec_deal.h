// The arithmetic of kr_spec_deal (kr_spec.hip: spec_deal_kernel), apart so that a host program can run it under a sanitizer
// (csrc/tools/spec_deal_check.cpp): which row a draft is dealt.
#pragma once

#if defined(__HIPCC__)
#define KR_SPEC_HD __host__ __device__
#else
#define KR_SPEC_HD
#endif

// How many drafts a slot takes part in the dealing with: none when it is finished, never more than k or than the cache rows behind
// its position.
KR_SPEC_HD inline int spec_deal_want(int n_want, int finished, int k, int ctx, int s_max) {
    if (finished) return 0;
    int w = n_want < k ? n_want : k;
    const int room = s_max - 1 - ctx;
    w = w < room ? w : room;
    return w > 0 ? w : 0;
}

// cnt[j], j = 1..k: the slots that want a draft of depth j.
KR_SPEC_HD inline int spec_deal_count(const int* want, int B, int j) {
    int c = 0;
    for (int s = 0; s < B; ++s) c += want[s] >= j ? 1 : 0;
    return c;
}

// The row of draft (slot, j), 1 <= j <= k: rows B .. R - 1 go breadth first — depth 1 of every slot in slot order, then depth 2, ... —
// so it is B + sum_{j' < j} cnt[j'] + #{s' < slot : want[s'] >= j}; -1 when the slot does not want that depth or the rows have run out.
KR_SPEC_HD inline int spec_deal_row(const int* want, const int* cnt, int B, int R, int slot, int j) {
    if (want[slot] < j) return -1;
    int r = B;
    for (int jj = 1; jj < j; ++jj) r += cnt[jj];
    for (int s = 0; s < slot; ++s) r += want[s] >= j ? 1 : 0;
    return r < R ? r : -1;
}
