// Host check of kr_spec_deal's arithmetic (csrc/kr_spec_deal.h), to be built with a sanitizer and run as a plain program BEFORE the
// kernel first runs on a GPU: a wrong row here is a K/V write outside a sequence's cache there.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I karanta_ocr_amd/csrc \
//       karanta_ocr_amd/csrc/tools/spec_deal_check.cpp -o spec_deal_check && ./spec_deal_check
// It replays spec_deal_kernel's phases thread by thread on heap arrays of exactly the sizes the kernel's buffers have, for the
// hand-worked cases of tests/test_spec_deal_cpu.py, for every (B, K, rows) the engine can ask for with random wants, and compares
// with the rule stated as a loop: for depth, for slot, take the next free row.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_spec_deal.h"

namespace {

struct Dealt {
    std::vector<int> n_draft, draft_row, owner;      // [B], [B * K], [rows] (-1: parked)
};

// the kernel's phases, serially; every array has the kernel's size, so the sanitizer sees an index the kernel would get wrong
Dealt kernel_phases(const std::vector<int>& n_want, const std::vector<int>& fin, const std::vector<int>& ctx, int K, int R, int s_max) {
    const int B = (int)n_want.size();
    std::vector<int> s_want(32), s_cnt(33, -12345), s_owner(32, -1);
    for (int tid = 0; tid < 32; ++tid) s_want[tid] = tid < B ? spec_deal_want(n_want[tid], fin[tid], K, ctx[tid], s_max) : 0;
    for (int tid = 1; tid <= K; ++tid) s_cnt[tid] = spec_deal_count(s_want.data(), B, tid);
    Dealt d{std::vector<int>(B), std::vector<int>(B * K), std::vector<int>(R, -1)};
    for (int e = 0; e < B * K; ++e) {
        const int slot = e / K, j = e - slot * K + 1;
        const int r = spec_deal_row(s_want.data(), s_cnt.data(), B, R, slot, j);
        d.draft_row[e] = r;
        if (r >= 0) {
            if (s_owner[r] != -1) { std::printf("row %d dealt twice\n", r); std::exit(1); }
            s_owner[r] = e;
        }
    }
    for (int tid = 0; tid < B; ++tid) {
        int nd = 0;
        for (int j = 1; j <= s_want[tid]; ++j)
            if (spec_deal_row(s_want.data(), s_cnt.data(), B, R, tid, j) >= 0) nd = j;
        d.n_draft[tid] = nd;
    }
    for (int tid = 0; tid < R - B; ++tid) d.owner[B + tid] = s_owner[B + tid];      // the row-state phase: r = B + tid < R
    return d;
}

// the rule as it is stated
Dealt rule(const std::vector<int>& n_want, const std::vector<int>& fin, const std::vector<int>& ctx, int K, int R, int s_max) {
    const int B = (int)n_want.size();
    Dealt d{std::vector<int>(B, 0), std::vector<int>(B * K, -1), std::vector<int>(R, -1)};
    int next = B;
    for (int j = 1; j <= K; ++j)
        for (int s = 0; s < B; ++s)
            if (!fin[s] && n_want[s] >= j && j <= s_max - 1 - ctx[s] && next < R) {
                d.draft_row[s * K + j - 1] = next;
                d.owner[next] = s * K + j - 1;
                d.n_draft[s] += 1;
                ++next;
            }
    return d;
}

int g_cases = 0;

void check(const std::vector<int>& n_want, const std::vector<int>& fin, const std::vector<int>& ctx, int K, int R, int s_max,
           const std::vector<int>* want_rows = nullptr) {
    const Dealt a = kernel_phases(n_want, fin, ctx, K, R, s_max), b = rule(n_want, fin, ctx, K, R, s_max);
    bool ok = a.n_draft == b.n_draft && a.draft_row == b.draft_row && a.owner == b.owner;
    if (want_rows) ok = ok && a.draft_row == *want_rows;
    const int B = (int)n_want.size();
    for (int s = 0; s < B && ok; ++s)       // a slot's dealt depths are a prefix, and every dealt row lies in B .. R - 1
        for (int j = 1; j <= K; ++j) {
            const int r = a.draft_row[s * K + j - 1];
            ok = ok && (r >= 0) == (j <= a.n_draft[s]) && (r < 0 || (r >= B && r < R));
        }
    if (!ok) {
        std::printf("MISMATCH B=%d K=%d rows=%d want=", B, K, R);
        for (int w : n_want) std::printf("%d ", w);
        std::printf("\n");
        std::exit(1);
    }
    ++g_cases;
}

}  // namespace

int main() {
    const int S = 64;
    const std::vector<int> live5(5, 0), c5(5, 10);
    // the hand-worked cases (tests/test_spec_deal_cpu.py), draft_row as [slot][depth]
    { std::vector<int> r{5, 8, 10, -1, -1, -1, 6, 9, -1, 7, -1, -1, -1, -1, -1};                  // everything fits
      check({3, 0, 2, 1, 0}, live5, c5, 3, 17, S, &r); }
    { std::vector<int> r{20, -1, 21, -1, 22, -1, 23, -1, 24, -1, 25, -1, 26, -1, 27, -1, 28, -1, 29, -1, 30, -1, 31, -1,
                         -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};          // the budget ends in depth 1
      check(std::vector<int>(20, 2), std::vector<int>(20, 0), std::vector<int>(20, 10), 2, 32, S, &r); }
    { std::vector<int> r{4, 8, -1, 5, 9, -1, 6, -1, -1, 7, -1, -1};                               // ... in the middle of depth 2
      check({3, 3, 3, 3}, {0, 0, 0, 0}, {10, 10, 10, 10}, 3, 10, S, &r); }
    { std::vector<int> r{-1, -1, -1, 5, 7, 8, -1, -1, -1, 6, -1, -1, -1, -1, -1};                  // finished / n_want = 0 take nothing
      check({3, 3, 0, 1, 2}, {1, 0, 0, 0, 1}, c5, 3, 17, S, &r); }
    { std::vector<int> r(31 * 3, -1); r[2 * 3] = 31;                                              // rows - B = 1: the first that wants
      std::vector<int> w(31, 0); w[2] = 2; w[7] = 3;
      check(w, std::vector<int>(31, 0), std::vector<int>(31, 10), 3, 32, S, &r); }
    { std::vector<int> r{2, -1, -1, 3, 4, 5};                                                     // ctx = s_max - 2: one cache row left
      check({3, 3}, {0, 0}, {S - 2, 10}, 3, 17, S, &r); }
    // every layout the entry point admits (1 <= B < rows <= 32, 1 <= K < 32), random wants (also outside 0..K), finished slots, tight caches
    unsigned x = 12345u;
    auto rnd = [&](int n) { x = x * 1664525u + 1013904223u; return (int)((x >> 8) % (unsigned)n); };
    for (int R = 2; R <= 32; ++R)
        for (int B = 1; B < R; ++B)
            for (int K = 1; K < 32; K += (K < 4 ? 1 : 9))
                for (int rep = 0; rep < 6; ++rep) {
                    std::vector<int> w(B), f(B), c(B);
                    for (int s = 0; s < B; ++s) {
                        w[s] = rep == 0 ? K : rep == 1 ? 0 : rnd(K + 4) - 1;
                        f[s] = rnd(5) == 0;
                        c[s] = rnd(4) == 0 ? S - 1 - rnd(3) : rnd(40);
                    }
                    check(w, f, c, K, R, S);
                }
    std::printf("spec_deal_check: %d cases ok\n", g_cases);
    return 0;
}
