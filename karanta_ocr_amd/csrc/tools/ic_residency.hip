// Micro-benchmark (round 5): do weight lines loaded with the DEFAULT cache policy stay in the 256 MiB Infinity Cache while a
// decode step's other weights stream past them with NONTEMPORAL loads?
// The decode linears read every weight byte with a nontemporal 16-byte load (WChunk::load, kr_decode_common.h), 1 KiB per
// wave-instruction.  qkv (176 MB over 28 layers of the 2B model) and o_proj (132 MB) are latency-bound, so they would gain from
// Infinity-Cache hits if their lines survived the 3.3 GB that gate/up, down_proj, lm_head and the KV cache stream in between.
// For table sizes T and stream sizes S, per repeat:
//   1. read the table once, default policy                                  (puts it on the die)
//   2. stream S bytes of ANOTHER buffer, nontemporal (or default policy: the control, which must evict the table)
//   3. time a default-policy re-read of the table with HIP events
// Every wave reads 4 KiB units (four 1 KiB wave-instructions in flight), unit u of wave w = u * n_waves + w; the trip count is
// a kernel argument, no kernel waits on another.  Two re-read grids: "full" (4 workgroups of 4 waves per CU: a bandwidth figure)
// and "thin" (1 workgroup of 4 waves per CU, closer to the latency-bound qkv / o_proj launches).
// S = 0 at T = 32 MB is served partly from the 8 x 4 MiB L2s, which any stream flushes; judge residency at T >= 64 MB.
// Build: hipcc -O3 --offload-arch=gfx950 ic_residency.hip -o /tmp/ic_residency ; run: /tmp/ic_residency
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr size_t UNIT = 4096;   // bytes per wave and trip: 4 wave-instructions of 1 KiB

// reads units [0, n_units) of p; wave w takes units w, w + n_waves, ...; `trips` = ceil(n_units / n_waves) bounds the loop
template <bool NT>
__global__ void __launch_bounds__(256) rd(const char* __restrict__ p, size_t n_units, int trips, unsigned* sink) {
    const int lane = threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t n_waves = (size_t)gridDim.x * 4;
    u32x4 acc = {0, 0, 0, 0};
    for (int u = 0; u < trips; ++u) {
        const size_t unit = (size_t)u * n_waves + wave;
        if (unit >= n_units) break;
        const u32x4* q = reinterpret_cast<const u32x4*>(p + unit * UNIT) + lane;
        u32x4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = NT ? __builtin_nontemporal_load(q + i * 64) : q[i * 64];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc ^= v[i];
    }
    if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1;
}

template <bool NT>
static void read_buf(const char* p, size_t bytes, int blocks, unsigned* sink, hipStream_t s) {
    const size_t n_units = bytes / UNIT, n_waves = (size_t)blocks * 4;
    if (!n_units) return;
    rd<NT><<<blocks, 256, 0, s>>>(p, n_units, (int)((n_units + n_waves - 1) / n_waves), sink);
}

struct Cell { float med_us, min_us; };

static Cell cell(const char* table, size_t t_bytes, const char* stream, size_t s_bytes, bool stream_nt, int reread_blocks,
                 unsigned* sink, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    constexpr int REP = 5;
    float us[REP];
    for (int r = 0; r < REP; ++r) {
        read_buf<false>(table, t_bytes, 1024, sink, s);
        if (stream_nt) read_buf<true>(stream, s_bytes, 1024, sink, s);
        else read_buf<false>(stream, s_bytes, 1024, sink, s);
        CK(hipEventRecord(e0, s));
        read_buf<false>(table, t_bytes, reread_blocks, sink, s);
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        us[r] = ms * 1e3f;
    }
    std::sort(us, us + REP);
    return {us[REP / 2], us[0]};
}

int main() {
    hipStream_t s; CK(hipStreamCreate(&s));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const size_t MB = 1000 * 1000;
    const size_t t_sizes[] = {32 * MB, 64 * MB, 128 * MB, 192 * MB, 240 * MB};
    const size_t s_sizes[] = {0, 500 * MB, 3300 * MB};
    char *table, *stream; unsigned* sink;
    CK(hipMalloc(&table, 240 * MB)); CK(hipMalloc(&stream, 3300 * MB)); CK(hipMalloc(&sink, 4));
    CK(hipMemset(table, 1, 240 * MB)); CK(hipMemset(stream, 2, 3300 * MB)); CK(hipMemset(sink, 0, 4));
    CK(hipDeviceSynchronize());
    // warm-up: code objects loaded, clocks up
    for (int i = 0; i < 3; ++i) read_buf<true>(stream, 3300 * MB, 1024, sink, s);
    CK(hipStreamSynchronize(s));

    for (int reread_blocks : {1024, 256}) {
        printf("\nre-read grid: %d workgroups x 4 waves (%s)\n", reread_blocks, reread_blocks == 1024 ? "full" : "thin");
        printf("%7s %8s %-8s %10s %10s %10s\n", "T (MB)", "S (GB)", "stream", "median us", "min us", "GB/s (med)");
        for (size_t t : t_sizes) {
            const size_t t_read = t / UNIT * UNIT;
            for (int nt = 1; nt >= 0; --nt) {
                for (size_t sb : s_sizes) {
                    if (!nt && sb == 0) continue;   // no stream: one row is enough
                    const Cell c = cell(table, t, stream, sb, nt, reread_blocks, sink, s, e0, e1);
                    printf("%7zu %8.1f %-8s %10.1f %10.1f %10.0f\n", t / MB, sb / 1e9, sb == 0 ? "-" : nt ? "nt" : "default",
                           c.med_us, c.min_us, t_read / (c.med_us * 1e-6) / 1e9);
                }
            }
        }
    }
    return 0;
}
