// T-GATE (Zhang et al. 2024, "Cross-Attention Makes Inference Cumbersome in Text-to-Image Diffusion Models"): the two
// elementwise kernels around a transformer block's cached prompt cross-attention output.
//
//   capture (the last step before the gate):  y [pair * rows][C] = attn2 after to_out and its bias, WITHOUT the residual
//       h2[m]    = bf16(float(res[m]) + float(y[m]))                          for all pair * rows rows
//       cache[m] = bf16((float(y[m]) + float(y[rows + m])) * 0.5)             for m < rows   (pair == 1: cache = y)
//   apply (every step from the gate on):
//       h2[m]    = bf16(float(h1[m]) + float(cache[m]))                       for all rows
//
// Both also write the LayerNorm partials of the STORED h2 that the norm3-folded GEGLU projection reads (GemmArgs::ln_rs,
// gemm_conv.hip::check_ln): rowstats[part][M][2] = (sum, sum of squares) of the bf16-rounded row, SD_TGATE_PARTS = 2 partials per
// row -- partial 0 over the row's first ceil(C / 16) 16-byte vectors, partial 1 over the rest.
//
// Work split.  Everything is HBM-bound: three (apply) or 2.5 (capture) row streams.  One wave owns one cache row -- and with
// it the `pair` rows of y / res / h2 that share it -- and its lanes run along the channels in 16-byte vectors (C / 8 of them:
// 40, 80 or 160 at the UNet's widths).  A lane keeps the two partials' sums in registers; the wave folds them with xor
// shuffles in a fixed order (deterministic) and lane 0 stores them.  Workgroups of four waves stride over the rows (the grid
// is capped: Guideline 11 of the HIP guide, ~8 workgroups per CU).  No LDS, no atomics.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int TGATE_THREADS = 256;
constexpr int TGATE_WAVES = TGATE_THREADS / 64;
constexpr int TGATE_MAX_BLOCKS = 2048;

__device__ __forceinline__ void unpack8(const u32x4 v, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[2 * j] = bflo(v[j]); f[2 * j + 1] = bfhi(v[j]); }
}

// out = bf16(a + b) per element; the rounded values' sum and sum of squares are added to (s, q)
__device__ __forceinline__ u32x4 add_round_stats(const float (&a)[8], const float (&b)[8], float& s, float& q) {
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = pack2bf(a[2 * j] + b[2 * j], a[2 * j + 1] + b[2 * j + 1]);
        const float lo = bflo(o[j]), hi = bfhi(o[j]);
        s += lo; q = __builtin_fmaf(lo, lo, q);
        s += hi; q = __builtin_fmaf(hi, hi, q);
    }
    return o;
}

__device__ __forceinline__ void store_partials(float* __restrict__ rowstats, long M, long row, float (&s)[2], float (&q)[2], int lane) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        s[p] = wave_sum(s[p]);
        q[p] = wave_sum(q[p]);
    }
    if (lane == 0) {
        *(f32x2_t*)(rowstats + row * 2) = f32x2_t{s[0], q[0]};
        *(f32x2_t*)(rowstats + (M + row) * 2) = f32x2_t{s[1], q[1]};
    }
}

// PAIR rows of (a, b) per cache row.  CAPTURE: a = y, b = res, and the cache row is written; else a = h1, b = cache (PAIR == 1).
template <int PAIR, bool CAPTURE>
__global__ __launch_bounds__(TGATE_THREADS) void tgate_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b,
                                                              bf16_t* __restrict__ h2, bf16_t* __restrict__ cache,
                                                              float* __restrict__ rowstats, long rows, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = C >> 3, half = (nv + 1) >> 1;      // 16-byte vectors per row, ... of partial 0
    const long M = rows * PAIR;
    for (long row = (long)blockIdx.x * TGATE_WAVES + wave; row < rows; row += (long)gridDim.x * TGATE_WAVES) {
        float s[PAIR][2], q[PAIR][2];
#pragma unroll
        for (int k = 0; k < PAIR; ++k) s[k][0] = s[k][1] = q[k][0] = q[k][1] = 0.f;
        for (int v = lane; v < nv; v += 64) {
            const int part = v >= half;
            float fa[PAIR][8];
#pragma unroll
            for (int k = 0; k < PAIR; ++k) {
                const long off = ((long)k * rows + row) * C + (long)v * 8;
                float fb[8];
                unpack8(*(const u32x4*)(a + off), fa[k]);
                unpack8(*(const u32x4*)(b + off), fb);
                float ps = 0.f, pq = 0.f;
                *(u32x4*)(h2 + off) = add_round_stats(fa[k], fb, ps, pq);
                // (selects, not an indexed array: the sums stay in registers)
                s[k][0] += part ? 0.f : ps; q[k][0] += part ? 0.f : pq;
                s[k][1] += part ? ps : 0.f; q[k][1] += part ? pq : 0.f;
            }
            if (CAPTURE) {
                u32x4 c;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (PAIR == 2) c[j] = pack2bf((fa[0][2 * j] + fa[PAIR - 1][2 * j]) * 0.5f, (fa[0][2 * j + 1] + fa[PAIR - 1][2 * j + 1]) * 0.5f);
                    else c[j] = pack2bf(fa[0][2 * j], fa[0][2 * j + 1]);
                }
                *(u32x4*)(cache + row * C + (long)v * 8) = c;
            }
        }
        if (rowstats) {
#pragma unroll
            for (int k = 0; k < PAIR; ++k) store_partials(rowstats, M, (long)k * rows + row, s[k], q[k], lane);
        }
    }
}

unsigned tgate_grid(long rows) {
    const long blocks = (rows + TGATE_WAVES - 1) / TGATE_WAVES;
    return (unsigned)(blocks < TGATE_MAX_BLOCKS ? blocks : TGATE_MAX_BLOCKS);
}

}  // namespace

int sd_tgate_check(long rows, int C, const char* who) {
    SD_REQUIRE(rows >= 1 && rows <= (1l << 40), "%s: rows=%ld (at least 1)", who, rows);
    SD_REQUIRE(C >= 8 && C % 8 == 0 && C <= 65536, "%s: C=%d (a multiple of 8: the rows are read in 16-byte vectors)", who, C);
    return 0;
}

int sd_launch_tgate_capture(const bf16_t* y, const bf16_t* res, bf16_t* h2, bf16_t* cache, float* rowstats, long rows, int C, int pair,
                            hipStream_t stream) {
    SD_REQUIRE(y && res && h2 && cache, "tgate_capture: null argument");
    SD_REQUIRE(pair == 1 || pair == 2, "tgate_capture: pair=%d (1, or 2 for a classifier-free-guidance pair [uncond | cond])", pair);
    if (sd_tgate_check(rows, C, "tgate_capture")) return -1;
    SD_REQUIRE(((uintptr_t)y | (uintptr_t)res | (uintptr_t)h2 | (uintptr_t)cache) % 16 == 0 && (uintptr_t)rowstats % 8 == 0,
               "tgate_capture: the tensors must be 16-byte aligned");
    SD_REQUIRE(h2 != y && h2 != res && cache != y && cache != h2 && cache != res, "tgate_capture: the outputs must be new tensors (the inputs are never modified)");
    if (pair == 2)
        hipLaunchKernelGGL((tgate_kernel<2, true>), dim3(tgate_grid(rows)), dim3(TGATE_THREADS), 0, stream, y, res, h2, cache, rowstats, rows, C);
    else
        hipLaunchKernelGGL((tgate_kernel<1, true>), dim3(tgate_grid(rows)), dim3(TGATE_THREADS), 0, stream, y, res, h2, cache, rowstats, rows, C);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_tgate_apply(const bf16_t* h1, const bf16_t* cache, bf16_t* h2, float* rowstats, long rows, int C, hipStream_t stream) {
    SD_REQUIRE(h1 && cache && h2, "tgate_apply: null argument");
    if (sd_tgate_check(rows, C, "tgate_apply")) return -1;
    SD_REQUIRE(((uintptr_t)h1 | (uintptr_t)cache | (uintptr_t)h2) % 16 == 0 && (uintptr_t)rowstats % 8 == 0,
               "tgate_apply: the tensors must be 16-byte aligned");
    SD_REQUIRE(h2 != cache && h2 != h1, "tgate_apply: the output must be a new tensor (the inputs are never modified)");
    hipLaunchKernelGGL((tgate_kernel<1, false>), dim3(tgate_grid(rows)), dim3(TGATE_THREADS), 0, stream, h1, cache, h2, (bf16_t*)nullptr,
                       rowstats, rows, C);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
