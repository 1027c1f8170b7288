// Self-attention guidance (Hong et al. 2023): the two kernels of a SAG step that are not a UNet forward.
//
// sag_attn_mass: how much attention each key token of a self-attention receives,
//     mass[b][k] = (1 / heads) * sum_h sum_q softmax_k(Q_h K_h^T)[q][k]            (the masses of a sample average exactly 1)
//   Q and K token-major bf16 with ONE row pitch (the q | k | v projection: Q = qkv, K = qkv + C, pitch 3 C); the softmax scale
//   sits in Q already.  exp2_units = 1: Q carries scale * log2 e (what W_q of attn1 is packed with, Op::qps) and the softmax is
//   exp2(s - max); 0: Q carries the scale alone, exp(s - max).
//   One workgroup of 8 waves per SAMPLE walks the heads: no scratch, no second launch, and the sum order is fixed.  Per head the
//   K rows of the head go to LDS (rows padded to 16 and zeroed, pitch D + 8), a wave takes the 16-query tiles qt = wave,
//   wave + 8, ...: Q fragments from global, S = Q K^T on v_mfma_f32_16x16x32_bf16 (K-slices past D are zero fragments) with all
//   <= 16 key tiles of the row in registers, so the softmax is the exact two-pass one in fp32 (row max, exp, row sum, one
//   reciprocal per row).  Column sums: per lane over its 4 rows in order, over the 4 row groups by two butterflies, into a per-wave
//   register accumulator over (head, then query tile); at the end the 8 waves' columns are summed in wave order through LDS and
//   scaled by 1 / heads.  No atomics: the result is the same bits on every run.
//
// sag_degrade: x [LB,4,H,W] fp32 and the model output m of the same samples -> the degraded, re-noised latents, one launch:
//     x0  = c0 x + c1 m,  eps = c2 x + c3 m          (the prediction type picks which of the four are trivial and skipped)
//     blur = 9x9 Gaussian (sigma 1) of x0 with reflect padding, separable
//     deg = mass[b][y / 8][x / 8] > 1 ? blur : x0     (strict; the mid grid is (H / 8) x (W / 8))
//     out = c4 deg + c5 eps
//   A workgroup owns a 32 x 32 pixel tile of one (sample, channel) plane: x0 of the tile and its 4-pixel halo (reflected
//   coordinates) in LDS, the horizontal pass into a second LDS image, the vertical pass from it.  Accumulation order of either
//   pass: acc = 0; for i = -4 .. 4: acc = fma(w[i], v[i], acc).  64-bit offsets.
#include "common.h"
#include "kernels.h"

#include <stdint.h>

#include <cmath>

namespace {

constexpr int SAG_THREADS = 512, SAG_WAVES = SAG_THREADS / 64;
constexpr int SAG_MAXN = 256, SAG_MAXT = SAG_MAXN / 16;

template <int D>
__global__ __launch_bounds__(SAG_THREADS) void sag_attn_mass_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, long ld,
                                                                    int N, int heads, int exp2_units, float* __restrict__ mass) {
    constexpr int NF = (D + 31) / 32, KST = D + 8, VPR = D / 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Np = (N + 15) & ~15, nkt = Np / 16;
    bf16_t* Ks = (bf16_t*)smem;                                   // [Np][KST]
    float* cs = (float*)(smem + (size_t)Np * KST * 2);            // [SAG_WAVES][Np]
    const int b = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const bf16_t* qb = Q + (long)b * N * ld;
    const bf16_t* kb = K + (long)b * N * ld;
    float col[SAG_MAXT];                    // sum over this wave's (head, query tile)s of P[.][kt * 16 + r16]
#pragma unroll
    for (int kt = 0; kt < SAG_MAXT; ++kt) col[kt] = 0.f;

    for (int h = 0; h < heads; ++h) {
        __syncthreads();                    // (the readers of the previous head's K are done)
        for (int i = threadIdx.x; i < Np * VPR; i += SAG_THREADS) {
            const int j = i / VPR, c = (i - j * VPR) * 8;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (j < N) v = *(const u32x4*)(kb + (long)j * ld + h * D + c);
            *(u32x4*)(Ks + j * KST + c) = v;
        }
        __syncthreads();
        for (int qt = wave; qt < nkt; qt += SAG_WAVES) {
            const int qrow = qt * 16 + r16;
            bf16x8 qa[NF];
#pragma unroll
            for (int s = 0; s < NF; ++s) {
                qa[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                if (qrow < N && 32 * s + 8 * g < D) qa[s] = *(const bf16x8*)(qb + (long)qrow * ld + h * D + 32 * s + 8 * g);
            }
            // lane holds S[row 4 g + r][key kt * 16 + r16]: a row lives on the 16 lanes of one group
            f32x4 sc[SAG_MAXT];
            float mx[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
#pragma unroll
            for (int kt = 0; kt < SAG_MAXT; ++kt) {
                if (kt < nkt) {
                    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < NF; ++s) {
                        bf16x8 kf = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                        if (32 * s + 8 * g < D) kf = *(const bf16x8*)(Ks + (kt * 16 + r16) * KST + 32 * s + 8 * g);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[s], kf, acc, 0, 0, 0);
                    }
                    const bool ok = kt * 16 + r16 < N;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = ok ? acc[r] : -1e30f;
                        sc[kt][r] = v;
                        mx[r] = fmaxf(mx[r], v);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o));
            float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kt = 0; kt < SAG_MAXT; ++kt) {
                if (kt < nkt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float t = sc[kt][r] - mx[r];        // (a masked key: about -1e30, its exponential is 0)
                        const float e = exp2_units ? exp2f(t) : expf(t);
                        sc[kt][r] = e;
                        sum[r] += e;
                    }
                }
            }
            float inv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o);
                inv[r] = qt * 16 + 4 * g + r < N ? 1.0f / sum[r] : 0.f;      // (query rows past N count nothing)
            }
#pragma unroll
            for (int kt = 0; kt < SAG_MAXT; ++kt) {
                if (kt < nkt) {
                    float p = sc[kt][0] * inv[0];
                    p = __builtin_fmaf(sc[kt][1], inv[1], p);
                    p = __builtin_fmaf(sc[kt][2], inv[2], p);
                    p = __builtin_fmaf(sc[kt][3], inv[3], p);
                    p += __shfl_xor(p, 16);
                    p += __shfl_xor(p, 32);
                    col[kt] += p;
                }
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int kt = 0; kt < SAG_MAXT; ++kt)
            if (kt < nkt) cs[wave * Np + kt * 16 + r16] = col[kt];
    }
    __syncthreads();
    const float inv_heads = 1.0f / (float)heads;
    for (int k = threadIdx.x; k < N; k += SAG_THREADS) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < SAG_WAVES; ++w) s += cs[w * Np + k];
        mass[(long)b * N + k] = s * inv_heads;
    }
}

constexpr int DG_TILE = 32, DG_HALO = 4, DG_IN = DG_TILE + 2 * DG_HALO, DG_THREADS = 256;

struct DegradeCoef { float c[6]; };
struct BlurTaps { float w[9]; };

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(DG_THREADS) void sag_degrade_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                                 const float* __restrict__ mass, int mh, int mw, int pred, DegradeCoef cf,
                                                                 BlurTaps tp, float* __restrict__ out, int H, int W, int tiles_x) {
    __shared__ float x0s[DG_IN][DG_IN + 1];       // x0 of the tile and its halo, reflected at the plane's edges
    __shared__ float hs[DG_IN][DG_TILE + 1];      // the horizontal pass, rows of the tile and its vertical halo
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const long plane = (long)blockIdx.z * gridDim.y + blockIdx.y;       // (sample, channel)
    const float* xp = x + plane * H * W;
    const float* mp = m + plane * H * W;
    const int y0 = ty * DG_TILE, x0c = tx * DG_TILE;
    for (int i = threadIdx.x; i < DG_IN * DG_IN; i += DG_THREADS) {
        const int r = i / DG_IN, c = i - r * DG_IN;
        // (a tile at the right / bottom edge of a plane that is no multiple of 32: clamp what lies past the reflection's reach,
        //  those pixels feed no stored output)
        const int yy = min(max(reflect_idx(y0 + r - DG_HALO, H), 0), H - 1), xx = min(max(reflect_idx(x0c + c - DG_HALO, W), 0), W - 1);
        const long o = (long)yy * W + xx;
        const float xv = xp[o], mv = mp[o];
        // epsilon: (x - sqrt(1-a) m) / sqrt(a) as c0 x + c1 m;  v_prediction: sqrt(a) x - sqrt(1-a) m;  sample: m itself
        x0s[r][c] = pred == 2 ? mv : __builtin_fmaf(cf.c[1], mv, cf.c[0] * xv);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DG_IN * DG_TILE; i += DG_THREADS) {
        const int r = i / DG_TILE, c = i - r * DG_TILE;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc = __builtin_fmaf(tp.w[k], x0s[r][c + k], acc);
        hs[r][c] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DG_TILE * DG_TILE; i += DG_THREADS) {
        const int r = i / DG_TILE, c = i - r * DG_TILE;
        const int yy = y0 + r, xx = x0c + c;
        if (yy >= H || xx >= W) continue;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc = __builtin_fmaf(tp.w[k], hs[r + k][c], acc);
        const float x0v = x0s[r + DG_HALO][c + DG_HALO];
        const bool on = mass[((long)blockIdx.z * mh + (yy >> 3)) * mw + (xx >> 3)] > 1.0f;
        const float deg = on ? acc : x0v;
        const long o = (long)yy * W + xx;
        const float xv = xp[o], mv = mp[o];
        const float e = pred == 0 ? mv : __builtin_fmaf(cf.c[3], mv, cf.c[2] * xv);
        out[plane * H * W + o] = __builtin_fmaf(cf.c[5], e, cf.c[4] * deg);
    }
}

}  // namespace

int sd_sag_mass_shape_ok(int B, int heads, int N, int D, long ld, int head_major, const char* who) {
    SD_REQUIRE(!head_major, "%s: head-major K is not built (the mid block's q | k | v projection is token-major)", who);
    SD_REQUIRE(B >= 1 && B <= 65535, "%s: batch %d (1 .. 65535)", who, B);
    SD_REQUIRE(N >= 16 && N <= SAG_MAXN, "%s: %d tokens (16 .. %d: a mid grid of 4 .. 16 per side)", who, N, SAG_MAXN);
    SD_REQUIRE(D == 64 || D == 80 || D == 160, "%s: head dim %d (64, 80 or 160)", who, D);
    SD_REQUIRE(heads >= 1 && heads <= 64, "%s: %d heads (1 .. 64)", who, heads);
    // (65535 samples of 256 rows of at most 2^30 elements: every element offset stays below 2^62)
    SD_REQUIRE(ld >= 2l * heads * D && ld % 8 == 0 && ld <= (1l << 30), "%s: row pitch %ld (a multiple of 8, at least 2 C = %d: Q and K of "
               "one row, at most 2^30)", who, ld, 2 * heads * D);
    return 0;
}

int sd_launch_sag_attn_mass(const bf16_t* Q, const bf16_t* K, long ld, float* mass, int B, int heads, int N, int D, int exp2_units,
                            hipStream_t stream) {
    if (sd_sag_mass_shape_ok(B, heads, N, D, ld, 0, "sag_attn_mass")) return -1;
    SD_REQUIRE(Q && K && mass && (uintptr_t)Q % 16 == 0 && (uintptr_t)K % 16 == 0, "sag_attn_mass: null or unaligned pointer (16 bytes)");
    const int Np = (N + 15) & ~15;
    const size_t smem = (size_t)Np * (D + 8) * 2 + (size_t)SAG_WAVES * Np * 4;
    const void* kern = D == 64 ? (const void*)sag_attn_mass_kernel<64> : D == 80 ? (const void*)sag_attn_mass_kernel<80> : (const void*)sag_attn_mass_kernel<160>;
    // (set per launch, as vit.hip and bert.hip do: no process-wide cache that another device or thread could find stale)
    SD_CHECK_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const dim3 grid((unsigned)B), block(SAG_THREADS);
    if (D == 64) hipLaunchKernelGGL(sag_attn_mass_kernel<64>, grid, block, smem, stream, Q, K, ld, N, heads, exp2_units, mass);
    else if (D == 80) hipLaunchKernelGGL(sag_attn_mass_kernel<80>, grid, block, smem, stream, Q, K, ld, N, heads, exp2_units, mass);
    else hipLaunchKernelGGL(sag_attn_mass_kernel<160>, grid, block, smem, stream, Q, K, ld, N, heads, exp2_units, mass);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_sag_degrade_shape_ok(int LB, int H, int W, int mh, int mw, int pred, const char* who) {
    SD_REQUIRE(LB >= 1 && LB <= 65535, "%s: batch %d (1 .. 65535)", who, LB);
    SD_REQUIRE(H >= 32 && H <= 128 && H % 8 == 0 && W >= 32 && W <= 128 && W % 8 == 0, "%s: latent %dx%d (multiples of 8 in 32 .. 128)", who, H, W);
    SD_REQUIRE(mh * 8 == H && mw * 8 == W, "%s: mid grid %dx%d under a %dx%d latent (the upsampling factor is 8)", who, mh, mw, H, W);
    SD_REQUIRE(pred >= 0 && pred <= 2, "%s: prediction type %d (0 epsilon, 1 v_prediction, 2 sample)", who, pred);
    return 0;
}

int sd_launch_sag_degrade(const float* x, const float* m, const float* mass, int mh, int mw, int pred, const float coef[6], float* out,
                          int LB, int H, int W, hipStream_t stream) {
    if (sd_sag_degrade_shape_ok(LB, H, W, mh, mw, pred, "sag_degrade")) return -1;
    SD_REQUIRE(x && m && mass && out && coef, "sag_degrade: null operand");
    SD_REQUIRE(out != x && out != m, "sag_degrade: the output aliases an input (the blur reads neighbours)");
    DegradeCoef cf;
    for (int i = 0; i < 6; ++i) {
        SD_REQUIRE(std::isfinite(coef[i]), "sag_degrade: coefficient %d = %g must be finite", i, (double)coef[i]);
        cf.c[i] = coef[i];
    }
    // the 1-D weights exp(-0.5 i^2), i = -4 .. 4, normalised in fp64, rounded once
    BlurTaps tp;
    double wsum = 0.0, wd[9];
    for (int i = 0; i < 9; ++i) { wd[i] = std::exp(-0.5 * (i - 4) * (i - 4)); wsum += wd[i]; }
    for (int i = 0; i < 9; ++i) tp.w[i] = (float)(wd[i] / wsum);
    const int tiles_x = (W + DG_TILE - 1) / DG_TILE, tiles_y = (H + DG_TILE - 1) / DG_TILE;
    hipLaunchKernelGGL(sag_degrade_kernel, dim3((unsigned)(tiles_x * tiles_y), 4, (unsigned)LB), dim3(DG_THREADS), 0, stream, x, m, mass, mh,
                       mw, pred, cf, tp, out, H, W, tiles_x);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
