// IP-Adapter image branch of the prompt cross-attention (diffusers IPAdapterAttnProcessor2_0, one adapter, T = 4 image tokens):
//
//   R'[m, :] = R[m, :] + sum_h softmax_T( LN(R[m, :]) . A_h[s]^T ) . B_h[s]          (s = sample of token row m)
//
// with the step-invariant per-sample operands sd_unet_set_ip_adapter_hw folds once per call
//   A_h = (K_ip,h / sqrt(d)) . W_q,h       [T x C]      B_h = scale . V_ip,h . W_o,h^T       [T x C]
// stacked over the heads into 32 key slots (slot = head * (32 / heads) + token: head * T + token for SD-1.5's 8 heads; with fewer
// heads the slots between are zero rows of A and get probability 0).
// R' then takes the place of the residual operand of whatever form the block's text cross-attention runs in, so the block
// computes h + to_out(text) + scale . to_out(image): the reference's sum with the linear to_out distributed.
//
// One workgroup (4 waves) owns a tile of 32 token rows of ONE sample (a tile never spans two samples; tail rows are neither
// read nor written).  The tile of R sits in LDS for the whole kernel:
//   1. R tile -> LDS (16-byte loads)                                   2. mean / rstd of every row from the row itself (two passes)
//   3. scores [32 rows x 32 slots] = LN(R) . A^T on 32x32x16 MFMAs: the row is NORMALISED IN THE KERNEL -- (x - mean) rstd gamma +
//      beta in fp32, rounded to bf16 as it becomes the MFMA operand (the same operand the separate LayerNorm launch would
//      hand to to_q) -- K split over the waves, partials summed through LDS in a fixed order
//   4. fp32 softmax over the T slots of each head, probabilities rounded to bf16
//   5. P . B on MFMAs per 32-channel tile, + R in fp32, ONE bf16 rounding, written back into the LDS tile
//   6. LDS tile -> R' (16-byte stores)
// HBM traffic: one read of R and one write of R'; A / B (2 x 32 x C bf16 per sample) come from L2.  No atomics, no row
// partials of a producer: deterministic and independent of the plan around it.
#include "kernels.h"

#include <atomic>

namespace {

constexpr int IP_ROWS = 32, IP_SLOTS = 32, IP_T = 4, IP_THREADS = 256, IP_WAVES = 4;
constexpr int IP_MAX_DEVICES = 64;      // devices whose LDS opt-in is remembered (sd_launch_ip_xattn)
constexpr int SC_LD = 33;        // fp32 score rows: +1 against bank conflicts
constexpr int PS_LD = 40;        // bf16 probability rows: 80 bytes (16-byte aligned fragments)

struct IpXattnParams {
    const bf16_t* R;
    bf16_t* Y;
    const bf16_t* A;             // [samples][32][C]
    const bf16_t* Bt;            // [samples][C][32]
    const float* gamma;
    const float* beta;
    float eps;
    int C, rows_per_sample, tiles_per_sample, gstride;       // gstride = 8 / heads: every gstride-th group of T slots is a head
};

__host__ __device__ inline int ip_row_stride(int C) { return C + 8; }      // bf16 elements: rows 16 bytes apart modulo 128
inline size_t ip_smem_bytes(int C) {
    return (size_t)IP_ROWS * ip_row_stride(C) * 2 + (size_t)IP_WAVES * IP_ROWS * SC_LD * 4 + (size_t)IP_ROWS * PS_LD * 2 +
           (size_t)IP_ROWS * 2 * 4;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(IP_THREADS) void ip_xattn_kernel(const IpXattnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = p.C, ld = ip_row_stride(C);
    bf16_t* xs = (bf16_t*)smem;                                                  // [32][ld]
    float* sc = (float*)(smem + (size_t)IP_ROWS * ld * 2);                       // [4][32][SC_LD]
    bf16_t* ps = (bf16_t*)((char*)sc + (size_t)IP_WAVES * IP_ROWS * SC_LD * 4);  // [32][PS_LD]
    float* st = (float*)((char*)ps + (size_t)IP_ROWS * PS_LD * 2);               // [32][2]: mean, rstd

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sample = blockIdx.x / p.tiles_per_sample, tile = blockIdx.x % p.tiles_per_sample;
    const int nrows = min(IP_ROWS, p.rows_per_sample - tile * IP_ROWS);
    const long row0 = (long)sample * p.rows_per_sample + (long)tile * IP_ROWS;
    const int cpr = C / 8;                                                       // 16-byte chunks per row

    // 1. the tile (rows past the sample's end: zeros, never read from memory)
    for (int i = tid; i < IP_ROWS * cpr; i += IP_THREADS) {
        const int r = i / cpr, ch = i % cpr;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r < nrows) v = *(const u32x4*)(p.R + (row0 + r) * C + ch * 8);
        *(u32x4*)(xs + (size_t)r * ld + ch * 8) = v;
    }
    __syncthreads();

    // 2. row statistics: 8 rows per wave, mean first, then the centred sum of squares
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        const bf16_t* row = xs + (size_t)r * ld;
        float s = 0.f;
        for (int c = lane * 2; c < C; c += 128) {
            const unsigned u = *(const unsigned*)(row + c);
            s += bflo(u) + bfhi(u);
        }
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
        for (int c = lane * 2; c < C; c += 128) {
            const unsigned u = *(const unsigned*)(row + c);
            const float a = bflo(u) - mean, b = bfhi(u) - mean;
            q += a * a + b * b;
        }
        const float var = wave_sum(q) / (float)C;
        if (lane == 0) { st[2 * r] = mean; st[2 * r + 1] = 1.0f / sqrtf(var + p.eps); }
    }
    __syncthreads();

    // 3. scores: wave w takes the 16-channel K steps w, w + 4, ...   (lane: row / slot = lane & 31, K half = lane >> 5)
    const int lr = lane & 31, lh = lane >> 5;
    {
        const float mean = st[2 * lr], rstd = st[2 * lr + 1];
        const bf16_t* arow = p.A + ((size_t)sample * IP_SLOTS + lr) * C;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int ks = wave; ks < C / 16; ks += IP_WAVES) {
            const int k0 = ks * 16 + lh * 8;
            const u32x4 xv = *(const u32x4*)(xs + (size_t)lr * ld + k0);
            const f32x4 g0 = *(const f32x4*)(p.gamma + k0), g1 = *(const f32x4*)(p.gamma + k0 + 4);
            const f32x4 b0 = *(const f32x4*)(p.beta + k0), b1 = *(const f32x4*)(p.beta + k0 + 4);
            u32x4 nv;
            nv[0] = pack2bf((bflo(xv[0]) - mean) * rstd * g0[0] + b0[0], (bfhi(xv[0]) - mean) * rstd * g0[1] + b0[1]);
            nv[1] = pack2bf((bflo(xv[1]) - mean) * rstd * g0[2] + b0[2], (bfhi(xv[1]) - mean) * rstd * g0[3] + b0[3]);
            nv[2] = pack2bf((bflo(xv[2]) - mean) * rstd * g1[0] + b1[0], (bfhi(xv[2]) - mean) * rstd * g1[1] + b1[1]);
            nv[3] = pack2bf((bflo(xv[3]) - mean) * rstd * g1[2] + b1[2], (bfhi(xv[3]) - mean) * rstd * g1[3] + b1[3]);
            const u32x4 av = *(const u32x4*)(arow + k0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, nv), __builtin_bit_cast(bf16x8, av), acc, 0, 0, 0);
        }
        float* mine = sc + (size_t)wave * IP_ROWS * SC_LD;
#pragma unroll
        for (int i = 0; i < 16; ++i) mine[((i & 3) + 8 * (i >> 2) + 4 * lh) * SC_LD + lr] = acc[i];      // [token][slot]
    }
    __syncthreads();

    // 4. softmax over the T slots of one (token, head) per thread
    {
        const int r = tid >> 3, h = tid & 7;
        float e[IP_T];
        float m = -3.0e38f;
#pragma unroll
        for (int t = 0; t < IP_T; ++t) {
            const int o = r * SC_LD + h * IP_T + t;
            e[t] = (sc[o] + sc[IP_ROWS * SC_LD + o]) + (sc[2 * IP_ROWS * SC_LD + o] + sc[3 * IP_ROWS * SC_LD + o]);
            m = fmaxf(m, e[t]);
        }
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < IP_T; ++t) { e[t] = __builtin_amdgcn_exp2f((e[t] - m) * 1.4426950408889634f); sum += e[t]; }
        const float inv = h % p.gstride == 0 ? 1.0f / sum : 0.f;                 // (slot groups between the heads: probability 0)
        u32x2 pk = {pack2bf(e[0] * inv, e[1] * inv), pack2bf(e[2] * inv, e[3] * inv)};
        *(u32x2*)(ps + r * PS_LD + h * IP_T) = pk;
    }
    __syncthreads();

    // 5. P . B + R per 32-channel tile, written back into the LDS tile (every element has exactly one owner lane)
    {
        const bf16x8 p0 = *(const bf16x8*)(ps + lr * PS_LD + lh * 8), p1 = *(const bf16x8*)(ps + lr * PS_LD + 16 + lh * 8);
        for (int ct = wave; ct < C / 32; ct += IP_WAVES) {
            const bf16_t* brow = p.Bt + ((size_t)sample * C + ct * 32 + lr) * IP_SLOTS + lh * 8;
            const bf16x8 f0 = *(const bf16x8*)brow, f1 = *(const bf16x8*)(brow + 16);
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p0, f0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p1, f1, acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                bf16_t* q = xs + (size_t)((i & 3) + 8 * (i >> 2) + 4 * lh) * ld + ct * 32 + lr;
                *q = f2bf(acc[i] + bf2f(*q));
            }
        }
    }
    __syncthreads();

    // 6. the tile's valid rows
    for (int i = tid; i < nrows * cpr; i += IP_THREADS) {
        const int r = i / cpr, ch = i % cpr;
        *(u32x4*)(p.Y + (row0 + r) * C + ch * 8) = *(const u32x4*)(xs + (size_t)r * ld + ch * 8);
    }
}

}  // namespace

bool sd_ip_xattn_applicable(int C, int heads, int T) {
    return C >= 32 && C % 32 == 0 && C <= 2048 && T == IP_T && (heads == 1 || heads == 2 || heads == 4 || heads == 8) && C % heads == 0;
}

int sd_launch_ip_xattn(const bf16_t* R, bf16_t* Y, const bf16_t* A, const bf16_t* Bt, const float* gamma, const float* beta,
                       float eps, long M, int C, int rows_per_sample, int heads, int T, hipStream_t stream) {
    SD_REQUIRE(R && Y && A && Bt && gamma && beta, "ip_xattn: null operand");
    SD_REQUIRE(R != Y, "ip_xattn: the output must not alias the input (tiles are re-read for the residual)");
    SD_REQUIRE(sd_ip_xattn_applicable(C, heads, T),
               "ip_xattn: C=%d heads=%d T=%d (built: C a multiple of 32 up to 2048, T = 4 image tokens, 1 / 2 / 4 / 8 heads)", C, heads, T);
    SD_REQUIRE(rows_per_sample >= 1 && M >= rows_per_sample && M % rows_per_sample == 0, "ip_xattn: M=%ld rows_per_sample=%d", M,
               rows_per_sample);
    SD_REQUIRE((((uintptr_t)R | (uintptr_t)Y | (uintptr_t)A | (uintptr_t)Bt | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0,
               "ip_xattn: operands must be 16-byte aligned");
    const uintptr_t bytes = (uintptr_t)M * (uintptr_t)C * sizeof(bf16_t);
    SD_REQUIRE((uintptr_t)R + bytes <= (uintptr_t)Y || (uintptr_t)Y + bytes <= (uintptr_t)R,
               "ip_xattn: the output must not overlap the input (tiles are re-read for the residual)");
    const long samples = M / rows_per_sample;
    const int tps = (rows_per_sample + IP_ROWS - 1) / IP_ROWS;
    SD_REQUIRE(samples * tps <= 0x7fffffffl, "ip_xattn: %ld tiles", samples * tps);
    const size_t smem = ip_smem_bytes(C);
    // the opt-in to more than 64 KiB of dynamic LDS is a property of the function ON ONE DEVICE: remembered per device, and
    // set again (harmless) when two threads race to it; a device index beyond the table sets it on every launch
    static std::atomic<size_t> attr_bytes[IP_MAX_DEVICES];
    int dev = 0;
    SD_CHECK_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= IP_MAX_DEVICES || smem > attr_bytes[dev].load(std::memory_order_acquire)) {
        SD_CHECK_HIP(hipFuncSetAttribute((const void*)ip_xattn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        if (dev >= 0 && dev < IP_MAX_DEVICES) {
            size_t seen = attr_bytes[dev].load(std::memory_order_relaxed);
            while (smem > seen && !attr_bytes[dev].compare_exchange_weak(seen, smem, std::memory_order_release)) {}
        }
    }
    IpXattnParams p{R, Y, A, Bt, gamma, beta, eps, C, rows_per_sample, tps, 8 / heads};
    hipLaunchKernelGGL(ip_xattn_kernel, dim3((unsigned)(samples * tps)), dim3(IP_THREADS), smem, stream, p);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
