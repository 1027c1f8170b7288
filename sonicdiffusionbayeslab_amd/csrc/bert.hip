// BLIP text-encoder pieces of the ImageReward metric (the reference's quality_metrics.image_reward: ImageReward-v1.0 = BLIP
// ViT-L/16 + a BERT encoder whose layers cross-attend to the image tokens + a linear reward head).  The GEMMs, LayerNorm, GELU
// and the embedding gather are the shared kernels; what lives here is
//   * masked attention of a short query block (head dim 64, <= 64 queries, <= 320 keys) on matrix cores: the BERT
//     self-attention with a key-padding mask and the cross-attention over the image tokens are the same kernel;
//   * the reward head: fp32 dot product of the class-token row with the folded linear chain, then (r - mean) / std.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Attention of one (sample, head): q [B * Lq][ldq], k / v [B * Lk][ldkv] (each pointer already at its column offset; the head's
// 64 columns at h * 64) -> out [B * Lq][ldo].  4 waves, 16 query rows each; the structure is vit.hip::vit_attn_kernel's:
// K (row-major) and V (transposed) of the head in LDS with the key count padded to a multiple of 32 by zero rows, S = Q K^T on
// 16x16x32 bf16 MFMAs with all key tiles in registers, whole-row fp32 softmax, P (bf16, unnormalised) through a per-wave LDS
// image into the A operand of O = P V, 1 / row-sum (of the ROUNDED P) applied to O in fp32.
// Key mask (int32 [B][Lk], null = all valid) by SELECT: a masked key's K and V rows are staged as zeros and its score is
// replaced before the row max, so no finite or non-finite value of a padded row reaches the output.
// LDS row pitches: a 16-row fragment is read with one 16-byte read per lane (row r16, column 8 g), which the LDS serves in
// four groups of 16 lanes over 64 four-byte banks.  With a pitch of 8 (mod 16) dwords -- 16 bf16 of padding on rows of 64 or of a
// multiple of 32 -- the 16 reads of every group fall on 64 distinct banks (a pad of 8 bf16, pitch 4 mod 16 dwords, is 2-way).
constexpr int BD = 64, BMAXQ = 64, BMAXK = 320, BKT = BMAXK / 16, BKST = BD + 16, BVPAD = 16;

struct BertAttnArgs {
    const bf16_t *q, *k, *v;
    bf16_t* out;
    const int* mask;
    long ldq, ldkv, ldo;
    int Lq, Lk;
    float scale;
};

__global__ __launch_bounds__(256) void bert_attn_kernel(BertAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Lq = a.Lq, Lk = a.Lk;
    const int Lp = (Lk + 31) & ~31, VST = Lp + BVPAD;
    bf16_t* Ks = (bf16_t*)smem;                   // [Lp][BKST]
    bf16_t* Vt = Ks + Lp * BKST;                  // [BD][VST]
    bf16_t* Ps = Vt + BD * VST;                   // [4 waves][16][VST]
    const int b = blockIdx.y, h = blockIdx.x;
    const bf16_t* kb = a.k + (long)b * Lk * a.ldkv + h * BD;
    const bf16_t* vb = a.v + (long)b * Lk * a.ldkv + h * BD;
    const int* mrow = a.mask ? a.mask + (long)b * Lk : nullptr;
    for (int i = threadIdx.x; i < Lp * 8; i += blockDim.x) {
        const int j = i >> 3, c = (i & 7) * 8;
        uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
        if (j < Lk && (!mrow || mrow[j] != 0)) {
            kv = *(const uint4*)(kb + (long)j * a.ldkv + c);
            vv = *(const uint4*)(vb + (long)j * a.ldkv + c);
        }
        *(uint4*)(Ks + j * BKST + c) = kv;
        const bf16_t* ve = (const bf16_t*)&vv;
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(c + e) * VST + j] = ve[e];
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int qw = wave * 16;                     // first query row of this wave (waves past Lq compute on zero rows, store nothing)
    const int qrow = qw + r16;
    const bf16_t* qb = a.q + (long)b * Lq * a.ldq + h * BD;
    bf16x8 qa[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (qrow < Lq) qa[s] = *(const bf16x8*)(qb + (long)qrow * a.ldq + 32 * s + 8 * g);
        else qa[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    const int nkt = Lp / 16;
    f32x4 sc[BKT];
    float mx[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
#pragma unroll
    for (int kt = 0; kt < BKT; ++kt) {
        if (kt < nkt) {
            const bf16_t* kr = Ks + (kt * 16 + r16) * BKST + 8 * g;   // B[k = 8g + j][col r16] = K[key][d]
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[0], *(const bf16x8*)kr, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[1], *(const bf16x8*)(kr + 32), acc, 0, 0, 0);
            const int key = kt * 16 + r16;
            const bool ok = key < Lk && (!mrow || mrow[key] != 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = ok ? acc[r] * a.scale : -1e30f;
                sc[kt][r] = v;
                mx[r] = fmaxf(mx[r], v);
            }
        }
    }
    // lane holds S[row 4g + r][key kt * 16 + r16]: a row lives on the 16 lanes of one group
#pragma unroll
    for (int r = 0; r < 4; ++r)
        for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o));
    bf16_t* Pw = Ps + wave * 16 * VST;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < BKT; ++kt) {
        if (kt < nkt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bf16_t e = f2bf(__expf(sc[kt][r] - mx[r]));
                sum[r] += bf2f(e);                // the row sum of the P that the PV product sees
                Pw[(4 * g + r) * VST + kt * 16 + r16] = e;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        for (int o = 1; o < 16; o <<= 1) sum[r] += __shfl_xor(sum[r], o);
    __syncthreads();

    f32x4 acc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nks = Lp / 32;
#pragma unroll
    for (int ks = 0; ks < BMAXK / 32; ++ks) {
        if (ks < nks) {
            const bf16x8 pa = *(const bf16x8*)(Pw + r16 * VST + ks * 32 + 8 * g);          // A[row r16][k] = P[q][key]
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const bf16x8 vb8 = *(const bf16x8*)(Vt + (db * 16 + r16) * VST + ks * 32 + 8 * g);   // B[k][col] = V[key][d]
                acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb8, acc[db], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = qw + 4 * g + r;
        if (q >= Lq) continue;
        const float inv = 1.0f / sum[r];
        bf16_t* orow = a.out + ((long)b * Lq + q) * a.ldo + h * BD + r16;
#pragma unroll
        for (int db = 0; db < 4; ++db) orow[db * 16] = f2bf(acc[db][r] * inv);
    }
}

// rewards[b] = (w . x_b + bias - mean) / std with x_b = the class-token row hidden[b * row_stride .. + H) in fp32; features
// (optional) [B][H] = x_b.  w / wb: the folded head (fp32 [H] and one fp32 bias).
__global__ void reward_head_kernel(const bf16_t* __restrict__ hidden, long row_stride, const float* __restrict__ w,
                                   const float* __restrict__ wb, float mean, float stdv, int H, float* __restrict__ rewards,
                                   float* __restrict__ features) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const bf16_t* x = hidden + (long)b * row_stride;
    float d = 0.f;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float xv = bf2f(x[c]);
        if (features) features[(long)b * H + c] = xv;
        d += xv * w[c];
    }
    d = wave_sum(d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += red[i];
        rewards[b] = (s + wb[0] - mean) / stdv;
    }
}

}  // namespace

int sd_bert_attention_check(int B, int Lq, int Lk, int heads) {
    SD_REQUIRE(Lq >= 1 && Lq <= BMAXQ, "bert_attention: Lq=%d query rows (1..%d are built)", Lq, BMAXQ);
    SD_REQUIRE(Lk >= 1 && Lk <= BMAXK, "bert_attention: Lk=%d keys (1..%d are built)", Lk, BMAXK);
    SD_REQUIRE(B >= 1 && B <= 65535 && heads >= 1 && heads <= 65535, "bert_attention: B=%d heads=%d", B, heads);
    return 0;
}

// every sample of a host copy of the key mask has a valid key
int sd_bert_mask_check(const int* host_mask, int B, int Lk) {
    for (int b = 0; b < B; ++b) {
        bool any = false;
        for (int j = 0; j < Lk && !any; ++j) any = host_mask[(long)b * Lk + j] != 0;
        SD_REQUIRE(any, "bert_attention: sample %d has no valid key (its mask row is all zero)", b);
    }
    return 0;
}

int sd_launch_bert_attention(const bf16_t* q, long ldq, const bf16_t* k, const bf16_t* v, long ldkv, const int* mask, bf16_t* out,
                             long ldo, int B, int heads, int Lq, int Lk, hipStream_t stream) {
    SD_REQUIRE(q && k && v && out, "bert_attention: null operand");
    if (sd_bert_attention_check(B, Lq, Lk, heads)) return -1;
    SD_REQUIRE(ldq >= (long)heads * BD && ldkv >= (long)heads * BD && ldo >= (long)heads * BD && ldq % 8 == 0 && ldkv % 8 == 0,
               "bert_attention: row pitches q %ld kv %ld out %ld (head dim 64 is built: at least heads * 64, multiples of 8)", ldq,
               ldkv, ldo);
    SD_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0, "bert_attention: q, k and v must be 16-byte aligned");
    const int Lp = (Lk + 31) & ~31, VST = Lp + BVPAD;
    const size_t smem = ((size_t)Lp * BKST + (size_t)BD * VST + (size_t)4 * 16 * VST) * sizeof(bf16_t);
    SD_CHECK_HIP(hipFuncSetAttribute((const void*)bert_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    BertAttnArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out; a.mask = mask; a.ldq = ldq; a.ldkv = ldkv; a.ldo = ldo; a.Lq = Lq; a.Lk = Lk;
    a.scale = 1.0f / sqrtf((float)BD);
    hipLaunchKernelGGL(bert_attn_kernel, dim3(heads, B), dim3(256), smem, stream, a);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_reward_head(const bf16_t* hidden, long row_stride, const float* w, const float* wb, float mean, float stdv, int B,
                          int H, float* rewards, float* features, hipStream_t stream) {
    SD_REQUIRE(hidden && w && wb && rewards, "reward_head: null operand");
    SD_REQUIRE(B >= 1 && H >= 1 && row_stride >= H, "reward_head: B=%d H=%d row stride %ld", B, H, row_stride);
    SD_REQUIRE(stdv > 0.f, "reward_head: std %g must be positive", stdv);
    hipLaunchKernelGGL(reward_head_kernel, dim3(B), dim3(256), 0, stream, hidden, row_stride, w, wb, mean, stdv, H, rewards,
                       features);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
