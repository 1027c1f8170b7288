// CLIP vision tower pieces (the CLIP-score model of the reference's quality metric: CLIPModel.get_image_features) and the
// score itself.  The transformer layers run on the shared bf16 MFMA GEMM, LayerNorm and quick_gelu; what lives here is
//   * CLIPImageProcessor (PIL backend) on uint8 images: shortest edge -> image_size with PIL's bicubic, centre crop,
//     (x / 255 - mean) / std, written straight into bf16 patch rows for the patch-embedding GEMM.  PIL resamples in integer
//     arithmetic (22 fractional bits, horizontal pass into a uint8 intermediate, then vertical), so the uint8 crop is
//     reproduced bit for bit: the tap tables are computed on the host in double exactly as Pillow's precompute_coeffs /
//     normalize_coeffs_8bpc do, and both passes are folded onto the crop window;
//   * the embedding rows (class token | patch rows) + position embedding;
//   * non-causal self-attention for ViT sequences (head dim 64, L <= 320) on matrix cores;
//   * pooled-row gather (class token / EOS token) and the per-pair score 100 cos(img, txt).
#include <cmath>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPrec = 22;                         // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)

__device__ __forceinline__ int clip8(int s) {     // Pillow clip8: value >> PRECISION_BITS clamped to [0, 255]
    s >>= kPrec;
    return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// Horizontal pass over the rows the vertical taps read: img uint8 [B][3][H][W] -> tmp uint8 [B][3][R][S] (R intermediate rows
// from input row y0, S crop columns).  One thread per intermediate pixel; the tap table holds the crop columns only.
__global__ void resize_h_kernel(const unsigned char* __restrict__ img, unsigned char* __restrict__ tmp,
                                const int* __restrict__ xmin, const int* __restrict__ xcnt, const int* __restrict__ xk, int ks,
                                int H, int W, int y0, int R, int S, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % S);
    const long t = i / S;
    const int r = (int)(t % R);
    const long plane = t / R;                     // b * 3 + c
    const unsigned char* row = img + (plane * H + y0 + r) * (long)W + xmin[x];
    const int* k = xk + (long)x * ks;
    int s = 1 << (kPrec - 1);
    const int n = xcnt[x];
    for (int j = 0; j < n; ++j) s += (int)row[j] * k[j];
    tmp[i] = (unsigned char)clip8(s);
}

// Vertical pass, normalisation and patchify: one thread per element of the bf16 patch rows [B * Np][Kp] (column order of
// patch_embedding.weight: c, kh, kw; columns >= 3 P^2 are zero).  Every crop pixel is computed exactly once.  crop (optional):
// the uint8 crop [B][3][S][S].
struct PatchArgs {
    const unsigned char* tmp;
    const int *ymin, *ycnt, *yk;
    int ks, R, S, P, Kp, Np;
    long total;
    bf16_t* patches;
    unsigned char* crop;
};

__global__ void resize_v_patch_kernel(PatchArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int k = (int)(i % a.Kp);
    const long row = i / a.Kp;
    const int PP = a.P * a.P;
    if (k >= 3 * PP) { a.patches[i] = 0; return; }
    const int b = (int)(row / a.Np), p = (int)(row % a.Np), G = a.S / a.P;
    const int c = k / PP, kh = (k / a.P) % a.P, kw = k % a.P;
    const int y = (p / G) * a.P + kh, x = (p % G) * a.P + kw;
    const unsigned char* col = a.tmp + ((long)(b * 3 + c) * a.R + a.ymin[y]) * a.S + x;
    const int* kk = a.yk + (long)y * a.ks;
    int s = 1 << (kPrec - 1);
    const int n = a.ycnt[y];
    for (int j = 0; j < n; ++j) s += (int)col[(long)j * a.S] * kk[j];
    const int v = clip8(s);
    if (a.crop) a.crop[(((long)b * 3 + c) * a.S + y) * a.S + x] = (unsigned char)v;
    // OPENAI_CLIP_MEAN / OPENAI_CLIP_STD (the checkpoint's preprocessor_config; the Python side refuses others)
    const float mean = c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f);
    const float stdv = c == 0 ? 0.26862954f : (c == 1 ? 0.26130258f : 0.27577711f);
    a.patches[i] = f2bf(((float)v / 255.0f - mean) / stdv);
}

// out[b, 0, :] = class_embedding + pos[0];  out[b, 1 + p, :] = patch_rows[b * Np + p, :] + pos[1 + p]   (fp32 sum, bf16 out)
__global__ void vit_embed_kernel(const bf16_t* __restrict__ prow, const float* __restrict__ cls, const bf16_t* __restrict__ pos,
                                 bf16_t* __restrict__ out, int Np, int H) {
    const int row = blockIdx.x, L = Np + 1;       // b * L + t
    const int b = row / L, t = row % L;
    const bf16_t* pr = pos + (long)t * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        const float e = t == 0 ? cls[c] : bf2f(prow[((long)b * Np + t - 1) * H + c]);
        out[(long)row * H + c] = f2bf(e + bf2f(pr[c]));
    }
}

// Non-causal self-attention of one (image, head, 64-query tile), head dim 64, L <= 320, on the fused projection output
// qkv [B * L][3 H] (q | k | v) -> out [B * L][H].  4 waves, 16 query rows each.  K (row-major) and V (transposed) of the
// head sit in LDS with the key count padded to a multiple of 32 and the pad rows zeroed, so every MFMA reads in bounds:
//   S = Q K^T   16x16x32 bf16 MFMAs, Q fragments from global, scores of all key tiles in registers (<= 20 tiles x 4);
//   softmax     fp32, whole row at once (no online rescaling): keys >= L masked, row max / sum across the 16 lanes of a row;
//   O = P V     P (bf16, unnormalised) through a per-wave LDS image into the A operand, V^T rows as the B operand;
// the 1 / row-sum is applied to O in fp32 and only rows < L are stored.
constexpr int VD = 64, VMAXL = 320, VKT = VMAXL / 16, KST = VD + 8;

__global__ __launch_bounds__(256) void vit_attn_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int L, int H,
                                                      float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Lp = (L + 31) & ~31, VST = Lp + 8;
    bf16_t* Ks = (bf16_t*)smem;                   // [Lp][KST]
    bf16_t* Vt = Ks + Lp * KST;                   // [VD][VST]
    bf16_t* Ps = Vt + VD * VST;                   // [4 waves][16][VST]
    const int b = blockIdx.z, h = blockIdx.y;
    const long ld = 3L * H;
    const bf16_t* base = qkv + (long)b * L * ld + h * VD;
    for (int i = threadIdx.x; i < Lp * 8; i += blockDim.x) {
        const int j = i >> 3, c = (i & 7) * 8;
        uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
        if (j < L) {
            kv = *(const uint4*)(base + (long)j * ld + H + c);
            vv = *(const uint4*)(base + (long)j * ld + 2 * H + c);
        }
        *(uint4*)(Ks + j * KST + c) = kv;
        const bf16_t* ve = (const bf16_t*)&vv;
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(c + e) * VST + j] = ve[e];
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * 64 + wave * 16;   // first query row of this wave (waves past L compute on zero rows, store nothing)
    const int qrow = qw + r16;
    bf16x8 qa[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (qrow < L) qa[s] = *(const bf16x8*)(base + (long)qrow * ld + 32 * s + 8 * g);
        else qa[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    const int nkt = Lp / 16;
    f32x4 sc[VKT];
    float mx[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
#pragma unroll
    for (int kt = 0; kt < VKT; ++kt) {
        if (kt < nkt) {
            const bf16_t* kr = Ks + (kt * 16 + r16) * KST + 8 * g;   // B[k = 8g + j][col r16] = K[key][d]
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[0], *(const bf16x8*)kr, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[1], *(const bf16x8*)(kr + 32), acc, 0, 0, 0);
            const bool ok = kt * 16 + r16 < L;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = ok ? acc[r] * scale : -1e30f;
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
    for (int kt = 0; kt < VKT; ++kt) {
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
    for (int ks = 0; ks < VMAXL / 32; ++ks) {
        if (ks < nks) {
            const bf16x8 pa = *(const bf16x8*)(Pw + r16 * VST + ks * 32 + 8 * g);          // A[row r16][k] = P[q][key]
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const bf16x8 vb = *(const bf16x8*)(Vt + (db * 16 + r16) * VST + ks * 32 + 8 * g);   // B[k][col] = V[key][d]
                acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, vb, acc[db], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = qw + 4 * g + r;
        if (q >= L) continue;
        const float inv = 1.0f / sum[r];
        bf16_t* orow = out + ((long)b * L + q) * H + h * VD + r16;
#pragma unroll
        for (int db = 0; db < 4; ++db) orow[db * 16] = f2bf(acc[db][r] * inv);
    }
}

// dst[b, :] = src[b * L + pos_b, :]: pos_b = 0 without ids (class token); with ids, eos_id < 0 -> argmax(ids[b]) (first
// occurrence, torch.argmax), else the first position holding eos_id (0 when there is none, as argmax of an all-zero row)
__global__ void pool_rows_kernel(const bf16_t* __restrict__ src, const int* __restrict__ ids, int L, int H, int eos_id,
                                 bf16_t* __restrict__ dst) {
    __shared__ int spos;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int pos = 0;
        if (ids) {
            const int* row = ids + (long)b * L;
            if (eos_id < 0) {
                for (int l = 1; l < L; ++l)
                    if (row[l] > row[pos]) pos = l;
            } else {
                for (int l = L - 1; l >= 0; --l)
                    if (row[l] == eos_id) pos = l;
            }
        }
        spos = pos;
    }
    __syncthreads();
    const bf16_t* s = src + ((long)b * L + spos) * H;
    for (int c = threadIdx.x; c < H; c += blockDim.x) dst[(long)b * H + c] = s[c];
}

// per pair: raw = 100 cos(img_b, txt_b), score = max(raw, 0)
__global__ void clip_score_kernel(const float* __restrict__ img, const float* __restrict__ txt, int P, float* __restrict__ raw,
                                  float* __restrict__ score) {
    __shared__ float red[3][4];
    const int b = blockIdx.x;
    const float* x = img + (long)b * P;
    const float* y = txt + (long)b * P;
    float d = 0.f, nx = 0.f, ny = 0.f;
    for (int c = threadIdx.x; c < P; c += blockDim.x) {
        d += x[c] * y[c];
        nx += x[c] * x[c];
        ny += y[c] * y[c];
    }
    d = wave_sum(d); nx = wave_sum(nx); ny = wave_sum(ny);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = d; red[1][w] = nx; red[2][w] = ny; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, bx = 0.f, by = 0.f;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) { a += red[0][i]; bx += red[1][i]; by += red[2][i]; }
        const float v = 100.0f * a / (fmaxf(sqrtf(bx), 1e-12f) * fmaxf(sqrtf(by), 1e-12f));
        if (raw) raw[b] = v;
        if (score) score[b] = fmaxf(v, 0.f);
    }
}

double bicubic(double x) {                        // Pillow's bicubic_filter (a = -0.5)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

}  // namespace

// Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for a resize of in_size -> out_size over the whole input,
// restricted to the output positions [first, first + count).  Returns the tap stride ksize; writes, when the arrays are
// given, xmin / xcnt [count] and coeffs [count][ksize] (22 fractional bits, unused taps 0).
extern "C" int sd_clip_resize_taps(int in_size, int out_size, int first, int count, int* xmin, int* xcnt, int* coeffs) {
    SD_REQUIRE(in_size >= 1 && out_size >= 1 && first >= 0 && count >= 0 && first + count <= out_size,
               "resize_taps: in %d out %d window [%d, %d)", in_size, out_size, first, first + count);
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (!xmin || !xcnt || !coeffs) return ksize;
    std::vector<double> k(ksize);
    for (int i = 0; i < count; ++i) {
        const int xx = first + i;
        const double center = (xx + 0.5) * scale, ss = 1.0 / filterscale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        const int n = hi - lo;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            k[x] = bicubic((x + lo - center + 0.5) * ss);
            ww += k[x];
        }
        for (int x = 0; x < n; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = n; x < ksize; ++x) k[x] = 0.0;
        for (int x = 0; x < ksize; ++x)
            coeffs[(long)i * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << kPrec)) : (int)(0.5 + k[x] * (1 << kPrec));
        xmin[i] = lo;
        xcnt[i] = n;
    }
    return ksize;
}

// CLIPImageProcessor geometry: shortest edge -> S (long edge int(S * long / short)), centre crop S x S
void sd_clip_resize_geometry(int H, int W, int S, int* rh, int* rw, int* top, int* left) {
    if (W <= H) { *rw = S; *rh = (int)((double)S * H / W); }
    else { *rh = S; *rw = (int)((double)S * W / H); }
    *top = (*rh - S) / 2;
    *left = (*rw - S) / 2;
}

int sd_clip_prep_tables(int H, int W, int S, std::vector<int>& tab, ClipPrepGeom& g) {
    int rh, rw, top, left;
    sd_clip_resize_geometry(H, W, S, &rh, &rw, &top, &left);
    const int ksx = sd_clip_resize_taps(W, rw, left, S, nullptr, nullptr, nullptr);
    const int ksy = sd_clip_resize_taps(H, rh, top, S, nullptr, nullptr, nullptr);
    SD_REQUIRE(ksx > 0 && ksy > 0, "clip preprocess: taps for %dx%d", H, W);
    g.S = S; g.ksx = ksx; g.ksy = ksy;
    g.o_xmin = 0; g.o_xcnt = S; g.o_xk = 2 * S;
    g.o_ymin = g.o_xk + S * ksx; g.o_ycnt = g.o_ymin + S; g.o_yk = g.o_ycnt + S;
    tab.assign((size_t)g.o_yk + (size_t)S * ksy, 0);
    int* t = tab.data();
    if (sd_clip_resize_taps(W, rw, left, S, t + g.o_xmin, t + g.o_xcnt, t + g.o_xk) < 0) return -1;
    if (sd_clip_resize_taps(H, rh, top, S, t + g.o_ymin, t + g.o_ycnt, t + g.o_yk) < 0) return -1;
    // rows of the input the vertical taps of the crop read; the intermediate holds exactly those
    int* ymin = t + g.o_ymin;
    const int* ycnt = t + g.o_ycnt;
    g.y0 = ymin[0];
    int y1 = 0;
    for (int i = 0; i < S; ++i) y1 = std::max(y1, ymin[i] + ycnt[i]);
    for (int i = 0; i < S; ++i) ymin[i] -= g.y0;
    g.R = y1 - g.y0;
    g.H = H; g.W = W;
    return 0;
}

int sd_launch_clip_preprocess(const unsigned char* img, int B, const ClipPrepGeom& g, const int* dtab, unsigned char* tmp,
                              bf16_t* patches, int P, int Kp, unsigned char* crop, hipStream_t stream) {
    SD_REQUIRE(img && dtab && tmp && patches && B > 0, "clip_preprocess: null operand");
    SD_REQUIRE(P > 0 && g.S % P == 0 && Kp >= 3 * P * P && Kp % 64 == 0, "clip_preprocess: crop %d patch %d Kp %d", g.S, P, Kp);
    const long th = (long)B * 3 * g.R * g.S;
    hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)((th + 255) / 256)), dim3(256), 0, stream, img, tmp, dtab + g.o_xmin,
                       dtab + g.o_xcnt, dtab + g.o_xk, g.ksx, g.H, g.W, g.y0, g.R, g.S, th);
    SD_CHECK_HIP(hipGetLastError());
    PatchArgs a;
    a.tmp = tmp; a.ymin = dtab + g.o_ymin; a.ycnt = dtab + g.o_ycnt; a.yk = dtab + g.o_yk; a.ks = g.ksy; a.R = g.R; a.S = g.S;
    a.P = P; a.Kp = Kp; a.Np = (g.S / P) * (g.S / P); a.total = (long)B * a.Np * Kp; a.patches = patches; a.crop = crop;
    hipLaunchKernelGGL(resize_v_patch_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, stream, a);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_vit_embed(const bf16_t* prow, const float* cls, const bf16_t* pos, bf16_t* out, int B, int Np, int H,
                        hipStream_t stream) {
    SD_REQUIRE(prow && cls && pos && out && B > 0 && Np > 0 && H > 0, "vit_embed: bad operands");
    hipLaunchKernelGGL(vit_embed_kernel, dim3((unsigned)(B * (Np + 1))), dim3(256), 0, stream, prow, cls, pos, out, Np, H);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_vit_attention(const bf16_t* qkv, bf16_t* out, int B, int L, int H, int heads, hipStream_t stream) {
    SD_REQUIRE(qkv && out, "vit_attention: null operand");
    SD_REQUIRE(heads > 0 && H % heads == 0 && H / heads == VD, "vit_attention: H=%d heads=%d (head dim 64 is built)", H, heads);
    SD_REQUIRE(L >= 1 && L <= VMAXL, "vit_attention: %d tokens (1..%d are built)", L, VMAXL);
    SD_REQUIRE(B >= 1 && B <= 65535 && heads <= 65535, "vit_attention: B=%d heads=%d", B, heads);
    SD_REQUIRE(((uintptr_t)qkv & 15) == 0, "vit_attention: qkv must be 16-byte aligned");
    const int Lp = (L + 31) & ~31, VST = Lp + 8;
    const size_t smem = ((size_t)Lp * KST + (size_t)VD * VST + (size_t)4 * 16 * VST) * sizeof(bf16_t);
    SD_CHECK_HIP(hipFuncSetAttribute((const void*)vit_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(vit_attn_kernel, dim3((L + 63) / 64, heads, B), dim3(256), smem, stream, qkv, out, L, H,
                       1.0f / sqrtf((float)VD));
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_pool_rows(const bf16_t* src, const int* ids, int B, int L, int H, int eos_id, bf16_t* dst, hipStream_t stream) {
    SD_REQUIRE(src && dst && B > 0 && L > 0 && H > 0, "pool_rows: bad operands");
    hipLaunchKernelGGL(pool_rows_kernel, dim3(B), dim3(256), 0, stream, src, ids, L, H, eos_id, dst);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_clip_score(const float* img, const float* txt, int B, int P, float* raw, float* score, hipStream_t stream) {
    SD_REQUIRE(img && txt && B > 0 && P > 0 && (raw || score), "clip_score: bad operands");
    hipLaunchKernelGGL(clip_score_kernel, dim3(B), dim3(256), 0, stream, img, txt, P, raw, score);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
