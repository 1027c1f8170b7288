// FID Inception-v3 ("pt_inception-2015-12-05", the network torch-fidelity's FeatureExtractorInceptionV3 wraps and
// torchmetrics' FrechetInceptionDistance scores with; reference src/metrics/metrics.py:98-112) and the FID statistics.
//   * TF1 legacy bilinear resize of uint8 images to 299 x 299 (no half-pixel offset) + (x - 128) / 128, NHWC;
//   * ONE implicit-GEMM conv kernel for every conv of the network: NHWC bf16, any kh x kw / stride / padding, any Cin and
//     Cout (tails in the kernel), contraction kh kw Cin on 16x16x32 bf16 MFMAs with fp32 accumulation, folded-BatchNorm bias
//     + ReLU in the epilogue, output row pitch + channel offset so that every branch of a Mixed block writes its slice of the
//     concatenated output (no concat pass);
//   * 3x3 max pooling (stride 2 pad 0, stride 1 pad 1), 3x3 average pooling that divides by the in-bounds tap count
//     (count_include_pad=False), global spatial mean to fp32;
//   * sd_fid_accumulate: the fp64 running sum / outer-product sum / count torchmetrics keeps as FID state;
//   * the handle: the layer table, BatchNorm-folded weights (bf16 OHWI) and the forward to one of the four taps.
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "../../include/sd_hip.h"

namespace {

// ---- implicit-GEMM conv ------------------------------------------------------------------------------------------------
// C[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]), act = none / relu / (relu = 2) SiLU;  m = (b, oy, ox), k = (ky, kx, ci), A gathered from the NHWC input (zero
// outside the image and past K).  Workgroup: 64 rows x 64 columns, 4 waves of 32 x 32 (2 x 2 MFMA tiles), K in steps of 32.
// Each thread stages one 8-element k-chunk of one A row and of one W row per step: global -> registers (issued before the
// step's MFMAs) -> the other half of a double-buffered LDS image; one barrier per step.  LDS rows are padded to 40 elements
// (80 bytes: 16-byte aligned fragment reads, rows 20 banks apart).
// VEC: Cin % 8 == 0 and 16-byte aligned operands, so a chunk is one 16-byte load inside one tap.  Otherwise element loads.
constexpr int BM = 64, BN = 64, BK = 32, LDSK = BK + 8;

struct ConvArgs {
    const bf16_t* x;
    const bf16_t* w;
    const float* bias;
    bf16_t* y;
    int Hin, Win, Cin, Hout, Wout, Cout, kh, kw, stride, ph, pw, K, ldy, coff, relu;
    long M;
};

template <bool VEC>
__global__ __launch_bounds__(256) void inception_conv_kernel(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t As[2][BM * LDSK];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[2][BN * LDSK];
    const int tid = threadIdx.x, lrow = tid >> 2, lch = (tid & 3) * 8;
    const long m = (long)blockIdx.x * BM + lrow;
    const int n = blockIdx.y * BN + lrow;
    const bool mval = m < a.M, nval = n < a.Cout;
    int iy0 = 0, ix0 = 0;
    const bf16_t* xb = a.x;
    if (mval) {
        const int ox = (int)(m % a.Wout);
        const long t = m / a.Wout;
        const int oy = (int)(t % a.Hout);
        xb += (t / a.Hout) * (long)a.Hin * a.Win * a.Cin;
        iy0 = oy * a.stride - a.ph;
        ix0 = ox * a.stride - a.pw;
    }
    const bf16_t* wr = a.w + (long)n * a.K;

    auto load_a = [&](int k0) -> u32x4 {
        u32x4 r = {0u, 0u, 0u, 0u};
        const int k = k0 + lch;
        if (!mval || k >= a.K) return r;
        int tap = k / a.Cin, ci = k - tap * a.Cin;
        if (VEC) {
            const int ky = tap / a.kw, kx = tap - ky * a.kw, iy = iy0 + ky, ix = ix0 + kx;
            if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) r = *(const u32x4*)(xb + ((long)iy * a.Win + ix) * a.Cin + ci);
            return r;
        }
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            e[j] = 0;
            if (k + j < a.K) {
                const int ky = tap / a.kw, kx = tap - ky * a.kw, iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) e[j] = xb[((long)iy * a.Win + ix) * a.Cin + ci];
            }
            if (++ci == a.Cin) { ci = 0; ++tap; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (unsigned)e[2 * j] | ((unsigned)e[2 * j + 1] << 16);
        return r;
    };
    auto load_b = [&](int k0) -> u32x4 {
        u32x4 r = {0u, 0u, 0u, 0u};
        const int k = k0 + lch;
        if (!nval || k >= a.K) return r;
        if (VEC) return *(const u32x4*)(wr + k);
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = k + j < a.K ? wr[k + j] : (unsigned short)0;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = (unsigned)e[2 * j] | ((unsigned)e[2 * j + 1] << 16);
        return r;
    };

    const int wave = tid >> 6, lane = tid & 63, r16 = lane & 15, g = lane >> 4;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (a.K + BK - 1) / BK;
    u32x4 ra = load_a(0), rb = load_b(0);
    *(u32x4*)(As[0] + lrow * LDSK + lch) = ra;
    *(u32x4*)(Bs[0] + lrow * LDSK + lch) = rb;
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int cur = ks & 1;
        const bool more = ks + 1 < nk;
        if (more) { ra = load_a((ks + 1) * BK); rb = load_b((ks + 1) * BK); }
        bf16x8 af[2], bfr[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = *(const bf16x8*)(As[cur] + (wm + i * 16 + r16) * LDSK + 8 * g);   // A[row r16][k = 8g + j]
#pragma unroll
        for (int j = 0; j < 2; ++j) bfr[j] = *(const bf16x8*)(Bs[cur] + (wn + j * 16 + r16) * LDSK + 8 * g);  // B[k = 8g + j][col r16]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        if (more) {
            *(u32x4*)(As[cur ^ 1] + lrow * LDSK + lch) = ra;
            *(u32x4*)(Bs[cur ^ 1] + lrow * LDSK + lch) = rb;
        }
        __syncthreads();
    }

    // accumulator: lane holds C[row 4g + r][col r16] of each 16 x 16 tile
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = blockIdx.y * BN + wn + j * 16 + r16;
        if (col >= a.Cout) continue;
        const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = (long)blockIdx.x * BM + wm + i * 16 + 4 * g + r;
                if (row >= a.M) continue;
                float v = acc[i][j][r] + bv;
                if (a.relu == 1) v = fmaxf(v, 0.f);
                else if (a.relu == 2) v = silu_f(v);
                a.y[row * a.ldy + a.coff + col] = f2bf(v);
            }
    }
}

// ---- pooling -----------------------------------------------------------------------------------------------------------
// 3x3 window, one thread per (output pixel, group of V channels); taps outside the image are skipped.  AVG divides the fp32
// sum by the number of in-bounds taps; max is exact.  V = 8: 16-byte loads / stores (C, ldy, coff multiples of 8).
struct PoolArgs {
    const bf16_t* x;
    bf16_t* y;
    int H, W, C, Hout, Wout, stride, pad, ldy, coff;
    long total;           // B * Hout * Wout * (C / V)
};

template <int V, bool AVG>
__global__ void inception_pool_kernel(PoolArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int CG = a.C / V;
    const int c = (int)(i % CG) * V;
    const long p = i / CG;
    const int ox = (int)(p % a.Wout);
    const long t = p / a.Wout;
    const int oy = (int)(t % a.Hout);
    const bf16_t* xb = a.x + (t / a.Hout) * (long)a.H * a.W * a.C;
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = AVG ? 0.f : -INFINITY;
    int cnt = 0;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * a.stride - a.pad + ky;
        if (iy < 0 || iy >= a.H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * a.stride - a.pad + kx;
            if (ix < 0 || ix >= a.W) continue;
            ++cnt;
            const bf16_t* s = xb + ((long)iy * a.W + ix) * a.C + c;
            if (V == 8) {
                const u32x4 q = *(const u32x4*)s;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float lo = bflo(q[e]), hi = bfhi(q[e]);
                    v[2 * e] = AVG ? v[2 * e] + lo : fmaxf(v[2 * e], lo);
                    v[2 * e + 1] = AVG ? v[2 * e + 1] + hi : fmaxf(v[2 * e + 1], hi);
                }
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) v[e] = AVG ? v[e] + bf2f(s[e]) : fmaxf(v[e], bf2f(s[e]));
            }
        }
    }
    if (AVG) {
        const float d = (float)cnt;
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = v[e] / d;
    }
    bf16_t* o = a.y + p * a.ldy + a.coff + c;
    if (V == 8) {
        *(u32x4*)o = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = f2bf(v[e]);
    }
}

// out[b][c] = mean over the HW pixels of x[b][p][c] in fp32: 64 channels x 4 pixel groups per workgroup, the four partial
// sums added in a fixed order
__global__ __launch_bounds__(256) void inception_mean_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, int HW, int C) {
    __shared__ float part[4][64];
    const int b = blockIdx.y, cl = threadIdx.x & 63, grp = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    float s = 0.f;
    if (c < C) {
        const bf16_t* xb = x + (long)b * HW * C + c;
        for (int p = grp; p < HW; p += 4) s += bf2f(xb[(long)p * C]);
    }
    part[grp][cl] = s;
    __syncthreads();
    if (grp == 0 && c < C) out[(long)b * C + c] = (((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl]) / (float)HW;
}

// ---- preprocessing -----------------------------------------------------------------------------------------------------
// uint8 [B][3][H][W] -> [B][S][S][3] (bf16, or fp32 for the parity test): TensorFlow-1 legacy bilinear (src = dst * (in / out),
// no half-pixel offset), lerp along x then along y, then (v - 128) / 128.  Contraction is off: the arithmetic is the sequence
// of fp32 roundings the specification names, not a fused variant of it.
__global__ void inception_resize_kernel(const unsigned char* __restrict__ img, void* __restrict__ out, int H, int W, int S,
                                        int out_fp32, long total) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % S);
    const long t = i / S;
    const int y = (int)(t % S);
    const long b = t / S;
    const float sy = (float)H / (float)S, sx = (float)W / (float)S;
    const float fy = (float)y * sy, fx = (float)x * sx;
    int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
    y0 = y0 > H - 1 ? H - 1 : y0;
    x0 = x0 > W - 1 ? W - 1 : x0;
    const int y1 = y0 + 1 > H - 1 ? H - 1 : y0 + 1, x1 = x0 + 1 > W - 1 ? W - 1 : x0 + 1;
    const float dy = fy - (float)y0, dx = fx - (float)x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned char* pl = img + (b * 3 + c) * (long)H * W;
        const float a00 = (float)pl[(long)y0 * W + x0], a01 = (float)pl[(long)y0 * W + x1];
        const float a10 = (float)pl[(long)y1 * W + x0], a11 = (float)pl[(long)y1 * W + x1];
        const float top = a00 + (a01 - a00) * dx, bot = a10 + (a11 - a10) * dx;
        const float v = ((top + (bot - top) * dy) - 128.0f) / 128.0f;
        if (out_fp32) ((float*)out)[i * 3 + c] = v;
        else ((bf16_t*)out)[i * 3 + c] = f2bf(v);
    }
}

// ---- FID statistics ----------------------------------------------------------------------------------------------------
// sum[j] += sum_b f[b][j];  cov[i][j] += sum_b f[b][i] f[b][j];  count += B -- fp64 state from fp32 features (the product of
// two fp32 values is exact in fp64).  One thread per (i, j); row 0 of the grid also owns the sums, thread (0, 0) the count.
__global__ void fid_accumulate_kernel(const float* __restrict__ f, int B, int D, double* __restrict__ sum,
                                      double* __restrict__ cov, long long* __restrict__ count) {
    const int j = blockIdx.x * 16 + threadIdx.x, i = blockIdx.y * 16 + threadIdx.y;
    if (i >= D || j >= D) return;
    double acc = 0.0, s = 0.0;
    for (int b = 0; b < B; ++b) {
        const double fj = (double)f[(long)b * D + j];
        acc += (double)f[(long)b * D + i] * fj;
        s += fj;
    }
    cov[(long)i * D + j] += acc;
    if (i == 0) sum[j] += s;
    if (i == 0 && j == 0) *count += B;
}

bf16_t host_f2bf(float f) {                      // round to nearest even (weights are finite)
    unsigned u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------

int sd_launch_inception_conv(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, int B, int Hin, int Win, int Cin,
                             int Cout, int kh, int kw, int stride, int ph, int pw, int ldy, int coff, int relu,
                             hipStream_t stream) {
    SD_REQUIRE(x && w && y, "inception_conv: null operand");
    SD_REQUIRE(B > 0 && Hin > 0 && Win > 0 && Cin > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && ph >= 0 && pw >= 0,
               "inception_conv: bad shape B=%d %dx%dx%d -> %d, kernel %dx%d stride %d pad (%d, %d)", B, Hin, Win, Cin, Cout, kh, kw,
               stride, ph, pw);
    SD_REQUIRE(Hin + 2 * ph >= kh && Win + 2 * pw >= kw, "inception_conv: kernel %dx%d larger than the padded %dx%d input", kh, kw,
               Hin, Win);
    SD_REQUIRE(coff >= 0 && ldy >= coff + Cout, "inception_conv: output pitch %d < offset %d + %d channels", ldy, coff, Cout);
    SD_REQUIRE((long)kh * kw * Cin < (1L << 30), "inception_conv: contraction too long");
    ConvArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.Cout = Cout; a.kh = kh; a.kw = kw; a.stride = stride; a.ph = ph; a.pw = pw;
    a.Hout = (Hin + 2 * ph - kh) / stride + 1;
    a.Wout = (Win + 2 * pw - kw) / stride + 1;
    a.K = kh * kw * Cin; a.ldy = ldy; a.coff = coff; a.relu = relu;
    a.M = (long)B * a.Hout * a.Wout;
    const long gx = (a.M + BM - 1) / BM;
    const int gy = (Cout + BN - 1) / BN;
    SD_REQUIRE(gx < (1L << 31) && gy <= 65535, "inception_conv: grid %ld x %d", gx, gy);
    const dim3 grid((unsigned)gx, (unsigned)gy);
    if (Cin % 8 == 0 && aligned16(x) && aligned16(w))
        hipLaunchKernelGGL(inception_conv_kernel<true>, grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(inception_conv_kernel<false>, grid, dim3(256), 0, stream, a);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_inception_pool(const bf16_t* x, bf16_t* y, int B, int H, int W, int C, int stride, int pad, int avg, int ldy,
                             int coff, hipStream_t stream) {
    SD_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0, "inception_pool: bad operands");
    SD_REQUIRE((stride == 1 || stride == 2) && (pad == 0 || pad == 1) && H + 2 * pad >= 3 && W + 2 * pad >= 3,
               "inception_pool: 3x3 window, stride %d pad %d on %dx%d", stride, pad, H, W);
    SD_REQUIRE(coff >= 0 && ldy >= coff + C, "inception_pool: output pitch %d < offset %d + %d channels", ldy, coff, C);
    PoolArgs a;
    a.x = x; a.y = y; a.H = H; a.W = W; a.C = C; a.stride = stride; a.pad = pad; a.ldy = ldy; a.coff = coff;
    a.Hout = (H + 2 * pad - 3) / stride + 1;
    a.Wout = (W + 2 * pad - 3) / stride + 1;
    const bool vec = C % 8 == 0 && ldy % 8 == 0 && coff % 8 == 0 && aligned16(x) && aligned16(y);
    a.total = (long)B * a.Hout * a.Wout * (vec ? C / 8 : C);
    const dim3 grid((unsigned)((a.total + 255) / 256));
    if (vec && avg) hipLaunchKernelGGL((inception_pool_kernel<8, true>), grid, dim3(256), 0, stream, a);
    else if (vec) hipLaunchKernelGGL((inception_pool_kernel<8, false>), grid, dim3(256), 0, stream, a);
    else if (avg) hipLaunchKernelGGL((inception_pool_kernel<1, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((inception_pool_kernel<1, false>), grid, dim3(256), 0, stream, a);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_inception_mean(const bf16_t* x, float* out, int B, int HW, int C, hipStream_t stream) {
    SD_REQUIRE(x && out && B > 0 && B <= 65535 && HW > 0 && C > 0, "inception_mean: bad operands");
    hipLaunchKernelGGL(inception_mean_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)B), dim3(256), 0, stream, x, out, HW, C);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_inception_resize(const unsigned char* img, void* out, int B, int H, int W, int S, int out_fp32, hipStream_t stream) {
    SD_REQUIRE(img && out && B > 0 && H >= 1 && W >= 1 && S >= 1, "inception_resize: bad operands");
    const long total = (long)B * S * S;
    hipLaunchKernelGGL(inception_resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, img, out, H, W, S,
                       out_fp32, total);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the handle --------------------------------------------------------------------------------------------------------

struct InceptionConv {
    int cin = 0, cout = 0, kh = 0, kw = 0;
    std::vector<bf16_t> w;            // host staging: [cout][kh][kw][cin]
    std::vector<float> b;
    size_t w_off = 0, b_off = 0;      // byte offsets in the device blob
    bool loaded = false;
};

struct sd_inception {
    std::map<std::string, InceptionConv> convs;
    std::vector<std::string> order;   // forward order
    char* blob = nullptr;             // device: every weight and bias
    bool finalized = false;
};

namespace {

constexpr int kSide = 299;
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Ten {                          // NHWC bf16 activation, rows of exactly C channels
    int buf = 0;                      // 0 / 1: the two block-level buffers, 2: scratch of the current block
    size_t off = 0;
    int H = 0, W = 0, C = 0;
};

// One description of the network serves three passes: DECLARE registers every conv's name and shape (sd_inception_create),
// PLAN sizes the workspace (two ping-pong buffers for block inputs / outputs, a scratch stack for a block's intermediates),
// EXEC enqueues the launches.
struct Runner {
    enum Mode { DECLARE, PLAN, EXEC };
    sd_inception* h;
    Mode mode;
    int B = 1;
    hipStream_t stream = nullptr;
    char* ws = nullptr;
    size_t main_bytes = 0, tmp_top = 0, tmp_max = 0;      // PLAN results (EXEC: main_bytes given)
    int rc = 0;

    size_t bytes(int H, int W, int C) const { return up256((size_t)B * H * W * C * sizeof(bf16_t)); }
    Ten main_buf(int which, int H, int W, int C) {
        Ten t; t.buf = which; t.H = H; t.W = W; t.C = C;
        if (mode == PLAN) main_bytes = std::max(main_bytes, bytes(H, W, C));
        return t;
    }
    Ten tmp(int H, int W, int C) {
        Ten t; t.buf = 2; t.off = tmp_top; t.H = H; t.W = W; t.C = C;
        tmp_top += bytes(H, W, C);
        tmp_max = std::max(tmp_max, tmp_top);
        return t;
    }
    bf16_t* ptr(const Ten& t) const {
        return (bf16_t*)(ws + (t.buf == 2 ? 2 * main_bytes + t.off : (size_t)t.buf * main_bytes));
    }

    // conv + folded BatchNorm + ReLU into channels [coff, coff + cout) of `out`
    void conv(const std::string& name, const Ten& in, int cout, int kh, int kw, int stride, int ph, int pw, const Ten& out, int coff) {
        if (rc) return;
        if (mode == DECLARE) {
            InceptionConv c; c.cin = in.C; c.cout = cout; c.kh = kh; c.kw = kw;
            h->convs[name] = c;
            h->order.push_back(name);
            return;
        }
        if (mode == PLAN) return;
        const InceptionConv& c = h->convs.at(name);
        rc = sd_launch_inception_conv(ptr(in), (const bf16_t*)(h->blob + c.w_off), (const float*)(h->blob + c.b_off), ptr(out), B, in.H,
                                      in.W, in.C, cout, kh, kw, stride, ph, pw, out.C, coff, 1, stream);
    }
    Ten conv_tmp(const std::string& name, const Ten& in, int cout, int kh = 1, int kw = 1, int stride = 1, int ph = 0, int pw = 0) {
        Ten o = tmp((in.H + 2 * ph - kh) / stride + 1, (in.W + 2 * pw - kw) / stride + 1, cout);
        conv(name, in, cout, kh, kw, stride, ph, pw, o, 0);
        return o;
    }
    void pool(const Ten& in, int stride, int pad, int avg, const Ten& out, int coff) {
        if (rc || mode != EXEC) return;
        rc = sd_launch_inception_pool(ptr(in), ptr(out), B, in.H, in.W, in.C, stride, pad, avg, out.C, coff, stream);
    }
    Ten pool_tmp(const Ten& in, int avg) {
        Ten o = tmp(in.H, in.W, in.C);
        pool(in, 1, 1, avg, o, 0);
        return o;
    }
    void mean(const Ten& in, float* out) {
        if (rc || mode != EXEC) return;
        rc = sd_launch_inception_mean(ptr(in), out, B, in.H * in.W, in.C, stream);
    }

    Ten block_a(const std::string& p, const Ten& in, int pf) {
        Ten out = main_buf(1 - in.buf, in.H, in.W, 64 + 64 + 96 + pf);
        tmp_top = 0;
        conv(p + "branch1x1", in, 64, 1, 1, 1, 0, 0, out, 0);
        Ten t = conv_tmp(p + "branch5x5_1", in, 48);
        conv(p + "branch5x5_2", t, 64, 5, 5, 1, 2, 2, out, 64);
        t = conv_tmp(p + "branch3x3dbl_1", in, 64);
        t = conv_tmp(p + "branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1);
        conv(p + "branch3x3dbl_3", t, 96, 3, 3, 1, 1, 1, out, 128);
        conv(p + "branch_pool", pool_tmp(in, 1), pf, 1, 1, 1, 0, 0, out, 224);
        return out;
    }
    Ten block_b(const std::string& p, const Ten& in) {
        const int Ho = (in.H - 3) / 2 + 1, Wo = (in.W - 3) / 2 + 1;
        Ten out = main_buf(1 - in.buf, Ho, Wo, 384 + 96 + in.C);
        tmp_top = 0;
        conv(p + "branch3x3", in, 384, 3, 3, 2, 0, 0, out, 0);
        Ten t = conv_tmp(p + "branch3x3dbl_1", in, 64);
        t = conv_tmp(p + "branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1);
        conv(p + "branch3x3dbl_3", t, 96, 3, 3, 2, 0, 0, out, 384);
        pool(in, 2, 0, 0, out, 480);
        return out;
    }
    Ten block_c(const std::string& p, const Ten& in, int c7) {
        Ten out = main_buf(1 - in.buf, in.H, in.W, 768);
        tmp_top = 0;
        conv(p + "branch1x1", in, 192, 1, 1, 1, 0, 0, out, 0);
        Ten t = conv_tmp(p + "branch7x7_1", in, c7);
        t = conv_tmp(p + "branch7x7_2", t, c7, 1, 7, 1, 0, 3);
        conv(p + "branch7x7_3", t, 192, 7, 1, 1, 3, 0, out, 192);
        t = conv_tmp(p + "branch7x7dbl_1", in, c7);
        t = conv_tmp(p + "branch7x7dbl_2", t, c7, 7, 1, 1, 3, 0);
        t = conv_tmp(p + "branch7x7dbl_3", t, c7, 1, 7, 1, 0, 3);
        t = conv_tmp(p + "branch7x7dbl_4", t, c7, 7, 1, 1, 3, 0);
        conv(p + "branch7x7dbl_5", t, 192, 1, 7, 1, 0, 3, out, 384);
        conv(p + "branch_pool", pool_tmp(in, 1), 192, 1, 1, 1, 0, 0, out, 576);
        return out;
    }
    Ten block_d(const std::string& p, const Ten& in) {
        const int Ho = (in.H - 3) / 2 + 1, Wo = (in.W - 3) / 2 + 1;
        Ten out = main_buf(1 - in.buf, Ho, Wo, 320 + 192 + in.C);
        tmp_top = 0;
        Ten t = conv_tmp(p + "branch3x3_1", in, 192);
        conv(p + "branch3x3_2", t, 320, 3, 3, 2, 0, 0, out, 0);
        t = conv_tmp(p + "branch7x7x3_1", in, 192);
        t = conv_tmp(p + "branch7x7x3_2", t, 192, 1, 7, 1, 0, 3);
        t = conv_tmp(p + "branch7x7x3_3", t, 192, 7, 1, 1, 3, 0);
        conv(p + "branch7x7x3_4", t, 192, 3, 3, 2, 0, 0, out, 320);
        pool(in, 2, 0, 0, out, 512);
        return out;
    }
    Ten block_e(const std::string& p, const Ten& in, int max_pool) {
        Ten out = main_buf(1 - in.buf, in.H, in.W, 2048);
        tmp_top = 0;
        conv(p + "branch1x1", in, 320, 1, 1, 1, 0, 0, out, 0);
        Ten t = conv_tmp(p + "branch3x3_1", in, 384);
        conv(p + "branch3x3_2a", t, 384, 1, 3, 1, 0, 1, out, 320);
        conv(p + "branch3x3_2b", t, 384, 3, 1, 1, 1, 0, out, 704);
        t = conv_tmp(p + "branch3x3dbl_1", in, 448);
        t = conv_tmp(p + "branch3x3dbl_2", t, 384, 3, 3, 1, 1, 1);
        conv(p + "branch3x3dbl_3a", t, 384, 1, 3, 1, 0, 1, out, 1088);
        conv(p + "branch3x3dbl_3b", t, 384, 3, 1, 1, 1, 0, out, 1472);
        conv(p + "branch_pool", pool_tmp(in, max_pool ? 0 : 1), 192, 1, 1, 1, 0, 0, out, 1856);
        return out;
    }

    // the forward up to `tap` (64 | 192 | 768 | 2048); DECLARE walks everything
    void run(int tap, const unsigned char* images, int H, int W, float* features) {
        Ten x = main_buf(0, kSide, kSide, 3);
        if (mode == EXEC) rc = sd_launch_inception_resize(images, ptr(x), B, H, W, kSide, 0, stream);
        Ten a = main_buf(1, 149, 149, 32);
        conv("Conv2d_1a_3x3", x, 32, 3, 3, 2, 0, 0, a, 0);
        Ten b = main_buf(0, 147, 147, 32);
        conv("Conv2d_2a_3x3", a, 32, 3, 3, 1, 0, 0, b, 0);
        Ten c = main_buf(1, 147, 147, 64);
        conv("Conv2d_2b_3x3", b, 64, 3, 3, 1, 1, 1, c, 0);
        Ten d = main_buf(0, 73, 73, 64);
        pool(c, 2, 0, 0, d, 0);
        if (tap == 64) { mean(d, features); return; }
        Ten e = main_buf(1, 73, 73, 80);
        conv("Conv2d_3b_1x1", d, 80, 1, 1, 1, 0, 0, e, 0);
        Ten f = main_buf(0, 71, 71, 192);
        conv("Conv2d_4a_3x3", e, 192, 3, 3, 1, 0, 0, f, 0);
        Ten t = main_buf(1, 35, 35, 192);
        pool(f, 2, 0, 0, t, 0);
        if (tap == 192) { mean(t, features); return; }
        t = block_a("Mixed_5b.", t, 32);
        t = block_a("Mixed_5c.", t, 64);
        t = block_a("Mixed_5d.", t, 64);
        t = block_b("Mixed_6a.", t);
        t = block_c("Mixed_6b.", t, 128);
        t = block_c("Mixed_6c.", t, 160);
        t = block_c("Mixed_6d.", t, 160);
        t = block_c("Mixed_6e.", t, 192);
        if (tap == 768) { mean(t, features); return; }
        t = block_d("Mixed_7a.", t);
        t = block_e("Mixed_7b.", t, 0);
        t = block_e("Mixed_7c.", t, 1);
        mean(t, features);
    }
};

bool tap_ok(int tap) { return tap == 64 || tap == 192 || tap == 768 || tap == 2048; }

}  // namespace

extern "C" int sd_inception_create(sd_inception** out) {
    SD_REQUIRE(out, "sd_inception_create: null argument");
    sd_inception* h = new sd_inception();
    Runner r{h, Runner::DECLARE};
    r.run(2048, nullptr, kSide, kSide, nullptr);
    *out = h;
    return 0;
}

extern "C" void sd_inception_destroy(sd_inception* h) {
    if (!h) return;
    if (h->blob) (void)hipFree(h->blob);
    delete h;
}

extern "C" int sd_inception_num_convs(const sd_inception* h) { return h ? (int)h->order.size() : -1; }

extern "C" int sd_inception_conv_info(const sd_inception* h, int index, char* name, int name_cap, long long shape[4]) {
    SD_REQUIRE(h && name && shape && index >= 0 && index < (int)h->order.size(), "inception_conv_info: bad index %d", index);
    const std::string& n = h->order[index];
    SD_REQUIRE((int)n.size() < name_cap, "inception_conv_info: name buffer too small");
    memcpy(name, n.c_str(), n.size() + 1);
    const InceptionConv& c = h->convs.at(n);
    shape[0] = c.cout; shape[1] = c.cin; shape[2] = c.kh; shape[3] = c.kw;
    return 0;
}

extern "C" int sd_inception_load_conv(sd_inception* h, const char* name, const float* weight_oihw, long long weight_numel,
                                      const float* bias, int cout) {
    SD_REQUIRE(h && name && weight_oihw && bias, "inception_load_conv: null argument");
    SD_REQUIRE(!h->finalized, "inception_load_conv: the handle is finalized");
    auto it = h->convs.find(name);
    SD_REQUIRE(it != h->convs.end(), "inception_load_conv: no conv named %s", name);
    InceptionConv& c = it->second;
    SD_REQUIRE(cout == c.cout && weight_numel == (long long)c.cout * c.cin * c.kh * c.kw,
               "inception_load_conv: %s expects [%d, %d, %d, %d], got %lld weights / %d biases", name, c.cout, c.cin, c.kh, c.kw,
               weight_numel, cout);
    const int taps = c.kh * c.kw;
    c.w.resize((size_t)weight_numel);
    for (int o = 0; o < c.cout; ++o)
        for (int i = 0; i < c.cin; ++i)
            for (int t = 0; t < taps; ++t)
                c.w[((size_t)o * taps + t) * c.cin + i] = host_f2bf(weight_oihw[((size_t)o * c.cin + i) * taps + t]);
    c.b.assign(bias, bias + cout);
    c.loaded = true;
    return 0;
}

extern "C" int sd_inception_finalize(sd_inception* h) {
    SD_REQUIRE(h, "inception_finalize: null handle");
    SD_REQUIRE(!h->finalized, "inception_finalize: already finalized");
    size_t total = 0;
    for (const std::string& n : h->order) {
        InceptionConv& c = h->convs.at(n);
        SD_REQUIRE(c.loaded, "inception_finalize: %s was never loaded", n.c_str());
        c.w_off = total; total += up256(c.w.size() * sizeof(bf16_t));
        c.b_off = total; total += up256(c.b.size() * sizeof(float));
    }
    std::vector<char> host(total, 0);
    for (const std::string& n : h->order) {
        const InceptionConv& c = h->convs.at(n);
        memcpy(host.data() + c.w_off, c.w.data(), c.w.size() * sizeof(bf16_t));
        memcpy(host.data() + c.b_off, c.b.data(), c.b.size() * sizeof(float));
    }
    SD_CHECK_HIP(hipMalloc((void**)&h->blob, total));
    SD_CHECK_HIP(hipMemcpy(h->blob, host.data(), total, hipMemcpyHostToDevice));
    for (const std::string& n : h->order) {
        InceptionConv& c = h->convs.at(n);
        std::vector<bf16_t>().swap(c.w);
        std::vector<float>().swap(c.b);
    }
    h->finalized = true;
    return 0;
}

extern "C" long long sd_inception_workspace_bytes(sd_inception* h, int batch, int tap) {
    SD_REQUIRE(h && batch > 0 && batch <= 65535, "inception_workspace_bytes: batch %d", batch);
    SD_REQUIRE(tap_ok(tap), "inception: tap %d (64, 192, 768 or 2048)", tap);
    Runner r{h, Runner::PLAN};
    r.B = batch;
    r.run(tap, nullptr, kSide, kSide, nullptr);
    return (long long)(2 * r.main_bytes + r.tmp_max);
}

extern "C" int sd_inception_features(sd_inception* h, void* stream, const unsigned char* images, int batch, int height, int width,
                                     int tap, float* features, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(h && h->finalized, "inception_features: the handle is not finalized");
    SD_REQUIRE(images && features && workspace && batch > 0 && batch <= 65535, "inception_features: null argument or batch %d", batch);
    SD_REQUIRE(height >= 1 && width >= 1 && (long long)height * width < (1LL << 31), "inception_features: image %dx%d", height, width);
    SD_REQUIRE(tap_ok(tap), "inception: tap %d (64, 192, 768 or 2048)", tap);
    SD_REQUIRE(((uintptr_t)workspace & 255) == 0, "inception_features: workspace must be 256-byte aligned");
    Runner p{h, Runner::PLAN};
    p.B = batch;
    p.run(tap, nullptr, kSide, kSide, nullptr);
    const long long need = (long long)(2 * p.main_bytes + p.tmp_max);
    SD_REQUIRE(need <= workspace_bytes, "inception_features: workspace too small (%lld < %lld)", workspace_bytes, need);
    Runner r{h, Runner::EXEC};
    r.B = batch; r.stream = (hipStream_t)stream; r.ws = (char*)workspace; r.main_bytes = p.main_bytes;
    r.run(tap, images, height, width, features);
    return r.rc;
}

extern "C" int sd_fid_accumulate(void* stream, const float* features, int batch, int dim, double* sum, double* cov_sum,
                                 long long* count) {
    SD_REQUIRE(features && sum && cov_sum && count && batch > 0 && dim > 0 && dim <= 16 * 65535, "fid_accumulate: bad operands");
    const unsigned g = (unsigned)((dim + 15) / 16);
    hipLaunchKernelGGL(fid_accumulate_kernel, dim3(g, g), dim3(16, 16), 0, (hipStream_t)stream, features, batch, dim, sum, cov_sum,
                       count);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- operator-level entry points ---------------------------------------------------------------------------------------

extern "C" int sd_op_inception_conv(void* stream, const void* X, const void* W, const float* bias, void* Y, int B, int Hin, int Win,
                                    int Cin, int Cout, int kh, int kw, int stride, int pad_h, int pad_w, int ldy, int coff, int relu) {
    return sd_launch_inception_conv((const bf16_t*)X, (const bf16_t*)W, bias, (bf16_t*)Y, B, Hin, Win, Cin, Cout, kh, kw, stride, pad_h,
                                    pad_w, ldy, coff, relu, (hipStream_t)stream);
}

extern "C" int sd_op_maxpool3x3(void* stream, const void* X, void* Y, int B, int H, int W, int C, int stride, int pad, int ldy, int coff) {
    return sd_launch_inception_pool((const bf16_t*)X, (bf16_t*)Y, B, H, W, C, stride, pad, 0, ldy, coff, (hipStream_t)stream);
}

extern "C" int sd_op_avgpool3x3(void* stream, const void* X, void* Y, int B, int H, int W, int C, int ldy, int coff) {
    return sd_launch_inception_pool((const bf16_t*)X, (bf16_t*)Y, B, H, W, C, 1, 1, 1, ldy, coff, (hipStream_t)stream);
}

extern "C" int sd_op_global_mean(void* stream, const void* X, float* out, int B, int HW, int C) {
    return sd_launch_inception_mean((const bf16_t*)X, out, B, HW, C, (hipStream_t)stream);
}

extern "C" int sd_op_inception_resize(void* stream, const unsigned char* images, int B, int H, int W, void* out, int out_fp32) {
    return sd_launch_inception_resize(images, out, B, H, W, kSide, out_fp32, (hipStream_t)stream);
}
