// libsdhip host side: the operator-level entry points of the C ABI (sd_op_*): single launches and the launch pairs the plan
// fuses, for parity tests, micro-benchmarks and tools.
#include "model.h"

#include <stdlib.h>

namespace sdhip {

// grow-only device scratch for the operator-level entry points (tests / micro-benchmarks only;
// the UNet plan carries its own slabs inside the caller's workspace)
static void* g_scratch = nullptr;
static size_t g_scratch_bytes = 0;
void* op_scratch(size_t bytes) {
    if (bytes > g_scratch_bytes) {
        (void)hipDeviceSynchronize();
        if (g_scratch) (void)hipFree(g_scratch);
        g_scratch = nullptr;
        g_scratch_bytes = 0;
        if (hipMalloc(&g_scratch, bytes) != hipSuccess) return nullptr;
        g_scratch_bytes = bytes;
    }
    return g_scratch;
}

}  // namespace sdhip

using namespace sdhip;

// GemmArgs of a 3x3 conv (padding 1; `up`: nearest-2x upsample first) on NHWC X [B, Hin, Win, Cin] -> Y [B, Hout, Wout, Cout]
static void conv3x3_args(GemmArgs& a, const void* X, const void* W, const float* bias, const float* bias2, const void* R, void* Y,
                         int B, int Hin, int Win, int Cin, int Cout, int stride, int up) {
    a.X = (const bf16_t*)X; a.W = (const bf16_t*)W; a.bias = bias; a.bias2 = bias2; a.R = (const bf16_t*)R; a.ldr = Cout;
    a.C = (bf16_t*)Y; a.ldc = Cout;
    a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.stride = stride; a.up = up;
    a.Hout = ((Hin << up) + 2 - 3) / stride + 1; a.Wout = ((Win << up) + 2 - 3) / stride + 1;
    a.M = B * a.Hout * a.Wout; a.N = Cout; a.K = 9 * Cin; a.K1 = a.K; a.zero_page = zero_page();
}

// ... of the sub-pixel form of upsample + conv: four 2x2 convs on the low-res input (GemmArgs::subpix), no split-K
static void conv3x3_subpixel_args(GemmArgs& a, const void* X, const void* W4, const float* bias, void* Y, int B, int Hin, int Win,
                                  int Cin, int Cout) {
    a.X = (const bf16_t*)X; a.W = (const bf16_t*)W4; a.bias = bias; a.C = (bf16_t*)Y; a.ldc = Cout;
    a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.stride = 1; a.up = 0; a.Hout = 2 * Hin; a.Wout = 2 * Win;
    a.M = 4 * B * Hin * Win; a.N = Cout; a.K = 4 * Cin; a.K1 = a.K; a.zero_page = zero_page(); a.splitk = 1;
    a.subpix = 1; a.w_batch_stride = (long)Cout * 4 * Cin;
}

// split-K > 1: the partial slabs come from op_scratch
static int splitk_slab(GemmArgs& a, const char* who) {
    if (a.splitk > 1) {
        a.slab = (float*)op_scratch((size_t)a.splitk * a.M * a.N * 4);
        SD_REQUIRE(a.slab, "%s: cannot allocate split-K scratch", who);
    }
    return 0;
}

// GroupNorm(+SiLU) of a conv's output Y [B * HW][Cout] -> Yn; stats1 = the block statistics of the conv's epilogue (null: the
// GroupNorm runs its own statistics pass)
static GroupNormArgs groupnorm_after_conv(const void* Y, int Cout, const float* gamma, const float* beta, void* Yn, int B, int HW,
                                          int groups, float eps, int silu, float* partial, const float* stats1) {
    GroupNormArgs g;
    g.x1 = (const bf16_t*)Y; g.C1 = Cout; g.gamma = gamma; g.beta = beta; g.y = (bf16_t*)Yn; g.B = B; g.HW = HW;
    g.groups = groups; g.eps = eps; g.silu = silu; g.nsplit = sd_groupnorm_nsplit(B, HW);
    g.partial = partial;
    g.stats1 = stats1;
    return g;
}

static XattnArgs xattn_args(const void* X, const void* R, void* Y, const void* At, const void* Bw, const float* bias, int M, int C,
                            int rows_per_sample, int L) {
    XattnArgs a;
    a.X = (const bf16_t*)X; a.R = (const bf16_t*)R; a.Y = (bf16_t*)Y; a.At = (const bf16_t*)At; a.Bw = (const bf16_t*)Bw;
    a.bias = bias; a.M = M; a.C = C; a.rows_per_sample = rows_per_sample; a.L = L;
    return a;
}

// Split factor of the plain-epilogue GEMM entry points: dtype 0 = sd_op_gemm (bf16), 1 = sd_op_gemm_fp8 (K in e4m3 elements:
// the heuristic counts 128-byte K tiles, and the fp8 kernel has the 128-row tile only)
static int op_gemm_splitk(int M, int N, int K, int dtype) {
    return dtype ? sd_gemm_splitk(M, N, K / 2, 128) : sd_gemm_splitk(M, N, K);
}

// Which variant sd_op_gemm / sd_op_gemm_fp8 run a plain-epilogue problem on (the tests assert the one they mean to hit)
extern "C" int sd_op_gemm_tile_rows(int M, int N, int K) {
    SD_REQUIRE(M > 0 && N > 0 && K >= 0, "gemm_tile_rows: bad arguments");
    return sd_gemm_tile_rows(M, N, K);
}
extern "C" int sd_op_gemm_splitk(int M, int N, int K, int dtype) {
    SD_REQUIRE(M > 0 && N > 0 && K > 0 && (dtype == 0 || dtype == 1), "gemm_splitk: bad arguments");
    return op_gemm_splitk(M, N, K, dtype);
}

extern "C" int sd_op_gemm(void* stream, const void* X, long long ldx, const void* X2, long long ldx2, int K1,
                          const void* W, const float* bias, const float* bias2, const void* R, long long ldr, void* C,
                          long long ldc, int M, int N, int K, int epi) {
    if (ensure_zero_page()) return -2;
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.X2 = (const bf16_t*)X2; a.ldx2 = ldx2; a.K1 = K1;
    a.W = (const bf16_t*)W; a.bias = bias; a.bias2 = bias2; a.R = (const bf16_t*)R; a.ldr = ldr;
    a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.zero_page = zero_page();
    a.splitk = epi ? 1 : op_gemm_splitk(M, N, K, 0);
    if (splitk_slab(a, "sd_op_gemm")) return -1;
    return sd_launch_gemm(a, epi, (hipStream_t)stream);
}

extern "C" int sd_op_gemm_batched(void* stream, const void* X, long long ldx, const void* W, long long w_batch_stride,
                                  int rows_per_batch, const float* bias, const void* R, long long ldr, void* C,
                                  long long ldc, int M, int N, int K, int epi, int sm_valid) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(epi == 0 || epi == 2, "sd_op_gemm_batched: epi %d (0 = std, 2 = softmax over 80-column groups)", epi);
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.K1 = K; a.W = (const bf16_t*)W; a.bias = bias; a.R = (const bf16_t*)R; a.ldr = ldr;
    a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.zero_page = zero_page();
    a.w_batch_stride = w_batch_stride; a.rows_per_batch = rows_per_batch; a.sm_valid = sm_valid; a.splitk = 1;
    return sd_launch_gemm(a, epi, (hipStream_t)stream);
}

// the softmax-epilogue GEMM over per-sample weights with a LayerNorm folded in: X = the un-normalised rows, W = per-sample
// [N][K] operands scaled by gamma (centred or not), c1 / c2 = per-sample [N] vectors (row sums of the rounded W, beta term),
// rowstats [parts][M][2]: P = softmax_80col( rstd_m * (X W^T - mean_m c1) + c2 )
extern "C" int sd_op_gemm_batched_softmax_ln(void* stream, const void* X, long long ldx, const void* W, long long w_batch_stride,
                                             int rows_per_batch, void* C, long long ldc, int M, int N, int K, int sm_valid,
                                             const float* rowstats, int parts, const float* c1, const float* c2, float eps) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(rowstats && c1 && c2, "sd_op_gemm_batched_softmax_ln: null operand");
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.K1 = K; a.W = (const bf16_t*)W; a.bias = c2;
    a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.zero_page = zero_page();
    a.w_batch_stride = w_batch_stride; a.rows_per_batch = rows_per_batch; a.sm_valid = sm_valid; a.splitk = 1;
    a.ln_rs = rowstats; a.ln_np = parts; a.ln_c1 = c1; a.ln_eps = eps; a.ln_per_sample = 1;
    return sd_launch_gemm(a, 2, (hipStream_t)stream);
}

extern "C" int sd_op_conv3x3(void* stream, const void* X, const void* W, const float* bias, const float* bias2,
                             const void* R, void* Y, int B, int Hin, int Win, int Cin, int Cout, int stride, int upsample) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(stride == 1 || stride == 2, "conv3x3: stride %d", stride);
    GemmArgs a;
    conv3x3_args(a, X, W, bias, bias2, R, Y, B, Hin, Win, Cin, Cout, stride, upsample ? 1 : 0);
    a.splitk = sd_conv3x3_splitk(a.M, a.N, Cin, Hin, Win, stride, a.up);
    if (splitk_slab(a, "sd_op_conv3x3")) return -1;
    return sd_launch_conv3x3(a, (hipStream_t)stream);
}

// The 64 -> 64 channel conv with LDS-resident weights (conv64.hip): X [B, Hin, Win, 64] bf16 NHWC, Wpacked = sd_op_conv64_pack's
// output, bias [64] fp32 or null, R [B, Hout, Wout, 64] or null (added before the ReLU) -> Y [B, Hout, Wout, 64];
// mode 0: pad 1, 1: nearest-2x upsample first (Hout = 2 Hin), 2: stride 2, pad 1 on all sides (Hout = (Hin - 1) / 2 + 1)
extern "C" int sd_op_conv64(void* stream, const void* X, const void* Wpacked, const float* bias, const void* R, void* Y, int B,
                            int Hin, int Win, int mode, int relu) {
    Conv64Args a;
    a.X = (const bf16_t*)X; a.Wp = (const bf16_t*)Wpacked; a.bias = bias; a.R = (const bf16_t*)R; a.Y = (bf16_t*)Y;
    a.B = B; a.Hin = Hin; a.Win = Win; a.mode = mode; a.relu = relu ? 1 : 0;
    return sd_launch_conv64(a, (hipStream_t)stream);
}

// host: OIHW fp32 [64][64][3][3] -> the 73,728 bytes sd_op_conv64 reads (returns that size; out null: the size only)
extern "C" long long sd_op_conv64_pack(const float* w_oihw, void* out) {
    if (out) {
        SD_REQUIRE(w_oihw, "conv64_pack: null weights");
        sd_conv64_pack(w_oihw, (bf16_t*)out);
    }
    return SD_CONV64_PACKED_BYTES;
}

// The tiny autoencoder's entry (fp32 NCHW [B, Cin, H, W] -> bf16 NHWC [B, H, W, 64]; Wt [Cin * 9][64] fp32; decoder: Cin = 4,
// tanh(x / 3) * 3 in the load and a ReLU; encoder: Cin = 3, neither) and exit (bf16 NHWC -> fp32 NCHW [B, Cout, H, W]; Wp
// [Cout][9][64] bf16; out_mode 0: y * 2 - 1, 1: clamp(y, 0, 1), 2: y) kernels
extern "C" int sd_op_taesd_entry(void* stream, const float* x, const float* Wt, const float* bias, void* y, int B, int H, int W,
                                 int Cin, int decoder) {
    return sd_launch_taesd_entry(x, Wt, bias, (bf16_t*)y, B, H, W, Cin, decoder, (hipStream_t)stream);
}
extern "C" int sd_op_taesd_exit(void* stream, const void* x, const void* Wp, const float* bias, float* y, int B, int H, int W,
                                int Cout, int out_mode) {
    return sd_launch_taesd_exit((const bf16_t*)x, (const bf16_t*)Wp, bias, y, B, H, W, Cout, out_mode, (hipStream_t)stream);
}

// A resnet's conv2 with its 1x1 shortcut folded in, as the plan runs the pair (conv_halo.hip SC):
//   Y = conv3x3(X, W) + [Xs1 | Xs2] . Wsc^T + bias,  X = [B, H, W, Cin], Xs1 / Xs2 = [B, H, W, Cs1 / Cs2] (Xs2 null when Cs2 =
//   0), Wsc = [Cout, Cs1 + Cs2], bias = the sum of the two biases.  Cin is independent of Cout (small sizes reach split-K).
// Returns the library's error code where sd_conv_halo_shortcut_applicable says no.
static int conv3x3_shortcut_args(GemmArgs& a, const void* X, const void* W, const float* bias, const void* Xs1, int Cs1,
                                 const void* Xs2, int Cs2, const void* Wsc, void* Y, int B, int H, int Wd, int Cin, int Cout) {
    SD_REQUIRE(X && W && Xs1 && Wsc && Y && B > 0 && H > 0 && Wd > 0 && Cin > 0 && Cout > 0 && Cs1 > 0 && Cs2 >= 0 && (Xs2 || Cs2 == 0),
               "conv3x3_shortcut: bad arguments");
    conv3x3_args(a, X, W, bias, nullptr, nullptr, Y, B, H, Wd, Cin, Cout, 1, 0);
    a.Xs1 = (const bf16_t*)Xs1; a.Csc1 = Cs1; a.Xs2 = (const bf16_t*)Xs2; a.Csc2 = Cs2; a.Wsc = (const bf16_t*)Wsc; a.ldwsc = Cs1 + Cs2;
    SD_REQUIRE(Cin % 64 == 0 && sd_conv_halo_shortcut_applicable(a),
               "conv3x3_shortcut: %dx%d, %d -> %d channels with a %d + %d channel shortcut is not a shape the halo kernel folds", H, Wd,
               Cin, Cout, Cs1, Cs2);
    return 0;
}

extern "C" int sd_op_conv3x3_shortcut(void* stream, const void* X, const void* W, const float* bias, const void* Xs1, int Cs1,
                                      const void* Xs2, int Cs2, const void* Wsc, void* Y, int B, int H, int Wd, int Cin, int Cout) {
    if (ensure_zero_page()) return -2;
    GemmArgs a;
    if (int rc = conv3x3_shortcut_args(a, X, W, bias, Xs1, Cs1, Xs2, Cs2, Wsc, Y, B, H, Wd, Cin, Cout)) return rc;
    a.splitk = sd_conv3x3_splitk(a.M, a.N, Cin, H, Wd, 1, 0);
    if (splitk_slab(a, "sd_op_conv3x3_shortcut")) return -1;
    return sd_launch_conv3x3(a, (hipStream_t)stream);
}

// The same launch feeding a GroupNorm(+SiLU) from its epilogue's block statistics (large images: H * W a multiple of 64 and
// not the single-launch GroupNorm's): Y = the conv output, Yn = the normalised output.
extern "C" int sd_op_conv3x3_shortcut_groupnorm(void* stream, const void* X, const void* W, const float* bias, const void* Xs1,
                                                int Cs1, const void* Xs2, int Cs2, const void* Wsc, void* Y, int B, int H, int Wd,
                                                int Cin, int Cout, const float* gamma, const float* beta, void* Yn, int groups,
                                                float eps, int silu) {
    if (ensure_zero_page()) return -2;
    const int HW = H * Wd;
    SD_REQUIRE(HW % 64 == 0 && !sd_groupnorm_uses_small(B, HW, Cout, 0, groups),
               "sd_op_conv3x3_shortcut_groupnorm: %dx%d pixels per sample: producer statistics come in 64-pixel blocks", H, Wd);
    GemmArgs a;
    if (int rc = conv3x3_shortcut_args(a, X, W, bias, Xs1, Cs1, Xs2, Cs2, Wsc, Y, B, H, Wd, Cin, Cout)) return rc;
    const size_t stats_bytes = (size_t)B * (HW / 64) * Cout * 2 * 4;
    char* scratch = (char*)op_scratch(stats_bytes + sd_groupnorm_scratch_bytes(B, HW, groups));
    SD_REQUIRE(scratch, "sd_op_conv3x3_shortcut_groupnorm: cannot allocate scratch");
    a.splitk = 1;
    a.stats = (float*)scratch;
    SD_REQUIRE(sd_conv_halo_mode(a) == 1, "sd_op_conv3x3_shortcut_groupnorm: the geometry mode delivers no block statistics");
    if (int rc = sd_launch_conv3x3(a, (hipStream_t)stream)) return rc;
    return sd_launch_groupnorm(groupnorm_after_conv(Y, Cout, gamma, beta, Yn, B, HW, groups, eps, silu, (float*)(scratch + stats_bytes),
                                                    (const float*)scratch), (hipStream_t)stream);
}

// 3x3 stride-2 conv padded on the right and bottom only (GemmArgs::asym; the AutoencoderKL encoder's downsampler): W packed as
// for sd_op_conv3x3, Hin and Win even, Y = [B, Hin / 2, Win / 2, Cout]
extern "C" int sd_op_conv3x3_down_asym(void* stream, const void* X, const void* W, const float* bias, void* Y, int B, int Hin,
                                       int Win, int Cin, int Cout) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(X && W && Y && B > 0 && Hin > 0 && Win > 0 && Hin % 2 == 0 && Win % 2 == 0,
               "conv3x3_down_asym: even input sides (%dx%d)", Hin, Win);
    GemmArgs a;
    conv3x3_args(a, X, W, bias, nullptr, nullptr, Y, B, Hin, Win, Cin, Cout, 2, 0);      // (even sides: Hout = Hin / 2 either way)
    a.asym = 1;
    a.splitk = sd_conv3x3_splitk(a.M, a.N, Cin, Hin, Win, 2, 0);
    if (splitk_slab(a, "sd_op_conv3x3_down_asym")) return -1;
    return sd_launch_conv3x3(a, (hipStream_t)stream);
}

// Which kernel sd_launch_conv3x3 runs a 3x3 conv of this shape on (the plan and the op entry points use the same predicates).
extern "C" int sd_op_conv3x3_kernel(int M, int N, int Cin, int Hin, int Win, int stride, int upsample, int dtype) {
    SD_REQUIRE(M > 0 && N > 0 && Cin > 0 && Hin > 0 && Win > 0 && (stride == 1 || stride == 2) && upsample >= 0 && upsample <= 2 &&
                   (dtype == 0 || dtype == 1), "conv3x3_kernel: bad arguments");
    GemmArgs a;
    a.M = M; a.N = N; a.Cin = Cin; a.Hin = Hin; a.Win = Win; a.stride = stride; a.dt = dtype;
    if (upsample == 2) {            // the sub-pixel form: four 2x2 convs on the low-res input, M = 4 B Hin Win
        a.subpix = 1; a.up = 0; a.K = 4 * Cin; a.ldw = a.K; a.Hout = 2 * Hin; a.Wout = 2 * Win;
        a.w_batch_stride = (long)N * a.K; a.splitk = 1;
        return sd_conv_halo_subpix_applicable(a) ? 2 : 0;
    }
    a.up = upsample; a.K = 9 * Cin; a.ldw = a.K;
    a.Hout = ((Hin << a.up) + 2 - 3) / stride + 1; a.Wout = ((Win << a.up) + 2 - 3) / stride + 1;
    return sd_conv_halo_mode(a) != 0 ? 1 : 0;       // (either geometry of the halo kernel)
}

// In-place row softmax of bf16 S [rows, cols] with scale, as the VAE mid-block attention runs it (<= 4096 columns: one wave
// per row; beyond: the long-row kernel)
extern "C" int sd_op_softmax_rows(void* stream, void* S, long long rows, int cols, float scale) {
    if (cols > 4096) return sd_launch_softmax_rows_long((bf16_t*)S, rows, cols, scale, (hipStream_t)stream);
    return sd_launch_softmax_rows((bf16_t*)S, rows, cols, scale, (hipStream_t)stream);
}

// Timing ablations of the halo conv kernel (csrc/conv_halo.hip, template parameter DIAG; WRONG results by design, Y is
// scratch): ablate = 1 no LDS-DMA waits, 2 no LDS-DMA at all, 4 no tap barrier either, 8 no fragment reads either = the bare
// MFMA stream of the kernel's own tile -- the rate the matrix pipe sustains at the clock the chip holds under that load,
// which bench.py reports next to the nominal peak.  Stride-1 shapes the halo kernel takes, no split-K.
extern "C" int sd_op_conv3x3_ablate(void* stream, const void* X, const void* W, void* Y, int B, int Hin, int Win, int Cin, int Cout,
                                    int ablate) {
    if (ensure_zero_page()) return -2;
    const int abl = ablate & ~256;               // bit 8: the 4-wave layout (128 x 80 per wave; modes 0 and 8 only)
    SD_REQUIRE(abl == 0 || abl == 8 || (!(ablate & 256) && (abl == 1 || abl == 2 || abl == 4)), "conv3x3_ablate: mode %d", ablate);
    GemmArgs a;
    conv3x3_args(a, X, W, nullptr, nullptr, nullptr, Y, B, Hin, Win, Cin, Cout, 1, 0);
    a.splitk = 1; a.tune = ablate;
    SD_REQUIRE(Cin % 64 == 0 && Cout % 4 == 0 && sd_conv_halo_applicable(a), "conv3x3_ablate: not a halo-kernel shape");
    return sd_launch_conv3x3_halo(a, (hipStream_t)stream);
}

// nearest-2x upsample + 3x3 conv computed as four 2x2 convs on the low-res input (GemmArgs::subpix); W4 =
// [4 phases][Cout][Cin/64][4 taps][64] with the 3x3 taps that read the same low-res pixel summed (Packer::conv3_subpixel)
extern "C" int sd_op_conv3x3_upsample_subpixel(void* stream, const void* X, const void* W4, const float* bias, void* Y, int B,
                                               int Hin, int Win, int Cin, int Cout) {
    if (ensure_zero_page()) return -2;
    GemmArgs a;
    conv3x3_subpixel_args(a, X, W4, bias, Y, B, Hin, Win, Cin, Cout);
    return sd_launch_conv3x3(a, (hipStream_t)stream);
}

// ... -> GroupNorm(+SiLU) as the plan runs the pair (the up-blocks' Upsample2D feeds the next resnet's norm1): the conv's
// epilogue delivers the block statistics in the row order (sample, phase, low-res pixel).  Y = conv output [B, 2 Hin, 2 Win,
// Cout], Yn = normalised output.  Low-res pixels per sample must be a multiple of 128.
extern "C" int sd_op_conv3x3_upsample_subpixel_groupnorm(void* stream, const void* X, const void* W4, const float* bias, void* Y,
                                                         int B, int Hin, int Win, int Cin, int Cout, const float* gamma,
                                                         const float* beta, void* Yn, int groups, float eps, int silu) {
    if (ensure_zero_page()) return -2;
    const int HW = 4 * Hin * Win;
    SD_REQUIRE((Hin * Win) % 128 == 0 && !sd_groupnorm_uses_small(B, HW, Cout, 0, groups),
               "sd_op_conv3x3_upsample_subpixel_groupnorm: %dx%d -> x2, %d channels: no producer statistics at this size", Hin, Win, Cout);
    const size_t stats_bytes = (size_t)B * (HW / 64) * Cout * 2 * 4;
    char* scratch = (char*)op_scratch(stats_bytes + sd_groupnorm_scratch_bytes(B, HW, groups));
    SD_REQUIRE(scratch, "sd_op_conv3x3_upsample_subpixel_groupnorm: cannot allocate scratch");
    GemmArgs a;
    conv3x3_subpixel_args(a, X, W4, bias, Y, B, Hin, Win, Cin, Cout);
    a.stats = (float*)scratch;
    if (int rc = sd_launch_conv3x3(a, (hipStream_t)stream)) return rc;
    return sd_launch_groupnorm(groupnorm_after_conv(Y, Cout, gamma, beta, Yn, B, HW, groups, eps, silu, (float*)(scratch + stats_bytes),
                                                    (const float*)scratch), (hipStream_t)stream);
}

extern "C" int sd_op_groupnorm(void* stream, const void* x1, int C1, const void* x2, int C2, const float* gamma,
                               const float* beta, void* y, int B, int HW, int groups, float eps, int silu) {
    GroupNormArgs a;
    a.x1 = (const bf16_t*)x1; a.C1 = C1; a.x2 = (const bf16_t*)x2; a.C2 = C2; a.gamma = gamma; a.beta = beta;
    a.y = (bf16_t*)y; a.B = B; a.HW = HW; a.groups = groups; a.eps = eps; a.silu = silu;
    a.nsplit = sd_groupnorm_nsplit(B, HW);
    a.partial = (float*)op_scratch(sd_groupnorm_scratch_bytes(B, HW, groups));
    SD_REQUIRE(a.partial, "sd_op_groupnorm: cannot allocate scratch");
    return sd_launch_groupnorm(a, (hipStream_t)stream);
}

// conv3x3 -> GroupNorm(+SiLU) as the plan runs the pair: the conv's epilogue delivers the per-64-row-block channel
// statistics, the GroupNorm skips its own statistics pass.  Y = conv output, Yn = normalised output.
extern "C" int sd_op_conv3x3_groupnorm(void* stream, const void* X, const void* W, const float* bias, const float* bias2,
                                       const void* R, void* Y, int B, int Hin, int Win, int Cin, int Cout,
                                       const float* gamma, const float* beta, void* Yn, int groups, float eps, int silu) {
    if (ensure_zero_page()) return -2;
    const int HW = Hin * Win;
    if (sd_groupnorm_uses_small(B, HW, Cout, 0, groups)) {
        // small images: the single-launch GroupNorm (no producer statistics); a split-K conv leaves its partial slabs to it
        // (GemmArgs::defer_reduce, plan.hip::fuse_deferred_reduce) instead of launching splitk_reduce_kernel
        GemmArgs a;
        conv3x3_args(a, X, W, bias, bias2, R, Y, B, Hin, Win, Cin, Cout, 1, 0);
        a.splitk = sd_conv3x3_splitk(a.M, a.N, Cin, Hin, Win, 1, 0);
        const size_t slab_bytes = a.splitk > 1 ? (size_t)a.splitk * a.M * a.N * 4 : 0;
        char* scratch = (char*)op_scratch(slab_bytes + sd_groupnorm_scratch_bytes(B, HW, groups));
        SD_REQUIRE(scratch, "sd_op_conv3x3_groupnorm: cannot allocate scratch");
        const bool slab_off = getenv("SD_GN_SLAB") && atoi(getenv("SD_GN_SLAB")) == 0;     // per call: the test compares both
        if (a.splitk > 1) { a.slab = (float*)scratch; a.defer_reduce = (slab_off || !sd_groupnorm_slab_ok(B, HW, Cout, 0, groups)) ? 0 : 1; }
        if (int rc = sd_launch_conv3x3(a, (hipStream_t)stream)) return rc;
        GroupNormArgs g = groupnorm_after_conv(Y, Cout, gamma, beta, Yn, B, HW, groups, eps, silu, (float*)(scratch + slab_bytes), nullptr);
        if (a.defer_reduce) {
            g.slab = a.slab; g.splitk = a.splitk; g.sbias = bias; g.sbias2 = bias2; g.sR = (const bf16_t*)R; g.sldr = Cout;
            g.x1w = (bf16_t*)Y;
        }
        return sd_launch_groupnorm(g, (hipStream_t)stream);
    }
    SD_REQUIRE(HW % 64 == 0, "sd_op_conv3x3_groupnorm: %dx%d pixels per sample: producer statistics come in 64-pixel blocks", Hin, Win);
    const size_t stats_bytes = (size_t)B * (HW / 64) * Cout * 2 * 4;
    char* scratch = (char*)op_scratch(stats_bytes + sd_groupnorm_scratch_bytes(B, HW, groups));
    SD_REQUIRE(scratch, "sd_op_conv3x3_groupnorm: cannot allocate scratch");
    GemmArgs a;
    conv3x3_args(a, X, W, bias, bias2, R, Y, B, Hin, Win, Cin, Cout, 1, 0);
    a.splitk = 1;
    a.stats = (float*)scratch;
    if (int rc = sd_launch_conv3x3(a, (hipStream_t)stream)) return rc;
    return sd_launch_groupnorm(groupnorm_after_conv(Y, Cout, gamma, beta, Yn, B, HW, groups, eps, silu, (float*)(scratch + stats_bytes),
                                                    (const float*)scratch), (hipStream_t)stream);
}

extern "C" int sd_op_conv3x3_splitk(int M, int Cout, int Cin, int Hin, int Win, int stride, int upsample) {
    return sd_conv3x3_splitk(M, Cout, Cin, Hin, Win, stride, upsample ? 1 : 0);
}

extern "C" int sd_op_layernorm(void* stream, const void* x, const float* gamma, const float* beta, void* y, int rows,
                               int C, float eps) {
    return sd_launch_layernorm((const bf16_t*)x, gamma, beta, (bf16_t*)y, rows, C, eps, (hipStream_t)stream);
}

extern "C" int sd_op_attention(void* stream, const void* Q, long long ldq, const void* K, long long ldk, const void* V,
                               long long ldv, void* O, long long ldo, int B, int heads, int Nq, int Nk, int D, float scale) {
    AttnArgs a;
    a.Q = (const bf16_t*)Q; a.ldq = ldq; a.K = (const bf16_t*)K; a.ldk = ldk; a.V = (const bf16_t*)V; a.ldv = ldv;
    a.O = (bf16_t*)O; a.ldo = ldo; a.B = B; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.D = D; a.scale = scale;
    if (ensure_zero_page()) return -2;
    a.consts = zero_page();
    return sd_launch_attention(a, (hipStream_t)stream);
}

// the CLIP text tower's causal self-attention on the fused projection output qkv [B * L][3 H] (q | k | v) -> out [B * L][H]
extern "C" int sd_op_clip_attention(void* stream, const void* qkv, void* out, int B, int L, int H, int heads) {
    return sd_launch_clip_attention((const bf16_t*)qkv, (bf16_t*)out, B, L, H, heads, (hipStream_t)stream);
}

extern "C" int sd_op_vit_attention(void* stream, const void* qkv, void* out, int B, int L, int H, int heads) {
    return sd_launch_vit_attention((const bf16_t*)qkv, (bf16_t*)out, B, L, H, heads, (hipStream_t)stream);
}

// the small kernels of the text / vision towers on their own (clip.hip, vit.hip).  sd_op_clip_embed CLAMPS an id outside
// [0, vocab) to the nearest row, as the kernel does; the Python wrapper (clip.py) refuses such ids before they get here.
extern "C" int sd_op_clip_embed(void* stream, const int* ids, const void* tok, const void* pos, void* out, int rows, int L, int H,
                                int vocab) {
    return sd_launch_clip_embed(ids, (const bf16_t*)tok, (const bf16_t*)pos, (bf16_t*)out, rows, L, H, vocab, (hipStream_t)stream);
}

extern "C" int sd_op_activation(void* stream, void* x, long long n, int kind) {
    SD_REQUIRE(kind == SD_ACT_QUICK_GELU || kind == SD_ACT_GELU, "sd_op_activation: kind %d (%d = quick_gelu, %d = gelu)", kind,
               SD_ACT_QUICK_GELU, SD_ACT_GELU);
    if (kind == SD_ACT_GELU) return sd_launch_gelu_erf((bf16_t*)x, (long)n, (hipStream_t)stream);
    return sd_launch_quick_gelu((bf16_t*)x, (long)n, (hipStream_t)stream);
}

extern "C" int sd_op_pool_rows(void* stream, const void* src, const int* ids, int B, int L, int H, int eos_id, void* dst) {
    return sd_launch_pool_rows((const bf16_t*)src, ids, B, L, H, eos_id, (bf16_t*)dst, (hipStream_t)stream);
}

extern "C" int sd_op_vit_embed(void* stream, const void* patch_rows, const float* cls, const void* pos, void* out, int B, int Np,
                               int H) {
    return sd_launch_vit_embed((const bf16_t*)patch_rows, cls, (const bf16_t*)pos, (bf16_t*)out, B, Np, H, (hipStream_t)stream);
}

// the BLIP text encoder's attention on its own; the key mask is copied to the host to refuse a sample without a valid key
extern "C" int sd_op_bert_attention(void* stream, const void* q, long long ldq, const void* k, const void* v, long long ldkv,
                                    const int* mask, void* out, long long ldo, int B, int heads, int Lq, int Lk) {
    if (sd_bert_attention_check(B, Lq, Lk, heads)) return -1;
    if (mask) {
        std::vector<int> hm((size_t)B * Lk);
        SD_CHECK_HIP(hipMemcpyAsync(hm.data(), mask, hm.size() * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
        SD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        if (sd_bert_mask_check(hm.data(), B, Lk)) return -1;
    }
    return sd_launch_bert_attention((const bf16_t*)q, ldq, (const bf16_t*)k, (const bf16_t*)v, ldkv, mask, (bf16_t*)out, ldo, B, heads,
                                    Lq, Lk, (hipStream_t)stream);
}

extern "C" int sd_op_reward_head(void* stream, const void* hidden, long long row_stride, const float* w, const float* bias,
                                 float mean, float std, int B, int H, float* rewards, float* features) {
    return sd_launch_reward_head((const bf16_t*)hidden, row_stride, w, bias, mean, std, B, H, rewards, features, (hipStream_t)stream);
}

// CLIPImageProcessor on device: uint8 images [B][3][H][W] -> the uint8 crop [B][3][S][S] and bf16 patch rows
// [B * (S/P)^2][Kp] (Kp = 3 P^2 rounded up to 64).  Synchronises the stream (the tap tables and the intermediate are
// allocated for the call).
extern "C" int sd_op_clip_preprocess(void* stream, const unsigned char* images, int B, int H, int W, int S, int P,
                                     unsigned char* crop, void* patches) {
    SD_REQUIRE(images && crop && patches && B > 0, "clip_preprocess: null argument");
    if (check_image_size(H, W, "clip_preprocess")) return -1;
    SD_REQUIRE(S >= 1 && P >= 1 && S % P == 0, "clip_preprocess: crop %d patch %d", S, P);
    std::vector<int> tab;
    ClipPrepGeom g;
    if (sd_clip_prep_tables(H, W, S, tab, g)) return -1;
    const int Kp = (3 * P * P + 63) / 64 * 64;
    int* dtab = nullptr;
    unsigned char* tmp = nullptr;
    SD_CHECK_HIP(hipMalloc((void**)&dtab, tab.size() * sizeof(int)));
    if (hipMalloc((void**)&tmp, (size_t)B * 3 * g.R * S) != hipSuccess) {
        (void)hipFree(dtab);
        SD_REQUIRE(false, "clip_preprocess: cannot allocate the intermediate");
    }
    int rc = 0;
    if (hipMemcpy(dtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        sd_set_error("clip_preprocess: tap table upload failed");
        rc = -2;
    }
    if (!rc) rc = sd_launch_clip_preprocess(images, B, g, dtab, tmp, (bf16_t*)patches, P, Kp, crop, (hipStream_t)stream);
    if (!rc && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        sd_set_error("clip_preprocess: stream synchronisation failed");
        rc = -2;
    }
    (void)hipFree(tmp);
    (void)hipFree(dtab);
    return rc;
}

// q|k|v projection the way the plan runs it at the 64x64 level: Q token-major [M][C], K and V head-major
// KV[2][M / tokens][C / 40][tokens][40] (GemmArgs::KV); W = [3 C][K] rows (q | k | v)
extern "C" int sd_op_gemm_qkv_headmajor(void* stream, const void* X, long long ldx, const void* W, void* Q, void* KV, int M,
                                        int C, int tokens, int K) {
    if (ensure_zero_page()) return -2;
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.K1 = K; a.W = (const bf16_t*)W; a.C = (bf16_t*)Q; a.ldc = C; a.M = M; a.N = 3 * C;
    a.K = K; a.zero_page = zero_page(); a.splitk = 1; a.KV = (bf16_t*)KV; a.hm_C = C; a.hm_tok = tokens;
    return sd_launch_gemm(a, 0, (hipStream_t)stream);
}

// self-attention with HEAD-MAJOR K / V ([B][heads][Nk][D] contiguous, as the plan's q|k|v projection stores them at the
// 64x64 level): d = 40, Nk a multiple of 64
extern "C" int sd_op_attention_headmajor(void* stream, const void* Q, long long ldq, const void* K, const void* V, void* O,
                                         long long ldo, int B, int heads, int Nq, int Nk, int D, float scale) {
    AttnArgs a;
    a.Q = (const bf16_t*)Q; a.ldq = ldq; a.K = (const bf16_t*)K; a.V = (const bf16_t*)V; a.kv_head_major = 1;
    a.O = (bf16_t*)O; a.ldo = ldo; a.B = B; a.heads = heads; a.Nq = Nq; a.Nk = Nk; a.D = D; a.scale = scale;
    if (ensure_zero_page()) return -2;
    a.consts = zero_page();
    return sd_launch_attention(a, (hipStream_t)stream);
}

// FreeU on one resnet's inputs (freeu.hip)
extern "C" int sd_op_freeu(void* stream, const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W,
                           int C_hidden, int C_skip, float b, float s) {
    return sd_launch_freeu((const bf16_t*)hidden, (const bf16_t*)skip, (bf16_t*)hidden_out, (bf16_t*)skip_out, B, H, W, C_hidden, C_skip,
                           b, s, (hipStream_t)stream);
}

// T-GATE's capture and apply kernels (tgate.hip); rowstats may be null
extern "C" int sd_op_tgate_capture(void* stream, const void* y, const void* res, void* h2, void* cache, float* rowstats, long long rows,
                                   int C, int pair) {
    return sd_launch_tgate_capture((const bf16_t*)y, (const bf16_t*)res, (bf16_t*)h2, (bf16_t*)cache, rowstats, (long)rows, C, pair,
                                   (hipStream_t)stream);
}
extern "C" int sd_op_tgate_apply(void* stream, const void* h1, const void* cache, void* h2, float* rowstats, long long rows, int C) {
    return sd_launch_tgate_apply((const bf16_t*)h1, (const bf16_t*)cache, (bf16_t*)h2, rowstats, (long)rows, C, (hipStream_t)stream);
}

// HyperTile's tile gather / scatter (hypertile.hip) and their shape rule
extern "C" int sd_hypertile_check(int B, int rh, int rw, int C, int nh, int nw, long long pitch) {
    return sd_hypertile_shape_ok(B, rh, rw, C, nh, nw, (long)pitch, "sd_hypertile_check");
}
extern "C" int sd_op_hypertile_gather(void* stream, const void* x, long long pitch, void* out, int B, int rh, int rw, int C, int nh, int nw) {
    return sd_launch_hypertile_gather((const bf16_t*)x, (long)pitch, (bf16_t*)out, B, rh, rw, C, nh, nw, (hipStream_t)stream);
}
extern "C" int sd_op_hypertile_scatter(void* stream, const void* y, void* out, long long pitch, int B, int rh, int rw, int C, int nh, int nw) {
    return sd_launch_hypertile_scatter((const bf16_t*)y, (bf16_t*)out, (long)pitch, B, rh, rw, C, nh, nw, (hipStream_t)stream);
}

// PAG's identity self-attention (pag.hip) and its shape rule
extern "C" int sd_pag_identity_check(long long rows_total, long long row0, long long rows, int C, int heads, long long ldv, int tok) {
    return sd_pag_identity_shape_ok((long)rows_total, (long)row0, (long)rows, C, heads, (long)ldv, tok, "sd_pag_identity_check");
}
extern "C" int sd_op_pag_identity(void* stream, const void* V, long long ldv, int tok, void* out, long long rows_total, long long row0,
                                  long long rows, int C, int heads) {
    return sd_launch_pag_identity((const bf16_t*)V, (long)ldv, tok, (bf16_t*)out, (long)rows_total, (long)row0, (long)rows, C, heads,
                                  (hipStream_t)stream);
}

// SAG's two kernels (sag.hip) and the mass kernel's shape rule
extern "C" int sd_sag_mass_check(int B, int heads, int N, int D, long long ld, int head_major) {
    return sd_sag_mass_shape_ok(B, heads, N, D, (long)ld, head_major, "sd_sag_mass_check");
}
extern "C" int sd_op_sag_attn_mass(void* stream, const void* Q, const void* K, long long ld, float* mass, int B, int heads, int N, int D,
                                   int exp2_units) {
    return sd_launch_sag_attn_mass((const bf16_t*)Q, (const bf16_t*)K, (long)ld, mass, B, heads, N, D, exp2_units ? 1 : 0, (hipStream_t)stream);
}
extern "C" int sd_op_sag_degrade(void* stream, const float* x, const float* m, const float* mass, int mh, int mw, int pred_type,
                                 const float coef[6], float* out, int LB, int H, int W) {
    return sd_launch_sag_degrade(x, m, mass, mh, mw, pred_type, coef, out, LB, H, W, (hipStream_t)stream);
}

// Token Merging, kernel by kernel (tome.hip); index lists in src / dst slot numbers, tok [h * w] from sd_op_tome_match
extern "C" int sd_op_tome_match(void* stream, const void* x, const unsigned char* choice, int B, int h, int w, int C,
                                float* node_max, int* node_idx, int* tok) {
    if (sd_tome_check(h, w, C, "sd_op_tome_match")) return -1;
    SD_REQUIRE(B >= 1, "sd_op_tome_match: B=%d", B);
    float* inv = (float*)op_scratch((size_t)B * h * w * 4);
    SD_REQUIRE(inv, "sd_op_tome_match: cannot allocate scratch");
    return sd_launch_tome_match((const bf16_t*)x, choice, B, h, w, C, node_max, node_idx, tok, inv, (hipStream_t)stream);
}

extern "C" int sd_op_tome_select(void* stream, const float* node_max, const int* node_idx, int B, int num_src, int r, int* kept,
                                 int* merged, int* dst_idx) {
    return sd_launch_tome_select(node_max, node_idx, B, num_src, r, kept, merged, dst_idx, (hipStream_t)stream);
}

extern "C" int sd_op_tome_merge(void* stream, const void* x, const int* tok, const int* kept, const int* merged, const int* dst_idx,
                                void* out, long long ldo, int B, int h, int w, int C, int r) {
    return sd_launch_tome_merge((const bf16_t*)x, tok, kept, merged, dst_idx, (bf16_t*)out, (long)ldo, B, h, w, C, r, (hipStream_t)stream);
}

extern "C" int sd_op_tome_unmerge(void* stream, const void* y, long long ldy, const void* residual, const int* tok, const int* kept,
                                  const int* merged, const int* dst_idx, void* out, int B, int h, int w, int C, int r) {
    return sd_launch_tome_unmerge((const bf16_t*)y, (long)ldy, (const bf16_t*)residual, tok, kept, merged, dst_idx, (bf16_t*)out, B, h, w,
                                  C, r, (hipStream_t)stream);
}

extern "C" int sd_op_conv_in_cond(void* stream, const float* x, int Bsrc, const float* cond, int Bcond, const float* Wt,
                                  const float* bias, void* y, int B, int H, int W, int Cout) {
    return sd_launch_conv_in_cond(x, Bsrc, cond, Bcond, Wt, bias, (bf16_t*)y, B, H, W, Cout, (hipStream_t)stream);
}

extern "C" int sd_op_conv_in_add(void* stream, const float* x, int Bsrc, const void* addend, int Badd, const float* Wt,
                                 const float* bias, void* y, int B, int H, int W, int Cout) {
    return sd_launch_conv_in_add(x, Bsrc, (const bf16_t*)addend, Badd, Wt, bias, (bf16_t*)y, B, H, W, Cout, (hipStream_t)stream);
}

extern "C" int sd_op_residual_add(void* stream, void* x, const long long* dst_off, const void* r, const long long* src_off,
                                  const long long* count, int nseg, float scale) {
    SD_REQUIRE(x && r && dst_off && src_off && count, "sd_op_residual_add: null argument");
    SD_REQUIRE(nseg >= 1 && nseg <= MAX_CONTROL_RES, "sd_op_residual_add: %d segments (1 .. %d)", nseg, MAX_CONTROL_RES);
    bf16_t* xs[MAX_CONTROL_RES];
    const bf16_t* rs[MAX_CONTROL_RES];
    long n[MAX_CONTROL_RES];
    for (int k = 0; k < nseg; ++k) {
        SD_REQUIRE(dst_off[k] >= 0 && src_off[k] >= 0 && count[k] > 0, "sd_op_residual_add: segment %d", k);
        xs[k] = (bf16_t*)x + dst_off[k]; rs[k] = (const bf16_t*)r + src_off[k]; n[k] = (long)count[k];
    }
    return sd_launch_residual_add(xs, rs, n, nseg, scale, (hipStream_t)stream);
}

extern "C" int sd_op_conv_in(void* stream, const float* x, int Bsrc, const float* Wt, const float* bias, void* y, int B,
                             int H, int W, int Cin, int Cout) {
    return sd_launch_conv_in(x, Bsrc, Wt, bias, (bf16_t*)y, B, H, W, Cin, Cout, (hipStream_t)stream);
}

extern "C" int sd_op_conv_out(void* stream, const void* x, const void* Wp, const float* bias, float* y, int B, int H,
                              int W, int Cin, int Cout) {
    return sd_launch_conv_out((const bf16_t*)x, (const bf16_t*)Wp, bias, y, B, H, W, Cin, Cout, (hipStream_t)stream);
}

extern "C" int sd_op_time_embedding(void* stream, float t, const void* W1, const float* b1, const void* W2,
                                    const float* b2, float* scratch, float* temb, int dim_in, int dim) {
    int rc;
    if ((rc = sd_launch_timestep_sinusoid(t, scratch, dim_in, (hipStream_t)stream))) return rc;
    if ((rc = sd_launch_gemv(scratch, (const bf16_t*)W1, b1, scratch + dim_in, dim, dim_in, 0, (hipStream_t)stream))) return rc;
    return sd_launch_gemv(scratch + dim_in, (const bf16_t*)W2, b2, temb, dim, dim, 1, (hipStream_t)stream);
}

extern "C" int sd_op_timestep_cond(void* stream, float t, const float* cond, const void* Wc, float* row, float* emb,
                                   int cond_dim, int dim) {
    SD_REQUIRE(cond && Wc && row && emb, "timestep_cond: null operand");
    SD_REQUIRE(((uintptr_t)cond & 15) == 0 && cond_dim > 0, "timestep_cond: cond must be 16-byte aligned, cond_dim > 0");
    int rc;
    if ((rc = sd_launch_gemv(cond, (const bf16_t*)Wc, nullptr, row, dim, cond_dim, 0, (hipStream_t)stream))) return rc;
    return sd_launch_timestep_sinusoid_row(t, row, emb, dim, (hipStream_t)stream);
}

// ---- fp8-e4m3 operand path, operator level (parity tests of SD_DTYPE_FP8_E4M3) ---------------------------------
extern "C" int sd_op_gemm_fp8(void* stream, const void* X, long long ldx, const void* W, const float* wscale, float xscale,
                              const float* bias, const void* R, long long ldr, void* C, long long ldc, int M, int N, int K,
                              int epi, int out_fp8, float oscale) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(epi == 0 || epi == 1, "sd_op_gemm_fp8: epi %d (0 = std, 1 = GEGLU)", epi);
    SD_REQUIRE(xscale > 0.f && (!out_fp8 || (epi == 1 && oscale > 0.f)), "sd_op_gemm_fp8: bad scales / fp8 output needs the GEGLU epilogue");
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.K1 = K; a.W = (const bf16_t*)W; a.bias = bias; a.R = (const bf16_t*)R; a.ldr = ldr;
    a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.zero_page = zero_page();
    a.dt = 1; a.wscale = wscale; a.xscale_inv = 1.0f / xscale; a.out_fp8 = out_fp8; a.oscale = oscale;
    a.splitk = epi ? 1 : op_gemm_splitk(M, N, K, 1);
    if (splitk_slab(a, "sd_op_gemm_fp8")) return -1;
    return sd_launch_gemm(a, epi, (hipStream_t)stream);
}

extern "C" int sd_op_conv3x3_fp8(void* stream, const void* X, const void* W, const float* wscale, float xscale,
                                 const float* bias, const float* bias2, const void* R, void* Y, int B, int Hin, int Win,
                                 int Cin, int Cout, int stride, int upsample) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(stride == 1 || stride == 2, "conv3x3 fp8: stride %d", stride);
    SD_REQUIRE(xscale > 0.f, "conv3x3 fp8: activation scale");
    GemmArgs a;
    conv3x3_args(a, X, W, bias, bias2, R, Y, B, Hin, Win, Cin, Cout, stride, upsample ? 1 : 0);
    a.dt = 1; a.wscale = wscale; a.xscale_inv = 1.0f / xscale;
    a.splitk = sd_conv3x3_splitk(a.M, a.N, Cin, Hin, Win, stride, a.up, 1);
    if (splitk_slab(a, "sd_op_conv3x3_fp8")) return -1;
    return sd_launch_conv3x3(a, (hipStream_t)stream);
}

extern "C" int sd_op_groupnorm_fp8(void* stream, const void* x1, int C1, const void* x2, int C2, const float* gamma,
                                   const float* beta, void* y, int B, int HW, int groups, float eps, int silu, int Cpad,
                                   float oscale) {
    GroupNormArgs a;
    a.x1 = (const bf16_t*)x1; a.C1 = C1; a.x2 = (const bf16_t*)x2; a.C2 = C2; a.gamma = gamma; a.beta = beta;
    a.y = (bf16_t*)y; a.B = B; a.HW = HW; a.groups = groups; a.eps = eps; a.silu = silu;
    a.out_fp8 = 1; a.Cpad = Cpad; a.oscale = oscale;
    a.nsplit = sd_groupnorm_nsplit(B, HW);
    a.partial = (float*)op_scratch(sd_groupnorm_scratch_bytes(B, HW, groups));
    SD_REQUIRE(a.partial, "sd_op_groupnorm_fp8: cannot allocate scratch");
    return sd_launch_groupnorm(a, (hipStream_t)stream);
}

extern "C" int sd_op_layernorm_fp8(void* stream, const void* x, const float* gamma, const float* beta, void* y, int rows,
                                   int C, int Cpad, float eps, float oscale) {
    return sd_launch_layernorm_fp8((const bf16_t*)x, gamma, beta, y, rows, C, Cpad, eps, oscale, (hipStream_t)stream);
}

extern "C" int sd_op_quantize_fp8(void* stream, const void* x_bf16, void* y_fp8, long long rows, int C, int Cpad, float scale) {
    return sd_launch_quantize_fp8((const bf16_t*)x_bf16, y_fp8, (long)rows, C, Cpad, scale, (hipStream_t)stream);
}

// the measurement behind sd_unet_calibrate_fp8, on its own: *out_code = the largest (byte & 0x7f) of the tensor
extern "C" int sd_op_amax_e4m3(void* stream, const void* codes, long long nbytes, unsigned* out_code) {
    SD_REQUIRE(out_code, "sd_op_amax_e4m3: null output");
    SD_CHECK_HIP(hipMemsetAsync(out_code, 0, sizeof(unsigned), (hipStream_t)stream));
    return sd_launch_amax_e4m3(codes, (long)nbytes, out_code, (hipStream_t)stream);
}

// ---- fused prompt cross-attention, operator level: Y = R + sum_h softmax_L(X A_h) B_h + b_o (xattn.hip) ----
// ---- LayerNorm folded into the consuming GEMM (the plan's norm1 -> q|k|v and norm3 -> GEGLU pairs) ----
// number of per-row partials a producer writes: kind 0 = GEMM with N output columns, kind 1 = fused cross-attention (M, C)
extern "C" int sd_op_ln_partials(int kind, int M, int N) { return kind == 0 ? (N + 159) / 160 * 2 : 2 * sd_xattn_slices(M, N); }
// producer: C = X W^T + bias + R, and rowstats[parts][M][2] = per-row (sum, sum of squares) partials of the stored C
extern "C" int sd_op_gemm_rowstats(void* stream, const void* X, long long ldx, const void* W, const float* bias, const void* R,
                                   long long ldr, void* C, long long ldc, int M, int N, int K, float* rowstats) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(rowstats, "sd_op_gemm_rowstats: null partials buffer");
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.K1 = K; a.W = (const bf16_t*)W; a.bias = bias; a.R = (const bf16_t*)R; a.ldr = ldr;
    a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.zero_page = zero_page(); a.splitk = 1; a.rowstats = rowstats;
    return sd_launch_gemm(a, 0, (hipStream_t)stream);
}
// The std-epilogue GEMM with EVERY side input / output the UNet plan combines on it (tests compare the lean kernel of
// gemm_lean.hip against the general one bit for bit through this entry, SD_GEMM_LEAN=0|1): second K segment, bias, bias2,
// residual, LayerNorm row partials and GroupNorm block statistics of the stored output (producer side), the LayerNorm fold
// (consumer side: ln_rs / ln_parts / ln_c1, bias = c2) and head-major K / V (hm_tokens > 0: N = 3 C, KV[2][M / tokens][C / 40][tokens][40]).
extern "C" int sd_op_gemm_plan(void* stream, const void* X, long long ldx, const void* X2, long long ldx2, int K1, const void* W,
                               const float* bias, const float* bias2, const void* R, long long ldr, void* C, long long ldc,
                               int M, int N, int K, float* rowstats, float* stats, const float* ln_rs, int ln_parts,
                               const float* ln_c1, float ln_eps, void* KV, int hm_tokens) {
    if (ensure_zero_page()) return -2;
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.X2 = (const bf16_t*)X2; a.ldx2 = ldx2; a.K1 = K1; a.W = (const bf16_t*)W;
    a.bias = bias; a.bias2 = bias2; a.R = (const bf16_t*)R; a.ldr = ldr; a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    a.zero_page = zero_page(); a.splitk = 1; a.rowstats = rowstats; a.stats = stats;
    a.ln_rs = ln_rs; a.ln_np = ln_parts; a.ln_c1 = ln_c1; a.ln_eps = ln_eps;
    if (hm_tokens > 0) {
        SD_REQUIRE(N % 3 == 0 && KV, "sd_op_gemm_plan: head-major K / V needs N = 3 C and a KV buffer");
        a.KV = (bf16_t*)KV; a.hm_C = N / 3; a.hm_tok = hm_tokens;
    }
    return sd_launch_gemm(a, 0, (hipStream_t)stream);
}
// consumer: C = epi(LayerNorm(X) W^T + b) computed from the UN-normalised X: Wg = bf16(W * gamma), c1[n] = sum_k Wg[n][k],
// c2[n] = sum_k W[n][k] beta[k] + b[n]; mean / rstd of a row from its `parts` partials.  epi 0 = plain, 1 = GEGLU.
extern "C" int sd_op_gemm_ln(void* stream, const void* X, long long ldx, const void* Wg, const float* c1, const float* c2,
                             const float* rowstats, int parts, float eps, void* C, long long ldc, int M, int N, int K, int epi) {
    if (ensure_zero_page()) return -2;
    SD_REQUIRE(epi == 0 || epi == 1, "sd_op_gemm_ln: epi %d (0 = plain, 1 = GEGLU)", epi);
    GemmArgs a;
    a.X = (const bf16_t*)X; a.ldx = ldx; a.K1 = K; a.W = (const bf16_t*)Wg; a.bias = c2;
    a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.zero_page = zero_page(); a.splitk = 1;
    a.ln_rs = rowstats; a.ln_np = parts; a.ln_c1 = c1; a.ln_eps = eps;
    return sd_launch_gemm(a, epi, (hipStream_t)stream);
}

extern "C" int sd_op_xattn_fused_rowstats(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                                          const float* bias, int M, int C, int rows_per_sample, int L, float* rowstats) {
    SD_REQUIRE(sd_xattn_fused_applicable(rows_per_sample, C, 8, L), "sd_op_xattn_fused_rowstats: shape not supported");
    XattnArgs a = xattn_args(X, R, Y, At, Bw, bias, M, C, rows_per_sample, L);
    a.rowstats = rowstats;
    return sd_launch_xattn_fused(a, (hipStream_t)stream);
}

// the IP-Adapter image branch on its own (ip_xattn.hip; the launch the "IP on" plan puts in front of a block's prompt
// cross-attention): Rout = R + sum_h softmax_T(LayerNorm(R; gamma, beta, eps) A_h^T) B_h
extern "C" int sd_op_ip_xattn(void* stream, const void* R, void* Rout, const void* A, const void* Bt, const float* gamma,
                              const float* beta, float eps, long long M, int C, int rows_per_sample, int heads, int T) {
    return sd_launch_ip_xattn((const bf16_t*)R, (bf16_t*)Rout, (const bf16_t*)A, (const bf16_t*)Bt, gamma, beta, eps, (long)M, C,
                              rows_per_sample, heads, T, (hipStream_t)stream);
}

// the builders of the prompt-side operands on their own (small.hip; sd_launch_xattn_fold / sd_launch_ip_fold of unet.hip: what
// sd_unet_set_context_hw / sd_unet_set_ip_adapter_hw run per layer)
extern "C" int sd_op_xattn_expand(void* stream, const void* kv, void* out, int B, int L, int C, int heads, int slots, int col_off,
                                  float scale) {
    SD_REQUIRE(col_off == 0 || col_off == C, "sd_op_xattn_expand: col_off %d (0 = the K half, C = the V half of a row)", col_off);
    return sd_launch_xattn_expand((const bf16_t*)kv, (bf16_t*)out, B, L, C, heads, col_off, scale, (hipStream_t)stream, slots);
}

extern "C" int sd_op_transpose_bf16(void* stream, const void* src, void* dst, int B, int R, int Cc, int perm16) {
    return sd_launch_transpose_bf16((const bf16_t*)src, (bf16_t*)dst, B, R, Cc, (hipStream_t)stream, perm16);
}

extern "C" int sd_op_retile32(void* stream, const void* src, void* dst, int B, int R, int K, int RT) {
    SD_REQUIRE(R > 0 && K > 0, "sd_op_retile32: R=%d K=%d", R, K);
    SD_REQUIRE(((((uintptr_t)src) | (uintptr_t)dst) & 15) == 0, "sd_op_retile32: operands must be 16-byte aligned");
    return sd_launch_retile32((const bf16_t*)src, (bf16_t*)dst, B, R, K, RT, (hipStream_t)stream);
}

extern "C" int sd_op_xattn_fold(void* stream, const void* kv, const void* wqT, const void* wo, const float* lnu, const float* ones,
                                void* at, void* bw, float* c1, float* c2, void* scratch, int UB, int L, int C, int heads, int perm) {
    if (ensure_zero_page()) return -2;
    return sd_launch_xattn_fold((const bf16_t*)kv, (const bf16_t*)wqT, (const bf16_t*)wo, lnu, ones, (bf16_t*)at, (bf16_t*)bw, c1, c2,
                                (bf16_t*)scratch, UB, L, C, heads, perm, (hipStream_t)stream);
}

extern "C" int sd_op_ip_fold(void* stream, const void* ip_kv, const void* wqT, const void* wo, void* at, void* bt, void* scratch,
                             int UB, int T, int C, int heads, float scale) {
    if (ensure_zero_page()) return -2;
    return sd_launch_ip_fold((const bf16_t*)ip_kv, (const bf16_t*)wqT, (const bf16_t*)wo, (bf16_t*)at, (bf16_t*)bt, (bf16_t*)scratch,
                             UB, T, C, heads, scale, (hipStream_t)stream);
}

extern "C" int sd_op_xattn_fused(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                                 const float* bias, int M, int C, int rows_per_sample, int L) {
    SD_REQUIRE(sd_xattn_fused_applicable(rows_per_sample, C, 8, L) || getenv("SD_XATTN_FUSED"),
               "sd_op_xattn_fused: shape not supported (8 heads x 80 key slots, 64 < L <= 80, C %% 32 == 0, tokens per sample %% 128 == 0)");
    return sd_launch_xattn_fused(xattn_args(X, R, Y, At, Bw, bias, M, C, rows_per_sample, L), (hipStream_t)stream);
}

// norm2 folded in (XattnArgs::ln_rs): X = the un-normalised rows, At = the CENTRED gamma-scaled operand, c2 [samples][640] fp32
extern "C" int sd_op_xattn_fused_ln(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                                    const float* bias, int M, int C, int rows_per_sample, int L, const float* ln_rowstats,
                                    int ln_parts, long long ln_rows, const float* c2, float eps, float* rowstats) {
    SD_REQUIRE(sd_xattn_fused_applicable(rows_per_sample, C, 8, L), "sd_op_xattn_fused_ln: shape not supported");
    SD_REQUIRE(ln_rowstats && c2, "sd_op_xattn_fused_ln: null operand");
    XattnArgs a = xattn_args(X, R, Y, At, Bw, bias, M, C, rows_per_sample, L);
    a.rowstats = rowstats;
    a.ln_rs = ln_rowstats; a.ln_np = ln_parts; a.ln_rows = ln_rows; a.ln_c2 = c2; a.ln_eps = eps;
    return sd_launch_xattn_fused(a, (hipStream_t)stream);
}

// diagnostic twin of sd_op_xattn_fused (tools/xattn_stamps.py): the kernel additionally stores 8 s_memtime stamps per
// workgroup to `stamps` (device memory, 8 * (M / 128) * slices 64-bit words, owned by the caller)
extern "C" int sd_op_xattn_fused_stamps(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                                        const float* bias, int M, int C, int rows_per_sample, int L, unsigned long long* stamps) {
    SD_REQUIRE(stamps, "sd_op_xattn_fused_stamps: null stamp buffer");
    SD_REQUIRE(sd_xattn_fused_applicable(rows_per_sample, C, 8, L), "sd_op_xattn_fused_stamps: shape not supported");
    XattnArgs a = xattn_args(X, R, Y, At, Bw, bias, M, C, rows_per_sample, L);
    a.stamps = stamps;
    return sd_launch_xattn_fused(a, (hipStream_t)stream);
}
