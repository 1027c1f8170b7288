// Internal launcher interface shared by the kernel translation units and the host units (unet.hip, plan.hip, ops.hip).
// Every launcher validates its operand shapes on the host BEFORE launching (a faulting kernel
// can take the whole GPU host down), enqueues on the caller's stream only, never synchronises,
// and returns 0 / negative with the message available through sd_last_error().
#pragma once
#include <vector>

#include "common.h"

struct GemmArgs {
    const bf16_t* X = nullptr;   // GEMM: [M, K1] rows (ldx);  CONV: NHWC input [B, Hin, Win, Cin]
    long ldx = 0;
    const bf16_t* X2 = nullptr;  // optional second K segment [M, K-K1] (channel concat), GEMM only
    long ldx2 = 0;
    int K1 = 0;                  // split point (== K when there is no second segment)
    const bf16_t* W = nullptr;   // [N, K] rows of stride ldw (conv: K = (slice, tap, channel))
    long ldw = 0;                // 0 = K (dense); a larger stride lets W be a column slice of an activation
    const float* bias = nullptr;   // [N] fp32, optional
    const float* bias2 = nullptr;  // [N] fp32, optional (time-embedding projection)
    const bf16_t* R = nullptr;     // residual [M, ldr], optional
    long ldr = 0;
    bf16_t* C = nullptr;           // output [M, ldc]
    long ldc = 0;
    int M = 0, N = 0, K = 0;
    // conv geometry
    int Hin = 0, Win = 0, Cin = 0, Hout = 0, Wout = 0, stride = 1, up = 0;
    // CONV, stride 2 only: the 3x3 window of output (oy, ox) starts AT input (2 oy, 2 ox) instead of (2 oy - 1, 2 ox - 1): the
    // AutoencoderKL encoder's downsampler, F.pad(x, (0, 1, 0, 1)) followed by an unpadded stride-2 conv.  The row below the
    // bottom edge and the column right of the right edge read as zero; Hin and Win are even and Hout = Hin / 2 exactly.
    int asym = 0;
    int splitk = 1;                   // > 1: K is split over blocks, fp32 partials go through `slab`
    float* slab = nullptr;            // [splitk, M, N] fp32 scratch (required when splitk > 1)
    // split-K only: leave the partial sums in `slab` and launch no splitk_reduce_kernel -- the consuming single-launch
    // GroupNorm finishes them (GroupNormArgs::slab: same sums in the same order, + bias + bias2 + R, and writes C as well)
    int defer_reduce = 0;
    const void* zero_page = nullptr;  // >= 16 zero bytes in device memory
    // per-sample W (cross-attention folded into two GEMMs): rows [b*rows_per_batch, (b+1)*rows_per_batch) of X use
    // W + b * w_batch_stride; rows_per_batch must be a multiple of the 128-row tile (0 = one W for all rows)
    long w_batch_stride = 0;
    int rows_per_batch = 0;
    int sm_valid = 0;                 // EPI 2: softmax over the first sm_valid of every 80 output columns
    int tiles_m = 0, tiles_n = 0;     // filled by the launcher
    int tune = 0;                     // experiment knobs, filled by the launcher from SD_GEMM_TUNE
    // GroupNorm statistics of the output from this kernel's epilogue (split-K = 1 only): [M / 64][N][2] fp32 partial
    // sums / sums of squares per 64-row block and channel (common.h::tile_channel_stats); null = off
    float* stats = nullptr;
    // LayerNorm folded into the consuming GEMM.  PRODUCER side (std epilogue, split-K = 1): rowstats = [2 tiles_n][M][2]
    // fp32, per row the (sum, sum of squares) of every N-wave's 80 output columns (common.h::tile_row_stats).
    // CONSUMER side: X holds the un-normalised rows, W = bf16(W * gamma), ln_c1[n] = sum_k W'[n][k], bias = W beta + b;
    // the epilogue turns the raw sums into  rstd_m * (acc - mean_m * c1[n]) + bias[n]  with mean / rstd of row m
    // from its ln_np partials ln_rs[part][M][2] (K = the normalised width).
    float* rowstats = nullptr;
    // q|k|v projection with HEAD-MAJOR K / V (std epilogue): columns [0, hm_C) (Q) go to C as usual, the 160-column tiles of
    // K (columns [hm_C, 2 hm_C)) and V are stored as KV[which][sample][head][token][40]: a 64-key tile of one head is one
    // contiguous 5 KiB block for the self-attention's LDS-DMA.  Needs head dim 40, hm_C % 160 == 0, hm_tok % 128 == 0.
    bf16_t* KV = nullptr;
    int hm_C = 0, hm_tok = 0;
    // CONV, nearest-2x upsample + 3x3 conv as FOUR 2x2 convs on the low-res input (sub-pixel phases (py, px) of the output):
    //   out[2y+py, 2x+px] = sum_{dy,dx in {0,1}} W4[ph][dy][dx] . in[y-1+py+dy, x-1+px+dx],  W4 = sums of the 3x3 taps that
    //   read the same low-res pixel -- 4/9 of the multiply-adds, exact.  Rows are ordered (sample, phase, low-res pixel);
    //   W holds [4 phases][Cout][Cin/64][4 taps][64] (w_batch_stride = one phase), K = 4 Cin, Hout = 2 Hin, M = 4 B Hin Win.
    int subpix = 0;
    const float* ln_rs = nullptr;
    const float* ln_c1 = nullptr;
    int ln_np = 0;
    float ln_eps = 1e-5f;
    int ln_per_sample = 0;            // per-sample weights (rows_per_batch > 0): ln_c1 and bias (c2) are [samples][N] as well
    // fp8-e4m3 operands (dt = 1): X and W hold OCP e4m3 bytes, K (and ldx / ldw / Cin) count fp8 elements and are
    // multiples of 128; the epilogue multiplies the fp32 sums by wscale[n] * xscale_inv before bias / residual.
    int dt = 0;
    const float* wscale = nullptr;    // [N] fp32: per-output-channel weight scale (W = W_fp8 * wscale[n])
    float xscale_inv = 1.0f;          // 1 / activation scale (X_fp8 = sat(X * xscale))
    int out_fp8 = 0;                  // GEGLU epilogue only: store e4m3 bytes (ldc in bytes) ...
    float oscale = 1.0f;              // ... of out * oscale
    // CONV on the halo kernel's 9-tap mode, bf16: the ResNet 1x1 shortcut folded into conv2 (conv_halo_kernel SC = 1):
    //   C = conv3x3(X, W) + [Xs1 | Xs2] . Wsc^T + bias,  Xs1 = [M, Csc1] and Xs2 = [M, Csc2] dense rows (Xs2 optional), Wsc =
    //   [N, ldwsc] rows with the Csc1 + Csc2 shortcut channels K-contiguous; Csc1 and Csc2 multiples of 64; bias = the SUM of
    //   the two biases; no bias2, no residual (sd_conv_halo_shortcut_applicable)
    const bf16_t* Xs1 = nullptr;
    const bf16_t* Xs2 = nullptr;
    const bf16_t* Wsc = nullptr;
    long ldwsc = 0;
    int Csc1 = 0, Csc2 = 0;
};

int sd_gemm_tile_rows(int M, int N, int K = 0);   // 64 or 128: M tile of the plain (std epilogue) GEMM (K = 0: not known)
// heuristic split factor (1 = none) for the std epilogue; rows = M tile of the kernel that will run (0 = the plain bf16 GEMM's choice)
int sd_gemm_splitk(int M, int N, int K, int rows = 0);   // heuristic split factor (1 = none) for the std epilogue
int sd_launch_gemm(const GemmArgs& a, int epi /*0 std, 1 geglu, 2 softmax over 80-column groups*/, hipStream_t stream);
int sd_launch_conv3x3(const GemmArgs& a, hipStream_t stream);
// gemm_lean.hip: the std-epilogue (epi 0; rows = 64 or 128: the M tile) and GEGLU (epi 1, 256 x 256 tile) GEMMs on full N
// tiles with buffer addressing
bool sd_gemm_lean_applicable(const GemmArgs& a, int epi);
int sd_launch_gemm_lean(const GemmArgs& a, int epi, int rows, hipStream_t stream);
void sd_launch_splitk_reduce(const GemmArgs& a, hipStream_t stream);   // slab -> C (+bias +bias2 +R)
// conv_halo.hip: LDS-resident-halo kernel for stride-1 convs on whole-row tiles
bool sd_conv_halo_applicable(const GemmArgs& a);
int sd_conv_halo_mode(const GemmArgs& a);   // 1: power-of-two geometry, 2: geometry mode (GEN), 0: implicit GEMM
int sd_conv3x3_splitk(int M, int N, int Cin, int Hin, int Win, int stride, int up, int dt = 0);
bool sd_conv_halo_subpix_applicable(const GemmArgs& a);      // the sub-pixel upsampler on the halo kernel's 4-tap mode
int sd_launch_conv3x3_halo(const GemmArgs& a, hipStream_t stream);
// the 1x1 shortcut fields of `a` (Xs1 ... Csc2) can ride on the launch sd_launch_conv3x3 makes for the conv of `a`
bool sd_conv_halo_shortcut_applicable(const GemmArgs& a);

// conv64.hip: 3x3 conv at 64 -> 64 channels with all nine taps' weights resident in LDS, on rectangular pixel tiles (the
// tiny autoencoder's only conv shape), and that autoencoder's entry / exit kernels
constexpr int SD_CONV64_PACKED_BYTES = 9 * 2 * 4 * 1024;      // sd_conv64_pack's output: [tap][k-step][row tile][lane][8] bf16
struct Conv64Args {
    const bf16_t* X = nullptr;      // NHWC bf16 [B, Hin, Win, 64]
    const bf16_t* Wp = nullptr;     // sd_conv64_pack'ed weights, SD_CONV64_PACKED_BYTES
    const float* bias = nullptr;    // [64] fp32, optional
    const bf16_t* R = nullptr;      // residual [B, Hout, Wout, 64], optional: added before the ReLU
    bf16_t* Y = nullptr;            // [B, Hout, Wout, 64]
    int B = 0, Hin = 0, Win = 0;
    int mode = 0;                   // 0: pad 1;  1: nearest-2x upsample, then pad 1 (Hout = 2 Hin);  2: stride 2, pad 1 (Hout = (Hin - 1) / 2 + 1)
    int relu = 0;
    int Hout = 0, Wout = 0, tiles_y = 0, tiles_x = 0, ntiles = 0;   // filled by the launcher
    unsigned xbytes = 0;
};
int sd_conv64_out_size(int in, int mode);
void sd_conv64_pack(const float* w_oihw /*[64][64][3][3]*/, bf16_t* out);      // host
int sd_launch_conv64(const Conv64Args& a, hipStream_t stream);
// entry: fp32 NCHW [B, Cin, H, W] -> conv3x3 Cin -> 64 (fp32, Wt [Cin * 9][64]) + bias -> bf16 NHWC.  decoder (Cin = 4): the
// input is tanh(x / 3) * 3 and a ReLU follows; encoder (Cin = 3): the [0, 1] image as it is, no activation
int sd_launch_taesd_entry(const float* x, const float* Wt, const float* bias, bf16_t* y, int B, int H, int W, int Cin, int decoder,
                          hipStream_t stream);
// exit: bf16 NHWC [B, H, W, 64] -> conv3x3 64 -> Cout <= 4 (Wp [Cout][9][64] bf16) + bias -> fp32 NCHW; out_mode 0: y * 2 - 1,
// 1: clamp(y, 0, 1), 2: y
int sd_launch_taesd_exit(const bf16_t* x, const bf16_t* Wp, const float* bias, float* y, int B, int H, int W, int Cout, int out_mode,
                         hipStream_t stream);

// GroupNorm over NHWC (optionally a two-tensor channel concat) -> bf16 [B, HW, C1+C2]
struct GroupNormArgs {
    const bf16_t* x1 = nullptr; int C1 = 0;
    const bf16_t* x2 = nullptr; int C2 = 0;   // optional
    const float* gamma = nullptr; const float* beta = nullptr;  // [C1+C2]
    bf16_t* y = nullptr;
    // out_fp8: y holds e4m3 bytes of sat(out * oscale), rows of Cpad >= C1+C2 bytes (a multiple of 128; the
    // pad channels are written as zeros: they are the K tail of the fp8 GEMM / conv that consumes y)
    int out_fp8 = 0, Cpad = 0;
    float oscale = 1.0f;
    // statistics delivered by the producers of x1 / x2 ([B * HW / 64][C1 or C2][2], see GemmArgs::stats): the statistics
    // pass over the tensor is skipped (both must be given when C2 > 0; HW a multiple of 64)
    const float* stats1 = nullptr; const float* stats2 = nullptr;
    // Single-launch kernel only: x1 has NOT been written yet -- its producer ran split-K with GemmArgs::defer_reduce and left
    // `splitk` fp32 partial slabs [splitk][B * HW][C1].  The kernel forms x1 = bf16(sum_s slab[s] + sbias + sbias2 + sR) exactly
    // as splitk_reduce_kernel would (same order of additions), normalises THAT, and stores it to x1w for x1's other readers:
    // one launch and one pass over the slabs instead of two launches (round 5: 27 such pairs per SD-1.5 forward at UNet batch 16).
    const float* slab = nullptr; int splitk = 0;
    const float* sbias = nullptr; const float* sbias2 = nullptr;   // [C1] fp32, optional
    const bf16_t* sR = nullptr; long sldr = 0;                     // residual rows, optional
    bf16_t* x1w = nullptr;                                         // [B * HW][C1]
    float* partial = nullptr;   // workspace of sd_groupnorm_scratch_bytes(): [B,nsplit,groups,2] partials + [B,groups,2] stats
    int B = 0, HW = 0, groups = 32, nsplit = 0;
    float eps = 1e-5f;
    int silu = 0;
};
int sd_groupnorm_nsplit(int B, int HW);
bool sd_groupnorm_uses_small(int B, int HW, int C1, int C2, int groups);
bool sd_groupnorm_slab_ok(int B, int HW, int C1, int C2, int groups);     // ... and may finish a deferred split-K reduce
size_t sd_groupnorm_scratch_bytes(int B, int HW, int groups);
int sd_launch_groupnorm(const GroupNormArgs& a, hipStream_t stream);

// in-place row softmax of bf16 scores: p = softmax(scale * s) over `cols` (multiple of 8)
int sd_launch_softmax_rows(bf16_t* s, long rows, int cols, float scale, hipStream_t stream);
int sd_launch_softmax_rows_long(bf16_t* s, long rows, int cols, float scale, hipStream_t stream);   // any cols % 8 == 0
// VAE post_quant_conv: y[b,co,p] = sum_ci W[co,ci] * (x[b,ci,p] * in_scale) + bias[co]  (fp32 NCHW, 4 -> 4)
int sd_launch_pqconv(const float* x, const float* W, const float* bias, float* y, int B, int HW, float in_scale,
                     hipStream_t stream);

int sd_launch_layernorm(const bf16_t* x, const float* gamma, const float* beta, bf16_t* y, int rows, int C,
                        float eps, hipStream_t stream);
// same, writing e4m3 bytes of sat(out * oscale) into rows of Cpad bytes (pad channels zero)
int sd_launch_layernorm_fp8(const bf16_t* x, const float* gamma, const float* beta, void* y, int rows, int C, int Cpad,
                            float eps, float oscale, hipStream_t stream);
// bf16 [rows, C] -> e4m3 [rows, Cpad] of sat(x * scale), pad zero (tests; operands whose producer has no fp8 epilogue)
// largest e4m3 magnitude code (byte & 0x7f) of `nbytes` e4m3 bytes -> atomicMax into *out (the caller zeroes it)
int sd_launch_amax_e4m3(const void* y, long nbytes, unsigned* out, hipStream_t stream);
int sd_launch_quantize_fp8(const bf16_t* x, void* y, long rows, int C, int Cpad, float scale, hipStream_t stream);

struct AttnArgs {
    const bf16_t* Q = nullptr; long ldq = 0;  // [B, Nq, heads*D] rows with stride ldq
    const bf16_t* K = nullptr; long ldk = 0;  // [B, Nk, ...]
    const bf16_t* V = nullptr; long ldv = 0;
    bf16_t* O = nullptr; long ldo = 0;
    int B = 0, heads = 0, Nq = 0, Nk = 0, D = 0;
    float scale = 0.f;
    const void* consts = nullptr;   // device page: 16 zero bytes at +0, the bf16 chunk {1,0,0,0,0,0,0,0} at +256
    // HEAD-MAJOR K / V ([B][heads][Nk][D] contiguous: a 64-key tile of one head is 64 * D * 2 contiguous bytes, so the
    // LDS-DMA pieces of the 64x64 self-attention touch 8 cache lines instead of ~26); 0 = token-major as Q (ldk / ldv)
    int kv_head_major = 0;
    // Q already carries scale * log2(e) (the UNet folds it into W_q before the weight's one rounding): the kernels take
    // the QK^T product as the exp2 argument as it is; `scale` is then ignored
    int q_prescaled = 0;
    // pipelined kernels: XCD-aware work order (all query blocks of a (sample, head) on one XCD); 0 = dispatch order (A/B: SD_ATTN_XCD=0)
    int xcd_order = 1;
};
int sd_launch_attention(const AttnArgs& a, hipStream_t stream);

// y[n] = sum_k W[n,k] * act_in(x[k]) + b[n]   (M = 1 path: timestep embedding MLP + projections)
int sd_launch_gemv(const float* x, const bf16_t* W, const float* b, float* y, int N, int K, int silu_in,
                   hipStream_t stream);
int sd_launch_timestep_sinusoid(float t, float* out, int dim, hipStream_t stream);
// out[i] = sinusoid(t)[i] + row[i]  (time embedding of a UNet with cond_proj, the row = cond_proj . condition)
int sd_launch_timestep_sinusoid_row(float t, const float* row, float* out, int dim, hipStream_t stream);
int sd_launch_f32_to_bf16(const float* src, bf16_t* dst, long n, hipStream_t stream);
// dst[b][c][r'] = src[b][r][c]; perm16: r' = r with bits 2 and 3 swapped (the k order in which a 32x32 MFMA
// accumulator tile is consumed as the next product's operand, see xattn.hip)
int sd_launch_transpose_bf16(const bf16_t* src, bf16_t* dst, int B, int R, int Cc, hipStream_t stream, int perm16 = 0);

int sd_launch_retile32(const bf16_t* src, bf16_t* dst, int B, int R, int K, int RT, hipStream_t stream);
int sd_launch_replicate(const void* src, void* dst, long bytes, int rep, hipStream_t stream);   // dst[r][i] = src[i], r < rep

// tome.hip: Token Merging around a block's self-attention on a level of h x w tokens (2x2 cells, one dst token per cell:
// position choice[cell] in 0..3; num_dst = h w / 4, num_src = 3 num_dst).  Index lists hold src / dst SLOT numbers (dst slots by
// cell, src slots by ascending token index); tok[N] maps slots to token indices, the src slots first.
int sd_tome_check(int h, int w, int C, const char* who);      // even sides, <= 16384 tokens, C % 64 == 0, C <= 1536
int sd_launch_tome_partition(const unsigned char* choice, int h, int w, int* tok, hipStream_t stream);
// x [B][N][C] -> node_max / node_idx [B][num_src]; writes tok [N] and the scratch inv [B][N] (fp32 inverse row norms)
int sd_launch_tome_match(const bf16_t* x, const unsigned char* choice, int B, int h, int w, int C, float* node_max, int* node_idx,
                         int* tok, float* inv, hipStream_t stream);
// top r of num_src (<= 12288) per sample -> kept [B][num_src - r], merged [B][r] (both ascending), dst_idx [B][r]
int sd_launch_tome_select(const float* node_max, const int* node_idx, int B, int num_src, int r, int* kept, int* merged, int* dst_idx,
                          hipStream_t stream);
// x [B][N][C] -> out [B][N - r] rows of pitch ldo: the kept src rows, then every dst row averaged with its members
int sd_launch_tome_merge(const bf16_t* x, const int* tok, const int* kept, const int* merged, const int* dst_idx, bf16_t* out,
                         long ldo, int B, int h, int w, int C, int r, hipStream_t stream);
// y [B][N - r] rows of pitch ldy -> out [B][N][C] = y[row of the token] + residual (residual may be null)
int sd_launch_tome_unmerge(const bf16_t* y, long ldy, const bf16_t* residual, const int* tok, const int* kept, const int* merged,
                           const int* dst_idx, bf16_t* out, int B, int h, int w, int C, int r, hipStream_t stream);

// freeu.hip: FreeU on the inputs of one up-block resnet, one launch: skip_out [B][H][W][C_skip] = fourier_filter(skip, threshold 1,
// scale s) per (sample, channel) plane, hidden_out [B][H][W][C_hidden] = hidden with its first C_hidden / 2 channels times b.  The
// outputs are new tensors.  H, W in [2, 128]; both channel counts multiples of 32; b, s finite and > 0.
int sd_freeu_check(int B, int H, int W, int C_hidden, int C_skip, const char* who);
int sd_launch_freeu(const bf16_t* hidden, const bf16_t* skip, bf16_t* hidden_out, bf16_t* skip_out, int B, int H, int W, int C_hidden,
                    int C_skip, float b, float s, hipStream_t stream);

// tgate.hip: T-GATE's two elementwise kernels (bf16 rows of C channels, C a multiple of 8; fp32 sums rounded once).  capture: y and
// res [pair * rows][C] -> h2 = res + y for every row, cache [rows][C] = the mean of the pair's two y rows (pair == 1: y itself).
// apply: h2 [rows][C] = h1 + cache.  rowstats (may be null): [SD_TGATE_PARTS][rows of h2][2] fp32 LayerNorm partials of the stored h2
// (GemmArgs::ln_rs).  The outputs are new tensors.
constexpr int SD_TGATE_PARTS = 2;
int sd_tgate_check(long rows, int C, const char* who);
int sd_launch_tgate_capture(const bf16_t* y, const bf16_t* res, bf16_t* h2, bf16_t* cache, float* rowstats, long rows, int C, int pair,
                            hipStream_t stream);
int sd_launch_tgate_apply(const bf16_t* h1, const bf16_t* cache, bf16_t* h2, float* rowstats, long rows, int C, hipStream_t stream);

// hypertile.hip: HyperTile's gather / scatter (one kernel): raster [B][rh][rw] rows of C bf16 channels and row pitch `pitch`
// <-> tile order [B][nh][nw][rh / nh][rw / nw] dense rows.  C a multiple of 8 (16-byte accesses), nh | rh, nw | rw, sides up to
// 256, pitch up to 2^30; 64-bit offsets.  shape_ok: the shape rule of both launchers and of the plan builder (no GPU work).
int sd_hypertile_shape_ok(int B, int rh, int rw, int C, int nh, int nw, long pitch, const char* who);
int sd_launch_hypertile_gather(const bf16_t* x, long pitch, bf16_t* out, int B, int rh, int rw, int C, int nh, int nw, hipStream_t stream);
int sd_launch_hypertile_scatter(const bf16_t* y, bf16_t* out, long pitch, int B, int rh, int rw, int C, int nh, int nw, hipStream_t stream);

// pag.hip: the identity self-attention of PAG's perturbed samples: out[r][h * D + d] = V(r, h, d) for the rows [row0, row0 + rows)
// of a token-major [rows_total][C] output, nothing else written.  tok == 0: token-major V with row pitch ldv; tok > 0: head-major
// V [rows_total / tok][heads][tok][D] (ldv not read).  D = C / heads a multiple of 8 (16-byte accesses), 64-bit offsets.
// shape_ok: the shape rule of the launcher and of the plan builder (no GPU work).
int sd_pag_identity_shape_ok(long rows_total, long row0, long rows, int C, int heads, long ldv, int tok, const char* who);
int sd_launch_pag_identity(const bf16_t* V, long ldv, int tok, bf16_t* out, long rows_total, long row0, long rows, int C, int heads,
                           hipStream_t stream);

// sag.hip: self-attention guidance.  sag_attn_mass: mass[b][k] = (1 / heads) sum_h sum_q softmax_k(Q_h K_h^T)[q][k] from token-major
// Q / K with one row pitch ld (Q already carries the softmax scale; exp2_units: it carries scale * log2 e, as W_q of attn1 does);
// one workgroup per sample, fixed summation order, no atomics.  sag_degrade: x0 / eps from (x, m), 9x9 Gaussian blur of x0 with
// reflect padding, blend where mass > 1 on the (H / 8) x (W / 8) grid, re-noise; coef = {x0 <- x, x0 <- m, eps <- x, eps <- m,
// sqrt(a), sqrt(1 - a)}; pred 0 epsilon / 1 v_prediction / 2 sample.  shape_ok: the shape rules (no GPU work).
int sd_sag_mass_shape_ok(int B, int heads, int N, int D, long ld, int head_major, const char* who);
int sd_launch_sag_attn_mass(const bf16_t* Q, const bf16_t* K, long ld, float* mass, int B, int heads, int N, int D, int exp2_units,
                            hipStream_t stream);
int sd_sag_degrade_shape_ok(int LB, int H, int W, int mh, int mw, int pred, const char* who);
int sd_launch_sag_degrade(const float* x, const float* m, const float* mass, int mh, int mw, int pred, const float coef[6], float* out,
                          int LB, int H, int W, hipStream_t stream);

// xattn.hip: fused prompt cross-attention  Y = R + sum_h softmax_L(X A_h) B_h + b_o  (one launch per block)
struct XattnArgs {
    const bf16_t* X = nullptr;    // [M, C] LayerNorm output
    const bf16_t* R = nullptr;    // [M, C] residual
    bf16_t* Y = nullptr;          // [M, C]
    // TILED operands (sd_launch_retile32): a 16-row x 64-byte DMA piece is one contiguous KiB
    const bf16_t* At = nullptr;   // [samples][C/32][640][32]: row (head, key slot) = scale * K_h[key] . W_q,h, zero rows for slots >= L
    const bf16_t* Bw = nullptr;   // [samples][C/32][20][32][32]: (channel tile, 32-slot slice, channel, slot in PERMUTED k order)
    const float* bias = nullptr;  // [C] to_out bias
    int M = 0, C = 0, rows_per_sample = 0, L = 0;
    float* rowstats = nullptr;    // [2 * channel slices][M][2]: LayerNorm partials of Y (GemmArgs::rowstats layout), null = off
    // LayerNorm (norm2) folded into the kernel: X holds the UN-normalised rows (usually X == R), ln_rs = their row partials
    // [ln_np][ln_rows][2] (sum, sum of squares; GemmArgs::rowstats of the producer; row m reads row m % ln_rows: a CFG pair
    // replicated after the producer ran shares them), At = rows of  scale K_h W_q,h diag(gamma)  CENTRED over the channel
    // (sum_c (x_c - mean) w_c = sum_c x_c (w_c - mean_c w): the row mean drops out of the product), ln_c2 [samples][640] fp32 =
    // the beta term of every key slot.  A score is then  rstd_m * (X . At)[m][n] + ln_c2[n].  null = X is already normalised.
    const float* ln_rs = nullptr; int ln_np = 0; long ln_rows = 0;
    const float* ln_c2 = nullptr;
    float ln_eps = 1e-5f;
    unsigned long long* stamps = nullptr;   // diagnostic: 8 s_memtime stamps per workgroup (SD_XATTN_STAMPS), else null
};
bool sd_xattn_fused_applicable(int rows_per_sample, int C, int heads, int L);
int sd_xattn_slices(int M, int C);     // channel slices of the launch (LayerNorm partials per row = 2 * slices)
int sd_launch_xattn_fused(const XattnArgs& a, hipStream_t stream);
// slots: key slots per head of the expansion (80 for the prompt; the IP-Adapter's image tokens use their own count)
int sd_launch_xattn_expand(const bf16_t* kv, bf16_t* out, int B, int L, int C, int NH, int col_off, float scale,
                           hipStream_t stream, int slots = 80);
// unet.hip: every operand of one folded prompt cross-attention layer (what sd_unet_set_context_hw runs per layer) from kv
// [UB * L][K | V] (2 C wide), wqT = attn2.to_q.weight.T (or .T.ln) [C][C], wo = attn2.to_out.0.weight [C][C]:
//   at_dst = rows (sample, head, slot) of (scale K)_masked . wqT^T, bw_dst = the per-sample transpose of V_masked . wo^T;
//   perm = 1: the fused kernel's layouts (XattnArgs::At / Bw: re-tiled, slots of Bw permuted), 0: [UB][NP][C] and [UB][C][NP];
//   c1 [UB][NP] = ones . rows of the stored at_dst (perm = 0 only), c2 [UB][NP] = lnu . rows of the K expansion; each may be null
//   together with its fp32 [C] vector.  scratch: three slabs of UB * NP * C bf16, NP = heads * 80.  1 <= L <= 80, C % 64 == 0.
int sd_launch_xattn_fold(const bf16_t* kv, const bf16_t* wqT, const bf16_t* wo, const float* lnu, const float* ones, bf16_t* at_dst,
                         bf16_t* bw_dst, float* c1, float* c2, bf16_t* scratch, int UB, int L, int C, int heads, int perm,
                         hipStream_t stream);
// ... and of one IP-Adapter block (sd_unet_set_ip_adapter_hw) from ip_kv [UB * T][K_ip | V_ip]: at [UB][32][C], bt [UB][C][32]
// (sd_launch_ip_xattn's A and Bt; V times the adapter scale).  scratch: three slabs of UB * 32 * C bf16.
int sd_launch_ip_fold(const bf16_t* ip_kv, const bf16_t* wqT, const bf16_t* wo, bf16_t* at, bf16_t* bt, bf16_t* scratch, int UB, int T,
                      int C, int heads, float scale, hipStream_t stream);
// ip_xattn.hip: the IP-Adapter image branch  Y = R + sum_h softmax_T(LN(R) A_h^T) B_h  (one launch per transformer block)
//   R, Y [M][C] (Y != R); A [samples][32][C]: row (head * (32 / heads) + token) = (K_ip,h[token] / sqrt(d)) . W_q,h, the other
//   rows zero; Bt [samples][C][32]: the same slots as columns = scale * V_ip,h[token] . W_o,h^T; gamma / beta [C]: norm2, applied
//   in the kernel from the row's own statistics.  C % 32 == 0, T = 4, heads in {1, 2, 4, 8}; any rows_per_sample >= 1.
bool sd_ip_xattn_applicable(int C, int heads, int T);
int sd_launch_ip_xattn(const bf16_t* R, bf16_t* Y, const bf16_t* A, const bf16_t* Bt, const float* gamma, const float* beta,
                       float eps, long M, int C, int rows_per_sample, int heads, int T, hipStream_t stream);
// clip.hip: CLIP text encoder pieces
int sd_launch_clip_embed(const int* ids, const bf16_t* tok, const bf16_t* pos, bf16_t* out, int rows, int L, int H,
                         int vocab, hipStream_t stream);
int sd_launch_clip_attention(const bf16_t* qkv, bf16_t* out, int B, int L, int H, int heads, hipStream_t stream);
int sd_launch_quick_gelu(bf16_t* x, long n, hipStream_t stream);
int sd_launch_gelu_erf(bf16_t* x, long n, hipStream_t stream);      // exact (erf) GELU in place: common.h::gelu_erf_f
int sd_launch_bf16_to_f32(const bf16_t* src, float* dst, long n, hipStream_t stream);

// vit.hip: CLIP vision tower pieces and the CLIP score
// geometry of one input size: crop S x S, the R intermediate rows from input row y0, and the offsets (in ints) of the tap
// tables in one int array: x min / count / coefficients of the S crop columns, then the same for the S crop rows (y min
// relative to y0)
struct ClipPrepGeom {
    int H = 0, W = 0, S = 0, y0 = 0, R = 0, ksx = 0, ksy = 0;
    int o_xmin = 0, o_xcnt = 0, o_xk = 0, o_ymin = 0, o_ycnt = 0, o_yk = 0;
};
void sd_clip_resize_geometry(int H, int W, int S, int* rh, int* rw, int* top, int* left);
int sd_clip_prep_tables(int H, int W, int S, std::vector<int>& tab, ClipPrepGeom& g);
// uint8 images [B][3][H][W] -> bf16 patch rows [B * (S/P)^2][Kp] (tmp: uint8 [B][3][R][S]; crop: optional uint8 [B][3][S][S])
int sd_launch_clip_preprocess(const unsigned char* img, int B, const ClipPrepGeom& g, const int* dtab, unsigned char* tmp,
                              bf16_t* patches, int P, int Kp, unsigned char* crop, hipStream_t stream);
int sd_launch_vit_embed(const bf16_t* prow, const float* cls, const bf16_t* pos, bf16_t* out, int B, int Np, int H,
                        hipStream_t stream);
int sd_launch_vit_attention(const bf16_t* qkv, bf16_t* out, int B, int L, int H, int heads, hipStream_t stream);
int sd_launch_pool_rows(const bf16_t* src, const int* ids, int B, int L, int H, int eos_id, bf16_t* dst, hipStream_t stream);
int sd_launch_clip_score(const float* img, const float* txt, int B, int P, float* raw, float* score, hipStream_t stream);

// bert.hip: the BLIP text encoder's attention and the ImageReward head
// masked attention of a short query block, head dim 64: q [B * Lq][ldq], k / v [B * Lk][ldkv] (pointers at their column
// offsets), key mask int32 [B][Lk] or null, 1 <= Lq <= 64, 1 <= Lk <= 320 -> out [B * Lq][ldo]
int sd_bert_attention_check(int B, int Lq, int Lk, int heads);
int sd_bert_mask_check(const int* host_mask, int B, int Lk);      // a HOST copy of the mask: every sample has a valid key
int sd_launch_bert_attention(const bf16_t* q, long ldq, const bf16_t* k, const bf16_t* v, long ldkv, const int* mask, bf16_t* out,
                             long ldo, int B, int heads, int Lq, int Lk, hipStream_t stream);
// rewards[b] = (w . x_b + wb[0] - mean) / std over the fp32 of row hidden[b * row_stride]; features (optional) [B][H] = x_b
int sd_launch_reward_head(const bf16_t* hidden, long row_stride, const float* w, const float* wb, float mean, float stdv, int B,
                          int H, float* rewards, float* features, hipStream_t stream);

// conv_in: NCHW fp32 latents [Bsrc,4,H,W] (batch index taken modulo Bsrc: CFG duplication is
// fused) -> NHWC bf16 [B,H,W,Cout]
int sd_launch_conv_in(const float* x, int Bsrc, const float* Wt /*[Cin*9][Cout] fp32*/, const float* bias,
                      bf16_t* y, int B, int H, int W, int Cin, int Cout, hipStream_t stream);
// conv_in of an inpainting UNet (Cin = 9): channels 0..3 from x [Bsrc,4,H,W], channels 4..8 from cond [Bcond,5,H,W] (both
// batch indices taken modulo their source batch) -> NHWC bf16 [B,H,W,Cout]; Wt [81][Cout] fp32
int sd_launch_conv_in_cond(const float* x, int Bsrc, const float* cond, int Bcond, const float* Wt, const float* bias,
                           bf16_t* y, int B, int H, int W, int Cout, hipStream_t stream);
constexpr int SD_MAX_RES_SEGMENTS = 16;      // segments of one residual-add launch (a ControlNet has 12 + 1)
// conv_in of a ControlNet: conv_in(x) + addend in one launch (addend NHWC bf16 [Badd,H,W,Cout], batch index modulo Badd; fp32
// sum, one bf16 rounding, 16-byte stores; Cout a multiple of 8)
int sd_launch_conv_in_add(const float* x, int Bsrc, const bf16_t* addend, int Badd, const float* Wt, const float* bias,
                          bf16_t* y, int B, int H, int W, int Cout, hipStream_t stream);
// x[k][j] <- bf16(float(x[k][j]) + scale * float(r[k][j])), j < n[k], for nseg <= 16 segments in ONE launch (host arrays of
// device pointers; 16-byte aligned; any n)
int sd_launch_residual_add(bf16_t* const* x, const bf16_t* const* r, const long* n, int nseg, float scale, hipStream_t stream);
int sd_launch_nchw_to_nhwc_bf16(const float* src, bf16_t* dst, int B, int C, long hw, hipStream_t stream);
// cond [B,5,hw] = [mask [B,1,hw] | masked [B,4,hw]] (fp32; hw a multiple of 4)
int sd_launch_inpaint_cond_pack(const float* mask, const float* masked, float* cond, int B, long hw, hipStream_t stream);
// inpainting, pixel space: masked [B,3,H,W] = mask >= 0.5 ? 0.5 : img, lmask [B,1,H/8,W/8] = (mask(8i, 8j) >= 0.5) as 0 / 1
int sd_launch_inpaint_prepare(const float* img, const float* mask, float* masked, float* lmask, int B, int H, int W,
                              hipStream_t stream);
// AutoencoderKL encoder entry: fp32 NCHW images [B,3,H,W] in [0,1] -> conv_in(2 x - 1) as NHWC bf16 [B,H,W,Cout]
// (the preprocessing is applied in the load; the zero padding is of the PREPROCESSED image)
int sd_launch_conv_in_image(const float* img, const float* Wt /*[27][Cout] fp32*/, const float* bias, bf16_t* y, int B, int H,
                            int W, int Cout, hipStream_t stream);
// AutoencoderKL encoder exit: conv_out (3x3, Cin -> 8, bf16 operands, fp32 sums) and quant_conv (1x1, 8 -> 8, fp32) in one
// launch: NHWC bf16 [B,H,W,Cin] -> moments NCHW fp32 [B,8,H,W]
int sd_launch_vae_enc_out(const bf16_t* x, const bf16_t* Wp /*[8][9][Cin]*/, const float* bias, const float* Wq /*[8][8]*/,
                          const float* bq, float* y, int B, int H, int W, int Cin, hipStream_t stream);
// DiagonalGaussianDistribution: z = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), or scale * mean when noise is
// null (mode()).  moments [B][2 C][hw] fp32 = [mean | logvar], noise / z [B][C][hw] fp32.
int sd_launch_vae_posterior(const float* moments, const float* noise, float scale, float* z, int B, int C, long hw,
                            hipStream_t stream);
// conv_out: NHWC bf16 [B,H,W,Cin] -> NCHW fp32 [B,Cout,H,W]  (Cout <= 4)
int sd_launch_conv_out(const bf16_t* x, const bf16_t* Wp /*[Cout][9][Cin]*/, const float* bias, float* y, int B,
                       int H, int W, int Cin, int Cout, hipStream_t stream);

// sched.hip: fused CFG combine + linear multistep scheduler update (DDIM / DPM-Solver(++) / LCM / PNDM)
struct StepCoef {
    float px, pe, p1, p2, pn;  // prev = px*x + pe*eps + p1*m1 + p2*m2 + p3*m3 + pn*noise
    float yx, ye;              // y2   = yx*x + ye*eps           (x0_pred / denoised)
    float mx, me;              // m0   = mx*x + me*eps           (history entry)
    float p3;                  // third history term (PNDM/PLMS order 4)
};
// k given: e := k[i / n_per_sample] * e (after the CFG combine, before every use).  init given: prev := mask ? prev :
// a * init + s * blend_noise; mask [n / n_per_sample][hw] fp32 0 / 1, broadcast over the n_per_sample / hw channels of its
// sample.  Neither: n_per_sample is not read.  `who`: the entry's name, the prefix of every refusal.  cfg: 0, 1 (CFG) or a PAG
// mode (sd_hip.h::SD_GUIDE_CFG_PAG / SD_GUIDE_PAG: eps holds three / two thirds and `pag` is the PAG scale; else pag is not read).
int sd_launch_sched_step(const char* who, const float* eps, int cfg, float guidance, float pag, const float* x, const float* m1,
                         const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                         StepCoef c, const float* k, long n_per_sample, long n, const float* init, const float* blend_noise,
                         const float* mask, float a, float s, long hw, hipStream_t stream);
// guidance_rescale: k_out[b] = r * std(c_b) / std(g_b) + (1 - r), g = u + s (c - u); eps = [u: batch | c: batch] samples
// (with_pag: [u | c | p] and g += pag (c - p))
int sd_launch_cfg_rescale_factors(const float* eps, int batch, long n_per_sample, float guidance, float rescale, float* k_out,
                                  hipStream_t stream, int with_pag = 0, float pag = 0.f);
// UniPC's predictor-corrector step (include/sd_hip.h::sd_sched_step_pc): corrector, predictor, history entry, x0 and the
// optional rescale / latent blend in one launch
struct PcCoef {
    float cm[2];  // m_t  = cm0*x + cm1*e
    float cy[2];  // y2   = cy0*x + cy1*e
    float cc[5];  // xc   = cc0*x_last + cc1*h1 + cc2*h2 + cc3*h3 + cc4*m_t
    float cp[4];  // prev = cp0*xc + cp1*m_t + cp2*h1 + cp3*h2
};
int sd_launch_sched_step_pc(const char* who, const float* eps, int cfg, float guidance, float pag, const float* x, const float* x_last, const float* h1,
                            const float* h2, const float* h3, float* prev, float* x_corr, float* y2, float* m_out, PcCoef c,
                            const float* k, long n_per_sample, long n, const float* init, const float* blend_noise,
                            const float* mask, float a, float s, long hw, hipStream_t stream);

// inception.hip: FID Inception-v3 pieces (general implicit-GEMM conv, 3x3 pools, global mean, TF1 bilinear preprocessing)
int sd_launch_inception_conv(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, int B, int Hin, int Win, int Cin,
                             int Cout, int kh, int kw, int stride, int ph, int pw, int ldy, int coff, int relu /* 2: SiLU */,
                             hipStream_t stream);
int sd_launch_inception_pool(const bf16_t* x, bf16_t* y, int B, int H, int W, int C, int stride, int pad, int avg, int ldy,
                             int coff, hipStream_t stream);
int sd_launch_inception_mean(const bf16_t* x, float* out, int B, int HW, int C, hipStream_t stream);
int sd_launch_inception_resize(const unsigned char* img, void* out, int B, int H, int W, int S, int out_fp32, hipStream_t stream);
