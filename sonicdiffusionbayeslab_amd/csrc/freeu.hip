// FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; diffusers apply_freeu / fourier_filter) on the inputs of one
// up-block resnet, ONE launch: the Fourier-filtered copy of the skip tensor and the copy of the hidden tensor whose first
// half of the channels is scaled by b.  bf16 NHWC in, bf16 NHWC out (new tensors: the inputs are never written).
//
// fourier_filter(x, threshold = 1, scale = s) multiplies the four modes {-1, 0} x {-1, 0} of every H x W plane by s and
// takes the real part.  No FFT is needed for four modes:
//   y[n] = x[n] + (s - 1) / (H W) * ( S0 + sum_k ( C_k cos a_k(n) + S_k sin a_k(n) ) ),   k in {(1,0), (0,1), (1,1)}
//   a_k(n) = 2 pi (k1 n1 / H + k2 n2 / W),  S0 = sum_m x[m],  C_k = sum_m x[m] cos a_k(m),  S_k = sum_m x[m] sin a_k(m)
// i.e. seven reductions and one elementwise pass per plane.  (The box is not symmetric: (-1, -1) is in it, (-1, +1) is not,
// hence the mixed term (1, 1) alone.)
//
// Work split.  Rows of one plane are C elements apart, so lanes run along the channels: a skip workgroup owns one sample
// and 32 channels (4 lanes x 16-byte loads), its 64 pixel slots stride over the plane.  Each thread keeps 7 x 8 fp32 sums;
// the 16 pixel slots of a wave are folded with shuffles, the 4 waves through LDS in a fixed order (deterministic).  The
// twiddles cos / sin (2 pi n1 / H), (2 pi n2 / W) are built once per workgroup in LDS (sincospif: exact argument
// reduction); the (1,1) pair is their angle sum.  The workgroups behind the skip ones copy / scale the hidden tensor.
//
// Rounding (tests/test_freeu_gpu.py, c_acc): a term x[m] t_k(m) t_k(n) of an output passes through at most SIX rounded
// factors -- the two table entries and the angle-sum combination of t_k(m), the fused multiply-add into the sum, the same
// combination for t_k(n) on the apply side and the scale (s - 1) / (H W) -- and through at most H W additions; everything
// is fp32 and the result is rounded once to bf16.  s = 1 gives x back value for value (the correction is an exact zero), and so
// does b = 1.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int FREEU_THREADS = 256;
constexpr int FREEU_MAX_SIDE = 128;
constexpr int FREEU_HID_VECS = 8;        // 16-byte vectors per thread of a hidden-tensor workgroup

__device__ __forceinline__ void unpack8(const u32x4 v, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[2 * j] = bflo(v[j]); f[2 * j + 1] = bfhi(v[j]); }
}

__global__ __launch_bounds__(FREEU_THREADS) void freeu_kernel(const bf16_t* __restrict__ hidden, const bf16_t* __restrict__ skip,
                                                              bf16_t* __restrict__ hidden_out, bf16_t* __restrict__ skip_out,
                                                              int H, int W, int Ch, int Cs, int skip_blocks, long hid_vecs,
                                                              float b, float g) {
    __shared__ float tw[4][FREEU_MAX_SIDE];          // cos, sin of 2 pi n1 / H; cos, sin of 2 pi n2 / W
    __shared__ float red[4][7][32];                  // [wave][sum][channel of the workgroup]
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= skip_blocks) {
        // ---- hidden: out = hidden, the first Ch / 2 channels times b (Ch % 32 == 0: a vector never straddles the half) ----
        const long v0 = ((long)blockIdx.x - skip_blocks) * (FREEU_THREADS * FREEU_HID_VECS) + tid;
        const int vpr = Ch / 8, half = Ch / 16;      // vectors per pixel row, ... of its scaled half
#pragma unroll
        for (int i = 0; i < FREEU_HID_VECS; ++i) {
            const long v = v0 + (long)i * FREEU_THREADS;
            if (v >= hid_vecs) break;
            u32x4 x = *(const u32x4*)(hidden + v * 8);
            if ((int)(v % vpr) < half) {
                float f[8];
                unpack8(x, f);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = pack2bf(f[2 * j] * b, f[2 * j + 1] * b);
            }
            *(u32x4*)(hidden_out + v * 8) = x;
        }
        return;
    }
    // ---- skip: one sample, 32 channels ----
    const int cgroups = Cs / 32;
    const int sample = blockIdx.x / cgroups, cg = blockIdx.x % cgroups;
    const int cl = tid & 3, slot = tid >> 2;         // channel lane (8 channels), pixel slot 0..63
    const int HW = H * W;
    if (tid < H) sincospif(2.0f * (float)tid / (float)H, &tw[1][tid], &tw[0][tid]);
    if (tid >= FREEU_MAX_SIDE && tid - FREEU_MAX_SIDE < W) {
        const int n = tid - FREEU_MAX_SIDE;
        sincospif(2.0f * (float)n / (float)W, &tw[3][n], &tw[2][n]);
    }
    __syncthreads();
    const long base = (long)sample * HW * Cs + (long)cg * 32 + cl * 8;
    float acc[7][8];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    for (int p = slot; p < HW; p += 64) {
        const int n1 = p / W, n2 = p - n1 * W;
        const float ch = tw[0][n1], sh = tw[1][n1], cw = tw[2][n2], sw = tw[3][n2];
        const float c11 = __builtin_fmaf(ch, cw, -(sh * sw)), s11 = __builtin_fmaf(sh, cw, ch * sw);
        float f[8];
        unpack8(*(const u32x4*)(skip + base + (long)p * Cs), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc[0][j] += f[j];
            acc[1][j] = __builtin_fmaf(f[j], ch, acc[1][j]);
            acc[2][j] = __builtin_fmaf(f[j], sh, acc[2][j]);
            acc[3][j] = __builtin_fmaf(f[j], cw, acc[3][j]);
            acc[4][j] = __builtin_fmaf(f[j], sw, acc[4][j]);
            acc[5][j] = __builtin_fmaf(f[j], c11, acc[5][j]);
            acc[6][j] = __builtin_fmaf(f[j], s11, acc[6][j]);
        }
    }
    // the 16 pixel slots of a wave (lane = slot-in-wave * 4 + channel lane), then the 4 waves in order
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = acc[k][j];
            v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
            acc[k][j] = v;
        }
    const int wave = tid >> 6, lane = tid & 63;
    if (lane < 4) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) red[wave][k][cl * 8 + j] = acc[k][j];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = cl * 8 + j;
            acc[k][j] = g * (((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c]);
        }
    for (int p = slot; p < HW; p += 64) {
        const int n1 = p / W, n2 = p - n1 * W;
        const float ch = tw[0][n1], sh = tw[1][n1], cw = tw[2][n2], sw = tw[3][n2];
        const float c11 = __builtin_fmaf(ch, cw, -(sh * sw)), s11 = __builtin_fmaf(sh, cw, ch * sw);
        const long off = base + (long)p * Cs;
        float f[8];
        unpack8(*(const u32x4*)(skip + off), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float d = acc[0][j];
            d = __builtin_fmaf(acc[1][j], ch, d);
            d = __builtin_fmaf(acc[2][j], sh, d);
            d = __builtin_fmaf(acc[3][j], cw, d);
            d = __builtin_fmaf(acc[4][j], sw, d);
            d = __builtin_fmaf(acc[5][j], c11, d);
            d = __builtin_fmaf(acc[6][j], s11, d);
            f[j] += d;
        }
        u32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = pack2bf(f[2 * j], f[2 * j + 1]);
        *(u32x4*)(skip_out + off) = y;
    }
}

}  // namespace

int sd_freeu_check(int B, int H, int W, int C_hidden, int C_skip, const char* who) {
    SD_REQUIRE(B >= 1 && B <= 4096, "%s: B=%d (1 .. 4096)", who, B);
    SD_REQUIRE(H >= 2 && W >= 2 && H <= FREEU_MAX_SIDE && W <= FREEU_MAX_SIDE, "%s: plane %dx%d (both sides in [2, %d])", who, H, W,
               FREEU_MAX_SIDE);
    SD_REQUIRE(C_hidden >= 32 && C_hidden % 32 == 0, "%s: C_hidden=%d (a multiple of 32)", who, C_hidden);
    SD_REQUIRE(C_skip >= 32 && C_skip % 32 == 0, "%s: C_skip=%d (a multiple of 32)", who, C_skip);
    return 0;
}

int sd_launch_freeu(const bf16_t* hidden, const bf16_t* skip, bf16_t* hidden_out, bf16_t* skip_out, int B, int H, int W, int C_hidden,
                    int C_skip, float b, float s, hipStream_t stream) {
    SD_REQUIRE(hidden && skip && hidden_out && skip_out, "freeu: null argument");
    if (sd_freeu_check(B, H, W, C_hidden, C_skip, "freeu")) return -1;
    SD_REQUIRE(b > 0.f && s > 0.f && b <= 3.0e38f && s <= 3.0e38f, "freeu: b=%g, s=%g (both must be finite and > 0)", b, s);
    SD_REQUIRE(hidden != hidden_out && skip != skip_out, "freeu: the outputs must be new tensors (the inputs are never modified)");
    const long hid_vecs = (long)B * H * W * (C_hidden / 8);
    const int skip_blocks = B * (C_skip / 32);
    const long per_block = (long)FREEU_THREADS * FREEU_HID_VECS;
    const long hid_blocks = (hid_vecs + per_block - 1) / per_block;
    const float g = (s - 1.0f) / (float)(H * W);
    hipLaunchKernelGGL(freeu_kernel, dim3((unsigned)(skip_blocks + hid_blocks)), dim3(FREEU_THREADS), 0, stream, hidden, skip,
                       hidden_out, skip_out, H, W, C_hidden, C_skip, skip_blocks, hid_vecs, b, g);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
