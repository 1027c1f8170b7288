// Small gfx950 kernels around the UNet body: timestep embedding (sinusoid + M=1 GEMV chain),
// conv_in (NCHW fp32 latents -> NHWC bf16, CFG batch duplication fused) and conv_out (NHWC bf16 ->
// NCHW fp32 noise prediction).  (The fused CFG-combine + scheduler.step update is sched.hip.)
#include "common.h"
#include "kernels.h"

namespace {

// ---- timestep sinusoid: flip_sin_to_cos=True, freq_shift=0 -> [cos(t f_k) | sin(t f_k)] ----
__device__ __forceinline__ float sinusoid_at(float t, int i, int dim) {
    const int half = dim / 2;
    const int k = i < half ? i : i - half;
    const float f = expf(-9.210340371976184f * (float)k / (float)half);  // ln(10000)
    const float e = t * f;
    return i < half ? cosf(e) : sinf(e);
}

__global__ void sinusoid_kernel(float t, float* __restrict__ out, int dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dim) return;
    out[i] = sinusoid_at(t, i, dim);
}

// the same plus a row (LCM-distilled UNets: TimestepEmbedding adds cond_proj(condition) to the sinusoid before linear_1;
// the row is that projection, computed once per condition by gemv_kernel)
__global__ void sinusoid_row_kernel(float t, const float* __restrict__ row, float* __restrict__ out, int dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dim) return;
    out[i] = sinusoid_at(t, i, dim) + row[i];
}

// ---- GEMV: one wave per output row --------------------------------------------------------
__global__ __launch_bounds__(256) void gemv_kernel(const float* __restrict__ x, const bf16_t* __restrict__ W,
                                                   const float* __restrict__ b, float* __restrict__ y, int N, int K,
                                                   int silu_in) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const bf16_t* wr = W + (long)n * K;
    float acc = 0.f;
    for (int ch = lane; ch < K / 8; ch += 64) {
        const u32x4 w = *(const u32x4*)(wr + ch * 8);
        const f32x4 x0 = *(const f32x4*)(x + ch * 8), x1 = *(const f32x4*)(x + ch * 8 + 4);
        float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        if (silu_in) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = silu_f(xv[j]);
        }
        acc += bflo(w[0]) * xv[0] + bfhi(w[0]) * xv[1] + bflo(w[1]) * xv[2] + bfhi(w[1]) * xv[3] +
               bflo(w[2]) * xv[4] + bfhi(w[2]) * xv[5] + bflo(w[3]) * xv[6] + bfhi(w[3]) * xv[7];
    }
    acc = wave_sum(acc);
    if (lane == 0) y[n] = acc + (b ? b[n] : 0.f);
}

// ---- conv_in: 3x3, Cin = 4, one block per output row, thread = 2 output channels ------------
// IMG (the AutoencoderKL encoder's entry, Cin = 3): x holds images in [0, 1] and the conv sees 2 x - 1, applied in the load
// to the pixels INSIDE the image -- the padding ring is zero in the preprocessed domain
template <int CIN, bool IMG = false>
__global__ void conv_in_kernel(const float* __restrict__ x, int Bsrc, const float* __restrict__ Wt,
                               const float* __restrict__ bias, bf16_t* __restrict__ y, int H, int W, int Cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* patch = (float*)smem;  // [CIN][3][W+2]
    const int yrow = blockIdx.x, b = blockIdx.y;
    const int bs = b % Bsrc;
    const int tid = threadIdx.x;
    const int PW = W + 2;
    for (int i = tid; i < CIN * 3 * PW; i += blockDim.x) {
        const int ci = i / (3 * PW), rem = i - ci * 3 * PW;
        const int dy = rem / PW, px = rem - dy * PW;
        const int iy = yrow + dy - 1, ix = px - 1;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            v = x[(((long)bs * CIN + ci) * H + iy) * W + ix];
            if (IMG) v = 2.f * v - 1.f;
        }
        patch[i] = v;
    }
    __syncthreads();
    const int co = tid * 2;
    if (co >= Cout) return;
    float w0[CIN * 9], w1[CIN * 9];
#pragma unroll
    for (int k = 0; k < CIN * 9; ++k) {
        w0[k] = Wt[k * Cout + co];
        w1[k] = Wt[k * Cout + co + 1];
    }
    const float b0 = bias[co], b1 = bias[co + 1];
    bf16_t* yr = y + (((long)b * H + yrow) * W) * Cout + co;
    for (int ox = 0; ox < W; ++ox) {
        float a0 = b0, a1 = b1;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = patch[(ci * 3 + dy) * PW + ox + dx];
                    a0 += v * w0[ci * 9 + dy * 3 + dx];
                    a1 += v * w1[ci * 9 + dy * 3 + dx];
                }
        *(unsigned*)(yr + (long)ox * Cout) = pack2bf(a0, a1);
    }
}

// ---- conv_in of an inpainting UNet: 3x3, Cin = 9 = [4 latent | 1 mask | 4 masked-image latent] channels ------------------
// Channels 0..3 come from the latents (batch index modulo Bsrc, as above), channels 4..8 from the condition the handle stores
// once per call ([Bcond][5][H][W] fp32, batch index modulo Bcond): the concatenated input exists only as this block's LDS
// patch.  One block per output row, thread = ONE output channel: 81 weights per channel live in registers (two channels per
// thread, as the 4-channel form has, would be 162).  The sum runs in the 4-channel kernel's order (bias, then ci, dy, dx), so
// with zero weights on channels 4..8 it is that kernel's sum followed by 45 additions of zero.
constexpr int INPAINT_CIN = 9, INPAINT_COND = 5;

// (launched with Cout threads rounded up to whole waves, at most 1024: the bound keeps it within 128 VGPRs)
__global__ __launch_bounds__(1024) void conv_in_cond_kernel(const float* __restrict__ x, int Bsrc,
                                                            const float* __restrict__ cond, int Bcond,
                                                            const float* __restrict__ Wt, const float* __restrict__ bias,
                                                            bf16_t* __restrict__ y, int H, int W, int Cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* patch = (float*)smem;  // [9][3][W+2]
    constexpr int CL = INPAINT_CIN - INPAINT_COND;
    const int yrow = blockIdx.x, b = blockIdx.y;
    const int bs = b % Bsrc, bc = b % Bcond;
    const int tid = threadIdx.x;
    const int PW = W + 2;
    for (int i = tid; i < INPAINT_CIN * 3 * PW; i += blockDim.x) {
        const int ci = i / (3 * PW), rem = i - ci * 3 * PW;
        const int dy = rem / PW, px = rem - dy * PW;
        const int iy = yrow + dy - 1, ix = px - 1;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W)
            v = ci < CL ? x[(((long)bs * CL + ci) * H + iy) * W + ix]
                        : cond[(((long)bc * INPAINT_COND + (ci - CL)) * H + iy) * W + ix];
        patch[i] = v;
    }
    __syncthreads();
    const int co = tid;
    if (co >= Cout) return;
    float w0[INPAINT_CIN * 9];
#pragma unroll
    for (int k = 0; k < INPAINT_CIN * 9; ++k) w0[k] = Wt[k * Cout + co];
    const float b0 = bias[co];
    bf16_t* yr = y + (((long)b * H + yrow) * W) * Cout + co;
    for (int ox = 0; ox < W; ++ox) {
        float a0 = b0;
#pragma unroll
        for (int ci = 0; ci < INPAINT_CIN; ++ci)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) a0 += patch[(ci * 3 + dy) * PW + ox + dx] * w0[ci * 9 + dy * 3 + dx];
        yr[(long)ox * Cout] = f2bf(a0);
    }
}

// ---- conv_in of a ControlNet: the 4-channel conv above plus an addend (the conditioning embedding the handle stores once
// per call, NHWC bf16 [Badd][H][W][Cout], batch index modulo Badd) in the SAME launch: the conv sum in the order of
// conv_in_kernel, the addend added in fp32, ONE bf16 rounding.  Thread = 2 output channels as above; the four lanes of a
// quad hold 8 consecutive channels, exchange their packed pairs and the quad's first lane stores 16 bytes.
// (launched with Cout / 2 threads rounded up to whole waves, at most 1024: the bound keeps it within 128 VGPRs)
__global__ __launch_bounds__(1024) void conv_in_add_kernel(const float* __restrict__ x, int Bsrc, const bf16_t* __restrict__ addend, int Badd,
                                   const float* __restrict__ Wt, const float* __restrict__ bias, bf16_t* __restrict__ y,
                                   int H, int W, int Cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* patch = (float*)smem;  // [4][3][W+2]
    constexpr int CIN = 4;
    const int yrow = blockIdx.x, b = blockIdx.y;
    const int bs = b % Bsrc, ba = b % Badd;
    const int tid = threadIdx.x;
    const int PW = W + 2;
    for (int i = tid; i < CIN * 3 * PW; i += blockDim.x) {
        const int ci = i / (3 * PW), rem = i - ci * 3 * PW;
        const int dy = rem / PW, px = rem - dy * PW;
        const int iy = yrow + dy - 1, ix = px - 1;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[(((long)bs * CIN + ci) * H + iy) * W + ix];
        patch[i] = v;
    }
    __syncthreads();
    const int co = tid * 2;
    if (co >= Cout) return;          // (Cout % 8 == 0: a quad is inside or outside as a whole)
    float w0[CIN * 9], w1[CIN * 9];
#pragma unroll
    for (int k = 0; k < CIN * 9; ++k) {
        w0[k] = Wt[k * Cout + co];
        w1[k] = Wt[k * Cout + co + 1];
    }
    const float b0 = bias[co], b1 = bias[co + 1];
    const bf16_t* ar = addend + (((long)ba * H + yrow) * W) * Cout + co;
    bf16_t* yr = y + (((long)b * H + yrow) * W) * Cout + co;
    const int lane = tid & 63, q0 = lane & ~3;
    for (int ox = 0; ox < W; ++ox) {
        float a0 = b0, a1 = b1;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float v = patch[(ci * 3 + dy) * PW + ox + dx];
                    a0 += v * w0[ci * 9 + dy * 3 + dx];
                    a1 += v * w1[ci * 9 + dy * 3 + dx];
                }
        const unsigned ad = *(const unsigned*)(ar + (long)ox * Cout);
        const int p = (int)pack2bf(a0 + bflo(ad), a1 + bfhi(ad));
        u32x4 v;
        v[0] = (unsigned)__shfl(p, q0); v[1] = (unsigned)__shfl(p, q0 + 1);
        v[2] = (unsigned)__shfl(p, q0 + 2); v[3] = (unsigned)__shfl(p, q0 + 3);
        if ((lane & 3) == 0) *(u32x4*)(yr + (long)ox * Cout) = v;
    }
}

// ---- ControlNet residuals into the UNet's skip path: x <- bf16(float(x) + scale * float(r)) in place over up to 16 segments
// in ONE launch.  The table rides in the kernel arguments; a block owns RES_ADD_BLOCK consecutive elements of one segment
// (first_block[k] = the first block of segment k), a thread one 16-byte vector of x and of r; the last vector of a segment
// whose length is no multiple of 8 goes element by element.
constexpr int RES_ADD_MAX = SD_MAX_RES_SEGMENTS, RES_ADD_BLOCK = 256 * 8;
struct ResAddArgs {
    bf16_t* x[RES_ADD_MAX];
    const bf16_t* r[RES_ADD_MAX];
    long n[RES_ADD_MAX];
    int first_block[RES_ADD_MAX];
    int nseg;
    float scale;
};
__global__ __launch_bounds__(256) void residual_add_kernel(ResAddArgs a) {
    const int blk = (int)blockIdx.x;
    bf16_t* x = a.x[0];
    const bf16_t* r = a.r[0];
    long n = a.n[0];
    int first = 0;
#pragma unroll
    for (int k = 1; k < RES_ADD_MAX; ++k)
        if (k < a.nseg && blk >= a.first_block[k]) { x = a.x[k]; r = a.r[k]; n = a.n[k]; first = a.first_block[k]; }
    const long i0 = ((long)(blk - first) * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    if (i0 + 8 <= n) {
        u32x4 xv = *(const u32x4*)(x + i0);
        const u32x4 rv = *(const u32x4*)(r + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = pack2bf(bflo(xv[j]) + a.scale * bflo(rv[j]), bfhi(xv[j]) + a.scale * bfhi(rv[j]));
        *(u32x4*)(x + i0) = xv;
    } else {
        for (long i = i0; i < n; ++i) x[i] = f2bf(bf2f(x[i]) + a.scale * bf2f(r[i]));
    }
}

// fp32 NCHW [B][C][hw] -> bf16 NHWC [B][hw][C] (the ControlNet's control image, once per call; C = 3)
__global__ void nchw_to_nhwc_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int C, long hw, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long b = i / hw, p = i - b * hw;
    for (int c = 0; c < C; ++c) dst[i * C + c] = f2bf(src[(b * C + c) * hw + p]);
}

// the five constant channels of a call, packed once: cond[b] = [mask[b] | masked_latents[b]] ([B][5][hw] fp32)
__global__ void inpaint_cond_pack_kernel(const float* __restrict__ mask, const float* __restrict__ masked,
                                         float* __restrict__ cond, long hw4, long n4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const long per = INPAINT_COND * hw4;
    const long b = i / per, j = i - b * per;
    ((f32x4*)cond)[i] = j < hw4 ? ((const f32x4*)mask)[b * hw4 + j]
                                : ((const f32x4*)masked)[b * (per - hw4) + (j - hw4)];
}

// ---- inpainting, pixel space: masked image and latent mask in one launch ----------------------------------------------
// thread = 4 pixels of one row.  masked = m >= 0.5 ? 0.5 : img  (the encoder's [0, 1] domain: 2 * 0.5 - 1 is exactly 0);
// latent mask (i, j) = (m(8 i, 8 j) >= 0.5) as fp32 0 / 1 (nearest resize to H/8 x W/8), written by the thread that holds
// that pixel.
__global__ void inpaint_prepare_kernel(const float* __restrict__ img, const float* __restrict__ mask,
                                       float* __restrict__ masked, float* __restrict__ lmask, int H, int W, long n4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int W4 = W / 4;
    const long hw4 = (long)H * W4;
    const long b = i / hw4, p = i - b * hw4;
    const int yy = (int)(p / W4), x4 = (int)(p - (long)yy * W4);
    const f32x4 m = ((const f32x4*)mask)[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f32x4 v = ((const f32x4*)img)[(b * 3 + c) * hw4 + p];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = m[j] >= 0.5f ? 0.5f : v[j];
        ((f32x4*)masked)[(b * 3 + c) * hw4 + p] = v;
    }
    if ((yy & 7) == 0 && (x4 & 1) == 0)
        lmask[(b * (H / 8) + yy / 8) * (W / 8) + x4 / 2] = m[0] >= 0.5f ? 1.f : 0.f;
}

// ---- conv_out: 3x3, Cout <= 4, one wave per output pixel ------------------------------------
__global__ __launch_bounds__(256) void conv_out_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ Wp,
                                                       const float* __restrict__ bias, float* __restrict__ y, int B,
                                                       int H, int W, int Cin, int Cout) {
    const int lane = threadIdx.x & 63;
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long npix = (long)B * H * W;
    if (pix >= npix) return;
    const int b = (int)(pix / (H * W));
    const int rem = (int)(pix - (long)b * H * W);
    const int oy = rem / W, ox = rem - oy * W;
    const int nchunks = Cin / 8;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = lane; ch < nchunks; ch += 64) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const u32x4 v = *(const u32x4*)(x + (((long)b * H + iy) * W + ix) * Cin + ch * 8);
            const float f[8] = {bflo(v[0]), bfhi(v[0]), bflo(v[1]), bfhi(v[1]),
                                bflo(v[2]), bfhi(v[2]), bflo(v[3]), bfhi(v[3])};
#pragma unroll
            for (int co = 0; co < 4; ++co) {
                if (co >= Cout) break;
                const u32x4 w = *(const u32x4*)(Wp + ((long)co * 9 + tap) * Cin + ch * 8);
                acc[co] += f[0] * bflo(w[0]) + f[1] * bfhi(w[0]) + f[2] * bflo(w[1]) + f[3] * bfhi(w[1]) +
                           f[4] * bflo(w[2]) + f[5] * bfhi(w[2]) + f[6] * bflo(w[3]) + f[7] * bfhi(w[3]);
            }
        }
    }
#pragma unroll
    for (int co = 0; co < 4; ++co) acc[co] = wave_sum(acc[co]);
    const float mine = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
    if (lane < Cout) y[(((long)b * Cout + lane) * H + oy) * W + ox] = mine + bias[lane];
}

// ---- conv_out on the matrix cores: D[cout (16 rows, <= 4 live)][16 pixels] += W[cout][k] . X[pixel][k], k = (tap, channel) ----
// The wave-per-pixel kernel above re-reads the 4 x 9 x Cin weights for every pixel (23 KB of L1 traffic per pixel at
// Cin = 320: 133 us for the 64x64 UNet output).  Here the weights sit in LDS once per workgroup, a wave owns T x 16 consecutive
// pixels (T MFMA tiles) and streams their 9 shifted input rows straight from global memory into the B operand
// (lane = (pixel, 8-channel group): 16 contiguous bytes each); out-of-image taps are zeroed after an unconditional load.
template <int T>
__global__ __launch_bounds__(256) void conv_out_mfma_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ Wp,
                                                            const float* __restrict__ bias, float* __restrict__ y, int B,
                                                            int H, int W, int Cin, int Cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // W rows 0..3: [4][9 * Cin] bf16 (rows >= Cout zero)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = 9 * Cin;
    for (int i = tid; i < 4 * (K / 8); i += 256) {
        const int row = i / (K / 8);
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < Cout) v = *(const u32x4*)(Wp + (long)i * 8);
        *(u32x4*)(smem + (long)i * 16) = v;
    }
    __syncthreads();
    const int l15 = lane & 15, kg = lane >> 4;
    const long npix = (long)B * H * W;
    const long pix0 = ((long)blockIdx.x * 4 + wave) * (16 * T);
    if (pix0 >= npix) return;
    int oy[T], ox[T];
    long base[T];
    bool valid[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const long pp = pix0 + t * 16 + l15;
        valid[t] = pp < npix;
        const long pc = valid[t] ? pp : npix - 1;
        const int b = (int)(pc / (H * W));
        const int rem = (int)(pc - (long)b * H * W);
        oy[t] = rem / W;
        ox[t] = rem - oy[t] * W;
        base[t] = (long)b * H * W;
    }
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* wrow = smem + ((long)(l15 & 3) * K + kg * 8) * 2;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const bf16_t* src[T];
        bool ok[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int iy = oy[t] + tap / 3 - 1, ix = ox[t] + tap % 3 - 1;
            ok[t] = valid[t] && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
            src[t] = x + (base[t] + (long)cy * W + cx) * Cin + kg * 8;
        }
#pragma unroll 10
        for (int c0 = 0; c0 < Cin; c0 += 32) {
            bf16x8 wf = *(const bf16x8*)(wrow + (tap * Cin + c0) * 2);
            wf = l15 < 4 ? wf : zero8;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                bf16x8 xf = *(const bf16x8*)(src[t] + c0);
                xf = ok[t] ? xf : zero8;
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[t], 0, 0, 0);
            }
        }
    }
    if (kg == 0) {          // lanes 0..15: rows (output channels) 0..3 of pixel l15
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (!valid[t]) continue;
            const long b = base[t] / ((long)H * W);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < Cout) y[((b * Cout + j) * H + oy[t]) * W + ox[t]] = acc[t][j] + bias[j];
        }
    }
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long n4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = ((const f32x4*)src)[i];
    u32x2 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
    ((u32x2*)dst)[i] = o;
}

// ---- AutoencoderKL encoder exit: conv_out 3x3 Cin -> 8 and quant_conv 1x1 8 -> 8, one wave per latent pixel ------------
// The 3x3 contracts bf16 operands into fp32 (lane = 8-channel chunk, as conv_out_kernel).  The butterfly reduction leaves all
// 8 sums in every lane, so lane co < 8 applies row co of quant_conv to them in fp32 and stores moment channel co.
__global__ __launch_bounds__(256) void vae_enc_out_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ Wp,
                                                          const float* __restrict__ bias, const float* __restrict__ Wq,
                                                          const float* __restrict__ bq, float* __restrict__ y, int B, int H,
                                                          int W, int Cin) {
    const int lane = threadIdx.x & 63;
    const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long npix = (long)B * H * W;
    if (pix >= npix) return;
    const int b = (int)(pix / (H * W));
    const int rem = (int)(pix - (long)b * H * W);
    const int oy = rem / W, ox = rem - oy * W;
    const int nchunks = Cin / 8;
    float acc[8];
#pragma unroll
    for (int co = 0; co < 8; ++co) acc[co] = 0.f;
    for (int ch = lane; ch < nchunks; ch += 64) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const u32x4 v = *(const u32x4*)(x + (((long)b * H + iy) * W + ix) * Cin + ch * 8);
            const float f[8] = {bflo(v[0]), bfhi(v[0]), bflo(v[1]), bfhi(v[1]),
                                bflo(v[2]), bfhi(v[2]), bflo(v[3]), bfhi(v[3])};
#pragma unroll
            for (int co = 0; co < 8; ++co) {
                const u32x4 w = *(const u32x4*)(Wp + ((long)co * 9 + tap) * Cin + ch * 8);
                acc[co] += f[0] * bflo(w[0]) + f[1] * bfhi(w[0]) + f[2] * bflo(w[1]) + f[3] * bfhi(w[1]) +
                           f[4] * bflo(w[2]) + f[5] * bfhi(w[2]) + f[6] * bflo(w[3]) + f[7] * bfhi(w[3]);
            }
        }
    }
#pragma unroll
    for (int co = 0; co < 8; ++co) acc[co] = wave_sum(acc[co]) + bias[co];
    if (lane < 8) {
        float q = bq[lane];
#pragma unroll
        for (int c = 0; c < 8; ++c) q += Wq[lane * 8 + c] * acc[c];
        y[(((long)b * 8 + lane) * H + oy) * W + ox] = q;
    }
}

// ---- DiagonalGaussianDistribution.sample() / .mode() times the scaling factor: one elementwise fp32 launch ----------
__global__ void vae_posterior_kernel(const float* __restrict__ moments, const float* __restrict__ noise, float scale,
                                     float* __restrict__ z, int C, long hw, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long chw = (long)C * hw;
    const long b = i / chw, r = i - b * chw;
    const float mean = moments[b * 2 * chw + r];
    float v = mean;
    if (noise) {
        const float lv = fminf(fmaxf(moments[b * 2 * chw + chw + r], -30.f), 20.f);
        v = mean + expf(0.5f * lv) * noise[i];
    }
    z[i] = scale * v;
}

__global__ void pqconv_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                              float* __restrict__ y, int B, int HW, float in_scale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * HW) return;
    const int b = (int)(i / HW);
    const long p = i - (long)b * HW;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = x[((long)b * 4 + c) * HW + p] * in_scale;
#pragma unroll
    for (int co = 0; co < 4; ++co)
        y[((long)b * 4 + co) * HW + p] = bias[co] + W[co * 4 + 0] * v[0] + W[co * 4 + 1] * v[1] + W[co * 4 + 2] * v[2] + W[co * 4 + 3] * v[3];
}

}  // namespace

int sd_launch_pqconv(const float* x, const float* W, const float* bias, float* y, int B, int HW, float in_scale,
                     hipStream_t stream) {
    SD_REQUIRE(x && W && bias && y && B > 0 && HW > 0, "pqconv: bad operand");
    const long n = (long)B * HW;
    hipLaunchKernelGGL(pqconv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, W, bias, y, B, HW, in_scale);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_vae_enc_out(const bf16_t* x, const bf16_t* Wp, const float* bias, const float* Wq, const float* bq, float* y,
                          int B, int H, int W, int Cin, hipStream_t stream) {
    SD_REQUIRE(x && Wp && bias && Wq && bq && y, "vae_enc_out: null operand");
    SD_REQUIRE(Cin % 8 == 0 && Cin > 0 && B > 0 && H > 0 && W > 0, "vae_enc_out: B=%d H=%d W=%d Cin=%d", B, H, W, Cin);
    const long npix = (long)B * H * W;
    hipLaunchKernelGGL(vae_enc_out_kernel, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, stream, x, Wp, bias, Wq, bq, y, B, H,
                       W, Cin);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_vae_posterior(const float* moments, const float* noise, float scale, float* z, int B, int C, long hw,
                            hipStream_t stream) {
    SD_REQUIRE(moments && z && B > 0 && C > 0 && hw > 0, "vae_posterior: bad operand");
    const long n = (long)B * C * hw;
    hipLaunchKernelGGL(vae_posterior_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, moments, noise, scale, z, C,
                       hw, n);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_f32_to_bf16(const float* src, bf16_t* dst, long n, hipStream_t stream) {
    SD_REQUIRE(src && dst && n > 0 && n % 4 == 0, "f32_to_bf16: n=%ld must be a positive multiple of 4", n);
    const long n4 = n / 4;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, src, dst, n4);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_timestep_sinusoid(float t, float* out, int dim, hipStream_t stream) {
    SD_REQUIRE(out && dim > 0 && dim % 2 == 0, "sinusoid: bad dim %d", dim);
    hipLaunchKernelGGL(sinusoid_kernel, dim3((dim + 255) / 256), dim3(256), 0, stream, t, out, dim);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_timestep_sinusoid_row(float t, const float* row, float* out, int dim, hipStream_t stream) {
    SD_REQUIRE(row && out && dim > 0 && dim % 2 == 0, "sinusoid_row: bad operands (dim %d)", dim);
    hipLaunchKernelGGL(sinusoid_row_kernel, dim3((dim + 255) / 256), dim3(256), 0, stream, t, row, out, dim);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_gemv(const float* x, const bf16_t* W, const float* b, float* y, int N, int K, int silu_in,
                   hipStream_t stream) {
    SD_REQUIRE(x && W && y, "gemv: null operand");
    SD_REQUIRE(K % 8 == 0 && N > 0, "gemv: K=%d must be a multiple of 8", K);
    hipLaunchKernelGGL(gemv_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, x, W, b, y, N, K, silu_in);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

// out[b][h*S + j][c] = (j < L and c in head h) ? scale * kv[b*L + j][col_off + c] : 0   (kv rows are [K | V], 2C wide; S key
// slots per head: 80 for the prompt)
__global__ void xattn_expand_kernel(const bf16_t* __restrict__ kv, bf16_t* __restrict__ out, int L, int C, int NH,
                                    int col_off, float scale, int S) {
    const int row = blockIdx.x;                       // b * NH * S + h * S + j
    const int j = row % S, h = (row / S) % NH, b = row / (S * NH);
    const int d = C / NH;
    const bf16_t* src = kv + ((long)b * L + (j < L ? j : 0)) * 2 * C + col_off;
    bf16_t* dst = out + (long)row * C;
    for (int c = threadIdx.x * 2; c < C; c += blockDim.x * 2) {
        unsigned v = 0;
        if (j < L && c / d == h) {                    // d is even: a channel pair never straddles heads
            const unsigned u = *(const unsigned*)(src + c);
            v = pack2bf(bflo(u) * scale, bfhi(u) * scale);
        }
        *(unsigned*)(dst + c) = v;
    }
}

// dst[b][c][r] = src[b][r][c]  (bf16, 32x32 tiles through LDS)
__global__ void transpose_bf16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int R, int Cc, int perm16) {
    __shared__ bf16_t tile[32][33];
    const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;        // 32 x 8
    const bf16_t* s = src + (long)b * R * Cc;
    bf16_t* d = dst + (long)b * R * Cc;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && c0 + tx < Cc) tile[i][tx] = s[(long)(r0 + i) * Cc + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < Cc && r0 + tx < R) {
            int rr = r0 + tx;
            if (perm16) rr = (rr & ~12) | ((rr & 4) << 1) | ((rr & 8) >> 1);
            d[(long)(c0 + i) * R + rr] = tile[tx][i];
        }
}

int sd_launch_transpose_bf16(const bf16_t* src, bf16_t* dst, int B, int R, int Cc, hipStream_t stream, int perm16) {
    SD_REQUIRE(src && dst && B > 0 && B <= 65535 && R > 0 && Cc > 0, "transpose: B=%d R=%d C=%d", B, R, Cc);
    SD_REQUIRE(!perm16 || R % 16 == 0, "transpose: the 16-group permutation needs R=%d to be a multiple of 16", R);
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3((Cc + 31) / 32, (R + 31) / 32, B), dim3(256), 0, stream, src, dst, R, Cc,
                       perm16);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

// dst[b][R / RT][K / 32][RT][32] = src[b][R][K] (bf16): every (row tile, 32-column slice) becomes RT contiguous 64-byte
// rows, so that a 16-row x 64-byte LDS-DMA piece of the fused cross-attention kernel is ONE contiguous KiB (8 full cache
// lines) instead of 16 half lines at the row stride.  One 16-byte chunk per thread.
__global__ void retile32_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int R, int K, int RT) {
    const long per = (long)R * K / 8;                            // 16-byte chunks per sample
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const int b = blockIdx.y;
    const int kc = (int)(i % (K / 8)), row = (int)(i / (K / 8));  // source chunk (row, 8 columns)
    const int ks = kc >> 2, cc = kc & 3;                          // 32-column slice, chunk inside it
    const long d = ((((long)(row / RT) * (K / 32) + ks) * RT + row % RT) * 4 + cc);
    const u32x4 v = *(const u32x4*)(src + ((long)b * R * K) + (long)row * K + kc * 8);
    *(u32x4*)(dst + ((long)b * R * K) + d * 8) = v;
}

// dst[r][i] = src[i] for r < rep: the prompt-independent prefix of a CFG forward is computed once per latent and handed
// to the conditional / unconditional halves (16-byte vectors; n16 = bytes / 16 of ONE copy)
__global__ void replicate_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, long n16, int rep) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n16) return;
    const u32x4 v = src[i];
    for (int r = 0; r < rep; ++r) dst[(long)r * n16 + i] = v;
}

int sd_launch_replicate(const void* src, void* dst, long bytes, int rep, hipStream_t stream) {
    SD_REQUIRE(src && dst && bytes > 0 && bytes % 16 == 0 && rep >= 1, "replicate: bytes=%ld rep=%d", bytes, rep);
    const long n16 = bytes / 16;
    hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, stream, (const u32x4*)src, (u32x4*)dst,
                       n16, rep);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_retile32(const bf16_t* src, bf16_t* dst, int B, int R, int K, int RT, hipStream_t stream) {
    SD_REQUIRE(src && dst && B > 0 && B <= 65535 && K % 32 == 0 && RT > 0 && R % RT == 0, "retile32: B=%d R=%d K=%d RT=%d", B, R, K, RT);
    const long per = (long)R * K / 8;
    hipLaunchKernelGGL(retile32_kernel, dim3((unsigned)((per + 255) / 256), B), dim3(256), 0, stream, src, dst, R, K, RT);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_xattn_expand(const bf16_t* kv, bf16_t* out, int B, int L, int C, int NH, int col_off, float scale,
                           hipStream_t stream, int slots) {
    SD_REQUIRE(kv && out && B > 0 && L > 0 && slots > 0 && L <= slots && NH > 0 && C % NH == 0 && (C / NH) % 2 == 0,
               "xattn_expand: B=%d L=%d C=%d heads=%d slots=%d", B, L, C, NH, slots);
    hipLaunchKernelGGL(xattn_expand_kernel, dim3(B * NH * slots), dim3(128), 0, stream, kv, out, L, C, NH, col_off, scale, slots);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_conv_in(const float* x, int Bsrc, const float* Wt, const float* bias, bf16_t* y, int B, int H, int W,
                      int Cin, int Cout, hipStream_t stream) {
    SD_REQUIRE(x && Wt && bias && y, "conv_in: null operand");
    SD_REQUIRE(Cin == 4, "conv_in: Cin=%d (only 4 is built)", Cin);
    SD_REQUIRE(Cout % 2 == 0 && Cout / 2 <= 1024, "conv_in: Cout=%d", Cout);
    SD_REQUIRE(Bsrc > 0 && B > 0 && B % Bsrc == 0, "conv_in: batch %d not a multiple of source batch %d", B, Bsrc);
    const int threads = (Cout / 2 + 63) / 64 * 64;
    const size_t smem = (size_t)Cin * 3 * (W + 2) * sizeof(float);
    hipLaunchKernelGGL((conv_in_kernel<4>), dim3(H, B), dim3(threads), smem, stream, x, Bsrc, Wt, bias, y, H, W, Cout);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_conv_in_cond(const float* x, int Bsrc, const float* cond, int Bcond, const float* Wt, const float* bias,
                           bf16_t* y, int B, int H, int W, int Cout, hipStream_t stream) {
    SD_REQUIRE(x && cond && Wt && bias && y, "conv_in_cond: null operand");
    SD_REQUIRE(Cout > 0 && Cout <= 1024, "conv_in_cond: Cout=%d", Cout);
    SD_REQUIRE(Bsrc > 0 && Bcond > 0 && B > 0 && B <= 65535 && B % Bsrc == 0 && B % Bcond == 0,
               "conv_in_cond: batch %d not a multiple of the latent batch %d and the condition batch %d", B, Bsrc, Bcond);
    SD_REQUIRE(H > 0 && W > 0, "conv_in_cond: H=%d W=%d", H, W);
    const int threads = (Cout + 63) / 64 * 64;
    const size_t smem = (size_t)INPAINT_CIN * 3 * (W + 2) * sizeof(float);
    SD_REQUIRE(smem <= 64 * 1024, "conv_in_cond: W=%d needs %zu bytes of LDS (64 KiB per workgroup)", W, smem);
    hipLaunchKernelGGL(conv_in_cond_kernel, dim3(H, B), dim3(threads), smem, stream, x, Bsrc, cond, Bcond, Wt, bias, y, H, W,
                       Cout);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_conv_in_add(const float* x, int Bsrc, const bf16_t* addend, int Badd, const float* Wt, const float* bias,
                          bf16_t* y, int B, int H, int W, int Cout, hipStream_t stream) {
    SD_REQUIRE(x && addend && Wt && bias && y, "conv_in_add: null operand");
    SD_REQUIRE(Cout > 0 && Cout % 8 == 0 && Cout <= 2048, "conv_in_add: Cout=%d (a multiple of 8, at most 2048)", Cout);
    SD_REQUIRE(Bsrc > 0 && Badd > 0 && B > 0 && B <= 65535 && B % Bsrc == 0 && B % Badd == 0,
               "conv_in_add: batch %d not a multiple of the latent batch %d and the addend batch %d", B, Bsrc, Badd);
    SD_REQUIRE(H > 0 && W > 0, "conv_in_add: H=%d W=%d", H, W);
    SD_REQUIRE((((uintptr_t)addend | (uintptr_t)y) & 15) == 0, "conv_in_add: addend and y must be 16-byte aligned");
    const int threads = (Cout / 2 + 63) / 64 * 64;
    const size_t smem = (size_t)4 * 3 * (W + 2) * sizeof(float);
    SD_REQUIRE(smem <= 64 * 1024, "conv_in_add: W=%d needs %zu bytes of LDS (64 KiB per workgroup)", W, smem);
    hipLaunchKernelGGL(conv_in_add_kernel, dim3(H, B), dim3(threads), smem, stream, x, Bsrc, addend, Badd, Wt, bias, y, H, W, Cout);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_residual_add(bf16_t* const* x, const bf16_t* const* r, const long* n, int nseg, float scale, hipStream_t stream) {
    SD_REQUIRE(x && r && n && nseg >= 1 && nseg <= RES_ADD_MAX, "residual_add: %d segments (1 .. %d)", nseg, RES_ADD_MAX);
    SD_REQUIRE(scale == scale && fabsf(scale) <= 1e4f, "residual_add: scale %g", scale);
    ResAddArgs a;
    long blocks = 0;
    for (int k = 0; k < RES_ADD_MAX; ++k) {
        const int s = k < nseg ? k : 0;
        SD_REQUIRE(x[s] && r[s] && n[s] > 0, "residual_add: segment %d is empty or null", s);
        SD_REQUIRE((((uintptr_t)x[s] | (uintptr_t)r[s]) & 15) == 0, "residual_add: segment %d is not 16-byte aligned", s);
        a.x[k] = x[s]; a.r[k] = r[s]; a.n[k] = n[s];
        a.first_block[k] = (int)blocks;
        if (k < nseg) blocks += (n[s] + RES_ADD_BLOCK - 1) / RES_ADD_BLOCK;
        SD_REQUIRE(blocks < (1L << 31), "residual_add: too many elements");
    }
    a.nseg = nseg; a.scale = scale;
    hipLaunchKernelGGL(residual_add_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_nchw_to_nhwc_bf16(const float* src, bf16_t* dst, int B, int C, long hw, hipStream_t stream) {
    SD_REQUIRE(src && dst && B > 0 && C > 0 && hw > 0, "nchw_to_nhwc_bf16: B=%d C=%d hw=%ld", B, C, hw);
    const long total = (long)B * hw;
    SD_REQUIRE((total + 255) / 256 < (1L << 31), "nchw_to_nhwc_bf16: too many pixels");
    hipLaunchKernelGGL(nchw_to_nhwc_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, dst, C, hw, total);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_inpaint_cond_pack(const float* mask, const float* masked, float* cond, int B, long hw, hipStream_t stream) {
    SD_REQUIRE(mask && masked && cond, "inpaint_cond_pack: null operand");
    SD_REQUIRE(B > 0 && hw > 0 && hw % 4 == 0, "inpaint_cond_pack: B=%d hw=%ld (a positive multiple of 4)", B, hw);
    const long n4 = (long)B * INPAINT_COND * (hw / 4);
    hipLaunchKernelGGL(inpaint_cond_pack_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, mask, masked, cond,
                       hw / 4, n4);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_inpaint_prepare(const float* img, const float* mask, float* masked, float* lmask, int B, int H, int W,
                              hipStream_t stream) {
    SD_REQUIRE(img && mask && masked && lmask, "inpaint_prepare: null operand");
    SD_REQUIRE(B > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0,
               "inpaint_prepare: B=%d H=%d W=%d (H and W must be positive multiples of 8)", B, H, W);
    const long n4 = (long)B * H * (W / 4);
    hipLaunchKernelGGL(inpaint_prepare_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, img, mask, masked,
                       lmask, H, W, n4);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_conv_in_image(const float* img, const float* Wt, const float* bias, bf16_t* y, int B, int H, int W, int Cout,
                            hipStream_t stream) {
    SD_REQUIRE(img && Wt && bias && y, "conv_in_image: null operand");
    SD_REQUIRE(Cout % 2 == 0 && Cout / 2 <= 1024, "conv_in_image: Cout=%d", Cout);
    SD_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && W <= 4096, "conv_in_image: B=%d H=%d W=%d", B, H, W);
    const int threads = (Cout / 2 + 63) / 64 * 64;
    const size_t smem = (size_t)3 * 3 * (W + 2) * sizeof(float);       // (36.9 KiB at the widest image, 1024)
    SD_REQUIRE(smem <= 64 * 1024, "conv_in_image: W=%d needs %zu bytes of LDS (64 KiB per workgroup)", W, smem);
    hipLaunchKernelGGL((conv_in_kernel<3, true>), dim3(H, B), dim3(threads), smem, stream, img, B, Wt, bias, y, H, W, Cout);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_conv_out(const bf16_t* x, const bf16_t* Wp, const float* bias, float* y, int B, int H, int W, int Cin,
                       int Cout, hipStream_t stream) {
    SD_REQUIRE(x && Wp && bias && y, "conv_out: null operand");
    SD_REQUIRE(Cin % 8 == 0 && Cout >= 1 && Cout <= 4, "conv_out: Cin=%d Cout=%d", Cin, Cout);
    const long npix = (long)B * H * W;
    static const bool no_mfma = getenv("SD_CONV_OUT_VALU") != nullptr;
    const size_t smem = (size_t)4 * 9 * Cin * 2;
    if (!no_mfma && Cin % 32 == 0 && smem <= 64 * 1024) {
        static const int tiles = getenv("SD_CONV_OUT_TILES") ? atoi(getenv("SD_CONV_OUT_TILES")) : 1;
        if (tiles == 2)
            hipLaunchKernelGGL(conv_out_mfma_kernel<2>, dim3((unsigned)((npix + 127) / 128)), dim3(256), smem, stream, x, Wp, bias, y,
                               B, H, W, Cin, Cout);
        else
            hipLaunchKernelGGL(conv_out_mfma_kernel<1>, dim3((unsigned)((npix + 63) / 64)), dim3(256), smem, stream, x, Wp, bias, y,
                               B, H, W, Cin, Cout);
        SD_CHECK_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(conv_out_kernel, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, stream, x, Wp, bias, y, B, H, W,
                       Cin, Cout);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
