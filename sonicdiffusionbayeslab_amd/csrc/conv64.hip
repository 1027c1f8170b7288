// 3x3 convolution at 64 -> 64 channels with the WHOLE weight tensor resident in LDS (gfx950), and the entry / exit kernels of
// the tiny autoencoder (AutoencoderTiny / TAESD) that is built from it.
//
// Every conv of the tiny autoencoder is 64 -> 64 channels on images up to 1024 pixels wide.  The halo kernel (conv_halo.hip)
// and the implicit-GEMM kernel (gemm_conv.hip) work on 160-output-channel tiles -- 60 % of their MFMA work would be padding
// here -- and the halo kernel owns whole image rows of <= 400 halo slots.  Here
//
//   * one pixel is one 128-byte slot (64 bf16 channels, NHWC), as in the halo kernel;
//   * the nine taps' weights (9 x 64 x 64 bf16 = 72 KiB) are staged into LDS ONCE per persistent workgroup, packed on the
//     host (sd_conv64_pack) in the order the kernel reads them: [tap][k-step][16-row tile a][lane][8 bf16], so that an A
//     fragment is one conflict-free `ds_read_b128` at lane * 16;
//   * a workgroup (4 waves, one per SIMD) walks rectangular output tiles of TR rows x TC columns -- tiles, not whole image
//     rows: the tile's input halo is staged once by buffer-addressed LDS-DMA (out-of-image slots are out of the buffer's range
//     and read zeros) into one of two halo buffers and read at nine shifted addresses; the NEXT tile's halo streams into the
//     other buffer under this tile's MFMAs;
//   * a wave owns TM x 16 pixels x all 64 output channels: acc[4][TM] of v_mfma_f32_16x16x32_bf16, fp32 sums, one rounding.
//
//   mode         tile (TR x TC)   halo (rows x cols, slots)                      TM   MFMAs / wave / tile
//   0  plain     8 x 32           10 x 34 = 340                                  4    288
//   1  UP        8 x 32 (output)  6 x 18 = 108 in the LOW-RES input              4    288
//   2  S2        4 x 16 (output)  9 x 33 = 297 (stride 2, pad 1 on all sides)    1    72
//
//   LDS: 72 KiB of weights + 2 halo buffers x 44 one-KiB DMA pieces = 160 KiB exactly; one workgroup per CU.
//   A halo slot holds its eight 16-byte chunks XOR-swizzled by (slot & 7), applied to the per-lane SOURCE address of the DMA:
//   the fragment read of 16 consecutive pixels of a tile row is then bank-conflict free at every tap shift (stride-2 reads of
//   mode 2 are 2-way).
//
// Output channel order inside the MFMA rows: row 4 q + j of tile a is channel 16 q + 4 a + j, so that a lane (q = lane >> 4)
// ends up with 16 CONSECUTIVE channels of its pixel: two 16-byte stores, and the four lanes of a pixel write its whole
// 128-byte slot.
//
// Epilogue: + bias (fp32, optional) + residual R (bf16, optional, added before the ReLU: the block's third conv) -> ReLU
// (optional) -> bf16.  No split-K, no atomics: an output pixel is computed by one wave in one fixed order, whatever the batch
// and whichever workgroup takes its tile.
#include "common.h"
#include "kernels.h"

#include <math.h>
#include <string.h>

namespace {

constexpr int WBYTES = SD_CONV64_PACKED_BYTES;        // 9 taps x 2 k-steps x 4 row tiles x 1 KiB
constexpr int HPIECES = 44;                           // one-KiB DMA pieces per halo buffer (8 slots each)
constexpr int HBYTES = HPIECES * 1024;
constexpr int SMEM = WBYTES + 2 * HBYTES;
static_assert(SMEM == 160 * 1024, "weights + two halo buffers fill the 160 KiB LDS exactly");
constexpr unsigned NOSRC = 0xffffffffu;

template <int MODE> struct Geo;
template <> struct Geo<0> { static constexpr int TR = 8, TC = 32, HR = 10, HC = 34, TM = 4; };
template <> struct Geo<1> { static constexpr int TR = 8, TC = 32, HR = 6, HC = 18, TM = 4; };
template <> struct Geo<2> { static constexpr int TR = 4, TC = 16, HR = 9, HC = 33, TM = 1; };

template <int MODE>
__global__ __launch_bounds__(256, 1) void conv64_kernel(const Conv64Args p) {
    using G = Geo<MODE>;
    constexpr int TR = G::TR, TC = G::TC, HC = G::HC, TM = G::TM;
    constexpr int HS = G::HR * G::HC;                 // halo slots in use
    constexpr int PPW = ((HS + 7) / 8 + 3) / 4;       // DMA pieces per wave and tile (piece j * 4 + wave)
    static_assert(PPW * 4 <= HPIECES, "halo does not fit its buffer");
    static_assert(TR * TC == 4 * TM * 16, "4 waves x TM x 16 pixels");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Wl = smem;
    char* const Hb0 = smem + WBYTES;
    char* const Hb1 = Hb0 + HBYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane & 15, lq = lane >> 4;

    // persistent workgroups, one per CU; the workgroups of one XCD (blockIdx % 8) take consecutive tiles, whose halos overlap
    const int nblk = gridDim.x;
    int work;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
        work = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    if (work >= p.ntiles) return;

    // ---- the weights: 72 linear one-KiB pieces, 18 per wave, once ---------------------------------------
    {
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.Wp, 0, WBYTES, 0x00020000);
#pragma unroll
        for (int i = 0; i < 18; ++i) {
            const int piece = wave * 18 + i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, LDS_PTR(Wl + piece * 1024), 16, lane * 16, piece * 1024, 0, 0);
        }
    }

    // ---- halo DMA descriptors (tile independent): piece j * 4 + wave, this lane fills chunk position lane & 7 of slot
    // piece * 8 + (lane >> 3) with source chunk (lane & 7) ^ (slot & 7); slot -> (halo row, halo column) once
    int hyx[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int slot = (j * 4 + wave) * 8 + (lane >> 3);
        const int hy = slot / HC, hx = slot - hy * HC;
        hyx[j] = slot < HS ? (hy << 16 | hx) : -1;
    }
    const unsigned csrc = (unsigned)(((lane & 7) ^ (lane >> 3)) << 4);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (int)p.xbytes, 0x00020000);
    const int tiles_img = p.tiles_y * p.tiles_x;

    auto issue_halo = [&](int t, char* hb) {
        const int b = t / tiles_img, rem = t - b * tiles_img;
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
        // input row / column of halo slot (0, 0)
        const int iy0 = MODE == 0 ? ty * TR - 1 : MODE == 1 ? ty * (TR / 2) - 1 : 2 * ty * TR - 1;
        const int ix0 = MODE == 0 ? tx * TC - 1 : MODE == 1 ? tx * (TC / 2) - 1 : 2 * tx * TC - 1;
        const unsigned base = (unsigned)b * (unsigned)(p.Hin * p.Win);
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            const int iy = iy0 + (hyx[j] >> 16), ix = ix0 + (hyx[j] & 0xffff);
            const bool ok = hyx[j] >= 0 && (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
            const unsigned off = ok ? (base + (unsigned)(iy * p.Win + ix)) * 128u + csrc : NOSRC;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, LDS_PTR(hb + (j * 4 + wave) * 1024), 16, (int)off, 0, 0, 0);
        }
    };

    // ---- fragment addressing (tile independent): this lane's pixel of pixel tile f, row / column inside the tile
    int pr[TM], pc[TM];
#pragma unroll
    for (int f = 0; f < TM; ++f) {
        const int px = (wave * TM + f) * 16 + lrow;
        pr[f] = px / TC;
        pc[f] = px % TC;
    }
    auto xaddr = [&](int f, int tap, int ks) -> int {
        const int ty = tap / 3, tx = tap % 3;
        int slot;
        if (MODE == 0) slot = (pr[f] + ty) * HC + pc[f] + tx;
        else if (MODE == 1) slot = (((pr[f] + ty - 1) >> 1) + 1) * HC + ((pc[f] + tx - 1) >> 1) + 1;
        else slot = (2 * pr[f] + ty) * HC + 2 * pc[f] + tx;
        return slot * 128 + (((ks * 4 + lq) ^ (slot & 7)) << 4);
    };

    // bias of this lane's 16 channels 16 lq + (0 .. 15): bv[a][j] = channel 16 lq + 4 a + j
    f32x4 bv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) bv[a] = p.bias ? *(const f32x4*)(p.bias + lq * 16 + a * 4) : f32x4{0.f, 0.f, 0.f, 0.f};

    int cur = 0;
    issue_halo(work, Hb0);
    for (int t = work; t < p.ntiles; t += nblk) {
        // the halo of tile t (and, the first time, the weights) has landed; every wave is done reading the other buffer
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* hcur = cur ? Hb1 : Hb0;
        if (t + nblk < p.ntiles) issue_halo(t + nblk, cur ? Hb0 : Hb1);

        f32x4 acc[4][TM];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int f = 0; f < TM; ++f) acc[a][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 wf[4], xf[TM];
#pragma unroll
                for (int a = 0; a < 4; ++a) wf[a] = *(const bf16x8*)(Wl + ((tap * 2 + ks) * 4 + a) * 1024 + lane * 16);
#pragma unroll
                for (int f = 0; f < TM; ++f) xf[f] = *(const bf16x8*)(hcur + xaddr(f, tap, ks));
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int f = 0; f < TM; ++f)
                        acc[a][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[a], xf[f], acc[a][f], 0, 0, 0);
            }
        }

        // ---- epilogue: lane (lrow, lq) holds channels 16 lq + 4 a + j of pixel (wave * TM + f) * 16 + lrow -------------
        const int b = t / tiles_img, rem = t - b * tiles_img;
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
#pragma unroll
        for (int f = 0; f < TM; ++f) {
            const int oy = ty * TR + pr[f], ox = tx * TC + pc[f];
            if (oy >= p.Hout || ox >= p.Wout) continue;
            const long o = (((long)b * p.Hout + oy) * p.Wout + ox) * 64 + lq * 16;
            float v[16];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[a * 4 + j] = acc[a][f][j] + bv[a][j];
            if (p.R) {
                const u32x4 r0 = *(const u32x4*)(p.R + o), r1 = *(const u32x4*)(p.R + o + 8);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[2 * i] += bflo(r0[i]); v[2 * i + 1] += bfhi(r0[i]);
                    v[8 + 2 * i] += bflo(r1[i]); v[8 + 2 * i + 1] += bfhi(r1[i]);
                }
            }
            if (p.relu) {
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = fmaxf(v[i], 0.f);
            }
            *(u32x4*)(p.Y + o) = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
            *(u32x4*)(p.Y + o + 8) = u32x4{pack2bf(v[8], v[9]), pack2bf(v[10], v[11]), pack2bf(v[12], v[13]), pack2bf(v[14], v[15])};
        }
        cur ^= 1;
    }
}

// ---- entry: fp32 NCHW [B, CIN, H, W] -> 3x3 conv CIN -> 64 in fp32 (+ bias) -> bf16 NHWC [B, H, W, 64] ------------------
// DEC: the decoder's entry.  The input is tanh(z / 3) * 3, computed in fp32 in the load (tanh(0) = 0: the zero padding is
// that of the transformed tensor), and the ReLU that follows the conv is applied.  Otherwise the encoder's: the [0, 1] image
// as it is (the pipeline's 2 x - 1 and the model's (x + 1) / 2 cancel), no activation.
// A thread owns 8 channels of one pixel (one 16-byte store); the weights Wt [CIN * 9][64] fp32 sit in LDS.
template <int CIN, int DEC>
__global__ __launch_bounds__(256) void taesd_entry_kernel(const float* __restrict__ x, const float* __restrict__ Wt,
                                                          const float* __restrict__ bias, bf16_t* __restrict__ y, int B, int H,
                                                          int W) {
    __shared__ float sw[CIN * 9 * 64];
    for (int i = threadIdx.x; i < CIN * 9 * 64; i += 256) sw[i] = Wt[i];
    __syncthreads();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long pix = idx >> 3;
    const int g = (int)(idx & 7);
    if (pix >= (long)B * H * W) return;
    const int b = (int)(pix / ((long)H * W));
    const int rem = (int)(pix - (long)b * H * W);
    const int oy = rem / W, ox = rem - oy * W;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bias[g * 8 + j];
#pragma unroll 1      // (all CIN * 9 loads and tanh chains in flight at once spill; one channel's nine taps do not)
    for (int c = 0; c < CIN; ++c) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
            float v = 0.f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                v = x[(((long)b * CIN + c) * H + iy) * W + ix];
                if (DEC) v = tanhf(v * (1.0f / 3.0f)) * 3.0f;
            }
            const float* w = sw + (c * 9 + tap) * 64 + g * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(v, w[j], acc[j]);
        }
    }
    if (DEC) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
    }
    *(u32x4*)(y + pix * 64 + g * 8) =
        u32x4{pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]), pack2bf(acc[4], acc[5]), pack2bf(acc[6], acc[7])};
}

// ---- exit: bf16 NHWC [B, H, W, 64] -> 3x3 conv 64 -> Cout <= 4 (bf16 operands, fp32 sums) + bias -> fp32 NCHW ------------
// The pattern of conv_out_mfma_kernel (small.hip) at Cin = 64: D[cout (16 rows, <= 4 live)][16 pixels], the weights
// [Cout][9][64] in LDS, a wave streams the nine shifted input slots of its 16 pixels from global memory into the B operand.
// out_mode 0: y * 2 - 1 (the decoder's [-1, 1] image), 1: clamp(y, 0, 1) (the image in unit range, what a pipeline's
// `/ 2 + 0.5` and clamp make of mode 0), 2: y (the encoder's latents).
__global__ __launch_bounds__(256) void taesd_exit_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ Wp,
                                                         const float* __restrict__ bias, float* __restrict__ y, int B, int H,
                                                         int W, int Cout, int out_mode) {
    __shared__ __attribute__((aligned(16))) char sw[4 * 576 * 2];      // rows >= Cout zero
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 4 * 72; i += 256) {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (i / 72 < Cout) v = *(const u32x4*)(Wp + (long)i * 8);
        *(u32x4*)(sw + i * 16) = v;
    }
    __syncthreads();
    const int l15 = lane & 15, kg = lane >> 4;
    const long npix = (long)B * H * W;
    const long pix0 = ((long)blockIdx.x * 4 + wave) * 16;
    if (pix0 >= npix) return;
    const long pp = pix0 + l15;
    const bool valid = pp < npix;
    const long pcl = valid ? pp : npix - 1;
    const int b = (int)(pcl / ((long)H * W));
    const int rem = (int)(pcl - (long)b * H * W);
    const int oy = rem / W, ox = rem - oy * W;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const char* wrow = sw + ((l15 & 3) * 576 + kg * 8) * 2;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        const bool ok = valid && iy >= 0 && iy < H && ix >= 0 && ix < W;
        const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
        const bf16_t* src = x + (((long)b * H + cy) * W + cx) * 64 + kg * 8;
#pragma unroll
        for (int c0 = 0; c0 < 64; c0 += 32) {
            bf16x8 wf = *(const bf16x8*)(wrow + (tap * 64 + c0) * 2);
            wf = l15 < 4 ? wf : zero8;
            bf16x8 xf = *(const bf16x8*)(src + c0);
            xf = ok ? xf : zero8;
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc, 0, 0, 0);
        }
    }
    if (kg == 0 && valid) {          // lanes 0..15: rows (output channels) 0..3 of pixel l15
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= Cout) break;
            float v = acc[j] + bias[j];
            if (out_mode == 0) v = v * 2.0f - 1.0f;
            else if (out_mode == 1) v = fminf(fmaxf(v, 0.f), 1.f);
            y[(((long)b * Cout + j) * H + oy) * W + ox] = v;
        }
    }
}

inline unsigned short f32_to_bf16_host(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    u = u + 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

}  // namespace

// OIHW fp32 [64][64][3][3] -> the kernel's LDS image [tap][k-step][row tile a][lane][8] bf16: lane (lrow = lane & 15,
// lq = lane >> 4) of tile a holds the A fragment row 16 a + lrow = output channel 16 (lrow >> 2) + 4 a + (lrow & 3), input
// channels 32 ks + 8 lq + (0 .. 7)
void sd_conv64_pack(const float* w, bf16_t* out) {
    for (int tap = 0; tap < 9; ++tap)
        for (int ks = 0; ks < 2; ++ks)
            for (int a = 0; a < 4; ++a)
                for (int lane = 0; lane < 64; ++lane) {
                    const int lrow = lane & 15, lq = lane >> 4;
                    const int co = 16 * (lrow >> 2) + 4 * a + (lrow & 3);
                    for (int e = 0; e < 8; ++e) {
                        const int ci = 32 * ks + 8 * lq + e;
                        out[((((tap * 2 + ks) * 4 + a) * 64) + lane) * 8 + e] = f32_to_bf16_host(w[((long)co * 64 + ci) * 9 + tap]);
                    }
                }
}

int sd_conv64_out_size(int in, int mode) { return mode == 1 ? 2 * in : mode == 2 ? (in - 1) / 2 + 1 : in; }

int sd_launch_conv64(const Conv64Args& a0, hipStream_t stream) {
    Conv64Args a = a0;
    SD_REQUIRE(a.X && a.Wp && a.Y, "conv64: null operand");
    SD_REQUIRE(a.mode >= 0 && a.mode <= 2, "conv64: mode %d (0 plain, 1 nearest-2x upsample, 2 stride 2)", a.mode);
    SD_REQUIRE(a.B > 0 && a.Hin > 0 && a.Win > 0 && a.Hin <= 4096 && a.Win <= 4096, "conv64: B=%d Hin=%d Win=%d", a.B, a.Hin, a.Win);
    SD_REQUIRE((((uintptr_t)a.X | (uintptr_t)a.Wp | (uintptr_t)a.Y | (uintptr_t)a.R) & 15) == 0 && ((uintptr_t)a.bias & 15) == 0,
               "conv64: operands must be 16-byte aligned");
    SD_REQUIRE(a.X != a.Y, "conv64: the conv cannot run in place");
    const long xb = (long)a.B * a.Hin * a.Win * 128;
    SD_REQUIRE(xb <= 0xf0000000l, "conv64: input of %ld bytes (32-bit DMA offsets: at most %ld; decode in smaller batches)", xb, 0xf0000000l);
    a.xbytes = (unsigned)xb;
    a.Hout = sd_conv64_out_size(a.Hin, a.mode);
    a.Wout = sd_conv64_out_size(a.Win, a.mode);
    const int TR = a.mode == 2 ? Geo<2>::TR : Geo<0>::TR, TC = a.mode == 2 ? Geo<2>::TC : Geo<0>::TC;
    a.tiles_y = (a.Hout + TR - 1) / TR;
    a.tiles_x = (a.Wout + TC - 1) / TC;
    const long nt = (long)a.B * a.tiles_y * a.tiles_x;
    SD_REQUIRE(nt < (1l << 30), "conv64: too many tiles");
    a.ntiles = (int)nt;
    static bool attr_set = false;
    if (!attr_set) {
        SD_CHECK_HIP(hipFuncSetAttribute((const void*)conv64_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
        SD_CHECK_HIP(hipFuncSetAttribute((const void*)conv64_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
        SD_CHECK_HIP(hipFuncSetAttribute((const void*)conv64_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM));
        attr_set = true;
    }
    const int grid = a.ntiles < 256 ? a.ntiles : 256;      // persistent: one workgroup per CU
    if (a.mode == 0) hipLaunchKernelGGL(conv64_kernel<0>, dim3(grid), dim3(256), SMEM, stream, a);
    else if (a.mode == 1) hipLaunchKernelGGL(conv64_kernel<1>, dim3(grid), dim3(256), SMEM, stream, a);
    else hipLaunchKernelGGL(conv64_kernel<2>, dim3(grid), dim3(256), SMEM, stream, a);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_taesd_entry(const float* x, const float* Wt, const float* bias, bf16_t* y, int B, int H, int W, int Cin, int decoder,
                          hipStream_t stream) {
    SD_REQUIRE(x && Wt && bias && y, "taesd_entry: null operand");
    SD_REQUIRE((Cin == 4 && decoder) || (Cin == 3 && !decoder), "taesd_entry: %d input channels (4: decoder, 3: encoder)", Cin);
    SD_REQUIRE(B > 0 && H > 0 && W > 0, "taesd_entry: B=%d H=%d W=%d", B, H, W);
    const long blocks = ((long)B * H * W * 8 + 255) / 256;
    SD_REQUIRE(blocks < (1l << 31), "taesd_entry: too many pixels");
    if (decoder) hipLaunchKernelGGL((taesd_entry_kernel<4, 1>), dim3((unsigned)blocks), dim3(256), 0, stream, x, Wt, bias, y, B, H, W);
    else hipLaunchKernelGGL((taesd_entry_kernel<3, 0>), dim3((unsigned)blocks), dim3(256), 0, stream, x, Wt, bias, y, B, H, W);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_taesd_exit(const bf16_t* x, const bf16_t* Wp, const float* bias, float* y, int B, int H, int W, int Cout, int out_mode,
                         hipStream_t stream) {
    SD_REQUIRE(x && Wp && bias && y, "taesd_exit: null operand");
    SD_REQUIRE(Cout >= 1 && Cout <= 4 && out_mode >= 0 && out_mode <= 2, "taesd_exit: Cout=%d out_mode=%d", Cout, out_mode);
    SD_REQUIRE(B > 0 && H > 0 && W > 0, "taesd_exit: B=%d H=%d W=%d", B, H, W);
    SD_REQUIRE((((uintptr_t)x | (uintptr_t)Wp) & 15) == 0, "taesd_exit: operands must be 16-byte aligned");
    const long blocks = ((long)B * H * W + 63) / 64;
    SD_REQUIRE(blocks < (1l << 31), "taesd_exit: too many pixels");
    hipLaunchKernelGGL(taesd_exit_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, Wp, bias, y, B, H, W, Cout, out_mode);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
