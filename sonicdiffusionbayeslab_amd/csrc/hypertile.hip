// HyperTile (tfernd/HyperTile): the two copy passes around a tiled transformer block, ONE kernel for both directions.
//
//   raster order:  [B][rh][rw] rows of C bf16 channels, row pitch `pitch` elements (>= C)
//   tile order:    [B][nh][nw][th][tw] rows of C channels, dense;  th = rh / nh, tw = rw / nw
//   tile (i, j) of a sample holds the tokens (i th + y, j tw + x), row-major inside the tile, the tiles row-major in the sample
//
//   gather:   tile[b][i][j][y][x] = raster[b][i th + y][j tw + x]
//   scatter:  raster[b][i th + y][j tw + x] = tile[b][i][j][y][x]
//
// Work split.  HBM-bound: one read and one write stream, nothing to compute but the row map.  One wave moves one whole row
// per pass, its lanes along the channels in 16-byte vectors (C / 8 of them: 40, 80 or 160 at the UNet's widths; a loop over
// 64-vector pieces, so no width is assumed to fit anything).  Consecutive waves take consecutive DESTINATION rows, so the
// writes of a workgroup and of neighbouring workgroups are contiguous; the reads are contiguous in runs of tw rows.  Every
// wave has HT_ROWS rows in flight (all loads issued before the first store).  Workgroups of four waves stride over the rows; the
// grid is capped (~8 workgroups per CU).  All row offsets are 64-bit.  No LDS, no atomics.
#include "common.h"
#include "kernels.h"

#include <stdint.h>

#include <algorithm>

namespace {

constexpr int HT_THREADS = 256;
constexpr int HT_WAVES = HT_THREADS / 64;
constexpr int HT_MAX_BLOCKS = 2048;
constexpr int HT_ROWS = 4;

struct HtGeom { int rh, rw, nw, th, tw; };

// the row on the SOURCE side that destination row d takes: scatter -- d is a raster row, the result a tile-order row; gather --
// the other way round
__device__ __forceinline__ long ht_source_row(long d, const HtGeom g, int scatter) {
    const int hw = g.rh * g.rw;
    const long b = d / hw;
    const int rem = (int)(d - b * hw);
    if (scatter) {
        const int Y = rem / g.rw, X = rem - Y * g.rw;
        const int i = Y / g.th, y = Y - i * g.th, j = X / g.tw, x = X - j * g.tw;
        return b * hw + ((long)(i * g.nw + j) * g.th + y) * g.tw + x;
    }
    const int tt = g.th * g.tw;
    const int t = rem / tt, e = rem - t * tt;
    const int i = t / g.nw, j = t - i * g.nw, y = e / g.tw, x = e - y * g.tw;
    return b * hw + (long)(i * g.th + y) * g.rw + j * g.tw + x;
}

__global__ __launch_bounds__(HT_THREADS) void hypertile_kernel(const bf16_t* __restrict__ src, long lds, bf16_t* __restrict__ dst, long ldd,
                                                               long rows, int vecs, HtGeom g, int scatter) {
    const int lane = threadIdx.x & 63;
    const long nwaves = (long)gridDim.x * HT_WAVES;
    for (long d0 = (long)blockIdx.x * HT_WAVES + (threadIdx.x >> 6); d0 < rows; d0 += nwaves * HT_ROWS) {
        const bf16_t* s[HT_ROWS];
        bf16_t* o[HT_ROWS];
        bool ok[HT_ROWS];
#pragma unroll
        for (int k = 0; k < HT_ROWS; ++k) {
            const long d = d0 + k * nwaves;
            ok[k] = d < rows;
            const long dd = ok[k] ? d : d0;
            s[k] = src + ht_source_row(dd, g, scatter) * lds;
            o[k] = dst + dd * ldd;
        }
        for (int c = lane; c < vecs; c += 64) {
            u32x4 v[HT_ROWS];
#pragma unroll
            for (int k = 0; k < HT_ROWS; ++k)
                if (ok[k]) v[k] = *(const u32x4*)(s[k] + c * 8);
#pragma unroll
            for (int k = 0; k < HT_ROWS; ++k)
                if (ok[k]) *(u32x4*)(o[k] + c * 8) = v[k];
        }
    }
}

}  // namespace

int sd_hypertile_shape_ok(int B, int rh, int rw, int C, int nh, int nw, long pitch, const char* who) {
    SD_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d (1 .. 65535)", who, B);
    SD_REQUIRE(rh >= 1 && rw >= 1 && rh <= 256 && rw <= 256, "%s: %dx%d tokens (sides of 1 .. 256)", who, rh, rw);
    SD_REQUIRE(nh >= 1 && nw >= 1 && rh % nh == 0 && rw % nw == 0, "%s: %dx%d tiles do not divide %dx%d tokens", who, nh, nw, rh, rw);
    SD_REQUIRE(C >= 8 && C % 8 == 0 && C <= 16384, "%s: C=%d (a multiple of 8, at most 16384: 16-byte accesses)", who, C);
    // (65535 x 256 x 256 rows of at most 2^30 elements: every element offset stays below 2^62)
    SD_REQUIRE(pitch >= C && pitch % 8 == 0 && pitch <= (1l << 30), "%s: row pitch %ld (a multiple of 8, at least C=%d, at most 2^30)", who,
               pitch, C);
    return 0;
}

static int launch(const bf16_t* src, long lds, bf16_t* dst, long ldd, int B, int rh, int rw, int C, int nh, int nw, int scatter,
                  hipStream_t stream) {
    const long rows = (long)B * rh * rw;
    const HtGeom g{rh, rw, nw, rh / nh, rw / nw};
    const long blocks = std::min<long>((rows + HT_WAVES - 1) / HT_WAVES, HT_MAX_BLOCKS);
    hipLaunchKernelGGL(hypertile_kernel, dim3((unsigned)blocks), dim3(HT_THREADS), 0, stream, src, lds, dst, ldd, rows, C / 8, g, scatter);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_hypertile_gather(const bf16_t* x, long pitch, bf16_t* out, int B, int rh, int rw, int C, int nh, int nw, hipStream_t stream) {
    if (sd_hypertile_shape_ok(B, rh, rw, C, nh, nw, pitch, "hypertile_gather")) return -1;
    SD_REQUIRE(x && out && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0, "hypertile_gather: null or unaligned pointer (16 bytes)");
    return launch(x, pitch, out, C, B, rh, rw, C, nh, nw, 0, stream);
}

int sd_launch_hypertile_scatter(const bf16_t* y, bf16_t* out, long pitch, int B, int rh, int rw, int C, int nh, int nw, hipStream_t stream) {
    if (sd_hypertile_shape_ok(B, rh, rw, C, nh, nw, pitch, "hypertile_scatter")) return -1;
    SD_REQUIRE(y && out && (uintptr_t)y % 16 == 0 && (uintptr_t)out % 16 == 0, "hypertile_scatter: null or unaligned pointer (16 bytes)");
    return launch(y, C, out, pitch, B, rh, rw, C, nh, nw, 1, stream);
}
