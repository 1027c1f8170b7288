// Perturbed-attention guidance (Ahn et al. 2024): the identity self-attention of the perturbed samples, ONE kernel.
//
// In a perturbed transformer block attn1 of a perturbed sample is to_out(to_v(norm1(h))): the attention matrix is the identity, so
// the attention output IS V as the q | k | v projection left it.  This kernel writes those rows of the attention output tensor --
// the rows of the LAST samples, behind the ones the attention kernel wrote -- so that to_out stays one GEMM over all rows.
//
//   token-major V:  row r at  V + r * ldv              (the projection's [rows][3 C] output: V = qkv + 2 C, ldv = 3 C)
//   head-major  V:  [sample][head][token][D] dense     (the 64x64-level projection: sample = r / tok, token = r % tok)
//   output:         token-major [rows][C], C = heads * D;  out[r][h * D + d] = V(r, h, d)
//
// Rows [row0, row0 + rows) are written, nothing else.  Work split as hypertile.hip's: HBM-bound, one read and one write stream.
// One wave moves one row per pass, its lanes along the channels in 16-byte vectors (D is a multiple of 8, so a vector never
// straddles two heads); consecutive waves take consecutive rows, PAG_ROWS rows in flight per wave (all loads before the first
// store); workgroups of four waves stride over the rows, the grid is capped.  64-bit offsets.  No LDS, no atomics.
#include "common.h"
#include "kernels.h"

#include <stdint.h>

#include <algorithm>

namespace {

constexpr int PAG_THREADS = 256;
constexpr int PAG_WAVES = PAG_THREADS / 64;
constexpr int PAG_MAX_BLOCKS = 2048;
constexpr int PAG_ROWS = 4;

__global__ __launch_bounds__(PAG_THREADS) void pag_identity_kernel(const bf16_t* __restrict__ V, long ldv, int tok, int heads, int vph,
                                                                   bf16_t* __restrict__ out, long row0, long rows, int head_major) {
    const int lane = threadIdx.x & 63;
    const int vecs = heads * vph;          // 16-byte vectors per row; vph = D / 8 of them per head
    const long nwaves = (long)gridDim.x * PAG_WAVES;
    for (long d0 = (long)blockIdx.x * PAG_WAVES + (threadIdx.x >> 6); d0 < rows; d0 += nwaves * PAG_ROWS) {
        long r[PAG_ROWS];
        bool ok[PAG_ROWS];
#pragma unroll
        for (int k = 0; k < PAG_ROWS; ++k) {
            const long d = d0 + k * nwaves;
            ok[k] = d < rows;
            r[k] = row0 + (ok[k] ? d : d0);
        }
        for (int c = lane; c < vecs; c += 64) {
            const int h = c / vph, v = c - h * vph;
            u32x4 val[PAG_ROWS];
#pragma unroll
            for (int k = 0; k < PAG_ROWS; ++k) {
                if (!ok[k]) continue;
                long src;
                if (head_major) {
                    const long smp = r[k] / tok, t = r[k] - smp * tok;
                    src = (((smp * heads + h) * tok + t) * vph + v) * 8;
                } else src = r[k] * ldv + (long)c * 8;
                val[k] = *(const u32x4*)(V + src);
            }
#pragma unroll
            for (int k = 0; k < PAG_ROWS; ++k)
                if (ok[k]) *(u32x4*)(out + (r[k] * vecs + c) * 8) = val[k];
        }
    }
}

}  // namespace

// rows_total: the rows of the output tensor (and of V); [row0, row0 + rows) are the perturbed ones.  tok: the tokens of a
// head-major sample (0 = token-major V with row pitch ldv).
int sd_pag_identity_shape_ok(long rows_total, long row0, long rows, int C, int heads, long ldv, int tok, const char* who) {
    SD_REQUIRE(rows_total >= 1 && rows_total <= (1l << 31), "%s: %ld rows (1 .. 2^31)", who, rows_total);
    SD_REQUIRE(row0 >= 0 && rows >= 1 && row0 + rows <= rows_total, "%s: rows [%ld, %ld) of %ld", who, row0, row0 + rows, rows_total);
    SD_REQUIRE(heads >= 1 && C >= 8 && C <= 16384 && C % heads == 0 && (C / heads) % 8 == 0,
               "%s: C=%d heads=%d (head dim a multiple of 8, C at most 16384: 16-byte accesses)", who, C, heads);
    if (tok > 0) {
        SD_REQUIRE(rows_total % tok == 0 && row0 % tok == 0 && rows % tok == 0, "%s: head-major samples of %d tokens do not divide rows [%ld, %ld) of %ld",
                   who, tok, row0, row0 + rows, rows_total);
    } else {
        // (2^31 rows of at most 2^30 elements: every element offset stays below 2^62)
        SD_REQUIRE(tok == 0 && ldv >= C && ldv % 8 == 0 && ldv <= (1l << 30), "%s: V row pitch %ld (a multiple of 8, at least C=%d, at most 2^30)",
                   who, ldv, C);
    }
    return 0;
}

int sd_launch_pag_identity(const bf16_t* V, long ldv, int tok, bf16_t* out, long rows_total, long row0, long rows, int C, int heads,
                           hipStream_t stream) {
    if (sd_pag_identity_shape_ok(rows_total, row0, rows, C, heads, ldv, tok, "pag_identity")) return -1;
    SD_REQUIRE(V && out && (uintptr_t)V % 16 == 0 && (uintptr_t)out % 16 == 0, "pag_identity: null or unaligned pointer (16 bytes)");
    const long blocks = std::min<long>((rows + PAG_WAVES - 1) / PAG_WAVES, PAG_MAX_BLOCKS);
    hipLaunchKernelGGL(pag_identity_kernel, dim3((unsigned)blocks), dim3(PAG_THREADS), 0, stream, V, ldv, tok, heads, C / heads / 8, out, row0,
                       rows, tok > 0 ? 1 : 0);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
