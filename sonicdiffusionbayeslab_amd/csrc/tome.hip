// Token Merging for Stable Diffusion (Bolya & Hoffman, "Token Merging for Fast Stable Diffusion"): the bipartite matching, the
// merge in front of a block's self-attention and the unmerge behind it.  DESIGN.md section 4n has the semantics; in short, on
// a level of h x w tokens cut into 2x2 cells one token per cell is a "dst" token (position choice[cell] in 0..3, row-major in
// the cell) and the other three are "src" tokens; dst tokens are numbered by cell (row-major), src tokens by ascending token
// index.  Every src token looks for its most similar dst token (cosine similarity), the r src tokens with the best match are
// averaged into their dst token, attention runs on the N - r remaining rows and its output is copied back to all N tokens.
//
//   tome_partition   choice -> tok[N]: the token index of every src slot (num_src entries), then of every dst slot
//   tome_rownorm     inv[b][token] = 1 / ||x||_2 in fp32 (0 for an all-zero row: its scores are 0, never NaN)
//   tome_match       node_max / node_idx [B][num_src]: max and argmax over dst of the cosine similarity, on
//                    v_mfma_f32_16x16x32_bf16; the score matrix is never written
//   tome_select      top r of num_src per sample by radix select (no sort), ordered compaction into kept / merged / dst_idx
//   tome_merge       [B][N - r][C]: kept src rows, then every dst row averaged with its members
//   tome_unmerge     out[token] = attn_out[row_of(token)] + residual[token]
//
// Precision of the match.  The MFMA multiplies the RAW bf16 rows (products exact in fp32, fp32 accumulation) and the
// accumulator is scaled afterwards, score = (acc * inv_src) * inv_dst: the unit rows are never rounded to bf16.  Against the
// exact cosine of the same bf16 rows the error is the accumulation's (at most C * 2^-24 relative to |x_s| |x_d|, i.e. absolute
// on the unit scale), the same again for each of the two fp32 sums of squares, and a few ulp for sqrt, divide and the two
// multiplies:  |score - exact| <= 4 C 2^-24  (tests/test_tome_gpu.py derives its eps from this line).
// Tie rules: equal scores resolve to the lowest dst index (match) and to the lowest src index at the top-r cut (select).
// Everything is deterministic: no floating-point atomics, and the integer LDS atomics only count (order-independent).
#include "kernels.h"

namespace {

// ---------------------------------------------------------------------------------------------
// partition: one thread per token
// ---------------------------------------------------------------------------------------------
__global__ void tome_partition_kernel(const unsigned char* __restrict__ choice, int h, int w, int* __restrict__ tok) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = h * w, wc = w >> 1, num_dst = (h >> 1) * wc, num_src = N - num_dst;
    if (t >= N) return;
    const int y = t / w, x = t - y * w, cy = y >> 1, cx = x >> 1;
    const unsigned char* crow = choice + (long)cy * wc;
    const int pos = (y & 1) * 2 + (x & 1);
    if ((crow[cx] & 3) == pos) {
        tok[num_src + cy * wc + cx] = t;
        return;
    }
    // src slot = number of src tokens with a smaller token index: 3 per cell of the cell rows above, the whole upper token row
    // of this cell row (if this token is in the lower one), and the tokens to the left in this token row
    int before = 3 * wc * cy;
    if (y & 1) {
        int top_dst = 0;
        for (int c = 0; c < wc; ++c) top_dst += (crow[c] & 3) < 2;
        before += w - top_dst;
    }
    int left_dst = 0;
    for (int c = 0; c <= cx; ++c) {
        const int p = crow[c] & 3;
        left_dst += (p >> 1) == (y & 1) && 2 * c + (p & 1) < x;
    }
    tok[before + x - left_dst] = t;
}

// ---------------------------------------------------------------------------------------------
// inverse row norms: one wave per token
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tome_rownorm_kernel(const bf16_t* __restrict__ x, float* __restrict__ inv, long rows, int C) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const u32x4* p = (const u32x4*)(x + row * C);
    float s = 0.f;
    for (int i = lane; i < C / 8; i += 64) {
        const u32x4 v = p[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = bflo(v[j]), b = bfhi(v[j]);
            s = __builtin_fmaf(a, a, s);
            s = __builtin_fmaf(b, b, s);
        }
    }
    s = wave_sum(s);
    // (s > 0 and finite; an all-zero row, or a sum of squares that overflowed, scores 0 against everything)
    if (lane == 0) inv[row] = (s > 0.f && s < __builtin_inff()) ? 1.0f / sqrtf(s) : 0.f;
}

// ---------------------------------------------------------------------------------------------
// match: 64 src rows x all dst rows per block, 4 waves x 16 src rows, dst in tiles of 64, K in chunks of 64
// ---------------------------------------------------------------------------------------------
constexpr int MT = 64;            // src rows and dst rows per tile
constexpr int KT = 64;            // bf16 elements of K per staged chunk (128 bytes per row)
constexpr int PITCH = KT + 8;     // LDS row pitch in elements: 144 bytes, so that the 16 rows of a fragment read spread over banks

__global__ __launch_bounds__(256) void tome_match_kernel(const bf16_t* __restrict__ x, const int* __restrict__ tok,
                                                         const float* __restrict__ inv, float* __restrict__ node_max,
                                                         int* __restrict__ node_idx, int N, int C, int num_src, int num_dst) {
    __shared__ __attribute__((aligned(16))) bf16_t As[MT * PITCH];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[MT * PITCH];
    __shared__ int a_tok[MT], b_tok[MT];
    __shared__ float a_inv[MT], b_inv[MT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, s0 = blockIdx.x * MT;
    const bf16_t* xb = x + (long)b * N * C;
    const float* invb = inv + (long)b * N;
    if (tid < MT) {
        const int s = s0 + tid;
        const int t = s < num_src ? tok[s] : -1;
        a_tok[tid] = t;
        a_inv[tid] = t >= 0 ? invb[t] : 0.f;
    }
    const int lrow = lane & 15, lq = lane >> 4;
    float best[4];
    int bidx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { best[j] = -__builtin_inff(); bidx[j] = 0; }

    for (int d0 = 0; d0 < num_dst; d0 += MT) {
        __syncthreads();          // (the previous tile's b_tok / b_inv and LDS operands are no longer read)
        if (tid < MT) {
            const int d = d0 + tid;
            const int t = d < num_dst ? tok[num_src + d] : -1;
            b_tok[tid] = t;
            b_inv[tid] = t >= 0 ? invb[t] : 0.f;
        }
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        // stage 64 rows x 128 bytes of each operand per K chunk: 512 16-byte pieces per operand, two per thread; rows past the
        // ragged end are zero.  The next chunk's global loads are issued before this chunk's MFMAs and land under them.
        u32x4 va[2], vb[2];
        auto load_chunk = [&](int k0) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int p = tid + 256 * i, row = p >> 3, c16 = p & 7;
                const int ta = a_tok[row], tb = b_tok[row];
                va[i] = ta >= 0 ? *(const u32x4*)(xb + (long)ta * C + k0 + c16 * 8) : u32x4{0, 0, 0, 0};
                vb[i] = tb >= 0 ? *(const u32x4*)(xb + (long)tb * C + k0 + c16 * 8) : u32x4{0, 0, 0, 0};
            }
        };
        load_chunk(0);
        for (int k0 = 0; k0 < C; k0 += KT) {
            if (k0) __syncthreads();          // (every wave has read the previous chunk)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int p = tid + 256 * i, row = p >> 3, c16 = p & 7;
                *(u32x4*)(As + row * PITCH + c16 * 8) = va[i];
                *(u32x4*)(Bs + row * PITCH + c16 * 8) = vb[i];
            }
            __syncthreads();
            if (k0 + KT < C) load_chunk(k0 + KT);
#pragma unroll
            for (int ks = 0; ks < KT / 32; ++ks) {
                // A[row lane & 15][k = 8 (lane >> 4) + j], B[k][col lane & 15] = dst row (lane & 15), the same k
                const bf16x8 af = *(const bf16x8*)(As + (wv * 16 + lrow) * PITCH + ks * 32 + lq * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16x8 bfr = *(const bf16x8*)(Bs + (j * 16 + lrow) * PITCH + ks * 32 + lq * 8);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[j], 0, 0, 0);
                }
            }
        }
        // accumulator: element r of lane = (src row 4 (lane >> 4) + r, dst column lane & 15) of sub-tile j.  Ascending dst order
        // with a strict compare: the lowest dst index wins a tie.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dl = j * 16 + lrow, d = d0 + dl;
            if (d < num_dst) {
                const float di = b_inv[dl];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sc = (acc[j][r] * a_inv[wv * 16 + lq * 4 + r]) * di;
                    if (sc > best[r]) { best[r] = sc; bidx[r] = d; }
                }
            }
        }
    }
    // the 16 lanes of a row group hold the candidates of 16 dst columns: reduce with (larger score, then lower index)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const float ov = __shfl_xor(best[r], o);
            const int oi = __shfl_xor(bidx[r], o);
            if (ov > best[r] || (ov == best[r] && oi < bidx[r])) { best[r] = ov; bidx[r] = oi; }
        }
        const int s = s0 + wv * 16 + lq * 4 + r;
        if (lrow == 0 && s < num_src) {
            node_max[(long)b * num_src + s] = best[r];
            node_idx[(long)b * num_src + s] = bidx[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// select: one block of 1024 threads per sample; thread t owns the items [t * ipt, (t + 1) * ipt)
// ---------------------------------------------------------------------------------------------
constexpr int SEL_THREADS = 1024;
constexpr int SEL_MAX_IPT = 12;          // 12288 scores at most

// order-preserving key: a larger score has a larger key; -0 and +0 share a key (they compare equal); NaN sorts lowest
__device__ __forceinline__ unsigned score_key(float f) {
    unsigned u = __builtin_bit_cast(unsigned, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix sum of one int per thread over the block (1024 threads = 16 waves); returns the total in `total`
__device__ __forceinline__ int block_exclusive_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(inc, o);
        if (lane >= o) inc += n;
    }
    __syncthreads();          // (wsum may still be read from the previous scan)
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < SEL_THREADS / 64; ++i) {
        const int s = wsum[i];
        if (i < wv) base += s;
        tot += s;
    }
    total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(SEL_THREADS) void tome_select_kernel(const float* __restrict__ node_max, const int* __restrict__ node_idx,
                                                                  int num_src, int r, int* __restrict__ kept, int* __restrict__ merged,
                                                                  int* __restrict__ dst_idx) {
    __shared__ int hist[256];
    __shared__ int wsum[SEL_THREADS / 64];
    __shared__ unsigned sh_prefix;
    __shared__ int sh_need;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int ipt = (num_src + SEL_THREADS - 1) / SEL_THREADS;
    const float* nm = node_max + (long)b * num_src;
    const int* ni = node_idx + (long)b * num_src;
    unsigned key[SEL_MAX_IPT];
#pragma unroll
    for (int i = 0; i < SEL_MAX_IPT; ++i) {
        const int s = tid * ipt + i;
        key[i] = (i < ipt && s < num_src) ? score_key(nm[s]) : 0u;
    }
    // radix select, 8 bits per pass from the top: the key T of the r-th largest score, and how many keys are above it
    unsigned prefix = 0;
    int need = r;          // how many of the keys that share the prefix are still wanted
    if (r > 0 && r < num_src) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
#pragma unroll
            for (int i = 0; i < SEL_MAX_IPT; ++i) {
                const int s = tid * ipt + i;
                if (i < ipt && s < num_src && (key[i] & himask) == prefix) atomicAdd(&hist[(key[i] >> shift) & 255], 1);
            }
            __syncthreads();
            if (tid < 64) {
                // the bin that holds the need-th largest key, by the first wave: lane l owns the bins 255 - 4 l - j (j = 0..3, descending),
                // an inclusive scan over the lanes counts the keys in the bins above (a serial walk over 256 bins by one thread
                // cost ~10 us per pass, four fifths of the kernel)
                int h4[4], loc = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h4[j] = hist[255 - 4 * tid - j]; loc += h4[j]; }
                int inc = loc;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int n = __shfl_up(inc, o);
                    if (tid >= o) inc += n;
                }
                const int above = inc - loc;
                if (above < need && need <= inc) {          // exactly one lane: 1 <= need <= the keys that share the prefix
                    int n = need - above, j = 0;
                    for (; j < 3; ++j) {
                        if (h4[j] >= n) break;
                        n -= h4[j];
                    }
                    sh_prefix = prefix | ((unsigned)(255 - 4 * tid - j) << shift);
                    sh_need = n;
                }
            }
            __syncthreads();
            prefix = sh_prefix;
            need = sh_need;
        }
    }
    // now: keys > prefix are merged, and the `need` lowest-indexed keys == prefix
    const bool all = r >= num_src, none = r <= 0;
    int n_eq = 0;
#pragma unroll
    for (int i = 0; i < SEL_MAX_IPT; ++i) {
        const int s = tid * ipt + i;
        n_eq += (i < ipt && s < num_src && key[i] == prefix);
    }
    int total;
    int eq_rank = block_exclusive_scan(n_eq, wsum, total);
    int n_m = 0;
    unsigned mflags = 0;
#pragma unroll
    for (int i = 0; i < SEL_MAX_IPT; ++i) {
        const int s = tid * ipt + i;
        if (i < ipt && s < num_src) {
            bool m;
            if (all) m = true;
            else if (none) m = false;
            else if (key[i] > prefix) m = true;
            else if (key[i] == prefix) m = eq_rank++ < need;
            else m = false;
            if (m) { mflags |= 1u << i; ++n_m; }
        }
    }
    int m_pos = block_exclusive_scan(n_m, wsum, total);
    int k_pos = tid * ipt - m_pos;          // items before this thread that are not merged
    if (k_pos > num_src) k_pos = num_src;   // (threads past the end own nothing)
    int* kb = kept + (long)b * (num_src - r);
    int* mb = merged + (long)b * r;
    int* db = dst_idx + (long)b * r;
#pragma unroll
    for (int i = 0; i < SEL_MAX_IPT; ++i) {
        const int s = tid * ipt + i;
        if (i < ipt && s < num_src) {
            if (mflags >> i & 1) {
                if (m_pos < r) { mb[m_pos] = s; db[m_pos] = ni[s]; }
                ++m_pos;
            } else {
                if (k_pos < num_src - r) kb[k_pos] = s;
                ++k_pos;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// merge: one wave per output row
// ---------------------------------------------------------------------------------------------
constexpr int ROW_CHUNKS = 3;          // 64 lanes x 8 elements x 3 = 1536 channels at most

__device__ __forceinline__ void row_add(float (&acc)[ROW_CHUNKS][8], const bf16_t* row, int C, int lane) {
#pragma unroll
    for (int c = 0; c < ROW_CHUNKS; ++c) {
        const int e = (c * 64 + lane) * 8;
        if (e < C) {
            const u32x4 v = *(const u32x4*)(row + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[c][2 * j] += bflo(v[j]); acc[c][2 * j + 1] += bfhi(v[j]); }
        }
    }
}

__global__ __launch_bounds__(256) void tome_merge_kernel(const bf16_t* __restrict__ x, const int* __restrict__ tok,
                                                         const int* __restrict__ kept, const int* __restrict__ merged,
                                                         const int* __restrict__ dst_idx, bf16_t* __restrict__ out, long ldo, int N, int C,
                                                         int num_src, int num_dst, int r) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int nk = num_src - r, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nk + num_dst) return;
    const bf16_t* xb = x + (long)b * N * C;
    bf16_t* orow = out + ((long)b * (nk + num_dst) + row) * ldo;
    if (row < nk) {          // a kept src row: copy
        const int s = kept[(long)b * nk + row];
        if ((unsigned)s >= (unsigned)num_src) return;
        const bf16_t* src = xb + (long)tok[s] * C;
        for (int e = lane * 8; e < C; e += 512) *(u32x4*)(orow + e) = *(const u32x4*)(src + e);
        return;
    }
    // a dst row: itself plus its members, in ascending position of the merged list (= ascending src index), fp32, rounded once
    const int d = row - nk;
    float acc[ROW_CHUNKS][8];
#pragma unroll
    for (int c = 0; c < ROW_CHUNKS; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[c][j] = 0.f;
    row_add(acc, xb + (long)tok[num_src + d] * C, C, lane);
    int count = 1;
    const int* mb = merged + (long)b * r;
    const int* db = dst_idx + (long)b * r;
    for (int i0 = 0; i0 < r; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < r && db[i] == d;
        const int s_lane = mine ? mb[i] : 0;
        unsigned long long m = __ballot(mine);
        while (m) {
            const int bit = __builtin_ctzll(m);
            m &= m - 1;
            const int s = __shfl(s_lane, bit);
            if ((unsigned)s < (unsigned)num_src) {
                row_add(acc, xb + (long)tok[s] * C, C, lane);
                ++count;
            }
        }
    }
    const float scale = 1.0f / (float)count;
#pragma unroll
    for (int c = 0; c < ROW_CHUNKS; ++c) {
        const int e = (c * 64 + lane) * 8;
        if (e < C) {
            u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = pack2bf(acc[c][2 * j] * scale, acc[c][2 * j + 1] * scale);
            *(u32x4*)(orow + e) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// unmerge: one wave per token; entry e of a sample is a kept src (e < nk), a dst (e < nk + num_dst) or a merged src
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tome_unmerge_kernel(const bf16_t* __restrict__ y, long ldy, const bf16_t* __restrict__ res,
                                                           const int* __restrict__ tok, const int* __restrict__ kept,
                                                           const int* __restrict__ merged, const int* __restrict__ dst_idx,
                                                           bf16_t* __restrict__ out, int N, int C, int num_src, int num_dst, int r) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int nk = num_src - r, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= N) return;
    int t, row;
    if (e < nk) {
        const int s = kept[(long)b * nk + e];
        if ((unsigned)s >= (unsigned)num_src) return;
        t = tok[s]; row = e;
    } else if (e < nk + num_dst) {
        t = tok[num_src + e - nk]; row = e;
    } else {
        const int j = e - nk - num_dst;
        const int s = merged[(long)b * r + j], d = dst_idx[(long)b * r + j];
        if ((unsigned)s >= (unsigned)num_src || (unsigned)d >= (unsigned)num_dst) return;
        t = tok[s]; row = nk + d;
    }
    const bf16_t* yr = y + ((long)b * (nk + num_dst) + row) * ldy;
    const bf16_t* rr = res ? res + ((long)b * N + t) * C : nullptr;
    for (int e8 = lane * 8; e8 < C; e8 += 512) {
        const u32x4 a = *(const u32x4*)(yr + e8);
        u32x4 o = a;
        if (rr) {
            const u32x4 c = *(const u32x4*)(rr + e8);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = pack2bf(bflo(a[j]) + bflo(c[j]), bfhi(a[j]) + bfhi(c[j]));
        }
        *(u32x4*)(out + ((long)b * N + t) * C + e8) = o;
    }
}

}  // namespace

int sd_tome_check(int h, int w, int C, const char* who) {
    SD_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && (long)h * w <= 16384, "%s: %dx%d tokens (even sides, at most 16384 tokens)", who, h, w);
    SD_REQUIRE(C >= 64 && C % 64 == 0 && C <= 1536, "%s: C=%d (a multiple of 64, at most 1536)", who, C);
    return 0;
}

int sd_launch_tome_partition(const unsigned char* choice, int h, int w, int* tok, hipStream_t stream) {
    SD_REQUIRE(choice && tok, "tome_partition: null argument");
    if (sd_tome_check(h, w, 64, "tome_partition")) return -1;
    const int N = h * w;
    hipLaunchKernelGGL(tome_partition_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, choice, h, w, tok);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_tome_match(const bf16_t* x, const unsigned char* choice, int B, int h, int w, int C, float* node_max, int* node_idx,
                         int* tok, float* inv, hipStream_t stream) {
    SD_REQUIRE(x && choice && node_max && node_idx && tok && inv && B >= 1 && B <= 65535, "tome_match: null argument or B=%d", B);
    if (sd_tome_check(h, w, C, "tome_match")) return -1;
    const int N = h * w, num_dst = (h / 2) * (w / 2), num_src = N - num_dst;
    if (int rc = sd_launch_tome_partition(choice, h, w, tok, stream)) return rc;
    const long rows = (long)B * N;
    hipLaunchKernelGGL(tome_rownorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, inv, rows, C);
    hipLaunchKernelGGL(tome_match_kernel, dim3((num_src + MT - 1) / MT, B), dim3(256), 0, stream, x, (const int*)tok, (const float*)inv,
                       node_max, node_idx, N, C, num_src, num_dst);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_tome_select(const float* node_max, const int* node_idx, int B, int num_src, int r, int* kept, int* merged, int* dst_idx,
                          hipStream_t stream) {
    SD_REQUIRE(node_max && node_idx && B >= 1, "tome_select: null argument");
    SD_REQUIRE(num_src >= 1 && num_src <= SEL_THREADS * SEL_MAX_IPT, "tome_select: %d scores per sample (at most %d)", num_src,
               SEL_THREADS * SEL_MAX_IPT);
    SD_REQUIRE(r >= 0 && r <= num_src, "tome_select: r=%d of %d", r, num_src);
    SD_REQUIRE((kept || r == num_src) && ((merged && dst_idx) || r == 0), "tome_select: null output");
    hipLaunchKernelGGL(tome_select_kernel, dim3(B), dim3(SEL_THREADS), 0, stream, node_max, node_idx, num_src, r, kept, merged, dst_idx);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_tome_merge(const bf16_t* x, const int* tok, const int* kept, const int* merged, const int* dst_idx, bf16_t* out,
                         long ldo, int B, int h, int w, int C, int r, hipStream_t stream) {
    SD_REQUIRE(x && tok && out && B >= 1 && B <= 65535, "tome_merge: null argument or B=%d", B);
    if (sd_tome_check(h, w, C, "tome_merge")) return -1;
    const int N = h * w, num_dst = (h / 2) * (w / 2), num_src = N - num_dst;
    SD_REQUIRE(r >= 0 && r <= num_src && ldo >= C && ldo % 8 == 0, "tome_merge: r=%d of %d, ldo=%ld", r, num_src, ldo);
    SD_REQUIRE((kept || r == num_src) && ((merged && dst_idx) || r == 0), "tome_merge: null index list");
    hipLaunchKernelGGL(tome_merge_kernel, dim3((N - r + 3) / 4, B), dim3(256), 0, stream, x, tok, kept, merged, dst_idx, out, ldo, N, C,
                       num_src, num_dst, r);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_tome_unmerge(const bf16_t* y, long ldy, const bf16_t* residual, const int* tok, const int* kept, const int* merged,
                           const int* dst_idx, bf16_t* out, int B, int h, int w, int C, int r, hipStream_t stream) {
    SD_REQUIRE(y && tok && out && B >= 1 && B <= 65535, "tome_unmerge: null argument or B=%d", B);
    if (sd_tome_check(h, w, C, "tome_unmerge")) return -1;
    const int N = h * w, num_dst = (h / 2) * (w / 2), num_src = N - num_dst;
    SD_REQUIRE(r >= 0 && r <= num_src && ldy >= C && ldy % 8 == 0, "tome_unmerge: r=%d of %d, ldy=%ld", r, num_src, ldy);
    SD_REQUIRE((kept || r == num_src) && ((merged && dst_idx) || r == 0), "tome_unmerge: null index list");
    hipLaunchKernelGGL(tome_unmerge_kernel, dim3((N + 3) / 4, B), dim3(256), 0, stream, y, ldy, residual, tok, kept, merged, dst_idx, out,
                       N, C, num_src, num_dst, r);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
