// The end of every sampling step: the fused CFG-combine + scheduler.step update (optional per-sample rescale, optional
// inpainting blend), the rescaled-CFG factors, UniPC's predictor-corrector step, and their C entry points: five plain ones and
// the three perturbed-attention-guidance (PAG) forms of the step, the predictor-corrector step and the factors, and the two
// self-attention-guidance (SAG) forms of the step and the predictor-corrector step.
#include "common.h"
#include "kernels.h"
#include "../../include/sd_hip.h"

namespace {

__device__ __forceinline__ f32x4 cfg_combine(f32x4 e, f32x4 et, float guidance) { return e + guidance * (et - e); }

// perturbed-attention guidance on top of a combined prediction g: g + s (c - p), c the conditional and p the perturbed output
__device__ __forceinline__ f32x4 pag_combine(f32x4 g, f32x4 c, f32x4 p, float pag) { return g + pag * (c - p); }

// the prediction a step works on: eps, combined as the guidance mode `cfg` says, scaled by its sample's factor when RESCALED.
//   0: eps as it is     1 (CFG): eps = [u | c], u + g (c - u)
//   SD_GUIDE_CFG_PAG: eps = [u | c | p], (u + g (c - u)) + s (c - p)     SD_GUIDE_PAG: eps = [c | p], c + s (c - p)
//   SD_GUIDE_CFG_SAG: eps = [u | c | d], (u + g (c - u)) + s (u - d)     SD_GUIDE_SAG: eps = [c | d], c + s (c - d)
template <bool RESCALED>
__device__ __forceinline__ f32x4 step_eps(const float* __restrict__ eps, int cfg, float guidance, float pag,
                                          const float* __restrict__ k, long n4s, long n4, long i) {
    f32x4 e = ((const f32x4*)eps)[i];
    if (cfg == 1) e = cfg_combine(e, ((const f32x4*)eps)[i + n4], guidance);
    else if (cfg == SD_GUIDE_CFG_PAG) {
        const f32x4 c = ((const f32x4*)eps)[i + n4];
        e = pag_combine(cfg_combine(e, c, guidance), c, ((const f32x4*)eps)[i + 2 * n4], pag);
    } else if (cfg == SD_GUIDE_CFG_SAG) {
        e = pag_combine(cfg_combine(e, ((const f32x4*)eps)[i + n4], guidance), e, ((const f32x4*)eps)[i + 2 * n4], pag);
    } else if (cfg == SD_GUIDE_PAG || cfg == SD_GUIDE_SAG) e = pag_combine(e, e, ((const f32x4*)eps)[i + n4], pag);
    if (RESCALED) e = k[i / n4s] * e;
    return e;
}

// inpainting with a 4-channel UNet: p := mask ? p : a * init + s * blend_noise, mask [B][1][hw] broadcast over the channels.
// s == 0 (after the last step: a = 1) skips the noise term, so the kept side is then a * init alone.
__device__ __forceinline__ f32x4 latent_blend(f32x4 p, const float* __restrict__ init, const float* __restrict__ blend_noise,
                                              const float* __restrict__ mask, float a, float s, long n4s, long hw4, long i) {
    const long b = i / n4s;
    const f32x4 mk = ((const f32x4*)mask)[b * hw4 + (i - b * n4s) % hw4];
    f32x4 keep = a * ((const f32x4*)init)[i];
    if (s != 0.f) keep += s * ((const f32x4*)blend_noise)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = mk[j] >= 0.5f ? p[j] : keep[j];
    return p;
}

// ---- fused CFG + scheduler update ---------------------------------------------------------
// RESCALED: e := k[b] * e before every use.  BLEND: the latent blend of prev; y2 and m_out do not see the mask.  An
// instantiation without one of them does not read that one's arguments.
template <bool RESCALED, bool BLEND>
__global__ void sched_step_kernel(const float* __restrict__ eps, int cfg, float guidance, float pag,
                                  const float* __restrict__ x, const float* __restrict__ m1,
                                  const float* __restrict__ m2, const float* __restrict__ m3,
                                  const float* __restrict__ noise, float* __restrict__ prev,
                                  float* __restrict__ y2, float* __restrict__ m_out, StepCoef c,
                                  const float* __restrict__ k, long n4s, long n4, const float* __restrict__ init,
                                  const float* __restrict__ blend_noise, const float* __restrict__ mask, float a,
                                  float s, long hw4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 e = step_eps<RESCALED>(eps, cfg, guidance, pag, k, n4s, n4, i);
    const f32x4 xv = ((const f32x4*)x)[i];
    f32x4 p = c.px * xv + c.pe * e;
    if (m1) p += c.p1 * ((const f32x4*)m1)[i];
    if (m2) p += c.p2 * ((const f32x4*)m2)[i];
    if (m3) p += c.p3 * ((const f32x4*)m3)[i];
    if (noise) p += c.pn * ((const f32x4*)noise)[i];
    if (y2) ((f32x4*)y2)[i] = c.yx * xv + c.ye * e;
    if (m_out) ((f32x4*)m_out)[i] = c.mx * xv + c.me * e;
    if (BLEND) p = latent_blend(p, init, blend_noise, mask, a, s, n4s, hw4, i);
    ((f32x4*)prev)[i] = p;
}

// ---- rescaled CFG (guidance_rescale): per-sample factor k_b, then the step with e := k_b * e ---------------------------
// g = u + s (c - u) is formed exactly as the step above forms it (same expression, same unit), so the std the factor sees
// is the std of the values the step scales.  One block per sample, fixed thread -> element assignment, double partials,
// wave butterflies and an in-order sum of the wave partials: k_b depends on sample b's data and n_per_sample only (not on
// the batch, the sample's position or the grid) -- dist.py's sharding invariant.  Two passes (mean, then centred sum).
// with_pag: eps = [u | c | p] and g carries the PAG term, as the step's does.
constexpr int RESCALE_THREADS = 512;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// in-order block sum of two doubles; every thread gets the totals
__device__ __forceinline__ void block_sum2_f64(double& a, double& b, double (*red)[RESCALE_THREADS / 64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum_f64(a);
    b = wave_sum_f64(b);
    if (lane == 0) {
        red[0][wave] = a;
        red[1][wave] = b;
    }
    __syncthreads();
    a = 0.0;
    b = 0.0;
#pragma unroll
    for (int w = 0; w < RESCALE_THREADS / 64; ++w) {
        a += red[0][w];
        b += red[1][w];
    }
    __syncthreads();
}

__global__ __launch_bounds__(RESCALE_THREADS) void cfg_rescale_factors_kernel(const float* __restrict__ eps, int batch,
                                                                              long n4s, float guidance, float rescale,
                                                                              float* __restrict__ k_out, int with_pag,
                                                                              float pag) {
    __shared__ double red[2][RESCALE_THREADS / 64];
    const int b = blockIdx.x;
    const f32x4* u = (const f32x4*)eps + (long)b * n4s;
    const f32x4* c = (const f32x4*)eps + ((long)batch + b) * n4s;
    const f32x4* p = (const f32x4*)eps + (2l * batch + b) * n4s;      // (the perturbed third: read with_pag only)
    double sc = 0.0, sg = 0.0;
    for (long i = threadIdx.x; i < n4s; i += RESCALE_THREADS) {
        const f32x4 et = c[i];
        f32x4 g = cfg_combine(u[i], et, guidance);
        if (with_pag) g = pag_combine(g, et, p[i], pag);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sc += (double)et[j];
            sg += (double)g[j];
        }
    }
    block_sum2_f64(sc, sg, red);
    const double n = 4.0 * (double)n4s;
    const double mc = sc / n, mg = sg / n;
    double qc = 0.0, qg = 0.0;
    for (long i = threadIdx.x; i < n4s; i += RESCALE_THREADS) {
        const f32x4 et = c[i];
        f32x4 g = cfg_combine(u[i], et, guidance);
        if (with_pag) g = pag_combine(g, et, p[i], pag);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double dc = (double)et[j] - mc, dg = (double)g[j] - mg;
            qc += dc * dc;
            qg += dg * dg;
        }
    }
    block_sum2_f64(qc, qg, red);
    // std(c) / std(g): the (n - 1) of torch.std cancels in the ratio
    if (threadIdx.x == 0) k_out[b] = (float)((double)rescale * sqrt(qc / qg) + (1.0 - (double)rescale));
}

// ---- UniPC: corrector and predictor of one step in one launch -----------------------------------------------------------
// e as sched_step_kernel forms it (step_eps), then
//   m_t  = cm0 x + cm1 e                                        (history entry)
//   y2   = cy0 x + cy1 e                                        (x0 prediction)
//   xc   = cc0 x_last + cc1 h1 + cc2 h2 + cc3 h3 + cc4 m_t      (corrector; x_last null: xc = x, the bits of x)
//   prev = cp0 xc + cp1 m_t + cp2 h1 + cp3 h2                   (predictor)
// and BLEND: latent_blend of prev.  Terms are added left to right; a null h term is skipped (the host side has checked that
// its coefficients are 0).  x_corr, y2 and m_out do not see the mask.
template <bool RESCALED, bool BLEND>
__global__ void sched_step_pc_kernel(const float* __restrict__ eps, int cfg, float guidance, float pag,
                                     const float* __restrict__ x,
                                     const float* __restrict__ x_last, const float* __restrict__ h1,
                                     const float* __restrict__ h2, const float* __restrict__ h3, float* __restrict__ prev,
                                     float* __restrict__ x_corr, float* __restrict__ y2, float* __restrict__ m_out,
                                     PcCoef c, const float* __restrict__ k, long n4s, long n4,
                                     const float* __restrict__ init, const float* __restrict__ blend_noise,
                                     const float* __restrict__ mask, float a, float s, long hw4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 e = step_eps<RESCALED>(eps, cfg, guidance, pag, k, n4s, n4, i);
    const f32x4 xv = ((const f32x4*)x)[i];
    const f32x4 mt = c.cm[0] * xv + c.cm[1] * e;
    f32x4 v1 = {0.f, 0.f, 0.f, 0.f}, v2 = v1;
    if (h1) v1 = ((const f32x4*)h1)[i];
    if (h2) v2 = ((const f32x4*)h2)[i];
    f32x4 xc = xv;
    if (x_last) {
        xc = c.cc[0] * ((const f32x4*)x_last)[i];
        if (h1) xc += c.cc[1] * v1;
        if (h2) xc += c.cc[2] * v2;
        if (h3) xc += c.cc[3] * ((const f32x4*)h3)[i];
        xc += c.cc[4] * mt;
    }
    f32x4 p = c.cp[0] * xc + c.cp[1] * mt;
    if (h1) p += c.cp[2] * v1;
    if (h2) p += c.cp[3] * v2;
    if (x_corr) ((f32x4*)x_corr)[i] = xc;
    if (y2) ((f32x4*)y2)[i] = c.cy[0] * xv + c.cy[1] * e;
    if (m_out) ((f32x4*)m_out)[i] = mt;
    if (BLEND) p = latent_blend(p, init, blend_noise, mask, a, s, n4s, hw4, i);
    ((f32x4*)prev)[i] = p;
}

}  // namespace

// ---- host checks the step and the predictor-corrector launchers share; `who` is the entry's name in the message -------
static int check_size(const char* who, const float* eps, const float* x, const float* prev, long n) {
    SD_REQUIRE(eps && x && prev, "%s: null operand", who);
    SD_REQUIRE(n > 0 && n % 4 == 0, "%s: n=%ld must be a positive multiple of 4", who, n);
    return 0;
}

static int check_per_sample(const char* who, long n_per_sample, long n) {
    SD_REQUIRE(n_per_sample > 0 && n_per_sample % 4 == 0 && n % n_per_sample == 0,
               "%s: n_per_sample=%ld must be a positive multiple of 4 dividing n=%ld", who, n_per_sample, n);
    return 0;
}

static int check_blend(const char* who, const float* blend_noise, const float* mask, float s, long hw, long n_per_sample) {
    SD_REQUIRE(mask, "%s: null operand (mask)", who);
    SD_REQUIRE(blend_noise || s == 0.f, "%s: s=%g needs blend_noise", who, (double)s);
    SD_REQUIRE(hw > 0 && hw % 4 == 0, "%s: hw=%ld must be a positive multiple of 4", who, hw);
    SD_REQUIRE(n_per_sample % hw == 0, "%s: n_per_sample=%ld must be a multiple of hw=%ld", who, n_per_sample, hw);
    return 0;
}

// kernel<RESCALED, BLEND> from (k != nullptr, init != nullptr), one thread per 16-byte vector
#define SD_LAUNCH_STEP(kernel, n4, ...)                                                                               \
    do {                                                                                                              \
        const dim3 grid((unsigned)(((n4) + 255) / 256));                                                              \
        if (k && init) hipLaunchKernelGGL((kernel<true, true>), grid, dim3(256), 0, stream, __VA_ARGS__);             \
        else if (k) hipLaunchKernelGGL((kernel<true, false>), grid, dim3(256), 0, stream, __VA_ARGS__);               \
        else if (init) hipLaunchKernelGGL((kernel<false, true>), grid, dim3(256), 0, stream, __VA_ARGS__);            \
        else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(256), 0, stream, __VA_ARGS__);                     \
    } while (0)

int sd_launch_sched_step(const char* who, const float* eps, int cfg, float guidance, float pag, const float* x, const float* m1,
                         const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                         StepCoef c, const float* k, long n_per_sample, long n, const float* init, const float* blend_noise,
                         const float* mask, float a, float s, long hw, hipStream_t stream) {
    if (int rc = check_size(who, eps, x, prev, n)) return rc;
    const bool per_sample = k || init;          // (neither: n_per_sample is not read)
    if (per_sample)
        if (int rc = check_per_sample(who, n_per_sample, n)) return rc;
    if (init)
        if (int rc = check_blend(who, blend_noise, mask, s, hw, n_per_sample)) return rc;
    const long n4 = n / 4, n4s = per_sample ? n_per_sample / 4 : n4, hw4 = init ? hw / 4 : 1;
    SD_LAUNCH_STEP(sched_step_kernel, n4, eps, cfg, guidance, pag, x, m1, m2, m3, noise, prev, y2, m_out, c, k, n4s, n4, init,
                   blend_noise, mask, a, s, hw4);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

int sd_launch_cfg_rescale_factors(const float* eps, int batch, long n_per_sample, float guidance, float rescale, float* k_out,
                                  hipStream_t stream, int with_pag, float pag) {
    SD_REQUIRE(eps && k_out, "cfg_rescale_factors: null operand");
    SD_REQUIRE(batch > 0 && batch <= 65535, "cfg_rescale_factors: batch=%d", batch);
    SD_REQUIRE(n_per_sample >= 4 && n_per_sample % 4 == 0,
               "cfg_rescale_factors: n_per_sample=%ld must be a positive multiple of 4", n_per_sample);
    hipLaunchKernelGGL(cfg_rescale_factors_kernel, dim3(batch), dim3(RESCALE_THREADS), 0, stream, eps, batch,
                       n_per_sample / 4, guidance, rescale, k_out, with_pag, pag);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}

// [p, p + bytes) and [q, q + bytes_q) share a byte
static bool pc_overlap(const void* p, size_t bytes, const void* q, size_t bytes_q) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + bytes_q && b < a + bytes;
}

int sd_launch_sched_step_pc(const char* who, const float* eps, int cfg, float guidance, float pag, const float* x, const float* x_last, const float* h1,
                            const float* h2, const float* h3, float* prev, float* x_corr, float* y2, float* m_out, PcCoef c,
                            const float* k, long n_per_sample, long n, const float* init, const float* blend_noise,
                            const float* mask, float a, float s, long hw, hipStream_t stream) {
    if (int rc = check_size(who, eps, x, prev, n)) return rc;
    if (int rc = check_per_sample(who, n_per_sample, n)) return rc;
    if (init) {
        if (int rc = check_blend(who, blend_noise, mask, s, hw, n_per_sample)) return rc;
        SD_REQUIRE(std::isfinite(a) && std::isfinite(s), "%s: blend coefficients a=%g s=%g must be finite", who,
                   (double)a, (double)s);
    }
    SD_REQUIRE(std::isfinite(guidance), "%s: guidance=%g must be finite", who, (double)guidance);
    const float* rows[4] = {c.cm, c.cy, c.cc, c.cp};
    const char* row_names[4] = {"cm", "cy", "cc", "cp"};
    const int row_len[4] = {2, 2, 5, 4};
    for (int r = 0; r < 4; ++r)
        for (int j = 0; j < row_len[r]; ++j)
            SD_REQUIRE(std::isfinite(rows[r][j]), "%s: coefficient %s[%d]=%g must be finite", who, row_names[r], j,
                       (double)rows[r][j]);
    // a null history entry carries no weight (the corrector's row is not read without x_last)
    SD_REQUIRE(h1 || (c.cp[2] == 0.f && (!x_last || c.cc[1] == 0.f)), "%s: h1 is null but has a coefficient", who);
    SD_REQUIRE(h2 || (c.cp[3] == 0.f && (!x_last || c.cc[2] == 0.f)), "%s: h2 is null but has a coefficient", who);
    SD_REQUIRE(h3 || !x_last || c.cc[3] == 0.f, "%s: h3 is null but has a coefficient", who);
    const size_t nb = (size_t)n * 4, batch = (size_t)(n / n_per_sample);
    const void* outs[4] = {prev, x_corr, y2, m_out};
    const char* out_names[4] = {"prev", "x_corr", "y2", "m_out"};
    const void* ins[10] = {eps, x, x_last, h1, h2, h3, k, init, blend_noise, mask};
    const char* in_names[10] = {"eps", "x", "x_last", "h1", "h2", "h3", "k", "init", "blend_noise", "mask"};
    const size_t in_bytes[10] = {cfg == SD_GUIDE_CFG_PAG || cfg == SD_GUIDE_CFG_SAG ? 3 * nb : cfg ? 2 * nb : nb, nb, nb, nb, nb, nb, batch * 4, nb, nb, init ? batch * (size_t)hw * 4 : 0};
    for (int o = 0; o < 4; ++o) {
        for (int j = 0; j < 10; ++j)
            SD_REQUIRE(!pc_overlap(outs[o], nb, ins[j], in_bytes[j]), "%s: output %s aliases input %s", who, out_names[o],
                       in_names[j]);
        for (int q = 0; q < o; ++q)
            SD_REQUIRE(!pc_overlap(outs[o], nb, outs[q], nb), "%s: output %s aliases output %s", who, out_names[o],
                       out_names[q]);
    }
    const long n4 = n / 4, n4s = n_per_sample / 4, hw4 = init ? hw / 4 : 1;
    SD_LAUNCH_STEP(sched_step_pc_kernel, n4, eps, cfg, guidance, pag, x, x_last, h1, h2, h3, prev, x_corr, y2, m_out, c, k, n4s,
                   n4, init, blend_noise, mask, a, s, hw4);
    SD_CHECK_HIP(hipGetLastError());
    return 0;
}
#undef SD_LAUNCH_STEP

// ---- the C entry points (include/sd_hip.h) ---------------------------------------------------------------------------
static StepCoef step_coef(const float coef[10]) {
    return StepCoef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
}

extern "C" int sd_sched_step(void* stream, const float* eps, int cfg, float guidance, const float* x, const float* m1,
                             const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                             const float coef[10], long long n) {
    SD_REQUIRE(coef, "sched_step: null coefficients");
    return sd_launch_sched_step("sched_step", eps, cfg != 0, guidance, 0.f, x, m1, m2, m3, noise, prev, y2, m_out, step_coef(coef),
                                nullptr, 0, (long)n, nullptr, nullptr, nullptr, 1.f, 0.f, 0, (hipStream_t)stream);
}

extern "C" int sd_cfg_rescale_factors(void* stream, const float* eps, int batch, long long n_per_sample, float guidance,
                                      float rescale, float* k_out) {
    return sd_launch_cfg_rescale_factors(eps, batch, (long)n_per_sample, guidance, rescale, k_out, (hipStream_t)stream);
}

extern "C" int sd_sched_step_rescaled(void* stream, const float* eps, int cfg, float guidance, const float* x,
                                      const float* m1, const float* m2, const float* m3, const float* noise, float* prev,
                                      float* y2, float* m_out, const float coef[10], long long n, const float* k,
                                      long long n_per_sample) {
    SD_REQUIRE(coef, "sched_step_rescaled: null coefficients");
    SD_REQUIRE(k, "sched_step_rescaled: null operand");
    return sd_launch_sched_step("sched_step_rescaled", eps, cfg != 0, guidance, 0.f, x, m1, m2, m3, noise, prev, y2, m_out,
                                step_coef(coef), k, (long)n_per_sample, (long)n, nullptr, nullptr, nullptr, 1.f, 0.f, 0,
                                (hipStream_t)stream);
}

extern "C" int sd_sched_step_inpaint(void* stream, const float* eps, int cfg, float guidance, const float* x, const float* m1,
                                     const float* m2, const float* m3, const float* noise, float* prev, float* y2,
                                     float* m_out, const float coef[10], long long n, const float* k, long long n_per_sample,
                                     const float* init, const float* blend_noise, const float* mask, float a, float s,
                                     long long hw) {
    SD_REQUIRE(coef, "sched_step_inpaint: null coefficients");
    SD_REQUIRE(init && mask, "sched_step_inpaint: null operand");
    return sd_launch_sched_step("sched_step_inpaint", eps, cfg != 0, guidance, 0.f, x, m1, m2, m3, noise, prev, y2, m_out,
                                step_coef(coef), k, (long)n_per_sample, (long)n, init, blend_noise, mask, a, s, (long)hw,
                                (hipStream_t)stream);
}

extern "C" int sd_sched_step_pc(void* stream, const float* eps, int cfg, float guidance, const float* x, const float* x_last,
                                const float* h1, const float* h2, const float* h3, float* prev, float* x_corr, float* y2,
                                float* m_out, const float coef[13], long long n, const float* k, long long n_per_sample,
                                const float* init, const float* blend_noise, const float* mask, float a, float s,
                                long long hw) {
    SD_REQUIRE(coef, "sched_step_pc: null coefficients");
    PcCoef c{{coef[0], coef[1]}, {coef[2], coef[3]}, {coef[4], coef[5], coef[6], coef[7], coef[8]},
             {coef[9], coef[10], coef[11], coef[12]}};
    return sd_launch_sched_step_pc("sched_step_pc", eps, cfg != 0, guidance, 0.f, x, x_last, h1, h2, h3, prev, x_corr, y2, m_out, c, k,
                                   (long)n_per_sample, (long)n, init, blend_noise, mask, a, s, (long)hw, (hipStream_t)stream);
}

// ---- perturbed-attention guidance: the same launchers with a PAG guidance mode ----------------------------------------
static int check_pag(const char* who, int mode, float guidance, float pag_scale) {
    SD_REQUIRE(mode == SD_GUIDE_CFG_PAG || mode == SD_GUIDE_PAG, "%s: mode=%d (SD_GUIDE_CFG_PAG = %d or SD_GUIDE_PAG = %d)", who, mode,
               SD_GUIDE_CFG_PAG, SD_GUIDE_PAG);
    SD_REQUIRE(std::isfinite(guidance), "%s: guidance=%g must be finite", who, (double)guidance);
    SD_REQUIRE(std::isfinite(pag_scale), "%s: pag_scale=%g must be finite", who, (double)pag_scale);
    return 0;
}

extern "C" int sd_sched_step_pag(void* stream, const float* eps, int mode, float guidance, float pag_scale, const float* x,
                                 const float* m1, const float* m2, const float* m3, const float* noise, float* prev, float* y2,
                                 float* m_out, const float coef[10], long long n, const float* k, long long n_per_sample,
                                 const float* init, const float* blend_noise, const float* mask, float a, float s, long long hw) {
    SD_REQUIRE(coef, "sched_step_pag: null coefficients");
    if (int rc = check_pag("sched_step_pag", mode, guidance, pag_scale)) return rc;
    return sd_launch_sched_step("sched_step_pag", eps, mode, guidance, pag_scale, x, m1, m2, m3, noise, prev, y2, m_out,
                                step_coef(coef), k, (long)n_per_sample, (long)n, init, blend_noise, mask, a, s, (long)hw,
                                (hipStream_t)stream);
}

extern "C" int sd_sched_step_pc_pag(void* stream, const float* eps, int mode, float guidance, float pag_scale, const float* x,
                                    const float* x_last, const float* h1, const float* h2, const float* h3, float* prev,
                                    float* x_corr, float* y2, float* m_out, const float coef[13], long long n, const float* k,
                                    long long n_per_sample, const float* init, const float* blend_noise, const float* mask,
                                    float a, float s, long long hw) {
    SD_REQUIRE(coef, "sched_step_pc_pag: null coefficients");
    if (int rc = check_pag("sched_step_pc_pag", mode, guidance, pag_scale)) return rc;
    PcCoef c{{coef[0], coef[1]}, {coef[2], coef[3]}, {coef[4], coef[5], coef[6], coef[7], coef[8]},
             {coef[9], coef[10], coef[11], coef[12]}};
    return sd_launch_sched_step_pc("sched_step_pc_pag", eps, mode, guidance, pag_scale, x, x_last, h1, h2, h3, prev, x_corr, y2, m_out, c,
                                   k, (long)n_per_sample, (long)n, init, blend_noise, mask, a, s, (long)hw, (hipStream_t)stream);
}

extern "C" int sd_cfg_rescale_factors_pag(void* stream, const float* eps, int batch, long long n_per_sample, float guidance,
                                          float pag_scale, float rescale, float* k_out) {
    if (int rc = check_pag("cfg_rescale_factors_pag", SD_GUIDE_CFG_PAG, guidance, pag_scale)) return rc;
    return sd_launch_cfg_rescale_factors(eps, batch, (long)n_per_sample, guidance, rescale, k_out, (hipStream_t)stream, 1, pag_scale);
}

// ---- self-attention guidance: the same launchers with a SAG guidance mode (the scale rides in the PAG slot) -----------------
static int check_sag(const char* who, int mode, float guidance, float sag_scale) {
    SD_REQUIRE(mode == SD_GUIDE_CFG_SAG || mode == SD_GUIDE_SAG, "%s: mode=%d (SD_GUIDE_CFG_SAG = %d or SD_GUIDE_SAG = %d)", who, mode,
               SD_GUIDE_CFG_SAG, SD_GUIDE_SAG);
    SD_REQUIRE(std::isfinite(guidance), "%s: guidance=%g must be finite", who, (double)guidance);
    SD_REQUIRE(std::isfinite(sag_scale), "%s: sag_scale=%g must be finite", who, (double)sag_scale);
    return 0;
}

extern "C" int sd_sched_step_sag(void* stream, const float* eps, int mode, float guidance, float sag_scale, const float* x,
                                 const float* m1, const float* m2, const float* m3, const float* noise, float* prev, float* y2,
                                 float* m_out, const float coef[10], long long n, const float* k, long long n_per_sample,
                                 const float* init, const float* blend_noise, const float* mask, float a, float s, long long hw) {
    SD_REQUIRE(coef, "sched_step_sag: null coefficients");
    if (int rc = check_sag("sched_step_sag", mode, guidance, sag_scale)) return rc;
    return sd_launch_sched_step("sched_step_sag", eps, mode, guidance, sag_scale, x, m1, m2, m3, noise, prev, y2, m_out,
                                step_coef(coef), k, (long)n_per_sample, (long)n, init, blend_noise, mask, a, s, (long)hw,
                                (hipStream_t)stream);
}

extern "C" int sd_sched_step_pc_sag(void* stream, const float* eps, int mode, float guidance, float sag_scale, const float* x,
                                    const float* x_last, const float* h1, const float* h2, const float* h3, float* prev,
                                    float* x_corr, float* y2, float* m_out, const float coef[13], long long n, const float* k,
                                    long long n_per_sample, const float* init, const float* blend_noise, const float* mask,
                                    float a, float s, long long hw) {
    SD_REQUIRE(coef, "sched_step_pc_sag: null coefficients");
    if (int rc = check_sag("sched_step_pc_sag", mode, guidance, sag_scale)) return rc;
    PcCoef c{{coef[0], coef[1]}, {coef[2], coef[3]}, {coef[4], coef[5], coef[6], coef[7], coef[8]},
             {coef[9], coef[10], coef[11], coef[12]}};
    return sd_launch_sched_step_pc("sched_step_pc_sag", eps, mode, guidance, sag_scale, x, x_last, h1, h2, h3, prev, x_corr, y2, m_out, c,
                                   k, (long)n_per_sample, (long)n, init, blend_noise, mask, a, s, (long)hw, (hipStream_t)stream);
}
