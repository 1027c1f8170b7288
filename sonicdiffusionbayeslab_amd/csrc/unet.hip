// libsdhip host side: error plumbing, the zero page, run_op (one plan op -> one launch) and the C ABI of the handles declared
// in include/sd_hip.h (UNet, VAE decoder / encoder, CLIP text / vision).  The data model is model.h, the weight packer pack.hip,
// the plan builder plan.hip, the operator-level entry points ops.hip.
//
// Replaces diffusers' UNet2DConditionModel.forward as called at src/models.py:227-235 of the
// reference, plus DeepCacheSDHelper's skip path (src/experiments/deep_cache.py:24-29) and the
// CFG + scheduler.step glue (src/models.py:238-261).
#include "model.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void sd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* sd_last_error(void) { return g_err; }
// (the latent-size entry points -- the _hw forms, sd_op_conv3x3_kernel, sd_op_softmax_rows -- are additions under version 3:
// resolve them by name; so are sd_unet_set_timestep_cond, sd_op_timestep_cond and sd_unet_config.time_cond_proj_dim, appended
// last: a caller zero-initialises the struct)
extern "C" int sd_abi_version(void) { return 3; }   // 2: sd_unet_config.weight_dtype, fp8 entry points; 3: round-2 fusion entry points

// ---------------------------------------------------------------------------------------------
// zero page, run_op
// ---------------------------------------------------------------------------------------------
static void* g_zero_page = nullptr;

namespace sdhip {

int ensure_zero_page() {
    if (g_zero_page) return 0;
    SD_CHECK_HIP(hipMalloc(&g_zero_page, 4096));
    SD_CHECK_HIP(hipMemset(g_zero_page, 0, 4096));
    const unsigned short one_chunk[8] = {0x3F80, 0, 0, 0, 0, 0, 0, 0};   // bf16 1.0 then zeros (attention ones column)
    SD_CHECK_HIP(hipMemcpy((char*)g_zero_page + 256, one_chunk, sizeof(one_chunk), hipMemcpyHostToDevice));
    return 0;
}
const void* zero_page() { return g_zero_page; }

int run_op(sd_unet* u, const Plan& pl, const Op& o, char* ws, const float* latents, int latent_batch, float* eps_out,
           float timestep, hipStream_t stream) {
    auto T = [&](int id) -> char* { return id >= 0 ? ws + pl.tensors[id].off : id == T_EPS ? (char*)eps_out : nullptr; };
    const char* wb = u->dweights;
    switch (o.kind) {
        case OP_SINUSOID:
            if (u->cond_set) return sd_launch_timestep_sinusoid_row(timestep, u->dcond, (float*)T(o.out), o.N, stream);
            return sd_launch_timestep_sinusoid(timestep, (float*)T(o.out), o.N, stream);
        case OP_GEMV:
            return sd_launch_gemv((const float*)T(o.x1), (const bf16_t*)(wb + o.w), (const float*)(wb + o.b),
                                  (float*)T(o.out), o.N, o.K, o.silu_in, stream);
        case OP_CONV_IN:
            if (u->kind == 0 && o.Cin == 9) {
                SD_REQUIRE(u->inpaint_b > 0, "forward: this UNet has in_channels = 9 and no inpainting condition is set "
                                             "(sd_unet_set_inpaint_cond_hw: mask and masked-image latents)");
                SD_REQUIRE(u->inpaint_h == o.Hin && u->inpaint_w == o.Win && o.B % u->inpaint_b == 0,
                           "forward: the inpainting condition was set for batch %d at %dx%d, the forward runs batch %d at %dx%d",
                           u->inpaint_b, u->inpaint_h, u->inpaint_w, o.B, o.Hin, o.Win);
                return sd_launch_conv_in_cond(latents, latent_batch, u->dinpaint, u->inpaint_b, (const float*)(wb + o.w),
                                              (const float*)(wb + o.b), (bf16_t*)T(o.out), o.B, o.Hin, o.Win, o.N, stream);
            }
            if (u->kind == 5) {
                SD_REQUIRE(u->cn_b > 0, "controlnet_forward: no conditioning image is set (sd_controlnet_set_cond_hw)");
                SD_REQUIRE(u->cn_h == o.Hin && u->cn_w == o.Win && o.B % u->cn_b == 0,
                           "controlnet_forward: the conditioning image was set for batch %d at %dx%d, the forward runs batch %d at %dx%d",
                           u->cn_b, u->cn_h, u->cn_w, o.B, o.Hin, o.Win);
                return sd_launch_conv_in_add(latents, latent_batch, u->cn_embed, u->cn_b, (const float*)(wb + o.w),
                                             (const float*)(wb + o.b), (bf16_t*)T(o.out), o.B, o.Hin, o.Win, o.N, stream);
            }
            return sd_launch_conv_in(o.x1 >= 0 ? (const float*)T(o.x1) : latents, o.x1 >= 0 ? o.B : latent_batch,
                                     (const float*)(wb + o.w), (const float*)(wb + o.b), (bf16_t*)T(o.out), o.B, o.Hin,
                                     o.Win, o.Cin, o.N, stream);
        case OP_PQCONV:
            return sd_launch_pqconv(latents, (const float*)(wb + o.w), (const float*)(wb + o.b), (float*)T(o.out), o.B,
                                    o.HW, timestep /* carries the latent scale for the VAE */, stream);
        case OP_SOFTMAX:
            if (o.N > 4096) return sd_launch_softmax_rows_long((bf16_t*)T(o.x1), o.M, o.N, o.scale, stream);
            return sd_launch_softmax_rows((bf16_t*)T(o.x1), o.M, o.N, o.scale, stream);
        case OP_GN: {
            GroupNormArgs a;
            a.x1 = (const bf16_t*)T(o.x1); a.C1 = o.C1; a.x2 = (const bf16_t*)T(o.x2); a.C2 = o.C2;
            a.gamma = (const float*)(wb + o.g); a.beta = (const float*)(wb + o.be);
            a.y = (bf16_t*)T(o.out); a.partial = (float*)T(o.aux);
            a.B = o.B; a.HW = o.HW; a.groups = u->cfg.norm_num_groups; a.nsplit = o.nsplit; a.eps = o.eps; a.silu = o.silu;
            a.out_fp8 = o.out_fp8; a.Cpad = o.Cpad; a.oscale = o.os;
            a.stats1 = (const float*)T(o.s1); a.stats2 = (const float*)T(o.s2);
            if (o.slab_t >= 0) {
                a.slab = (const float*)T(o.slab_t); a.splitk = o.slab_k; a.x1w = (bf16_t*)T(o.x1);
                a.sbias = o.slab_b != NOFF ? (const float*)(wb + o.slab_b) : nullptr;
                a.sbias2 = o.slab_b2t >= 0 ? (const float*)T(o.slab_b2t) + o.slab_b2idx : nullptr;
                a.sR = (const bf16_t*)T(o.slab_r); a.sldr = o.C1;
            }
            return sd_launch_groupnorm(a, stream);
        }
        case OP_CONV3: {
            GemmArgs a;
            a.X = (const bf16_t*)T(o.x1); a.W = (const bf16_t*)(wb + o.w); a.bias = (const float*)(wb + o.b);
            a.bias2 = o.b2t >= 0 ? (const float*)T(o.b2t) + o.b2idx : nullptr;
            a.R = (const bf16_t*)T(o.r); a.ldr = o.N; a.C = (bf16_t*)T(o.out); a.ldc = o.N;
            a.M = o.M; a.N = o.N; a.K = o.K; a.K1 = o.K;
            a.Hin = o.Hin; a.Win = o.Win; a.Cin = o.Cin; a.Hout = o.Hout; a.Wout = o.Wout; a.stride = o.stride; a.up = o.up;
            a.zero_page = g_zero_page; a.splitk = o.splitk; a.slab = (float*)T(o.aux); a.defer_reduce = o.defer;
            if (o.dt) { a.dt = 1; a.wscale = (const float*)(wb + o.wsc); a.xscale_inv = 1.0f / o.xs; }
            a.stats = (float*)T(o.stats);
            a.asym = o.asym;
            if (o.subpix) { a.subpix = 1; a.up = 0; a.w_batch_stride = (long)o.N * 4 * o.Cin; }
            if (o.scw != NOFF) {
                a.Xs1 = (const bf16_t*)T(o.scx1); a.Csc1 = o.scc1; a.Xs2 = (const bf16_t*)T(o.scx2); a.Csc2 = o.scc2;
                a.Wsc = (const bf16_t*)(wb + o.scw); a.ldwsc = o.scc1 + o.scc2;
            }
            return sd_launch_conv3x3(a, stream);
        }
        case OP_GEMM: {
            GemmArgs a;
            a.X = o.wx != NOFF ? (const bf16_t*)(wb + o.wx) : (const bf16_t*)T(o.x1) + o.xoff;
            a.ldx = o.ldx_o ? o.ldx_o : o.K1; a.X2 = (const bf16_t*)T(o.x2); a.ldx2 = o.K - o.K1; a.K1 = o.K1;
            a.W = o.wt >= 0 ? (const bf16_t*)T(o.wt) + o.woff_el : (const bf16_t*)(wb + o.w); a.ldw = o.ldw_o;
            a.bias = o.b != NOFF ? (const float*)(wb + o.b) : nullptr;
            a.R = (const bf16_t*)T(o.r); a.ldr = o.N; a.C = (bf16_t*)T(o.out) + o.coff;
            a.ldc = o.ldc_o ? o.ldc_o : (o.epi == 1 ? o.N / 2 : o.N);
            a.M = o.M; a.N = o.N; a.K = o.K; a.zero_page = g_zero_page; a.splitk = o.splitk; a.slab = (float*)T(o.aux);
            a.defer_reduce = o.defer;
            a.w_batch_stride = o.wbs; a.rows_per_batch = o.rpb; a.sm_valid = o.sm_valid;
            if (o.dt) { a.dt = 1; a.wscale = (const float*)(wb + o.wsc); a.xscale_inv = 1.0f / o.xs; }
            if (o.out_fp8) { a.out_fp8 = 1; a.oscale = o.os; a.ldc = o.Cpad; }
            a.stats = (float*)T(o.stats);
            a.rowstats = (float*)T(o.rs);
            if (o.hm) { a.hm_C = o.N / 3; a.hm_tok = o.HW; a.ldc = a.hm_C; a.KV = (bf16_t*)T(o.out) + (long)o.M * a.hm_C; }
            if (o.lnrs >= 0) { a.ln_rs = (const float*)T(o.lnrs); a.ln_np = o.lnnp; a.ln_c1 = (const float*)(wb + o.c1); a.ln_eps = 1e-5f; }
            if (o.lnrs >= 0 && o.s1 >= 0) { a.ln_c1 = (const float*)T(o.s1); a.bias = (const float*)T(o.s2); a.ln_per_sample = 1; }   // per-sample weights
            return sd_launch_gemm(a, o.epi, stream);
        }
        case OP_LN:
            if (o.out_fp8)
                return sd_launch_layernorm_fp8((const bf16_t*)T(o.x1), (const float*)(wb + o.g), (const float*)(wb + o.be),
                                               T(o.out), o.M, o.N, o.Cpad, o.eps, o.os, stream);
            return sd_launch_layernorm((const bf16_t*)T(o.x1), (const float*)(wb + o.g), (const float*)(wb + o.be),
                                       (bf16_t*)T(o.out), o.M, o.N, o.eps, stream);
        case OP_ATTN: {
            AttnArgs a;
            a.Q = (const bf16_t*)T(o.x1) + o.qoff; a.ldq = o.ldq;
            a.K = (const bf16_t*)T(o.x2) + o.koff; a.ldk = o.ldk;
            a.V = (const bf16_t*)T(o.x2) + o.voff; a.ldv = o.ldv;
            a.O = (bf16_t*)T(o.out); a.ldo = o.ldo;
            a.B = o.B; a.heads = o.heads; a.Nq = o.Nq; a.Nk = o.Nk; a.D = o.D;
            a.scale = 1.0f / sqrtf((float)o.D);
            a.q_prescaled = o.qps;
            a.consts = g_zero_page;
            a.kv_head_major = o.hm;
            return sd_launch_attention(a, stream);
        }
        case OP_XATTN: {
            XattnArgs a;
            a.X = (const bf16_t*)T(o.x1); a.R = (const bf16_t*)T(o.r); a.Y = (bf16_t*)T(o.out);
            a.At = (const bf16_t*)T(o.wt); a.Bw = (const bf16_t*)T(o.x2); a.bias = (const float*)(wb + o.b);
            a.M = o.M; a.C = o.N; a.rows_per_sample = o.rpb; a.L = o.sm_valid;
            a.rowstats = (float*)T(o.rs);
            if (o.lnrs >= 0) {      // norm2 folded in: X = the un-normalised residual stream
                a.ln_rs = (const float*)T(o.lnrs); a.ln_np = o.lnnp; a.ln_rows = o.ldx_o; a.ln_c2 = (const float*)T(o.s1); a.ln_eps = 1e-5f;
            }
            return sd_launch_xattn_fused(a, stream);
        }
        case OP_IP_XATTN:
            return sd_launch_ip_xattn((const bf16_t*)T(o.x1), (bf16_t*)T(o.out), (const bf16_t*)T(o.wt), (const bf16_t*)T(o.x2),
                                      (const float*)(wb + o.g), (const float*)(wb + o.be), o.eps, o.M, o.N, o.rpb, o.heads,
                                      u->cfg.ip_adapter_tokens, stream);
        case OP_RES_ADD: {
            SD_REQUIRE(u->ctrl_res && o.nres == (int)pl.cn_off.size() && o.nres <= MAX_CONTROL_RES, "forward: no ControlNet residuals are set");
            bf16_t* x[MAX_CONTROL_RES];
            const bf16_t* r[MAX_CONTROL_RES];
            long n[MAX_CONTROL_RES];
            for (int k = 0; k < o.nres; ++k) {
                x[k] = (bf16_t*)T(o.res_t[k]); r[k] = (const bf16_t*)(u->ctrl_res + pl.cn_off[k]); n[k] = pl.cn_count[k];
                SD_REQUIRE((size_t)n[k] * 2 <= pl.tensors[o.res_t[k]].bytes, "forward: ControlNet residual %d exceeds its tensor", k);
            }
            return sd_launch_residual_add(x, r, n, o.nres, u->ctrl_scale, stream);
        }
        case OP_FREEU:      // (the factors of the handle as they are NOW: a change between two forwards rebuilds nothing)
            SD_REQUIRE(u->freeu_on && (o.epi == 0 || o.epi == 1), "forward: FreeU is off (sd_unet_set_freeu)");
            return sd_launch_freeu((const bf16_t*)T(o.x1), (const bf16_t*)T(o.x2), (bf16_t*)T(o.out), (bf16_t*)T(o.aux), o.B, o.Hin, o.Win,
                                   o.C1, o.C2, u->freeu_b[o.epi], u->freeu_s[o.epi], stream);
        case OP_TGATE_ZERO:
            SD_CHECK_HIP(hipMemsetAsync(T(o.out), 0, pl.tensors[o.out].bytes, stream));
            return 0;
        case OP_TGATE_CAPTURE:
        case OP_TGATE_APPLY: {      // (sd_unet_forward_hw has checked the handle's cache against this plan's layout)
            SD_REQUIRE(u->tg_cache && o.b2idx >= 0 && o.b2idx < (long)pl.tg_off.size() &&
                           pl.tg_off[o.b2idx] + (size_t)pl.tg_rows[o.b2idx] * o.N * 2 <= (size_t)u->tg_bytes,
                       "forward: no T-GATE cache for block %ld (sd_unet_set_tgate_hw)", o.b2idx);
            bf16_t* slice = (bf16_t*)(u->tg_cache + pl.tg_off[o.b2idx]);
            if (o.kind == OP_TGATE_APPLY)
                return sd_launch_tgate_apply((const bf16_t*)T(o.x1), slice, (bf16_t*)T(o.out), (float*)T(o.rs), o.M, o.N, stream);
            return sd_launch_tgate_capture((const bf16_t*)T(o.x1), (const bf16_t*)T(o.r), (bf16_t*)T(o.out), slice, (float*)T(o.rs),
                                           o.M / o.K, o.N, o.K, stream);
        }
        case OP_REPLICATE:
            return sd_launch_replicate(T(o.x1), T(o.out), (long)o.M * 16, o.N, stream);
        case OP_HT_GATHER:       // (K = nh, K1 = nw; the raster side is dense here: pitch = C)
            return sd_launch_hypertile_gather((const bf16_t*)T(o.x1), o.N, (bf16_t*)T(o.out), o.B, o.Hin, o.Win, o.N, o.K, o.K1, stream);
        case OP_HT_SCATTER:
            return sd_launch_hypertile_scatter((const bf16_t*)T(o.x1), (bf16_t*)T(o.out), o.N, o.B, o.Hin, o.Win, o.N, o.K, o.K1, stream);
        case OP_PAG_IDENTITY:    // (qoff / koff: the first perturbed row and their count; HW: tokens of a head-major sample, 0 = token-major)
            return sd_launch_pag_identity((const bf16_t*)T(o.x1) + o.voff, o.ldv, o.HW, (bf16_t*)T(o.out), o.M, o.qoff, o.koff, o.N, o.heads, stream);
        case OP_SAG_MASS:        // (koff / ldk: K's offset in a projection row and the row pitch; the mass goes to the handle's buffer)
            SD_REQUIRE(u->sag_mass && (long long)o.B * o.Nk <= u->sag_mass_floats, "forward: SAG capture is on and the mass buffer holds %lld "
                       "floats, batch %d at a %dx%d mid grid takes %lld (sd_unet_set_sag_buffer)", u->sag_mass ? u->sag_mass_floats : 0ll, o.B,
                       o.Hin, o.Win, (long long)o.B * o.Nk);
            return sd_launch_sag_attn_mass((const bf16_t*)T(o.x1), (const bf16_t*)T(o.x1) + o.koff, o.ldk, u->sag_mass, o.B, o.heads, o.Nk, o.D, 1, stream);
        case OP_TOME_MATCH:
            SD_REQUIRE(u->tome_choice && o.b2idx + (long)(o.Hin / 2) * (o.Win / 2) <= u->tome_choice_n, "forward: no Token Merging choice array");
            return sd_launch_tome_match((const bf16_t*)T(o.x1), u->tome_choice + o.b2idx, o.B, o.Hin, o.Win, o.N, (float*)T(o.out),
                                        (int*)T(o.aux), (int*)T(o.stats), (float*)T(o.rs), stream);
        case OP_TOME_SELECT:
            return sd_launch_tome_select((const float*)T(o.x1), (const int*)T(o.x2), o.B, o.M, o.K, (int*)T(o.out), (int*)T(o.aux),
                                         (int*)T(o.stats), stream);
        case OP_TOME_MERGE:
            return sd_launch_tome_merge((const bf16_t*)T(o.x1), (const int*)T(o.x2), (const int*)T(o.r), (const int*)T(o.wt),
                                        (const int*)T(o.s1), (bf16_t*)T(o.out), o.N, o.B, o.Hin, o.Win, o.N, o.K, stream);
        case OP_TOME_UNMERGE:
            return sd_launch_tome_unmerge((const bf16_t*)T(o.x1), o.N, (const bf16_t*)T(o.r), (const int*)T(o.x2), (const int*)T(o.wt),
                                          (const int*)T(o.s1), (const int*)T(o.s2), (bf16_t*)T(o.out), o.B, o.Hin, o.Win, o.N, o.K, stream);
        case OP_CLIP_EMBED:
            if (u->kind == 6)       // (the plan's input is the image batch: the ids are the call's, on the handle)
                return sd_launch_clip_embed(u->ir_ids, (const bf16_t*)(wb + o.w), (const bf16_t*)(wb + o.g), (bf16_t*)T(o.out),
                                            o.M, o.Nk, o.N, u->ir.vocab_size, stream);
            return sd_launch_clip_embed((const int*)latents, (const bf16_t*)(wb + o.w), (const bf16_t*)(wb + o.g),
                                        (bf16_t*)T(o.out), o.M, o.Nk, o.N, u->clip.vocab_size, stream);
        case OP_BERT_ATTN:
            return sd_launch_bert_attention((const bf16_t*)T(o.x1) + o.qoff, o.ldq, (const bf16_t*)T(o.x2) + o.koff,
                                            (const bf16_t*)T(o.x2) + o.voff, o.ldk, o.key_mask ? u->ir_mask : nullptr,
                                            (bf16_t*)T(o.out), o.ldo, o.B, o.heads, o.Nq, o.Nk, stream);
        case OP_REWARD_HEAD:
            return sd_launch_reward_head((const bf16_t*)T(o.x1), (long)o.Nq * o.N, (const float*)(wb + o.w), (const float*)(wb + o.b),
                                         u->ir.reward_mean, u->ir.reward_std, o.B, o.N, eps_out, u->ir_features, stream);
        case OP_CLIP_ATTN:
            return sd_launch_clip_attention((const bf16_t*)T(o.x1), (bf16_t*)T(o.out), o.B, o.Nq, o.N, o.heads, stream);
        case OP_QGELU:
            if (o.epi) return sd_launch_gelu_erf((bf16_t*)T(o.x1), (long)o.M * o.N, stream);
            return sd_launch_quick_gelu((bf16_t*)T(o.x1), (long)o.M * o.N, stream);
        case OP_VIT_PREP:
            return sd_launch_clip_preprocess((const unsigned char*)latents, o.B, pl.geom, pl.dtab, (unsigned char*)T(o.aux),
                                             (bf16_t*)T(o.out), o.Cin, o.K, nullptr, stream);
        case OP_VIT_EMBED:
            return sd_launch_vit_embed((const bf16_t*)T(o.x1), (const float*)(wb + o.b), (const bf16_t*)(wb + o.g),
                                       (bf16_t*)T(o.out), o.B, o.Nq, o.N, stream);
        case OP_VIT_ATTN:
            return sd_launch_vit_attention((const bf16_t*)T(o.x1), (bf16_t*)T(o.out), o.B, o.Nq, o.N, o.heads, stream);
        case OP_POOL:
            return sd_launch_pool_rows((const bf16_t*)T(o.x1), o.pool_by_ids ? (const int*)latents : nullptr, o.B, o.Nq, o.N, u->eos_id,
                                       (bf16_t*)T(o.out), stream);
        case OP_TO_F32:
            return sd_launch_bf16_to_f32((const bf16_t*)T(o.x1), eps_out, (long)o.M * o.N, stream);
        case OP_CONV_IN_IMG:
            return sd_launch_conv_in_image(latents, (const float*)(wb + o.w), (const float*)(wb + o.b), (bf16_t*)T(o.out), o.B,
                                           o.Hin, o.Win, o.N, stream);
        case OP_ENC_OUT:
            return sd_launch_vae_enc_out((const bf16_t*)T(o.x1), (const bf16_t*)(wb + o.w), (const float*)(wb + o.b),
                                         (const float*)(wb + o.g), (const float*)(wb + o.be), eps_out, o.B, o.Hin, o.Win, o.Cin,
                                         stream);
        case OP_CONV_OUT:
            return sd_launch_conv_out((const bf16_t*)T(o.x1), (const bf16_t*)(wb + o.w), (const float*)(wb + o.b), eps_out,
                                      o.B, o.Hin, o.Win, o.Cin, o.N, stream);
    }
    sd_set_error("unet: unknown op kind %d", o.kind);
    return -1;
}

}  // namespace sdhip

using namespace sdhip;

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// cfg null: a CLIP tower (its config lives in sd_unet::clip / vis; no tap readback)
static sd_unet* new_handle(int kind, const sd_unet_config* cfg) {
    sd_unet* u = new sd_unet();   // no device work here: parameter enumeration also runs on a CPU-only box
    u->kind = kind;
    if (cfg) {
        u->cfg = *cfg;
        if (kind != 0) u->cfg.ip_adapter_tokens = u->cfg.ip_adapter_embed_dim = 0;      // (UNet fields)
        if (kind != 0 && kind != 5) u->cfg.time_cond_proj_dim = 0;
        u->debug_taps = getenv("SD_DEBUG_TAPS") != nullptr;
    } else {
        memset(&u->cfg, 0, sizeof(u->cfg));
        u->cfg.num_levels = 1;
    }
    return u;
}

static int check_vae_levels(const sd_unet_config* cfg, const char* who) {
    for (int i = 0; i < cfg->num_levels; ++i) {
        const int c = cfg->block_out_channels[i], cpg = cfg->norm_num_groups ? c / cfg->norm_num_groups : 0;
        SD_REQUIRE(c % 64 == 0 && c % cfg->norm_num_groups == 0 && (cpg >= 8 || cpg == 4),
                   "%s: block_out_channels[%d]=%d must be a multiple of 64 with 4 or >= 8 channels per group", who, i, c);
    }
    return 0;
}

static int check_workspace(const Plan& pl, const char* who, const void* workspace, long long workspace_bytes) {
    SD_REQUIRE((long long)pl.total_bytes <= workspace_bytes, "%s: workspace too small (%lld < %zu)", who, workspace_bytes,
               pl.total_bytes);
    SD_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    return 0;
}

// the tail of every entry point that runs a plan; `scalar` = the timestep (UNet) or the latent scale (VAE decoder)
static int run_plan(sd_unet* u, const Plan& pl, const char* who, void* workspace, long long workspace_bytes, const void* in,
                    int batch, float* out, float scalar, void* stream, int cache_mode = SD_CACHE_OFF) {
    if (check_workspace(pl, who, workspace, workspace_bytes)) return -1;
    for (size_t i = 0; i < pl.ops.size(); ++i) {
        if (cache_mode == SD_CACHE_SKIP && pl.skipped[i]) continue;
        if (int rc = run_op(u, pl, pl.ops[i], (char*)workspace, (const float*)in, batch, out, scalar, (hipStream_t)stream)) return rc;
    }
    return 0;
}

// what a UNet and the ControlNet paired with it share (`who` names the entry point in the messages)
static int check_unet_config(const sd_unet_config* cfg, const char* who) {
    SD_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= 8, "%s: num_levels %d", who, cfg->num_levels);
    SD_REQUIRE(cfg->in_channels == 4 || cfg->in_channels == 9,
               "%s: in_channels %d (4, or 9 for an inpainting UNet: latents | mask | masked-image latents)", who,
               cfg->in_channels);
    SD_REQUIRE(cfg->out_channels >= 1 && cfg->out_channels <= 4, "%s: out_channels %d", who, cfg->out_channels);
    {   // num_heads_per_level: all zeros (num_heads everywhere) or a positive count for every level
        int set = 0;
        for (int i = 0; i < 8; ++i) {
            SD_REQUIRE(cfg->num_heads_per_level[i] >= 0 && (i < cfg->num_levels || cfg->num_heads_per_level[i] == 0),
                       "%s: num_heads_per_level[%d]=%d (%d levels)", who, i, cfg->num_heads_per_level[i], cfg->num_levels);
            set += cfg->num_heads_per_level[i] > 0;
        }
        SD_REQUIRE(set == 0 || set == cfg->num_levels, "%s: num_heads_per_level names %d of %d levels (all zeros, or every level)",
                   who, set, cfg->num_levels);
    }
    for (int i = 0; i < cfg->num_levels; ++i) {
        const int c = cfg->block_out_channels[i];
        SD_REQUIRE(c % 64 == 0 && c % cfg->norm_num_groups == 0 && c / cfg->norm_num_groups >= 8,
                   "%s: block_out_channels[%d]=%d must be a multiple of 64 with >= 8 channels per group", who, i, c);
        if (cfg->attn_levels[i]) {
            const int nh = level_heads(*cfg, i), d = nh > 0 ? c / nh : 0;
            SD_REQUIRE(nh > 0 && c % nh == 0 && (d == 40 || d == 64 || d == 80 || d == 160),
                       "%s: head dim %d at level %d (%d channels, %d heads) not built (40/64/80/160)", who, d, i, c, nh);
        }
    }
    const int nhmid = level_heads(*cfg, cfg->num_levels - 1);
    const int cmid = cfg->block_out_channels[cfg->num_levels - 1], dmid = nhmid > 0 ? cmid / nhmid : 0;
    SD_REQUIRE(nhmid > 0 && cmid % nhmid == 0 && (dmid == 40 || dmid == 64 || dmid == 80 || dmid == 160),
               "%s: mid-block head dim %d (%d channels, %d heads) not built (40/64/80/160)", who, dmid, cmid, nhmid);
    SD_REQUIRE(cfg->cross_attention_dim % 64 == 0, "%s: cross_attention_dim must be a multiple of 64", who);
    SD_REQUIRE(cfg->sample_size % (1 << (cfg->num_levels - 1)) == 0, "%s: sample_size not divisible", who);
    SD_REQUIRE(cfg->context_len >= 1, "%s: context_len", who);
    SD_REQUIRE(cfg->weight_dtype == SD_DTYPE_BF16 || cfg->weight_dtype == SD_DTYPE_FP8_E4M3,
               "%s: weight_dtype %d (0 = bf16, 1 = fp8 e4m3)", who, cfg->weight_dtype);
    SD_REQUIRE(cfg->fp8_act_scale_norm >= 0.f && cfg->fp8_act_scale_ff >= 0.f, "%s: negative fp8 activation scale", who);
    SD_REQUIRE(cfg->time_cond_proj_dim >= 0 && cfg->time_cond_proj_dim % 8 == 0,
               "%s: time_cond_proj_dim %d must be 0 (none) or a positive multiple of 8 (the GEMV reads 8 at a time)", who,
               cfg->time_cond_proj_dim);
    if (cfg->ip_adapter_tokens != 0 || cfg->ip_adapter_embed_dim != 0) {
        SD_REQUIRE(cfg->ip_adapter_tokens == 4, "%s: ip_adapter_tokens %d (4 image tokens are built: the plain ip-adapter_sd15 "
                   "family; the \"plus\" / \"full-face\" adapters with 16 or 257 tokens are not)", who, cfg->ip_adapter_tokens);
        SD_REQUIRE(cfg->ip_adapter_embed_dim > 0 && cfg->ip_adapter_embed_dim % 64 == 0,
                   "%s: ip_adapter_embed_dim %d must be a positive multiple of 64", who, cfg->ip_adapter_embed_dim);
        SD_REQUIRE(cfg->cross_attention_dim <= 1536, "%s: an IP-Adapter needs cross_attention_dim <= 1536 (the token LayerNorm)", who);
        for (int i = 0; i < cfg->num_levels; ++i)
            SD_REQUIRE(sd_ip_xattn_applicable(cfg->block_out_channels[i], level_heads(*cfg, i), cfg->ip_adapter_tokens),
                       "%s: an IP-Adapter needs 1, 2, 4 or 8 heads and channels that are a multiple of 32 up to 2048 "
                       "(level %d: %d channels, %d heads)", who, i, cfg->block_out_channels[i], level_heads(*cfg, i));
    }
    return 0;
}

extern "C" int sd_unet_create(const sd_unet_config* cfg, sd_unet** out) {
    SD_REQUIRE(cfg && out, "sd_unet_create: null argument");
    if (check_unet_config(cfg, "sd_unet_create")) return -1;
    sd_unet* u = new_handle(0, cfg);
    u->fp8 = cfg->weight_dtype == SD_DTYPE_FP8_E4M3;
    if (cfg->fp8_act_scale_norm > 0.f) u->s_norm = cfg->fp8_act_scale_norm;
    if (cfg->fp8_act_scale_ff > 0.f) u->s_ff = cfg->fp8_act_scale_ff;
    enumerate_params(u);
    *out = u;
    return 0;
}

// ---- AutoencoderKL decoder: `self.vae.decode(latents / scaling_factor)` of src/models.py:287-302 ----
extern "C" int sd_vae_create(const sd_unet_config* cfg, sd_unet** out) {
    SD_REQUIRE(cfg && out, "sd_vae_create: null argument");
    SD_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= 8, "sd_vae_create: num_levels %d", cfg->num_levels);
    SD_REQUIRE(cfg->in_channels == 4 && cfg->out_channels >= 1 && cfg->out_channels <= 4, "sd_vae_create: in/out channels");
    if (check_vae_levels(cfg, "sd_vae_create")) return -1;
    SD_REQUIRE(cfg->sample_size >= 8 && cfg->sample_size <= 128 && (cfg->sample_size * cfg->sample_size) % 64 == 0,
               "sd_vae_create: latent size %d (8 .. 128, HW a multiple of 64)", cfg->sample_size);
    sd_unet* u = new_handle(1, cfg);
    enumerate_params_vae(u);
    *out = u;
    return 0;
}

extern "C" int sd_vae_decode(sd_unet* u, void* stream, const float* latents, int batch, float latent_scale,
                             float* images_out, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 1, "vae_decode: not a VAE handle");
    return sd_vae_decode_hw(u, stream, latents, batch, u->cfg.sample_size, u->cfg.sample_size, latent_scale, images_out,
                            workspace, workspace_bytes);
}

extern "C" int sd_vae_decode_hw(sd_unet* u, void* stream, const float* latents, int batch, int latent_h, int latent_w,
                                float latent_scale, float* images_out, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 1, "vae_decode: not a VAE handle");
    SD_REQUIRE(latents && images_out && workspace && batch > 0, "vae_decode: null argument");
    if (check_latent_size(u, latent_h, latent_w, "vae_decode")) return -1;
    Plan* pl;
    int rc = get_plan(u, plan_variant(u, batch, -1, latent_h, latent_w), &pl);
    if (rc) return rc;
    return run_plan(u, *pl, "vae_decode", workspace, workspace_bytes, latents, batch, images_out, latent_scale, stream);
}

// ---- AutoencoderKL encoder: `vae.encode(image)` of diffusers' StableDiffusionImg2ImgPipeline.prepare_latents (upstream-recall) ----
extern "C" int sd_vae_encoder_create(const sd_unet_config* cfg, sd_unet** out) {
    SD_REQUIRE(cfg && out, "sd_vae_encoder_create: null argument");
    SD_REQUIRE(cfg->num_levels >= 1 && cfg->num_levels <= 8, "sd_vae_encoder_create: num_levels %d", cfg->num_levels);
    SD_REQUIRE(cfg->in_channels == 4 && cfg->out_channels == 3,
               "sd_vae_encoder_create: %d latent / %d image channels (4 / 3 are built: 8 moment channels, RGB entry conv)",
               cfg->in_channels, cfg->out_channels);
    SD_REQUIRE(cfg->num_levels == 4, "sd_vae_encoder_create: %d levels (4 are built: the image is 8 x the latent, and a latent side that is a "
               "multiple of 8 keeps every level's sides even)", cfg->num_levels);
    if (check_vae_levels(cfg, "sd_vae_encoder_create")) return -1;
    SD_REQUIRE(cfg->sample_size >= 8 && cfg->sample_size <= 128 && cfg->sample_size % 8 == 0,
               "sd_vae_encoder_create: latent size %d (a multiple of 8 in [8, 128])", cfg->sample_size);
    sd_unet* u = new_handle(4, cfg);
    enumerate_params_vae_encoder(u);
    *out = u;
    return 0;
}

extern "C" int sd_vae_encode_hw(sd_unet* u, void* stream, const float* images, int batch, int latent_h, int latent_w,
                                float* moments_out, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 4, "vae_encode: not a VAE encoder handle");
    SD_REQUIRE(images && moments_out && workspace && batch > 0, "vae_encode: null argument");
    if (check_latent_size(u, latent_h, latent_w, "vae_encode")) return -1;
    Plan* pl;
    int rc = get_plan(u, plan_variant(u, batch, -1, latent_h, latent_w), &pl);
    if (rc) return rc;
    return run_plan(u, *pl, "vae_encode", workspace, workspace_bytes, images, batch, moments_out, 0.f, stream);
}

extern "C" int sd_vae_posterior_sample(void* stream, const float* moments, const float* noise_or_null, float scale,
                                       float* latents_out, int batch, long long hw) {
    SD_REQUIRE(moments && latents_out && batch > 0 && hw > 0, "vae_posterior_sample: null argument");
    return sd_launch_vae_posterior(moments, noise_or_null, scale, latents_out, batch, 4, (long)hw, (hipStream_t)stream);
}

// ---- CLIP text encoder: `self.text_encoder(text_input_ids)[0]` inside encode_prompt (src/models.py:139-155) ----
extern "C" int sd_clip_create(const sd_clip_config* cfg, sd_unet** out) {
    SD_REQUIRE(cfg && out, "sd_clip_create: null argument");
    SD_REQUIRE(cfg->hidden_size % 64 == 0 && cfg->intermediate_size % 64 == 0,
               "sd_clip_create: hidden %d / intermediate %d must be multiples of 64", cfg->hidden_size, cfg->intermediate_size);
    SD_REQUIRE(cfg->hidden_size <= 1536, "sd_clip_create: hidden size %d (LayerNorm kernel handles <= 1536)", cfg->hidden_size);
    SD_REQUIRE(cfg->num_heads > 0 && cfg->hidden_size % cfg->num_heads == 0, "sd_clip_create: heads");
    const int d = cfg->hidden_size / cfg->num_heads;
    SD_REQUIRE(d == 64 || d == 16, "sd_clip_create: head dim %d (64 and 16 are built)", d);
    SD_REQUIRE(cfg->max_positions >= 1 && cfg->max_positions <= 128, "sd_clip_create: max_positions %d", cfg->max_positions);
    SD_REQUIRE(cfg->vocab_size >= 1 && cfg->num_layers >= 1, "sd_clip_create: vocab/layers");
    SD_REQUIRE(fabsf(cfg->layer_norm_eps - 1e-5f) < 1e-9f, "sd_clip_create: layer_norm_eps %g (1e-5 is built)", cfg->layer_norm_eps);
    SD_REQUIRE(cfg->hidden_act == SD_ACT_QUICK_GELU || cfg->hidden_act == SD_ACT_GELU,
               "sd_clip_create: hidden_act %d (0 = quick_gelu, 1 = gelu)", cfg->hidden_act);
    sd_unet* u = new_handle(2, nullptr);
    u->clip = *cfg;
    enumerate_params_clip(u);
    *out = u;
    return 0;
}

extern "C" int sd_clip_encode(sd_unet* u, void* stream, const int* input_ids, int batch, float* hidden_out,
                              void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 2, "clip_encode: not a CLIP handle");
    SD_REQUIRE(input_ids && hidden_out && workspace && batch > 0, "clip_encode: null argument");
    Plan* pl;
    int rc = get_plan(u, plan_variant(u, batch), &pl);
    if (rc) return rc;
    return run_plan(u, *pl, "clip_encode", workspace, workspace_bytes, input_ids, batch, hidden_out, 0.f, stream);
}

// ---- CLIP score (quality_metrics.clip_score): text_projection on the pooled text row, the vision tower, the score ----
extern "C" int sd_clip_create_projected(const sd_clip_config* cfg, int projection_dim, int eos_token_id, sd_unet** out) {
    SD_REQUIRE(cfg && out, "sd_clip_create_projected: null argument");
    SD_REQUIRE(projection_dim > 0 && projection_dim % 4 == 0 && cfg->hidden_size % 64 == 0,
               "sd_clip_create_projected: projection_dim %d must be a positive multiple of 4", projection_dim);
    sd_clip_config c = *cfg;
    sd_unet* u = nullptr;
    int rc = sd_clip_create(&c, &u);
    if (rc) return rc;
    u->params.clear(); u->pindex.clear();
    u->text_proj = projection_dim;
    u->eos_id = eos_token_id;
    enumerate_params_clip(u);
    *out = u;
    return 0;
}

extern "C" long long sd_clip_text_embeds_workspace_bytes(sd_unet* u, int batch) {
    SD_REQUIRE(u && u->kind == 2 && u->text_proj > 0, "clip_text_embeds: not a projected CLIP text handle");
    Plan* pl;
    PlanVariant v = plan_variant(u, batch);
    v.rep = REP_TEXT_POOLED;
    if (get_plan(u, v, &pl)) return -1;
    return (long long)pl->total_bytes;
}

extern "C" int sd_clip_text_embeds(sd_unet* u, void* stream, const int* input_ids, int batch, float* text_embeds,
                                   void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 2 && u->text_proj > 0, "clip_text_embeds: not a projected CLIP text handle");
    SD_REQUIRE(input_ids && text_embeds && workspace && batch > 0, "clip_text_embeds: null argument");
    Plan* pl;
    PlanVariant v = plan_variant(u, batch);
    v.rep = REP_TEXT_POOLED;
    int rc = get_plan(u, v, &pl);
    if (rc) return rc;
    return run_plan(u, *pl, "clip_text_embeds", workspace, workspace_bytes, input_ids, batch, text_embeds, 0.f, stream);
}

int sdhip::check_image_size(int H, int W, const char* who) {
    SD_REQUIRE(H >= 1 && W >= 1 && H <= 8192 && W <= 8192, "%s: image %dx%d (sides 1..8192 are accepted)", who, H, W);
    return 0;
}

extern "C" int sd_clip_vision_create(const sd_clip_vision_config* cfg, sd_unet** out) {
    SD_REQUIRE(cfg && out, "sd_clip_vision_create: null argument");
    const sd_clip_vision_config& c = *cfg;
    SD_REQUIRE(c.hidden_size % 64 == 0 && c.hidden_size > 0 && c.intermediate_size % 64 == 0 && c.intermediate_size > 0,
               "sd_clip_vision_create: hidden %d / intermediate %d must be positive multiples of 64", c.hidden_size,
               c.intermediate_size);
    SD_REQUIRE(c.hidden_size <= 1536, "sd_clip_vision_create: hidden size %d (LayerNorm kernel handles <= 1536)", c.hidden_size);
    SD_REQUIRE(c.num_heads > 0 && c.hidden_size % c.num_heads == 0 &&
                   (c.hidden_size / c.num_heads == 64 || c.hidden_size / c.num_heads == 80),
               "sd_clip_vision_create: head dim %d (64 and 80 are built)", c.num_heads > 0 ? c.hidden_size / c.num_heads : 0);
    SD_REQUIRE(c.hidden_act == SD_ACT_QUICK_GELU || c.hidden_act == SD_ACT_GELU,
               "sd_clip_vision_create: hidden_act %d (0 = quick_gelu, 1 = gelu)", c.hidden_act);
    SD_REQUIRE(c.patch_size >= 1 && c.image_size >= c.patch_size && c.image_size % c.patch_size == 0,
               "sd_clip_vision_create: image_size %d / patch_size %d", c.image_size, c.patch_size);
    const int G = c.image_size / c.patch_size;
    SD_REQUIRE(G * G + 1 <= 320, "sd_clip_vision_create: %d tokens (at most 320 are built)", G * G + 1);
    SD_REQUIRE(c.projection_dim > 0 && c.projection_dim % 4 == 0, "sd_clip_vision_create: projection_dim %d", c.projection_dim);
    SD_REQUIRE(c.num_layers >= 1, "sd_clip_vision_create: num_layers %d", c.num_layers);
    SD_REQUIRE(fabsf(c.layer_norm_eps - 1e-5f) < 1e-9f, "sd_clip_vision_create: layer_norm_eps %g (1e-5 is built)", c.layer_norm_eps);
    sd_unet* u = new_handle(3, nullptr);
    u->vis = c;
    enumerate_params_vit(u);
    *out = u;
    return 0;
}

extern "C" long long sd_clip_vision_workspace_bytes(sd_unet* u, int batch, int height, int width) {
    SD_REQUIRE(u && u->kind == 3, "clip_vision: not a CLIP vision handle");
    if (check_image_size(height, width, "clip_vision")) return -1;
    Plan* pl;
    if (get_plan(u, plan_variant(u, batch, -1, height, width), &pl)) return -1;
    return (long long)pl->total_bytes;
}

extern "C" int sd_clip_vision_encode(sd_unet* u, void* stream, const unsigned char* images, int batch, int height, int width,
                                     float* image_embeds, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 3, "clip_vision: not a CLIP vision handle");
    SD_REQUIRE(images && image_embeds && workspace && batch > 0, "clip_vision: null argument");
    if (check_image_size(height, width, "clip_vision")) return -1;
    Plan* pl;
    int rc = get_plan(u, plan_variant(u, batch, -1, height, width), &pl);
    if (rc) return rc;
    return run_plan(u, *pl, "clip_vision", workspace, workspace_bytes, images, batch, image_embeds, 0.f, stream);
}

// ---- ImageReward (quality_metrics.image_reward): BLIP ViT + BLIP text encoder + reward head, one plan ----
extern "C" int sd_image_reward_create(const sd_image_reward_config* cfg, sd_unet** out) {
    SD_REQUIRE(cfg && out, "sd_image_reward_create: null argument");
    const sd_image_reward_config& c = *cfg;
    SD_REQUIRE(c.vision_hidden_size > 0 && c.vision_hidden_size % 64 == 0 && c.vision_hidden_size <= 1536,
               "sd_image_reward_create: vision_hidden_size %d (a multiple of 64 up to 1536 is built)", c.vision_hidden_size);
    SD_REQUIRE(c.hidden_size > 0 && c.hidden_size % 64 == 0 && c.hidden_size <= 1536,
               "sd_image_reward_create: hidden_size %d (a multiple of 64 up to 1536 is built)", c.hidden_size);
    SD_REQUIRE(c.vision_intermediate_size > 0 && c.vision_intermediate_size % 64 == 0 && c.intermediate_size > 0 &&
                   c.intermediate_size % 64 == 0,
               "sd_image_reward_create: vision_intermediate_size %d / intermediate_size %d must be positive multiples of 64",
               c.vision_intermediate_size, c.intermediate_size);
    SD_REQUIRE(c.vision_num_heads > 0 && c.vision_hidden_size == 64 * c.vision_num_heads,
               "sd_image_reward_create: vision_num_heads %d at vision_hidden_size %d (head dim 64 is built)", c.vision_num_heads,
               c.vision_hidden_size);
    SD_REQUIRE(c.num_heads > 0 && c.hidden_size == 64 * c.num_heads,
               "sd_image_reward_create: num_heads %d at hidden_size %d (head dim 64 is built)", c.num_heads, c.hidden_size);
    SD_REQUIRE(c.patch_size >= 1 && c.image_size >= c.patch_size && c.image_size % c.patch_size == 0,
               "sd_image_reward_create: image_size %d / patch_size %d", c.image_size, c.patch_size);
    const int G = c.image_size / c.patch_size;
    SD_REQUIRE(G * G + 1 <= 320, "sd_image_reward_create: image_size %d gives %d image tokens (at most 320 are built)", c.image_size,
               G * G + 1);
    SD_REQUIRE(c.max_text_len >= 1 && c.max_text_len <= 64 && c.max_text_len <= c.max_positions,
               "sd_image_reward_create: max_text_len %d (1..64 and at most max_positions = %d)", c.max_text_len, c.max_positions);
    SD_REQUIRE(c.hidden_act == SD_ACT_GELU, "sd_image_reward_create: hidden_act %d (only gelu = %d is built)", c.hidden_act, SD_ACT_GELU);
    SD_REQUIRE(c.position_embedding_absolute == 1, "sd_image_reward_create: position_embedding_absolute %d (only absolute positions are built)",
               c.position_embedding_absolute);
    SD_REQUIRE(c.vision_num_layers >= 1 && c.num_layers >= 1 && c.vocab_size >= 1,
               "sd_image_reward_create: vision_num_layers %d / num_layers %d / vocab_size %d", c.vision_num_layers, c.num_layers, c.vocab_size);
    SD_REQUIRE(c.vision_layer_norm_eps > 0.f && c.layer_norm_eps > 0.f && c.reward_std > 0.f,
               "sd_image_reward_create: vision_layer_norm_eps %g / layer_norm_eps %g / reward_std %g must be positive",
               c.vision_layer_norm_eps, c.layer_norm_eps, c.reward_std);
    sd_unet* u = new_handle(6, nullptr);
    u->ir = c;
    enumerate_params_image_reward(u);
    *out = u;
    return 0;
}

extern "C" long long sd_image_reward_workspace_bytes(sd_unet* u, int batch, int height, int width) {
    SD_REQUIRE(u && u->kind == 6, "image_reward: not an ImageReward handle");
    if (check_image_size(height, width, "image_reward")) return -1;
    Plan* pl;
    PlanVariant v = plan_variant(u, batch, -1, height, width);
    v.rep = u->ir.max_text_len;
    if (get_plan(u, v, &pl)) return -1;
    return (long long)pl->total_bytes;
}

extern "C" int sd_image_reward_score(sd_unet* u, void* stream, const unsigned char* images, const int* input_ids,
                                     const int* attention_mask, int batch, int text_len, int height, int width, float* rewards,
                                     float* features_or_null, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 6, "image_reward: not an ImageReward handle");
    SD_REQUIRE(images && input_ids && attention_mask && rewards && workspace && batch > 0, "image_reward: null argument");
    SD_REQUIRE(text_len >= 1 && text_len <= u->ir.max_text_len, "image_reward: text_len %d (1..max_text_len = %d)", text_len,
               u->ir.max_text_len);
    if (check_image_size(height, width, "image_reward")) return -1;
    Plan* pl;
    PlanVariant v = plan_variant(u, batch, -1, height, width);
    v.rep = text_len;
    int rc = get_plan(u, v, &pl);
    if (rc) return rc;
    if (check_workspace(*pl, "image_reward", workspace, workspace_bytes)) return -1;
    {   // a prompt whose mask row is all zero has no key to attend to: refused here, before anything is launched
        std::vector<int> hm((size_t)batch * text_len);
        SD_CHECK_HIP(hipMemcpyAsync(hm.data(), attention_mask, hm.size() * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
        SD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        if (sd_bert_mask_check(hm.data(), batch, text_len)) return -1;
    }
    u->ir_ids = input_ids; u->ir_mask = attention_mask; u->ir_features = features_or_null;
    rc = run_plan(u, *pl, "image_reward", workspace, workspace_bytes, images, batch, rewards, 0.f, stream);
    u->ir_ids = u->ir_mask = nullptr; u->ir_features = nullptr;
    return rc;
}

extern "C" int sd_clip_score(void* stream, const float* image_embeds, const float* text_embeds, int batch, int dim,
                             float* raw, float* score) {
    return sd_launch_clip_score(image_embeds, text_embeds, batch, dim, raw, score, (hipStream_t)stream);
}

extern "C" void sd_unet_destroy(sd_unet* u) {
    if (!u) return;
    if (u->dweights) (void)hipFree(u->dweights);
    if (u->dcond) (void)hipFree(u->dcond);
    if (u->dinpaint) (void)hipFree(u->dinpaint);
    if (u->tome_choice) (void)hipFree(u->tome_choice);
    if (u->cn_embed) (void)hipFree(u->cn_embed);
    if (u->cn_scratch) (void)hipFree(u->cn_scratch);
    for (auto& kv : u->prep_tabs)
        if (kv.second) (void)hipFree(kv.second);
    delete u;
}

extern "C" int sd_unet_num_params(const sd_unet* u) { return u ? (int)u->params.size() : -1; }

extern "C" int sd_unet_param_info(const sd_unet* u, int index, char* name, int name_cap, long long shape[4], int* ndim) {
    SD_REQUIRE(u && index >= 0 && index < (int)u->params.size(), "param_info: bad index %d", index);
    const ParamSpec& p = u->params[index];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", p.name.c_str());
    for (int i = 0; i < 4; ++i) shape[i] = i < (int)p.shape.size() ? p.shape[i] : 1;
    if (ndim) *ndim = (int)p.shape.size();
    return 0;
}

extern "C" int sd_unet_load_param(sd_unet* u, const char* name, const float* host_data, long long numel) {
    SD_REQUIRE(u && name && host_data, "load_param: null argument");
    SD_REQUIRE(!u->finalized, "load_param: handle already finalized");
    auto it = u->pindex.find(name);
    SD_REQUIRE(it != u->pindex.end(), "load_param: unknown parameter '%s'", name);
    ParamSpec& p = u->params[it->second];
    SD_REQUIRE(p.numel() == numel, "load_param: '%s' expects %lld elements, got %lld", name, p.numel(), numel);
    p.data.assign(host_data, host_data + numel);
    p.loaded = true;
    return 0;
}

extern "C" int sd_unet_finalize(sd_unet* u) {
    SD_REQUIRE(u, "finalize: null handle");
    SD_REQUIRE(!u->finalized, "finalize: already finalized");
    for (auto& p : u->params) SD_REQUIRE(p.loaded, "finalize: parameter '%s' was never loaded", p.name.c_str());
    const auto tp0 = std::chrono::steady_clock::now();
    {   // one reservation for the staging blob: growing it piecemeal re-copied it again and again (19 of the 22 s a UNet
        // finalize used to take).  In AGGREGATE the packed blob (2.26 GB for the bf16 UNet: bf16 weights, some of them twice --
        // sub-pixel upsamplers, *.ln copies, ff_out, attn2.to_q.T) stays below the fp32 parameters' bytes (3.44 GB), so this
        // rarely grows; if it has to, HostBlob::resize re-maps at twice the size.
        size_t total = 0;
        for (auto& p : u->params) total += p.data.size() * 4;
        SD_REQUIRE(u->hblob.reserve(total + (64u << 20)), "finalize: cannot map %zu bytes of host staging memory", total + (64u << 20));
    }
    try {
        if (pack_all(u)) return -1;      // host-only: repacks / quantises into the staging blob (runs without a GPU too)
    } catch (const std::bad_alloc&) {
        u->hblob.release();
        sd_set_error("finalize: out of host memory while packing the weights");
        return -2;
    }
    if (getenv("SD_PACK_TIMING"))
        fprintf(stderr, "libsdhip: pack %.2f s (of which staging-blob growth %.2f s), %zu bytes\n",
                std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count(), pack_alloc_seconds(), u->hblob.size());
    if (ensure_zero_page()) return -2;
    SD_CHECK_HIP(hipMalloc((void**)&u->dweights, u->hblob.size()));
    SD_CHECK_HIP(hipMemcpy(u->dweights, u->hblob.data(), u->hblob.size(), hipMemcpyHostToDevice));
    if (u->unet_like() && u->cfg.time_cond_proj_dim > 0)
        SD_CHECK_HIP(hipMalloc((void**)&u->dcond, (size_t)u->cfg.block_out_channels[0] * sizeof(float)));
    u->hblob.release();
    for (auto& p : u->params) std::vector<float>().swap(p.data);
    u->finalized = true;
    return 0;
}

extern "C" long long sd_unet_debug_packed(const sd_unet* u, const char* key, void* host_out, long long nbytes) {
    SD_REQUIRE(u && key, "debug_packed: null argument");
    auto it = u->woff.find(key);
    SD_REQUIRE(it != u->woff.end(), "debug_packed: no packed item '%s'", key);
    SD_REQUIRE(!u->hblob.empty(), "debug_packed: the host staging blob is released once the weights are on the device");
    SD_REQUIRE(nbytes >= 0 && it->second + (size_t)nbytes <= u->hblob.size(), "debug_packed: '%s' + %lld bytes exceeds the blob", key, nbytes);
    if (host_out && nbytes) memcpy(host_out, u->hblob.data() + it->second, (size_t)nbytes);
    return (long long)it->second;
}

extern "C" long long sd_unet_workspace_bytes(sd_unet* u, int unet_batch, int cache_branch_id) {
    SD_REQUIRE(u, "workspace_bytes: null handle");
    return sd_unet_workspace_bytes_hw(u, unet_batch, cache_branch_id, u->cfg.sample_size, u->cfg.sample_size);
}

extern "C" long long sd_unet_workspace_bytes_hw(sd_unet* u, int unet_batch, int cache_branch_id, int latent_h, int latent_w) {
    SD_REQUIRE(u, "workspace_bytes: null handle");
    if (u->kind == 7 || u->kind == 8) return taesd_workspace_bytes(u, unet_batch, latent_h, latent_w);
    if (check_latent_size(u, latent_h, latent_w, "workspace_bytes")) return -1;
    Plan* pl;
    PlanVariant v = plan_variant(u, unet_batch, cache_branch_id, latent_h, latent_w);
    if (check_options("workspace_bytes", variant_options(u, v)) || get_plan(u, v, &pl)) return -1;
    size_t bytes = pl->total_bytes;
    auto cover = [&]() {          // the largest of the variants so far
        if (get_plan(u, v, &pl)) return -1;
        bytes = std::max(bytes, pl->total_bytes);
        return 0;
    };
    if (v.pag_mask) {       // PAG: the plans of 2 and of 3 copies of a latent batch, no other variant exists
        for (v.rep = 2; v.rep <= 3; ++v.rep)
            if (unet_batch % v.rep == 0 && cover()) return -1;
        return (long long)bytes;
    }
    const bool pair = unet_batch % 2 == 0 && plan_rep(u, unet_batch / 2, unet_batch) == 2;      // the CFG-pair variant of the plan
    const bool tg = v.tgate != TGATE_OFF;       // (T-GATE capture / reuse: no IP-Adapter and no control variants exist)
    for (v.ip = 0; v.ip <= (u->kind == 0 && u->cfg.ip_adapter_tokens > 0 && !tg ? 1 : 0); ++v.ip)         // ... and the IP-Adapter variants
        for (v.rep = 1; v.rep <= (pair ? 2 : 1); ++v.rep)
            for (v.cn = 0; v.cn <= (u->kind == 0 && u->ctrl_enabled && cache_branch_id < 0 && !tg ? 1 : 0); ++v.cn)      // ... and, once a ControlNet's residuals were set, the control variants
                if (cover()) return -1;
    return (long long)bytes;
}

// out [rows][N] = X [rows][K] . W [N][K]^T (bf16, the plain GEMM of the operand builders below)
static int fold_gemm(const bf16_t* X, int rows, int K, const bf16_t* W, int N, const float* bias, bf16_t* out, hipStream_t stream) {
    GemmArgs a;
    a.X = X; a.ldx = K; a.K1 = K; a.K = K; a.M = rows; a.N = N;
    a.W = W; a.bias = bias;
    a.C = out; a.ldc = N;
    a.zero_page = g_zero_page;
    return sd_launch_gemm(a, 0, stream);
}

// The operands of ONE folded prompt cross-attention layer from its projected prompt kv [UB * L][K | V] (kernels.h).  scratch =
// three slabs of UB * NP * C bf16 (NP = heads * 80).  What they hold when the last launch has run: slab 0 = B^T [UB * NP][C] in
// natural slot order (the second GEMM overwrites the K expansion there AFTER the c2 GEMV has read it), slab 1 = the V expansion,
// slab 2 = the permuted transpose of B^T before its re-tiling (perm; untouched otherwise).  (Slabs counted from 0.)
int sd_launch_xattn_fold(const bf16_t* kv, const bf16_t* wqT, const bf16_t* wo, const float* lnu, const float* ones, bf16_t* at_dst,
                         bf16_t* bw_dst, float* c1, float* c2, bf16_t* scratch, int UB, int L, int C, int heads, int perm,
                         hipStream_t stream) {
    SD_REQUIRE(kv && wqT && wo && at_dst && bw_dst && scratch, "xattn_fold: null operand");
    SD_REQUIRE((c1 != nullptr) == (ones != nullptr) && (c2 != nullptr) == (lnu != nullptr),
               "xattn_fold: null operand (c1 goes with ones, c2 with lnu)");
    SD_REQUIRE(UB > 0 && L > 0 && L <= 80, "xattn_fold: UB=%d, %d prompt keys (1..80 fit the 80 key slots of a head)", UB, L);
    SD_REQUIRE(heads > 0 && C > 0 && C % heads == 0, "xattn_fold: heads=%d does not divide C=%d", heads, C);
    SD_REQUIRE((C / heads) % 2 == 0, "xattn_fold: odd head dim %d (C=%d heads=%d)", C / heads, C, heads);
    SD_REQUIRE(C % 64 == 0, "xattn_fold: C=%d must be a multiple of 64 (the GEMMs' K)", C);
    SD_REQUIRE(!perm || c1 == nullptr, "xattn_fold: c1 is read from the natural layout of A^T (the tiled form takes none)");
    int rc;
    const int NH = heads, NP = NH * 80, d = C / NH;
    bf16_t* kexp = scratch;
    bf16_t* vexp = kexp + (size_t)UB * NP * C;
    if ((rc = sd_launch_xattn_expand(kv, kexp, UB, L, C, NH, 0, 1.0f / sqrtf((float)d), stream))) return rc;
    if ((rc = sd_launch_xattn_expand(kv, vexp, UB, L, C, NH, C, 1.0f, stream))) return rc;
    // fused kernel: both operands are re-tiled ([32-column slice][rows][64 B]) so that its DMA pieces are contiguous;
    // the plain layouts land in the third scratch slab first
    bf16_t* tmp = scratch + (size_t)2 * UB * NP * C;
    {   // A^T [UB*NP, C]: rows (sample, head, key), K-contiguous over the UNet channel -> W operand of GEMM 1
        if ((rc = fold_gemm(kexp, UB * NP, C, wqT, C, nullptr, perm ? tmp : at_dst, stream))) return rc;
        if (perm && (rc = sd_launch_retile32(tmp, at_dst, UB, NP, C, NP, stream))) return rc;
    }
    if (c1) {    // what is left of the mean term: c1[sample][slot] = sum over the channel of the ROUNDED centred row
        if ((rc = sd_launch_gemv(ones, at_dst, nullptr, c1, UB * NP, C, 0, stream))) return rc;
    }
    if (c2) {    // beta term of every key slot: c2[sample][slot] = (scale K_h[slot]) . u   (fp32 GEMV over the expanded rows)
        if ((rc = sd_launch_gemv(lnu, kexp, nullptr, c2, UB * NP, C, 0, stream))) return rc;
    }
    {   // B^T [UB*NP, C] = V_masked . W_o^T (one GEMM, into the K expansion's scratch), then transposed per sample
        // to [C, NP]: K-contiguous over (head, key) -> W operand of GEMM 2
        if ((rc = fold_gemm(vexp, UB * NP, C, wo, C, nullptr, kexp, stream))) return rc;
        if ((rc = sd_launch_transpose_bf16(kexp, perm ? tmp : bw_dst, UB, NP, C, stream, perm ? 1 : 0))) return rc;
        if (perm && (rc = sd_launch_retile32(tmp, bw_dst, UB, C, NP, 32, stream))) return rc;
    }
    return 0;
}

// The operands of ONE IP-Adapter block from its projected image tokens ip_kv [UB * T][K_ip | V_ip]: per-head expansions over 32
// key slots (32 / heads per head, T of them used) and the folds
//   at [UB][32][C] = (K_ip / sqrt d)_expanded . W_q      bt [UB][C][32] = ((scale V_ip)_expanded . W_o^T)^T
// scratch = three slabs of UB * 32 * C bf16 (counted from 0); afterwards slab 0 = the K expansion, slab 1 = the V expansion (times scale),
// slab 2 = bt before the transpose ([UB * 32][C]).
int sd_launch_ip_fold(const bf16_t* ip_kv, const bf16_t* wqT, const bf16_t* wo, bf16_t* at, bf16_t* bt, bf16_t* scratch, int UB, int T,
                      int C, int heads, float scale, hipStream_t stream) {
    SD_REQUIRE(ip_kv && wqT && wo && at && bt && scratch, "ip_fold: null operand");
    SD_REQUIRE(heads > 0 && C > 0 && C % heads == 0, "ip_fold: heads=%d does not divide C=%d", heads, C);
    SD_REQUIRE((C / heads) % 2 == 0, "ip_fold: odd head dim %d (C=%d heads=%d)", C / heads, C, heads);
    SD_REQUIRE(32 % heads == 0 && UB > 0 && T > 0 && T <= 32 / heads, "ip_fold: UB=%d, %d image tokens in the %d key slots of a head "
               "(32 slots over %d heads)", UB, T, 32 % heads == 0 ? 32 / heads : 0, heads);
    SD_REQUIRE(C % 64 == 0, "ip_fold: C=%d must be a multiple of 64 (the GEMMs' K)", C);
    int rc;
    const int NH = heads, SPH = 32 / NH, d = C / NH;
    bf16_t* kexp = scratch;
    bf16_t* vexp = kexp + (size_t)UB * 32 * C;
    bf16_t* tmp = vexp + (size_t)UB * 32 * C;
    if ((rc = sd_launch_xattn_expand(ip_kv, kexp, UB, T, C, NH, 0, 1.0f / sqrtf((float)d), stream, SPH))) return rc;
    if ((rc = sd_launch_xattn_expand(ip_kv, vexp, UB, T, C, NH, C, scale, stream, SPH))) return rc;
    if ((rc = fold_gemm(kexp, UB * 32, C, wqT, C, nullptr, at, stream))) return rc;
    if ((rc = fold_gemm(vexp, UB * 32, C, wo, C, nullptr, tmp, stream))) return rc;
    return sd_launch_transpose_bf16(tmp, bt, UB, 32, C, stream);
}

extern "C" int sd_unet_set_context(sd_unet* u, void* stream, const float* ehs, int unet_batch, int cache_branch_id,
                                   void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u, "set_context: null handle");
    return sd_unet_set_context_hw(u, stream, ehs, unet_batch, cache_branch_id, u->cfg.sample_size, u->cfg.sample_size,
                                  workspace, workspace_bytes);
}

// The context tensors of a (batch, branch) sit at the same offsets in every plan variant of ONE latent size: a size change
// needs its own set_context.
extern "C" int sd_unet_set_context_hw(sd_unet* u, void* stream, const float* ehs, int unet_batch, int cache_branch_id,
                                      int latent_h, int latent_w, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->unet_like(), "set_context: not a UNet or ControlNet handle");
    SD_REQUIRE(ehs && workspace, "set_context: null argument");
    SD_REQUIRE(u->tg_mode != TGATE_REUSE, "set_context: the handle is in T-GATE reuse mode, whose plans read no prompt context "
                                         "(sd_unet_set_tgate_hw: mode 0 or 1 first)");
    if (check_latent_size(u, latent_h, latent_w, "set_context")) return -1;
    Plan* plp;
    int rc = get_plan(u, plan_variant(u, unet_batch, cache_branch_id, latent_h, latent_w), &plp);
    if (rc) return rc;
    Plan& pl = *plp;
    if (check_workspace(pl, "set_context", workspace, workspace_bytes)) return -1;
    char* ws = (char*)workspace;
    const int L = u->cfg.context_len, CD = u->cfg.cross_attention_dim, M = unet_batch * L;
    bf16_t* cb = (bf16_t*)(ws + pl.tensors[pl.ctx_bf16].off);
    if ((rc = sd_launch_f32_to_bf16(ehs, cb, (long)M * CD, (hipStream_t)stream))) return rc;
    auto gemm = [&](const bf16_t* X, int rows, int K, size_t w, int N, bf16_t* out) {      // out [rows][N] = X [rows][K] . W[N][K]^T
        GemmArgs a;
        a.X = X; a.ldx = K; a.K1 = K; a.K = K; a.M = rows; a.N = N;
        a.W = (const bf16_t*)(u->dweights + w);
        a.C = out; a.ldc = N;
        a.zero_page = g_zero_page;
        return sd_launch_gemm(a, 0, (hipStream_t)stream);
    };
    for (size_t i = 0; i < pl.ctx_kv.size(); ++i)
        if ((rc = gemm(cb, M, CD, pl.ctx_w[i], 2 * pl.ctx_c[i], (bf16_t*)(ws + pl.tensors[pl.ctx_kv[i]].off)))) return rc;
    // folded prompt cross-attention: A^T = (scale K)_masked . W_q  and  B = W_o . V_masked^T per sample and layer
    for (const Plan::Fold& f : pl.ctx_fold) {
        auto WB = [&](size_t off) { return (const bf16_t*)(u->dweights + off); };
        auto WF = [&](size_t off) { return (const float*)(u->dweights + off); };
        if ((rc = sd_launch_xattn_fold((const bf16_t*)(ws + pl.tensors[f.kv].off), WB(f.wqT), WB(f.wo), f.c2 >= 0 ? WF(f.lnu) : nullptr,
                                       f.c1 >= 0 ? WF(f.ones) : nullptr, (bf16_t*)(ws + pl.tensors[f.at].off),
                                       (bf16_t*)(ws + pl.tensors[f.bw].off), f.c1 >= 0 ? (float*)(ws + pl.tensors[f.c1].off) : nullptr,
                                       f.c2 >= 0 ? (float*)(ws + pl.tensors[f.c2].off) : nullptr,
                                       (bf16_t*)(ws + pl.tensors[pl.ctx_fold_scratch].off), unet_batch, L, f.C, f.heads, f.perm ? 1 : 0,
                                       (hipStream_t)stream))) return rc;
    }
    return 0;
}

extern "C" int sd_unet_set_timestep_cond(sd_unet* u, void* stream, const float* cond) {
    SD_REQUIRE(u && u->unet_like(), "set_timestep_cond: not a UNet or ControlNet handle");
    if (!cond) {
        u->cond_set = false;
        return 0;
    }
    const int d = u->cfg.time_cond_proj_dim, c0 = u->cfg.block_out_channels[0];
    SD_REQUIRE(d > 0, "set_timestep_cond: the UNet has no time_embedding.cond_proj (time_cond_proj_dim = 0)");
    SD_REQUIRE(u->finalized && u->dcond, "set_timestep_cond: parameters not finalized");
    SD_REQUIRE(((uintptr_t)cond & 15) == 0, "set_timestep_cond: cond must be 16-byte aligned");
    const int rc = sd_launch_gemv(cond, (const bf16_t*)(u->dweights + u->woff.at("time_embedding.cond_proj.weight")), nullptr,
                                  u->dcond, c0, d, 0, (hipStream_t)stream);
    if (rc) return rc;
    u->cond_set = true;
    return 0;
}

extern "C" int sd_unet_set_inpaint_cond_hw(sd_unet* u, void* stream, const float* mask, const float* masked_latents, int batch,
                                           int latent_h, int latent_w) {
    SD_REQUIRE(u && u->kind == 0, "set_inpaint_cond: not a UNet handle");
    SD_REQUIRE(u->cfg.in_channels == 9, "set_inpaint_cond: the UNet has in_channels = %d (an inpainting UNet has 9)",
               u->cfg.in_channels);
    if (!mask && !masked_latents) {     // clear: the next forward needs a condition of its own
        u->inpaint_b = 0;
        return 0;
    }
    SD_REQUIRE(mask && masked_latents && batch > 0, "set_inpaint_cond: null argument");
    SD_REQUIRE((((uintptr_t)mask | (uintptr_t)masked_latents) & 15) == 0, "set_inpaint_cond: operands must be 16-byte aligned");
    if (check_latent_size(u, latent_h, latent_w, "set_inpaint_cond")) return -1;
    const size_t bytes = (size_t)batch * 5 * latent_h * latent_w * sizeof(float);
    if (bytes > u->inpaint_cap) {
        if (u->dinpaint) (void)hipFree(u->dinpaint);     // (synchronises: no earlier forward still reads it)
        u->dinpaint = nullptr; u->inpaint_cap = 0; u->inpaint_b = 0;
        SD_CHECK_HIP(hipMalloc((void**)&u->dinpaint, bytes));
        u->inpaint_cap = bytes;
    }
    u->inpaint_b = 0;
    const int rc = sd_launch_inpaint_cond_pack(mask, masked_latents, u->dinpaint, batch, (long)latent_h * latent_w,
                                               (hipStream_t)stream);
    if (rc) return rc;
    u->inpaint_b = batch; u->inpaint_h = latent_h; u->inpaint_w = latent_w;
    return 0;
}

// ---- IP-Adapter image prompt (diffusers IPAdapterAttnProcessor2_0 + ImageProjection, upstream-recall) ----
// a forward of a handle that has an image prompt set somewhere must find one for ITS (batch, branch, size)
static int check_ip_set(const sd_unet* u, const char* who, int unet_batch, int cache_branch_id, int latent_h, int latent_w) {
    SD_REQUIRE(ip_active(u, unet_batch, cache_branch_id, latent_h, latent_w),
               "%s: the handle runs with an IP-Adapter image prompt, but none is set for batch %d, cache branch %d at %dx%d "
               "(sd_unet_set_ip_adapter_hw after sd_unet_set_context_hw, same workspace; image_embeds = NULL clears the others)",
               who, unet_batch, cache_branch_id < 0 ? -1 : cache_branch_id, latent_h, latent_w);
    return 0;
}

extern "C" int sd_unet_set_ip_adapter_hw(sd_unet* u, void* stream, const float* image_embeds, int unet_batch, int cache_branch_id,
                                         int latent_h, int latent_w, float scale, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 0, "set_ip_adapter: not a UNet handle");
    const sd_unet_config& c = u->cfg;
    SD_REQUIRE(c.ip_adapter_tokens > 0, "set_ip_adapter: the UNet was created without an IP-Adapter (ip_adapter_tokens = 0)");
    const auto key = std::make_tuple(unet_batch, cache_branch_id < 0 ? -1 : cache_branch_id, latent_h, latent_w);
    if (!image_embeds) {        // clear: nothing is launched
        u->ip_keys.erase(key);
        return 0;
    }
    SD_REQUIRE(workspace, "set_ip_adapter: null workspace");
    SD_REQUIRE(((uintptr_t)image_embeds & 15) == 0, "set_ip_adapter: image_embeds must be 16-byte aligned");
    SD_REQUIRE(scale == scale && fabsf(scale) <= 1e4f, "set_ip_adapter: scale %g", scale);
    if (check_latent_size(u, latent_h, latent_w, "set_ip_adapter")) return -1;
    Plan* plp;
    PlanVariant v = plan_variant(u, unet_batch, cache_branch_id, latent_h, latent_w);
    v.ip = 1;
    int rc = get_plan(u, v, &plp);
    if (rc) return rc;
    const Plan& pl = *plp;
    if (check_workspace(pl, "set_ip_adapter", workspace, workspace_bytes)) return -1;
    u->ip_keys.erase(key);      // (set again only once every launch below is enqueued)
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    auto TP = [&](int id) { return (bf16_t*)(ws + pl.tensors[id].off); };
    auto WF = [&](const char* k) { return (const float*)(u->dweights + u->woff.at(k)); };
    auto gemm = [&](const bf16_t* X, int rows, int K, size_t w, int N, const float* bias, bf16_t* out) {      // out [rows][N] = X [rows][K] . W[N][K]^T + bias
        GemmArgs a;
        a.X = X; a.ldx = K; a.K1 = K; a.K = K; a.M = rows; a.N = N;
        a.W = (const bf16_t*)(u->dweights + w); a.bias = bias;
        a.C = out; a.ldc = N;
        a.zero_page = g_zero_page;
        return sd_launch_gemm(a, 0, st);
    };
    const int T = c.ip_adapter_tokens, E = c.ip_adapter_embed_dim, CD = c.cross_attention_dim, UB = unet_batch;
    const std::string ipj = "encoder_hid_proj.image_projection_layers.0.";
    // ImageProjection: tokens = LayerNorm(Linear(image_embeds).reshape(UB, T, CD))
    if ((rc = sd_launch_f32_to_bf16(image_embeds, TP(pl.ip_e), (long)UB * E, st))) return rc;
    if ((rc = gemm(TP(pl.ip_e), UB, E, u->woff.at(ipj + "image_embeds.weight"), T * CD, WF((ipj + "image_embeds.bias").c_str()), TP(pl.ip_proj))))
        return rc;
    if ((rc = sd_launch_layernorm(TP(pl.ip_proj), WF((ipj + "norm.weight").c_str()), WF((ipj + "norm.bias").c_str()), TP(pl.ip_tok), UB * T,
                                  CD, 1e-5f, st))) return rc;
    // per block: K_ip | V_ip, their per-head expansions over 32 key slots (32 / heads per head, T of them used), and the folds
    //   A [UB][32][C] = (K_ip / sqrt d)_expanded . W_q      Bt [UB][C][32] = ((scale V_ip)_expanded . W_o^T)^T
    for (const Plan::IpFold& f : pl.ip_fold) {
        auto WB = [&](size_t off) { return (const bf16_t*)(u->dweights + off); };
        if ((rc = gemm(TP(pl.ip_tok), UB * T, CD, f.wkv, 2 * f.C, nullptr, TP(pl.ip_kv)))) return rc;
        if ((rc = sd_launch_ip_fold(TP(pl.ip_kv), WB(f.wqT), WB(f.wo), TP(f.at), TP(f.bt), TP(pl.ctx_fold_scratch), UB, T, f.C, f.heads,
                                    scale, st))) return rc;
    }
    u->ip_keys.insert(key);
    return 0;
}

// ---- ControlNet (diffusers ControlNetModel, upstream-recall) ----
extern "C" int sd_controlnet_create(const sd_unet_config* cfg, const int cond_embed_channels[4], sd_unet** out) {
    SD_REQUIRE(cfg && cond_embed_channels && out, "sd_controlnet_create: null argument");
    SD_REQUIRE(cfg->weight_dtype != SD_DTYPE_FP8_E4M3, "sd_controlnet_create: weight_dtype=\"fp8\" is not built for a ControlNet (bf16 is "
               "the only path)");
    if (check_unet_config(cfg, "sd_controlnet_create")) return -1;
    SD_REQUIRE(cfg->in_channels == 4, "sd_controlnet_create: in_channels %d (4 is built)", cfg->in_channels);
    SD_REQUIRE(cfg->ip_adapter_tokens == 0 && cfg->ip_adapter_embed_dim == 0, "sd_controlnet_create: a ControlNet takes no IP-Adapter");
    SD_REQUIRE(cfg->block_out_channels[0] % 8 == 0, "sd_controlnet_create: block_out_channels[0]");
    int nres = 1;
    for (int i = 0; i < cfg->num_levels; ++i) nres += cfg->layers_per_block + (i < cfg->num_levels - 1 ? 1 : 0);
    SD_REQUIRE(nres + 1 <= MAX_CONTROL_RES, "sd_controlnet_create: %d residuals (at most %d are built)", nres + 1, MAX_CONTROL_RES);
    for (int i = 0; i < 4; ++i)
        SD_REQUIRE(cond_embed_channels[i] > 0 && cond_embed_channels[i] % 8 == 0 && cond_embed_channels[i] <= 1024,
                   "sd_controlnet_create: cond_embed_channels[%d]=%d (conditioning_embedding_out_channels: four positive multiples "
                   "of 8)", i, cond_embed_channels[i]);
    sd_unet* u = new_handle(5, cfg);
    for (int i = 0; i < 4; ++i) u->cond_embed[i] = cond_embed_channels[i];
    enumerate_params(u);
    *out = u;
    return 0;
}

extern "C" long long sd_controlnet_residual_bytes_hw(const sd_unet* u, int unet_batch, int latent_h, int latent_w) {
    SD_REQUIRE(u && u->unet_like(), "controlnet_residual_bytes: not a UNet or ControlNet handle");
    SD_REQUIRE(unet_batch > 0 && unet_batch <= 4096, "controlnet_residual_bytes: bad batch %d", unet_batch);
    if (check_latent_size(u, latent_h, latent_w, "controlnet_residual_bytes")) return -1;
    std::vector<size_t> off;
    std::vector<long> count;
    return (long long)control_segments(u->cfg, unet_batch, latent_h, latent_w, &off, &count);
}

extern "C" int sd_controlnet_set_cond_hw(sd_unet* u, void* stream, const float* cond_image, int batch, int latent_h, int latent_w) {
    SD_REQUIRE(u && u->kind == 5, "controlnet_set_cond: not a ControlNet handle");
    if (!cond_image) {
        u->cn_b = 0;
        return 0;
    }
    SD_REQUIRE(u->finalized, "controlnet_set_cond: parameters not finalized");
    SD_REQUIRE(batch > 0 && batch <= 4096, "controlnet_set_cond: bad batch %d", batch);
    SD_REQUIRE(((uintptr_t)cond_image & 15) == 0, "controlnet_set_cond: cond_image must be 16-byte aligned");
    if (check_latent_size(u, latent_h, latent_w, "controlnet_set_cond")) return -1;
    std::string names[8];
    int cin[8], cout[8], stride[8];
    cond_embed_convs(u, names, cin, cout, stride);
    // scratch: the bf16 NHWC image, then two buffers the chain alternates between, each as large as its largest tensor
    const int H = 8 * latent_h, W = 8 * latent_w, c0 = u->cfg.block_out_channels[0];
    auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
    size_t big = 0;
    {
        int h = H, w = W;
        for (int i = 0; i < 7; ++i) {
            h = (h + 2 - 3) / stride[i] + 1; w = (w + 2 - 3) / stride[i] + 1;
            big = std::max(big, (size_t)batch * h * w * cout[i] * 2);
        }
        SD_REQUIRE(h == latent_h && w == latent_w, "controlnet_set_cond: the embedding of a %dx%d image is %dx%d, not the latent %dx%d", H,
                   W, h, w, latent_h, latent_w);
    }
    const size_t img_bytes = up256((size_t)batch * H * W * 3 * 2), buf_bytes = up256(big);
    const size_t need = img_bytes + 2 * buf_bytes, out_bytes = (size_t)batch * latent_h * latent_w * c0 * 2;
    u->cn_b = 0;
    if (need > u->cn_scratch_cap) {
        if (u->cn_scratch) (void)hipFree(u->cn_scratch);     // (synchronises: no earlier launch still uses it)
        u->cn_scratch = nullptr; u->cn_scratch_cap = 0;
        SD_CHECK_HIP(hipMalloc((void**)&u->cn_scratch, need));
        u->cn_scratch_cap = need;
    }
    if (out_bytes > u->cn_embed_cap) {
        if (u->cn_embed) (void)hipFree(u->cn_embed);
        u->cn_embed = nullptr; u->cn_embed_cap = 0;
        SD_CHECK_HIP(hipMalloc((void**)&u->cn_embed, out_bytes));
        u->cn_embed_cap = out_bytes;
    }
    hipStream_t st = (hipStream_t)stream;
    bf16_t* img = (bf16_t*)u->cn_scratch;
    bf16_t* buf[2] = {(bf16_t*)(u->cn_scratch + img_bytes), (bf16_t*)(u->cn_scratch + img_bytes + buf_bytes)};
    int rc = sd_launch_nchw_to_nhwc_bf16(cond_image, img, batch, 3, (long)H * W, st);
    if (rc) return rc;
    const bf16_t* x = img;
    int h = H, w = W;
    for (int i = 0; i < 8; ++i) {
        bf16_t* y = i == 7 ? u->cn_embed : buf[i & 1];
        rc = sd_launch_inception_conv(x, (const bf16_t*)(u->dweights + u->woff.at(names[i] + "weight")),
                                      (const float*)(u->dweights + u->woff.at(names[i] + "bias")), y, batch, h, w, cin[i], cout[i], 3, 3,
                                      stride[i], 1, 1, cout[i], 0, i == 7 ? 0 : 2 /* SiLU */, st);
        if (rc) return rc;
        h = (h + 2 - 3) / stride[i] + 1; w = (w + 2 - 3) / stride[i] + 1;
        x = y;
    }
    u->cn_b = batch; u->cn_h = latent_h; u->cn_w = latent_w;
    return 0;
}

extern "C" int sd_controlnet_forward_hw(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch, int latent_h,
                                        int latent_w, float timestep, void* residuals, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 5, "controlnet_forward: not a ControlNet handle");
    SD_REQUIRE(latents && residuals && workspace, "controlnet_forward: null argument");
    SD_REQUIRE(((uintptr_t)residuals & 255) == 0, "controlnet_forward: the residual buffer must be 256-byte aligned");
    if (check_latent_size(u, latent_h, latent_w, "controlnet_forward")) return -1;
    SD_REQUIRE(latent_batch > 0 && unet_batch % latent_batch == 0, "controlnet_forward: unet batch %d not a multiple of latent batch %d",
               unet_batch, latent_batch);
    Plan* pl;
    u->last = plan_variant(u, unet_batch, -1, latent_h, latent_w);
    u->last.rep = plan_rep(u, latent_batch, unet_batch);
    int rc = get_plan(u, u->last, &pl);
    if (rc) return rc;
    return run_plan(u, *pl, "controlnet_forward", workspace, workspace_bytes, latents, latent_batch, (float*)residuals, timestep, stream);
}

extern "C" int sd_unet_set_control_residuals_hw(sd_unet* u, const void* residuals, float scale, int unet_batch, int latent_h, int latent_w) {
    SD_REQUIRE(u && u->kind == 0, "set_control_residuals: not a UNet handle");
    if (!residuals) {
        u->ctrl_res = nullptr;
        return 0;
    }
    if (check_options("set_control_residuals", active_options(u) | opt_bit(OPT_CONTROL))) return -1;
    SD_REQUIRE(((uintptr_t)residuals & 255) == 0, "set_control_residuals: the residual buffer must be 256-byte aligned");
    SD_REQUIRE(scale == scale && fabsf(scale) <= 1e4f, "set_control_residuals: scale %g", scale);
    SD_REQUIRE(unet_batch > 0 && unet_batch <= 4096, "set_control_residuals: bad batch %d", unet_batch);
    if (check_latent_size(u, latent_h, latent_w, "set_control_residuals")) return -1;
    u->ctrl_enabled = true;
    u->ctrl_res = (const char*)residuals; u->ctrl_scale = scale;
    u->ctrl_ub = unet_batch; u->ctrl_h = latent_h; u->ctrl_w = latent_w;
    return 0;
}

// a forward of a handle with ControlNet residuals set must be the one they were laid out for
static int check_control_set(const sd_unet* u, const char* who, int unet_batch, int latent_h, int latent_w) {
    SD_REQUIRE(u->ctrl_ub == unet_batch && u->ctrl_h == latent_h && u->ctrl_w == latent_w,
               "%s: the ControlNet residuals were set for batch %d at %dx%d, the forward runs batch %d at %dx%d "
               "(sd_unet_set_control_residuals_hw; residuals = NULL clears them)", who, u->ctrl_ub, u->ctrl_h, u->ctrl_w, unet_batch,
               latent_h, latent_w);
    return 0;
}

// a forward of a handle in a T-GATE mode must be the one its cache is laid out for; reuse needs a capture before it
// (batch 2 b of a capture = the CFG pair [uncond | cond] of b latents, whether the caller passes b latents or all 2 b rows)
static int check_tgate_forward(const sd_unet* u, const char* who, int latent_batch, int unet_batch, int latent_h, int latent_w) {
    SD_REQUIRE(u->tg_h == latent_h && u->tg_w == latent_w,
               "%s: the T-GATE cache was set for %d latents at %dx%d, the forward runs at %dx%d (sd_unet_set_tgate_hw)", who,
               u->tg_b, u->tg_h, u->tg_w, latent_h, latent_w);
    SD_REQUIRE(latent_batch > 0 && unet_batch % latent_batch == 0, "%s: unet batch %d not a multiple of latent batch %d (T-GATE cache set "
               "for %d latents)", who, unet_batch, latent_batch, u->tg_b);
    if (u->tg_mode == TGATE_REUSE) {
        SD_REQUIRE(u->tg_captured, "%s: T-GATE reuse before any capture: the cache holds nothing for %d latents at %dx%d (run one forward "
                   "in capture mode first)", who, u->tg_b, u->tg_h, u->tg_w);
        SD_REQUIRE(unet_batch == u->tg_b, "%s: a T-GATE reuse forward runs at the batch of the capture's latents (%d), not %d: there is no "
                   "classifier-free guidance behind the gate", who, u->tg_b, unet_batch);
    } else {
        SD_REQUIRE(unet_batch == u->tg_b || unet_batch == 2 * u->tg_b, "%s: a T-GATE capture forward runs at the latent batch or twice it "
                   "(%d latents, UNet batch %d)", who, u->tg_b, unet_batch);
    }
    return 0;
}

// the last forward's variant (its size, replication, image prompt and residuals) at a batch and branch, under the handle's options now
static PlanVariant last_variant(const sd_unet* u, int unet_batch, int branch) {
    PlanVariant v = plan_variant(u, unet_batch, branch, u->last.lh > 0 ? u->last.lh : -1, u->last.lw > 0 ? u->last.lw : -1);
    v.rep = u->last.rep; v.ip = u->last.ip; v.cn = u->last.cn;
    return v;
}

// The variant a forward runs -- the handle's options with its image prompt and residuals, where set -- into u->last, refused
// where two of its options are not built together or what is set on the handle was laid out for another forward
static int forward_variant(sd_unet* u, const char* who, int latent_batch, int unet_batch, int cache_mode, int branch, int latent_h,
                           int latent_w) {
    PlanVariant v = plan_variant(u, unet_batch, branch, latent_h, latent_w);
    v.rep = plan_rep(u, latent_batch, unet_batch);
    v.ip = u->ip_keys.empty() ? 0 : 1;
    v.cn = u->ctrl_res ? 1 : 0;
    if (check_options(who, variant_options(u, v) | (cache_mode != SD_CACHE_OFF ? opt_bit(OPT_DEEPCACHE) : 0))) return -1;
    if (v.ip && check_ip_set(u, who, unet_batch, branch, latent_h, latent_w)) return -1;
    if (v.cn && check_control_set(u, who, unet_batch, latent_h, latent_w)) return -1;
    if (v.tgate && check_tgate_forward(u, who, latent_batch, unet_batch, latent_h, latent_w)) return -1;
    // with a PAG mask the forward runs [uncond | cond | perturbed] or [cond | perturbed] over ONE set of latents
    SD_REQUIRE(!v.pag_mask || unet_batch == 3 * latent_batch || unet_batch == 2 * latent_batch, "%s: with PAG on the UNet batch is 3 or 2 "
               "times the latent batch, [uncond | cond | perturbed] or [cond | perturbed] (UNet batch %d, %d latents; sd_unet_set_pag(u, 0) = "
               "off)", who, unet_batch, latent_batch);
    SD_REQUIRE(!v.sag || u->sag_mass, "%s: SAG capture is on and no mass buffer is set (sd_unet_set_sag_buffer)", who);
    u->last = v;
    return 0;
}

// the handle's dst-choice array for the plan about to run: n bytes, zero (position 0 of every cell) unless set for this size
static int ensure_tome_choice(sd_unet* u, long n, void* stream) {
    if (n <= 0 || (u->tome_choice && u->tome_choice_n == n)) return 0;
    if ((size_t)n > u->tome_choice_cap) {
        if (u->tome_choice) (void)hipFree(u->tome_choice);      // (synchronises: no earlier forward still reads it)
        u->tome_choice = nullptr; u->tome_choice_cap = 0;
        SD_CHECK_HIP(hipMalloc((void**)&u->tome_choice, (size_t)n));
        u->tome_choice_cap = (size_t)n;
    }
    SD_CHECK_HIP(hipMemsetAsync(u->tome_choice, 0, (size_t)n, (hipStream_t)stream));
    u->tome_choice_n = n;
    return 0;
}

extern "C" int sd_unet_forward(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                               float timestep, float* eps_out, void* workspace, long long workspace_bytes,
                               int cache_mode, int cache_branch_id) {
    SD_REQUIRE(u && u->kind == 0, "forward: not a UNet handle");
    return sd_unet_forward_hw(u, stream, latents, latent_batch, unet_batch, u->cfg.sample_size, u->cfg.sample_size, timestep,
                              eps_out, workspace, workspace_bytes, cache_mode, cache_branch_id);
}

extern "C" int sd_unet_forward_hw(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                                  int latent_h, int latent_w, float timestep, float* eps_out, void* workspace,
                                  long long workspace_bytes, int cache_mode, int cache_branch_id) {
    SD_REQUIRE(u && u->kind == 0, "forward: not a UNet handle");
    SD_REQUIRE(latents && eps_out && workspace, "forward: null argument");
    if (check_latent_size(u, latent_h, latent_w, "forward")) return -1;
    SD_REQUIRE(latent_batch > 0 && unet_batch % latent_batch == 0, "forward: unet batch %d not a multiple of latent batch %d",
               unet_batch, latent_batch);
    SD_REQUIRE(cache_mode >= 0 && cache_mode <= 2, "forward: cache_mode %d", cache_mode);
    SD_REQUIRE(cache_mode == SD_CACHE_OFF || cache_branch_id >= 0, "forward: DeepCache modes need cache_branch_id >= 0");
    Plan* pl;
    if (forward_variant(u, "forward", latent_batch, unet_batch, cache_mode, cache_branch_id, latent_h, latent_w)) return -1;
    int rc = get_plan(u, u->last, &pl);
    if (rc) return rc;
    if ((rc = ensure_tome_choice(u, pl->tome_choice_bytes, stream))) return rc;
    rc = run_plan(u, *pl, "forward", workspace, workspace_bytes, latents, latent_batch, eps_out, timestep, stream, cache_mode);
    if (u->tg_mode == TGATE_CAPTURE) u->tg_captured = rc == 0;
    return rc;
}

// ---- FreeU (freeu.hip; the plan side is the up loop of Builder::build) ----------------------------------------------------
extern "C" int sd_unet_set_freeu(sd_unet* u, float s1, float s2, float b1, float b2) {
    SD_REQUIRE(u && u->kind == 0, "set_freeu: not a UNet handle");
    if (check_options("set_freeu", active_options(u) | opt_bit(OPT_FREEU))) return -1;
    const float f[4] = {s1, s2, b1, b2};
    for (int i = 0; i < 4; ++i)
        SD_REQUIRE(f[i] > 0.f && f[i] <= 3.0e38f, "set_freeu: s1=%g s2=%g b1=%g b2=%g (all four must be finite and > 0)", s1, s2, b1, b2);
    u->freeu_s[0] = s1; u->freeu_s[1] = s2; u->freeu_b[0] = b1; u->freeu_b[1] = b2;
    u->freeu_on = true;
    return 0;
}

extern "C" int sd_unet_disable_freeu(sd_unet* u) {
    SD_REQUIRE(u && u->kind == 0, "disable_freeu: not a UNet handle");
    u->freeu_on = false;
    return 0;
}

// ---- T-GATE (tgate.hip; the plan side is Builder::transformer) ------------------------------------------------------------
static int check_tgate_handle(const sd_unet* u, const char* who) {
    SD_REQUIRE(u && u->kind == 0, "%s: not a UNet handle", who);
    return check_options(who, (active_options(u) & (opt_bit(OPT_FP8) | opt_bit(OPT_INPAINT9) | opt_bit(OPT_IP_MODEL))) | opt_bit(OPT_TGATE));
}

extern "C" long long sd_unet_tgate_bytes_hw(sd_unet* u, int latent_batch, int latent_h, int latent_w) {
    if (check_tgate_handle(u, "tgate_bytes")) return -1;
    SD_REQUIRE(latent_batch > 0 && latent_batch <= 4096, "tgate_bytes: bad batch %d", latent_batch);
    if (check_latent_size(u, latent_h, latent_w, "tgate_bytes")) return -1;
    std::vector<size_t> off; std::vector<long> rows; std::vector<int> ch;
    return (long long)tgate_segments(u->cfg, latent_batch, latent_h, latent_w, &off, &rows, &ch);
}

extern "C" int sd_unet_tgate_block_info_hw(sd_unet* u, int block, int latent_batch, int latent_h, int latent_w, long long* offset,
                                           long long* rows, int* channels) {
    if (check_tgate_handle(u, "tgate_block_info")) return -1;
    SD_REQUIRE(latent_batch > 0 && latent_batch <= 4096, "tgate_block_info: bad batch %d", latent_batch);
    if (check_latent_size(u, latent_h, latent_w, "tgate_block_info")) return -1;
    std::vector<size_t> off; std::vector<long> r; std::vector<int> ch;
    tgate_segments(u->cfg, latent_batch, latent_h, latent_w, &off, &r, &ch);
    if (block < 0) return (int)off.size();          // (the block count)
    SD_REQUIRE(block < (int)off.size(), "tgate_block_info: block %d of %zu", block, off.size());
    if (offset) *offset = (long long)off[block];
    if (rows) *rows = r[block];
    if (channels) *channels = ch[block];
    return (int)off.size();
}

extern "C" int sd_unet_set_tgate_hw(sd_unet* u, int mode, void* cache, long long bytes, int latent_batch, int latent_h, int latent_w) {
    SD_REQUIRE(u && u->kind == 0, "set_tgate: not a UNet handle");
    if (mode == TGATE_OFF) {
        SD_REQUIRE(!cache, "set_tgate: mode 0 takes cache = NULL (it clears the setting)");
        u->tg_mode = TGATE_OFF; u->tg_cache = nullptr; u->tg_bytes = 0; u->tg_b = u->tg_h = u->tg_w = 0; u->tg_captured = false;
        return 0;
    }
    SD_REQUIRE(mode == TGATE_CAPTURE || mode == TGATE_REUSE, "set_tgate: mode %d (0 = off, 1 = capture, 2 = reuse)", mode);
    if (check_options("set_tgate", active_options(u) | opt_bit(OPT_TGATE))) return -1;
    SD_REQUIRE(cache && ((uintptr_t)cache & 255) == 0, "set_tgate: the cache buffer must be a 256-byte aligned device pointer");
    const long long need = sd_unet_tgate_bytes_hw(u, latent_batch, latent_h, latent_w);
    if (need < 0) return -1;
    SD_REQUIRE(bytes >= need, "set_tgate: the cache buffer holds %lld bytes, %d latents at %dx%d need %lld (sd_unet_tgate_bytes_hw)", bytes,
               latent_batch, latent_h, latent_w, need);
    // what a capture wrote stays valid only for the same buffer and layout
    const bool captured = u->tg_captured && (char*)cache == u->tg_cache && latent_batch == u->tg_b && latent_h == u->tg_h && latent_w == u->tg_w;
    if (mode == TGATE_REUSE) {
        SD_REQUIRE(u->tg_captured, "set_tgate: reuse before any capture (set mode 1 and run one forward first)");
        SD_REQUIRE(captured, "set_tgate: reuse for %d latents at %dx%d, but the capture filled its buffer for %d latents at %dx%d", latent_batch,
                   latent_h, latent_w, u->tg_b, u->tg_h, u->tg_w);
    }
    u->tg_captured = captured;
    u->tg_mode = mode; u->tg_cache = (char*)cache; u->tg_bytes = bytes;
    u->tg_b = latent_batch; u->tg_h = latent_h; u->tg_w = latent_w;
    return 0;
}

extern "C" const char* sd_unet_option_name(int i) { return option_name(i); }

extern "C" const char* sd_unet_option_conflict(int a, int b) {
    return a >= 0 && a < OPT_COUNT && b >= 0 && b < OPT_COUNT ? option_conflict(a, b) : nullptr;
}

extern "C" int sd_unet_plan_count(const sd_unet* u) {
    SD_REQUIRE(u, "plan_count: null handle");
    return (int)u->plans.size();
}

// ---- PAG (pag.hip; the plan side is Builder::transformer) ------------------------------------------------------------------
extern "C" int sd_unet_pag_block_count(const sd_unet* u) {
    SD_REQUIRE(u && u->kind == 0, "pag_block_count: not a UNet handle");
    return transformer_block_count(u->cfg);
}

extern "C" int sd_unet_set_pag(sd_unet* u, long long layer_mask) {
    SD_REQUIRE(u && u->kind == 0, "set_pag: not a UNet handle");
    if (layer_mask == 0) {          // off: the plans of a handle that never saw PAG
        u->pag_mask = 0;
        return 0;
    }
    const int nb = transformer_block_count(u->cfg);
    SD_REQUIRE(nb < 63 && layer_mask > 0 && (layer_mask >> nb) == 0, "set_pag: layer mask 0x%llx (bits 0 .. %d: the UNet has %d transformer "
               "blocks; 0 = off)", (unsigned long long)layer_mask, nb - 1, nb);
    if (check_options("set_pag", active_options(u) | opt_bit(OPT_PAG))) return -1;
    u->pag_mask = layer_mask;
    return 0;
}

// ---- SAG (sag.hip; the plan side is Builder::transformer_block) ------------------------------------------------------------
extern "C" int sd_unet_set_sag(sd_unet* u, int on) {
    SD_REQUIRE(u && u->kind == 0, "set_sag: not a UNet handle");
    if (!on) {                      // off: the plans of a handle that never saw SAG
        u->sag_on = false;
        return 0;
    }
    if (check_options("set_sag", active_options(u) | opt_bit(OPT_SAG))) return -1;
    u->sag_on = true;
    return 0;
}

extern "C" int sd_unet_set_sag_buffer(sd_unet* u, float* mass, long long floats) {
    SD_REQUIRE(u && u->kind == 0, "set_sag_buffer: not a UNet handle");
    SD_REQUIRE((mass && floats > 0) || (!mass && floats == 0), "set_sag_buffer: a buffer with its size in floats, or null and 0");
    u->sag_mass = mass;
    u->sag_mass_floats = floats;
    return 0;
}

// ---- HyperTile (hypertile.hip; the plan side is Builder::transformer) --------------------------------------------------------
extern "C" int sd_unet_set_hypertile(sd_unet* u, int tile_tokens, int max_depth) {
    SD_REQUIRE(u && u->kind == 0, "set_hypertile: not a UNet handle");
    if (tile_tokens == 0) {         // off: the plans of a handle that never saw HyperTile
        u->ht_tokens = 0; u->ht_max_depth = 0;
        return 0;
    }
    SD_REQUIRE(tile_tokens >= 8 && tile_tokens <= 256, "set_hypertile: tile side of %d tokens (8 .. 256, or 0 = off)", tile_tokens);
    SD_REQUIRE(max_depth >= 0 && max_depth <= 3, "set_hypertile: max_depth %d (0 .. 3)", max_depth);
    if (check_options("set_hypertile", active_options(u) | opt_bit(OPT_HYPERTILE))) return -1;
    u->ht_tokens = tile_tokens; u->ht_max_depth = max_depth;
    return 0;
}

// the tiled blocks depend on the latent size and the setting alone: read them from the plain plan of batch 1
static int hypertile_layout(sd_unet* u, const char* who, int latent_h, int latent_w, Plan** pl) {
    SD_REQUIRE(u && u->kind == 0, "%s: not a UNet handle", who);
    if (check_latent_size(u, latent_h, latent_w, who)) return -1;
    PlanVariant v = plan_variant(u, 1, -1, latent_h, latent_w);
    v.tgate = TGATE_OFF; v.tg_pair = 1;
    return get_plan(u, v, pl);
}

extern "C" int sd_unet_hypertile_block_count_hw(sd_unet* u, int latent_h, int latent_w) {
    Plan* pl;
    if (hypertile_layout(u, "hypertile_block_count", latent_h, latent_w, &pl)) return -1;
    return (int)pl->hypertile.size();
}

extern "C" int sd_unet_hypertile_block_info_hw(sd_unet* u, int block, int latent_h, int latent_w, int* rh, int* rw, int* nh, int* nw) {
    Plan* pl;
    if (hypertile_layout(u, "hypertile_block_info", latent_h, latent_w, &pl)) return -1;
    SD_REQUIRE(block >= 0 && block < (int)pl->hypertile.size(), "hypertile_block_info: block %d of %zu", block, pl->hypertile.size());
    const Plan::HtBlock& hb = pl->hypertile[block];
    if (rh) *rh = hb.rh;
    if (rw) *rw = hb.rw;
    if (nh) *nh = hb.nh;
    if (nw) *nw = hb.nw;
    return 0;
}

// ---- Token Merging (tome.hip; the plan side is Builder::transformer) -----------------------------------------------------
extern "C" int sd_unet_set_tome(sd_unet* u, double ratio, int max_downsample) {
    SD_REQUIRE(u && u->kind == 0, "set_tome: not a UNet handle");
    if (!(ratio > 0.0)) {          // off: the plans of a handle that never saw Token Merging
        SD_REQUIRE(ratio == 0.0, "set_tome: ratio %g (0 .. 0.75)", ratio);
        u->tome_ratio = 0.0; u->tome_max_downsample = 0;
        return 0;
    }
    SD_REQUIRE(ratio <= 0.75, "set_tome: ratio %g (0 .. 0.75: a 2x2 cell has three src tokens)", ratio);
    SD_REQUIRE(max_downsample == 1 || max_downsample == 2, "set_tome: max_downsample %d (1 or 2)", max_downsample);
    if (check_options("set_tome", active_options(u) | opt_bit(OPT_TOME))) return -1;
    u->tome_ratio = ratio; u->tome_max_downsample = max_downsample;
    return 0;
}

// the plan whose merging blocks the entry points below describe: the plain variant of (batch 1, latent size) -- the blocks,
// their order and their choice slices depend on the latent size and the setting alone
static int tome_layout(sd_unet* u, const char* who, int latent_h, int latent_w, Plan** pl) {
    SD_REQUIRE(u && u->kind == 0, "%s: not a UNet handle", who);
    if (check_latent_size(u, latent_h, latent_w, who)) return -1;
    return get_plan(u, plan_variant(u, 1, -1, latent_h, latent_w), pl);
}

extern "C" int sd_unet_tome_block_count_hw(sd_unet* u, int latent_h, int latent_w) {
    Plan* pl;
    if (tome_layout(u, "tome_block_count", latent_h, latent_w, &pl)) return -1;
    return (int)pl->tome.size();
}

extern "C" int sd_unet_tome_block_info_hw(sd_unet* u, int block, int latent_h, int latent_w, int* h, int* w, int* r, long long* choice_off) {
    Plan* pl;
    if (tome_layout(u, "tome_block_info", latent_h, latent_w, &pl)) return -1;
    SD_REQUIRE(block >= 0 && block < (int)pl->tome.size(), "tome_block_info: block %d of %zu", block, pl->tome.size());
    const Plan::TomeBlock& tb = pl->tome[block];
    if (h) *h = tb.h;
    if (w) *w = tb.w;
    if (r) *r = tb.r;
    if (choice_off) *choice_off = tb.choice_off;
    return 0;
}

extern "C" int sd_unet_set_tome_choice_hw(sd_unet* u, void* stream, const unsigned char* choice, long long n, int latent_h, int latent_w) {
    Plan* pl;
    if (tome_layout(u, "set_tome_choice", latent_h, latent_w, &pl)) return -1;
    SD_REQUIRE(pl->tome_choice_bytes > 0, "set_tome_choice: Token Merging is off (sd_unet_set_tome)");
    SD_REQUIRE(choice && n == pl->tome_choice_bytes, "set_tome_choice: %lld bytes, the merging blocks at %dx%d take %ld", n, latent_h, latent_w,
               pl->tome_choice_bytes);
    if (int rc = ensure_tome_choice(u, n, stream)) return rc;
    SD_CHECK_HIP(hipMemcpyAsync(u->tome_choice, choice, (size_t)n, hipMemcpyDefault, (hipStream_t)stream));
    return 0;
}

// The matching of merging block `block` in the last forward (synchronises the stream): kept [B][num_src - r], merged [B][r],
// dst_idx [B][r] in src / dst slot numbers and tok [h * w] (host pointers, any may be null); *batch = B, the samples the block
// matched (half the UNet batch for the first block of a CFG pair: the prompt-independent prefix runs once per latent).
extern "C" int sd_unet_tome_matching_hw(sd_unet* u, void* stream, int block, int unet_batch, int cache_branch_id, void* workspace,
                                        int* kept, int* merged, int* dst_idx, int* tok, int* r, int* batch) {
    SD_REQUIRE(u && u->kind == 0 && workspace, "tome_matching: not a UNet handle, or null workspace");
    SD_REQUIRE(u->last.lh > 0, "tome_matching: no forward has run");
    Plan* pl;
    int rc = get_plan(u, last_variant(u, unet_batch, cache_branch_id), &pl);
    if (rc) return rc;
    SD_REQUIRE(block >= 0 && block < (int)pl->tome.size(), "tome_matching: block %d of %zu", block, pl->tome.size());
    const Plan::TomeBlock& tb = pl->tome[block];
    const int N = tb.h * tb.w, num_src = N - N / 4;
    SD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    auto get = [&](int* dst, int t, size_t count) -> int {
        if (!dst || !count) return 0;
        SD_CHECK_HIP(hipMemcpy(dst, (char*)workspace + pl->tensors[t].off, count * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    if ((rc = get(kept, tb.kept, (size_t)tb.B * (num_src - tb.r)))) return rc;
    if ((rc = get(merged, tb.merged, (size_t)tb.B * tb.r))) return rc;
    if ((rc = get(dst_idx, tb.dst_idx, (size_t)tb.B * tb.r))) return rc;
    if ((rc = get(tok, tb.tok, (size_t)N))) return rc;
    if (r) *r = tb.r;
    if (batch) *batch = tb.B;
    return 0;
}

// ---- fp8 activation-scale calibration (SD_DTYPE_FP8_E4M3 handles) -------------------------------------------------------
// e4m3 is a floating-point format: a per-tensor scale buys no precision, it only positions the representable range
// (+-448 down to 2^-9) over the tensor's values.  The static defaults (8 for norm outputs, 2 for the GEGLU product) clip
// at |x| > 56 / 224; real checkpoints have layers beyond that.  Calibration runs ONE forward of the plan on the caller's
// inputs op by op; every op that writes an e4m3 activation tensor is run twice: first with a probe scale under which
// nothing can saturate, its largest |value| is read back from the e4m3 codes (a small reduction kernel + one host sync per
// tensor: ~125 per forward, calibration only), then with its final scale  448 / (margin * amax)  so that the ops
// downstream see correctly quantised inputs.  amax accumulates (max) over calls: calibrate on several timesteps / prompts,
// then every plan is rebuilt with the new scales.
static float e4m3_code_value(unsigned c) {
    c &= 0x7f;
    if (c == 0x7f) return 448.f;                       // NaN code: only a saturated probe could produce it
    const int e = (int)(c >> 3), m = (int)(c & 7);
    return e == 0 ? m * (1.f / 512.f) : (1.f + m / 8.f) * ldexpf(1.f, e - 7);
}

extern "C" int sd_unet_calibrate_fp8(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                                     float timestep, float margin, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(u && u->kind == 0 && u->fp8, "calibrate_fp8: not an fp8 UNet handle");
    SD_REQUIRE(latents && workspace && latent_batch > 0 && unet_batch % latent_batch == 0, "calibrate_fp8: bad arguments");
    SD_REQUIRE(margin >= 1.f && margin <= 64.f, "calibrate_fp8: margin %g (1 .. 64: headroom over the observed amax)", margin);
    Plan* plp;
    const int rep = plan_rep(u, latent_batch, unet_batch);
    PlanVariant v = plan_variant(u, unet_batch);
    v.rep = rep;
    int rc = get_plan(u, v, &plp);
    if (rc) return rc;
    if (check_workspace(*plp, "calibrate_fp8", workspace, workspace_bytes)) return -1;
    // calibration runs the plan WITHOUT an image prompt, whose activations lie where the "IP on" plan keeps the folded
    // image operands: every image prompt of the handle is gone after it, so a later forward asks for it by name
    u->ip_keys.clear();
    hipStream_t st = (hipStream_t)stream;
    unsigned* dmax = (unsigned*)op_scratch(256);
    SD_REQUIRE(dmax, "calibrate_fp8: cannot allocate scratch");
    std::vector<float> eps((size_t)unet_batch * u->cfg.out_channels * u->cfg.sample_size * u->cfg.sample_size);
    float* deps = nullptr;
    SD_CHECK_HIP(hipMalloc((void**)&deps, eps.size() * 4));
    std::map<int, float> cur;                          // e4m3 tensor -> scale it was written with in THIS pass
    const Plan& pl = *plp;
    auto measure = [&](const Op& o, float probe, float* amax) -> int {
        Op t = o; t.os = probe;
        int r = run_op(u, pl, t, (char*)workspace, latents, latent_batch, deps, timestep, st);
        if (r) return r;
        SD_CHECK_HIP(hipMemsetAsync(dmax, 0, 4, st));
        const Tn& tn = pl.tensors[o.out];
        const long rows = o.kind == OP_GN ? (long)o.B * o.HW : (long)o.M;
        if ((r = sd_launch_amax_e4m3((char*)workspace + tn.off, rows * o.Cpad, dmax, st))) return r;
        unsigned code = 0;
        SD_CHECK_HIP(hipMemcpyAsync(&code, dmax, 4, hipMemcpyDeviceToHost, st));
        SD_CHECK_HIP(hipStreamSynchronize(st));
        *amax = code >= 0x7e ? -1.f : e4m3_code_value(code) / probe;       // -1: the probe itself saturated
        return 0;
    };
    for (size_t i = 0; i < pl.ops.size() && !rc; ++i) {
        Op o = pl.ops[i];
        if (o.dt) {                                    // consumer of an e4m3 tensor: the scale it was just written with
            auto it = cur.find(o.x1);
            if (it != cur.end()) o.xs = it->second;
        }
        if (o.out_fp8 && o.sname >= 0) {
            float amax = 0.f;
            rc = measure(o, 448.f / 4096.f, &amax);                        // |x| up to 4096, resolved down to ~0.15
            if (!rc && amax < 0.f) rc = measure(o, 448.f / 1048576.f, &amax);
            if (rc) break;
            if (amax < 0.f) amax = 1048576.f;
            float& seen = u->act_amax[o.sname];
            seen = std::max(seen, amax);
            // a power-of-two scale: the e4m3 grid is then an exact sub-grid of bf16 / fp32 values (reproducible emulation)
            const float want = 448.f / (margin * std::max(seen, 1e-6f));
            const float sc = ldexpf(1.f, (int)floorf(log2f(want)));
            u->act_scale[o.sname] = std::min(std::max(sc, ldexpf(1.f, -20)), ldexpf(1.f, 20));
            o.os = u->act_scale[o.sname];
            cur[o.out] = o.os;
        }
        rc = run_op(u, pl, o, (char*)workspace, latents, latent_batch, deps, timestep, st);
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(deps);
    if (rc) return rc;
    u->plans.clear();                                  // every plan variant is rebuilt with the calibrated scales
    return 0;
}

extern "C" int sd_unet_fp8_scale_count(const sd_unet* u) { return u ? (int)u->act_names.size() : -1; }

extern "C" int sd_unet_fp8_scale_info(const sd_unet* u, int index, char* name, int name_cap, float* scale, float* amax) {
    SD_REQUIRE(u && index >= 0 && index < (int)u->act_names.size(), "fp8_scale_info: bad index %d", index);
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", u->act_names[index].c_str());
    if (scale) *scale = u->act_scale[index];
    if (amax) *amax = u->act_amax[index];
    return 0;
}

extern "C" int sd_unet_set_fp8_scale(sd_unet* u, const char* name, float scale) {
    SD_REQUIRE(u && u->kind == 0 && u->fp8 && name, "set_fp8_scale: not an fp8 UNet handle");
    SD_REQUIRE(scale > 0.f && scale == scale, "set_fp8_scale: scale %g", scale);
    auto it = u->act_index.find(name);
    SD_REQUIRE(it != u->act_index.end(), "set_fp8_scale: no e4m3 activation tensor '%s' (build a plan first: sd_unet_workspace_bytes)", name);
    u->act_scale[it->second] = scale;
    u->plans.clear();
    return 0;
}

// algorithmic work of one op: flops for the contraction kernels, minimal HBM bytes for the rest
static void op_work(const Op& o, double* flops, double* bytes) {
    *flops = 0; *bytes = 0;
    switch (o.kind) {
        case OP_CONV3:
        case OP_GEMM: {
            const double K = o.Kalg ? o.Kalg : o.K, esz = o.dt ? 1.0 : 2.0;
            *flops = 2.0 * o.M * o.N * K;
            *bytes = esz * ((double)o.M * K + (double)o.N * K) + (o.out_fp8 ? 1.0 : 2.0) * (double)o.M * (o.epi == 1 ? o.N / 2 : o.N);
            break;
        }
        case OP_XATTN:   // to_q + Q K^T + P V + to_out of the block (to_k / to_v are hoisted out of the loop); X, R in, Y out
            *flops = 4.0 * o.M * (double)o.N * o.N + 4.0 * o.M * (double)o.sm_valid * o.N;
            *bytes = 3.0 * 2.0 * o.M * o.N;
            break;
        case OP_ATTN:
            *flops = 4.0 * o.B * o.heads * (double)o.Nq * o.Nk * o.D;
            *bytes = 2.0 * o.B * o.heads * o.D * (2.0 * o.Nq + 2.0 * o.Nk);
            break;
        case OP_GN:
            *bytes = 2.0 * 2.0 * o.B * (double)o.HW * (o.C1 + o.C2);   // read once + write once, bf16
            break;
        case OP_LN:
            *bytes = 2.0 * 2.0 * (double)o.M * o.N;
            break;
        case OP_REPLICATE:
            *bytes = 16.0 * o.M * (1.0 + o.N);
            break;
        case OP_TOME_MATCH: {     // src x dst cosine scores
            const double N = (double)o.Hin * o.Win;
            *flops = 2.0 * o.B * (0.75 * N) * (0.25 * N) * o.N;
            *bytes = 2.0 * o.B * N * o.N;
            break;
        }
        case OP_TOME_MERGE:
        case OP_TOME_UNMERGE:
            *bytes = 2.0 * o.B * (2.0 * o.Hin * o.Win - o.K) * (double)o.N;
            break;
        case OP_FREEU:      // hidden and skip in (the skip twice: the sums, then the apply pass), both out
            *flops = 2.0 * 14.0 * o.B * (double)o.Hin * o.Win * o.C2;
            *bytes = 2.0 * o.B * (double)o.Hin * o.Win * (2.0 * o.C1 + 3.0 * o.C2);
            break;
        case OP_SAG_MASS:       // Q K^T of every head, Q and K in, the masses out
            *flops = 2.0 * o.B * o.heads * (double)o.Nk * o.Nk * o.D;
            *bytes = 2.0 * 2.0 * o.B * (double)o.Nk * o.heads * o.D + 4.0 * o.B * o.Nk;
            break;
        case OP_PAG_IDENTITY:   // the perturbed rows in and out
            *bytes = 2.0 * 2.0 * (double)o.koff * o.N;
            break;
        case OP_HT_GATHER:
        case OP_HT_SCATTER:     // every row in, every row out
            *bytes = 2.0 * 2.0 * o.B * (double)o.Hin * o.Win * o.N;
            break;
        case OP_RES_ADD:    // x and r in, x out
            *bytes = 3.0 * 2.0 * (double)o.M;      // (M: the elements of all segments)
            break;
        case OP_TGATE_CAPTURE:      // y and res in, h2 and one cache row per `pair` rows out
            *bytes = 2.0 * (double)o.M * o.N * (3.0 + 1.0 / o.K);
            break;
        case OP_TGATE_APPLY:        // h1 and the cache in, h2 out
            *bytes = 3.0 * 2.0 * (double)o.M * o.N;
            break;
        case OP_IP_XATTN:   // scores and P B over the 32 image-key slots; R in, R' out
            *flops = 4.0 * o.M * 32.0 * o.N;
            *bytes = 2.0 * 2.0 * o.M * o.N;
            break;
        default:
            break;
    }
}

// One forward with ONE event between consecutive launches (op j's time = e[j+1] - e[j]): a pair per launch put two markers
// between any two kernels and over-read every launch by ~10 us against the rocprofv3 kernel trace of the same forward; one
// marker leaves ~4-5 us (the launch latency a free-running stream hides under the previous kernel).
static int profiled_run(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch, float timestep,
                        float* eps_out, void* workspace, long long workspace_bytes, int cache_mode, int cache_branch_id,
                        Plan** plan, std::vector<std::pair<int, float>>* per_op) {
    SD_REQUIRE(latents && eps_out && workspace, "forward_profiled: null argument");
    SD_REQUIRE(latent_batch > 0 && unet_batch % latent_batch == 0, "forward_profiled: bad batch");
    Plan* pl;
    if (forward_variant(u, "forward_profiled", latent_batch, unet_batch, cache_mode, cache_branch_id, u->cfg.sample_size, u->cfg.sample_size)) return -1;
    int rc = get_plan(u, u->last, &pl);
    if (rc) return rc;
    *plan = pl;
    if ((rc = ensure_tome_choice(u, pl->tome_choice_bytes, stream))) return rc;
    SD_REQUIRE((long long)pl->total_bytes <= workspace_bytes, "forward_profiled: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    std::vector<hipEvent_t> ev;
    std::vector<int> which;
    auto mark = [&]() -> int {
        hipEvent_t e;
        SD_CHECK_HIP(hipEventCreate(&e));
        SD_CHECK_HIP(hipEventRecord(e, st));
        ev.push_back(e);
        return 0;
    };
    if (mark()) return -2;
    for (size_t i = 0; i < pl->ops.size(); ++i) {
        if (cache_mode == SD_CACHE_SKIP && pl->skipped[i]) continue;
        rc = run_op(u, *pl, pl->ops[i], (char*)workspace, latents, latent_batch, eps_out, timestep, st);
        if (mark()) return -2;
        which.push_back((int)i);
        if (rc) break;
    }
    SD_CHECK_HIP(hipStreamSynchronize(st));
    if (u->tg_mode == TGATE_CAPTURE) u->tg_captured = rc == 0;
    for (size_t j = 0; j < which.size(); ++j) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[j], ev[j + 1]);
        per_op->push_back({which[j], ms});
    }
    for (auto e : ev) (void)hipEventDestroy(e);
    return rc;
}

extern "C" int sd_unet_forward_profiled(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                                        float timestep, float* eps_out, void* workspace, long long workspace_bytes,
                                        int cache_mode, int cache_branch_id, double kind_ms[SD_PROFILE_KINDS],
                                        long long kind_launches[SD_PROFILE_KINDS], double kind_flops[SD_PROFILE_KINDS],
                                        double kind_bytes[SD_PROFILE_KINDS]) {
    SD_REQUIRE(kind_ms && kind_launches && kind_flops && kind_bytes, "forward_profiled: null argument");
    Plan* pl = nullptr;
    std::vector<std::pair<int, float>> per_op;
    const int rc = profiled_run(u, stream, latents, latent_batch, unet_batch, timestep, eps_out, workspace, workspace_bytes,
                                cache_mode, cache_branch_id, &pl, &per_op);
    if (!pl) return rc;
    for (int k = 0; k < SD_PROFILE_KINDS; ++k) { kind_ms[k] = 0; kind_launches[k] = 0; kind_flops[k] = 0; kind_bytes[k] = 0; }
    for (auto& [i, ms] : per_op) {
        const Op& o = pl->ops[i];
        double fl, by;
        op_work(o, &fl, &by);
        // 4: the stride-1 convs on conv_halo_kernel's 9-tap mode (the roofline kernel); 21: the sub-pixel upsamplers that
        // sd_launch_conv3x3 puts on its 4-tap mode; 20: what runs on the implicit-GEMM kernel -- the stride-2 convs and the
        // sub-pixel upsamplers the 4-tap mode does not take (8x8 -> 16x16 at the bench batch).  The SAME predicate as the launch.
        bool halo4 = false;
        if (o.kind == OP_CONV3 && !o.dt && o.subpix) {
            GemmArgs a;
            a.M = o.M; a.N = o.N; a.K = o.K; a.K1 = o.K; a.Hin = o.Hin; a.Win = o.Win; a.Cin = o.Cin; a.Hout = o.Hout; a.Wout = o.Wout;
            a.stride = o.stride; a.up = 0; a.subpix = 1; a.splitk = o.splitk; a.slab = (float*)(o.aux >= 0 ? (void*)1 : nullptr);
            a.w_batch_stride = (long)o.N * 4 * o.Cin;
            halo4 = sd_conv_halo_subpix_applicable(a);
        }
        // (24 / 25 / 26: T-GATE's capture, apply and the capture plan's zero fill -- the op kinds of those numbers never run on a UNet)
        // (9 / 10: HyperTile's gather and scatter, likewise)
        // (11: PAG's identity self-attention, likewise)
        // (12: SAG's attention mass, likewise)
        const int kd = o.kind == OP_SAG_MASS ? 12 : o.kind == OP_PAG_IDENTITY ? 11 : o.kind == OP_HT_GATHER ? 9 : o.kind == OP_HT_SCATTER ? 10 : o.kind == OP_TGATE_CAPTURE ? 24 : o.kind == OP_TGATE_APPLY ? 25 : o.kind == OP_TGATE_ZERO ? 26 : o.kind == OP_XATTN ? 18 : o.kind == OP_REPLICATE ? 19 : o.kind == OP_IP_XATTN ? 22 : o.kind == OP_RES_ADD ? 23 : halo4 ? 21 :
                       (o.kind == OP_CONV3 && !o.dt && (o.subpix || o.stride != 1)) ? 20 :
                       (o.dt ? (o.kind == OP_CONV3 ? 16 : 17) : o.kind);
        kind_ms[kd] += ms; kind_launches[kd] += 1; kind_flops[kd] += fl; kind_bytes[kd] += by;
    }
    return rc;
}

// The same measurement, one text line per launch: "index kind M N K ms GFLOP MB" (development: which shapes carry a group's
// time).  Returns the number of bytes written (without the terminator), < 0 on error.
extern "C" long long sd_unet_forward_op_times(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                                              float timestep, float* eps_out, void* workspace, long long workspace_bytes,
                                              int cache_mode, int cache_branch_id, char* text, long long cap) {
    SD_REQUIRE(text && cap > 0, "forward_op_times: null argument");
    Plan* pl = nullptr;
    std::vector<std::pair<int, float>> per_op;
    const int rc = profiled_run(u, stream, latents, latent_batch, unet_batch, timestep, eps_out, workspace, workspace_bytes,
                                cache_mode, cache_branch_id, &pl, &per_op);
    if (rc) return rc;
    long long n = 0;
    for (auto& [i, ms] : per_op) {
        const Op& o = pl->ops[i];
        double fl, by;
        op_work(o, &fl, &by);
        // (a GroupNorm that finishes its producer's deferred split-K reduce reports the split factor in the K column)
        const int w = snprintf(text + n, (size_t)(cap - n), "%d %d %d %d %d %.5f %.3f %.3f\n", i, (int)o.kind, o.M, o.N,
                               o.kind == OP_GN ? o.slab_k : o.K, ms, fl * 1e-9, by * 1e-6);
        if (w < 0 || n + w >= cap) break;
        n += w;
    }
    return n;
}

extern "C" int sd_unet_debug_tensor(sd_unet* u, void* stream, const char* name, float* host_out, long long numel,
                                    void* workspace, int unet_batch, int cache_branch_id) {
    SD_REQUIRE(u && u->debug_taps, "debug_tensor: create the handle with SD_DEBUG_TAPS=1 in the environment");
    if (u->kind == 5 && name && !strcmp(name, "cond_embedding")) {      // the stored conditioning embedding [cn_b][h w][c0]
        SD_REQUIRE(u->cn_b > 0, "debug_tensor: no conditioning image is set");
        const size_t have = (size_t)u->cn_b * u->cn_h * u->cn_w * u->cfg.block_out_channels[0];
        SD_REQUIRE(numel >= 0 && (size_t)numel <= have, "debug_tensor: 'cond_embedding' holds %zu elements", have);
        std::vector<unsigned short> tmp(numel);
        SD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        SD_CHECK_HIP(hipMemcpy(tmp.data(), u->cn_embed, (size_t)numel * 2, hipMemcpyDeviceToHost));
        for (long long i = 0; i < numel; ++i) {
            unsigned v = (unsigned)tmp[i] << 16;
            memcpy(&host_out[i], &v, 4);
        }
        return 0;
    }
    Plan* pl;
    int rc = get_plan(u, last_variant(u, unet_batch, cache_branch_id), &pl);
    if (rc) return rc;
    auto it = pl->taps.find(name);
    SD_REQUIRE(it != pl->taps.end(), "debug_tensor: unknown tap '%s'", name);
    const Tn& t = pl->tensors[it->second];
    SD_REQUIRE((size_t)numel * 2 <= t.bytes, "debug_tensor: '%s' holds at most %zu elements", name, t.bytes / 2);
    std::vector<unsigned short> tmp(numel);
    SD_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    SD_CHECK_HIP(hipMemcpy(tmp.data(), (char*)workspace + t.off, (size_t)numel * 2, hipMemcpyDeviceToHost));
    for (long long i = 0; i < numel; ++i) {
        unsigned v = (unsigned)tmp[i] << 16;
        memcpy(&host_out[i], &v, 4);
    }
    return 0;
}

extern "C" int sd_inpaint_prepare(void* stream, const float* image, const float* mask, float* masked_image, float* latent_mask,
                                  int batch, int height, int width) {
    return sd_launch_inpaint_prepare(image, mask, masked_image, latent_mask, batch, height, width, (hipStream_t)stream);
}
