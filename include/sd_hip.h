/* libsdhip -- C ABI of the MI355X-native (gfx950) Stable Diffusion sampling hot path.
 *
 * The reference (Kotstantinovskiy/SonicDiffusionBayesLab) is pure Python over diffusers and has
 * no FFI of its own; each entry point below names the reference call site it replaces.  The
 * reference-side binding a maintainer would add (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: pointers and sizes only, no torch / C++ types.
 *   - every function returns 0 on success, a negative code on failure; the message is available
 *     through sd_last_error() (thread-local).  No exception crosses the ABI.
 *   - `stream` is a hipStream_t passed as void*; work is only ever enqueued on that stream and
 *     the library never synchronises the device inside a forward/step call.
 *   - device buffers handed in are BORROWED for the duration of the call; the caller (PyTorch in
 *     this repo) owns all I/O tensors and the workspace.  UNet weights are owned by the handle.
 *   - activations are bf16 NHWC inside the library; latents / noise predictions cross the ABI as
 *     fp32 NCHW, exactly the tensors the reference loop holds (src/models.py:173-182,227-261).
 */
#ifndef SD_HIP_H
#define SD_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sd_unet sd_unet;

/* diffusers UNet2DConditionModel config subset used by SD-1.5 */
typedef struct sd_unet_config {
    int sample_size;             /* default latent H = W (64 for 512x512); the _hw entry points take other sizes */
    int in_channels;             /* 4 */
    int out_channels;            /* 4 */
    int num_levels;              /* 4 */
    int block_out_channels[8];   /* 320,640,1280,1280 */
    int layers_per_block;        /* 2 */
    int attn_levels[8];          /* 1,1,1,0 : level carries Transformer2DModel blocks */
    int cross_attention_dim;     /* 768 */
    int num_heads;               /* 8 (diffusers attention_head_dim=8 is used as head COUNT); see num_heads_per_level */
    int norm_num_groups;         /* 32 */
    float norm_eps;              /* 1e-5 */
    int context_len;             /* 77 */
    /* Weight / operand type of the MFMA contractions (BASELINE configs[4]: "fp8 MFMA weights"):
     *   SD_DTYPE_BF16     - bf16 operands everywhere (v_mfma_f32_16x16x32_bf16);
     *   SD_DTYPE_FP8_E4M3 - OCP e4m3 weights with one fp32 scale per output channel, and e4m3 activations with a
     *                       static per-tensor scale written by the producing GroupNorm / LayerNorm / GEGLU epilogue,
     *                       for the 3x3 resnet convs, proj_in, the self-attention QKV projection and both
     *                       feed-forward GEMMs (v_mfma_f32_16x16x128_f8f6f4, fp32 accumulate, dequantised in the
     *                       epilogue).  Attention, the prompt cross-attention, to_out / proj_out / shortcut GEMMs,
     *                       the down/upsampler convs and conv_in / conv_out stay bf16.
     * fp8_act_scale_*: DEFAULT activation scales x_fp8 = sat(x * scale) (0 = 8 and 2) of tensors that
     * sd_unet_calibrate_fp8 / sd_unet_set_fp8_scale have not given a scale of their own. */
    int weight_dtype;
    float fp8_act_scale_norm;    /* GroupNorm(+SiLU) / LayerNorm outputs */
    float fp8_act_scale_ff;      /* GEGLU outputs (input of ff.net.2) */
    /* LCM-distilled UNets (diffusers time_cond_proj_dim; 0 = none, SD-1.5): the time embedding carries
     * time_embedding.cond_proj.weight [block_out_channels[0], time_cond_proj_dim] and adds cond_proj(cond) to the timestep
     * sinusoid before linear_1 (sd_unet_set_timestep_cond).  A multiple of 8.  VAE and CLIP handles ignore it.
     * (Appended under ABI 3: zero-initialise the struct.) */
    int time_cond_proj_dim;
    /* IP-Adapter image prompts (diffusers IPAdapterAttnProcessor2_0 + ImageProjection, the plain ip-adapter_sd15 family; both
     * 0 = none).  ip_adapter_tokens: image tokens per sample (4 is built); ip_adapter_embed_dim: width E of image_embeds (1024
     * for the published adapter; a multiple of 64).  With them set the handle additionally takes
     *   encoder_hid_proj.image_projection_layers.0.image_embeds.{weight [tokens * cross_attention_dim, E], bias},
     *   encoder_hid_proj.image_projection_layers.0.norm.{weight, bias} [cross_attention_dim], and per attn2 layer
     *   <block>.attn2.processor.to_k_ip.0.weight / to_v_ip.0.weight [C, cross_attention_dim]
     * and sd_unet_set_ip_adapter_hw conditions its forwards.  Every level's head count must be 1, 2, 4 or 8.  (Appended under
     * ABI 3.) */
    int ip_adapter_tokens;
    int ip_adapter_embed_dim;
    /* Head COUNT of the transformer blocks per resolution level (Stable Diffusion 2.x: 5, 10, 20, 20 = head dim 64 at every
     * level; diffusers' attention_head_dim list).  All zeros = num_heads at every level (SD-1.5).  Otherwise every one of the
     * num_levels entries is positive; the mid block uses the last level's count and the up blocks mirror the down blocks.
     * Channels / heads of an attention level must be 40, 64, 80 or 160.  An IP-Adapter needs 1, 2, 4 or 8 heads at every
     * level.  (Appended under ABI 3: zero-initialise the struct.) */
    int num_heads_per_level[8];
} sd_unet_config;
enum { SD_DTYPE_BF16 = 0, SD_DTYPE_FP8_E4M3 = 1 };

const char* sd_last_error(void);
int sd_abi_version(void);

/* ---- UNet handle: replaces `self.unet` of StableDiffusionPipeline (src/models.py:227-235) ---- */
int sd_unet_create(const sd_unet_config* cfg, sd_unet** out);
void sd_unet_destroy(sd_unet* u);

/* Parameters use the diffusers state_dict names and layouts (conv OIHW, linear [out,in]), fp32 on
 * the HOST; the library repacks (OHWI bf16, fused QKV, GEGLU interleave ...) and uploads them in
 * sd_unet_finalize().  Replaces `from_pretrained(...).to(device)` for the UNet
 * (src/experiments/base_experiment.py:55-64). */
int sd_unet_num_params(const sd_unet* u);
int sd_unet_param_info(const sd_unet* u, int index, char* name, int name_cap, long long shape[4], int* ndim);
int sd_unet_load_param(sd_unet* u, const char* name, const float* host_data, long long numel);
int sd_unet_finalize(sd_unet* u);

/* Parity hook for the HOST side of sd_unet_finalize (weight repacking / fp8 quantisation): finalize packs into a host
 * staging blob first and uploads second, so on a box without a GPU it fails at the upload with the blob intact; this
 * copies `nbytes` of the packed item `key` (a diffusers parameter name; fp8 items: name + ".fp8" / ".scale") out of
 * it.  Returns the item's byte offset, < 0 on error (unknown key, blob already released after a successful upload). */
long long sd_unet_debug_packed(const sd_unet* u, const char* key, void* host_out, long long nbytes);

/* ---- fp8 activation scales (SD_DTYPE_FP8_E4M3 handles; no reference counterpart: the reference runs fp16,
 * configs/consistency_model_config.yaml:1-34).  Every e4m3 ACTIVATION tensor of the plan is named after the module that
 * writes it -- "<resnet>.norm1|norm2", "<Transformer2DModel>.norm", "<block>.norm1|norm3", "<block>.ff.net.0" (the GEGLU
 * product) -- and carries one per-tensor scale, x_fp8 = sat(x * scale); e4m3 is a floating-point format, so the scale only
 * positions the +-448 .. 2^-9 range over the tensor's values.
 *   sd_unet_calibrate_fp8: ONE forward on the caller's inputs (sd_unet_set_context first, as for sd_unet_forward); every
 *     producer of an e4m3 tensor is first run with a probe scale under which nothing saturates, the tensor's largest
 *     |value| is read back, and its scale becomes the largest power of two <= 448 / (margin * amax) -- amax is the
 *     maximum over all calibration calls so far (call it for a few timesteps).  Synchronises the stream ~125 times; all
 *     plans are rebuilt afterwards (same workspace layout).  margin in [1, 64].
 *   sd_unet_fp8_scale_count / _info: the named tensors known so far (names appear when a plan is built), their scale and
 *     observed amax (0 = never calibrated);  sd_unet_set_fp8_scale: restore a saved calibration. */
int sd_unet_calibrate_fp8(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch, float timestep,
                          float margin, void* workspace, long long workspace_bytes);
int sd_unet_fp8_scale_count(const sd_unet* u);
int sd_unet_fp8_scale_info(const sd_unet* u, int index, char* name, int name_cap, float* scale, float* amax);
int sd_unet_set_fp8_scale(sd_unet* u, const char* name, float scale);

/* Workspace the caller must provide for a given UNet batch (2*B with CFG).  `cache_branch_id`
 * < 0 disables the DeepCache plan; >= 0 reserves the cached tensors of that branch
 * (DeepCacheSDHelper.set_params, src/experiments/deep_cache.py:25-28). The SAME workspace must be
 * passed to set_context and to every forward of one sampling run. */
long long sd_unet_workspace_bytes(sd_unet* u, int unet_batch, int cache_branch_id);

/* Latent height / width per call (additions to ABI 3).  Each entry point without the suffix is its _hw form at
 * (sample_size, sample_size).  A UNet handle takes sides that are multiples of 2^(num_levels - 1) (8 for SD-1.5) up to
 * 256; a VAE handle (sd_vae_decode_hw; size its workspace with sd_unet_workspace_bytes_hw, cache_branch_id = -1) takes
 * sides that are multiples of 8 in [8, 128].  A handle keeps one plan per (batch, branch, variant, latent_h, latent_w):
 * sizes may alternate on one handle, and a workspace sized for one size serves another only if it is large enough.
 * set_context prepares the forwards of ONE latent size: call it again (same workspace) after changing the size. */
long long sd_unet_workspace_bytes_hw(sd_unet* u, int unet_batch, int cache_branch_id, int latent_h, int latent_w);

/* Prompt conditioning: device fp32 [unet_batch, context_len, cross_attention_dim]
 * (`prompt_embeds` after the CFG concat, src/models.py:154-155).  Projects K/V of all
 * cross-attention layers once -- they are step-invariant. */
int sd_unet_set_context(sd_unet* u, void* stream, const float* encoder_hidden_states, int unet_batch,
                        int cache_branch_id, void* workspace, long long workspace_bytes);
int sd_unet_set_context_hw(sd_unet* u, void* stream, const float* encoder_hidden_states, int unet_batch,
                           int cache_branch_id, int latent_h, int latent_w, void* workspace, long long workspace_bytes);

/* Timestep condition of an LCM-distilled UNet (time_cond_proj_dim > 0; src/models.py:195-202,231 of the reference pass
 * timestep_cond = get_guidance_scale_embedding(guidance_scale - 1)).  `cond`: device fp32 [time_cond_proj_dim], 16-byte
 * aligned.  One GEMV on `stream` stores row = cond_proj.weight . cond ([block_out_channels[0]] fp32, fp32 accumulation) in
 * the handle; every later forward of the handle (any batch, size or DeepCache branch) adds the row to its timestep sinusoid
 * -- the same launches as without it.  One condition per forward, as there is one timestep per forward.  cond = NULL clears
 * it: forwards are then those of a UNet without cond_proj (what diffusers does for timestep_cond=None).  Issue it on the
 * stream of the forwards that should see it (or order the streams). */
int sd_unet_set_timestep_cond(sd_unet* u, void* stream, const float* cond);

/* Condition of an inpainting UNet (in_channels = 9: conv_in reads [latents 4 | mask 1 | masked-image latents 4], diffusers'
 * StableDiffusionInpaintPipeline).  `mask` [batch,1,latent_h,latent_w] (fp32 0 / 1; 1 = repaint) and `masked_latents`
 * [batch,4,latent_h,latent_w] (the scaled encoding of the image with the repainted region blanked), both device fp32 and
 * 16-byte aligned, are packed into the handle ONCE per call (one launch on `stream`), the way sd_unet_set_context_hw stores the
 * prompt.  Every later forward at that latent size reads channels 0..3 from its latents and channels 4..8 from the stored
 * condition, each with the batch index taken modulo its source batch (CFG duplication stays fused; unet_batch must be a
 * multiple of `batch`): no concatenated tensor is built per forward, and the launch count of a forward is unchanged.  A forward
 * on a 9-channel handle with no condition set, or at another size or batch, fails and says so.  A 4-channel handle refuses the
 * call.  The operands may be freed once the stream has run the launch.  mask = masked_latents = NULL clears the condition
 * (nothing is launched; batch and size are ignored): forwards fail again until one is set. */
int sd_unet_set_inpaint_cond_hw(sd_unet* u, void* stream, const float* mask, const float* masked_latents, int batch,
                                int latent_h, int latent_w);

/* Image prompt of a handle with an IP-Adapter (ip_adapter_tokens > 0): decoupled cross-attention, per attn2 layer
 *   attn = softmax_77(q k^T / sqrt d) v + scale * softmax_T(q K_ip^T / sqrt d) V_ip,   h = h + to_out(attn).
 * Call it AFTER sd_unet_set_context_hw with the same batch, branch, size and workspace.  `image_embeds`: device fp32
 * [unet_batch, ip_adapter_embed_dim], 16-byte aligned, the CFG halves already concatenated (negative first; diffusers uses
 * zeros there).  It runs the token projection + LayerNorm, to_k_ip | to_v_ip of every layer and folds, per sample and head,
 *   A = (K_ip / sqrt d) W_q   and   B = scale * V_ip W_o^T
 * into context tensors of the workspace; `scale` lives in B, so changing it means calling again.  From then on every forward
 * of the handle runs the "IP on" plan variant: one extra launch per transformer block (profile kind 22) writes
 * R' = h + sum_heads softmax_T(LN(h) A^T) B, which the block's prompt cross-attention takes as its residual.  While any
 * (batch, branch, size) of the handle has an image prompt set, a forward for which it has NOT been set fails and says so.
 * image_embeds = NULL clears the prompt of that (batch, branch, size) (nothing is launched; workspace may be NULL): once none
 * is left the handle runs the plans of a handle without an adapter, bit for bit.  sd_unet_workspace_bytes_hw of such a handle
 * covers both variants.  sd_unet_calibrate_fp8 always runs without the image prompt and CLEARS every image prompt of the
 * handle (its plan uses the workspace where the folded operands lie): call this again after calibrating. */
int sd_unet_set_ip_adapter_hw(sd_unet* u, void* stream, const float* image_embeds, int unet_batch, int cache_branch_id,
                              int latent_h, int latent_w, float scale, void* workspace, long long workspace_bytes);

/* ---- ControlNet (diffusers ControlNetModel, guess_mode = False).  Additions under ABI 3: resolve by name. ----
 * The handle is again an `sd_unet` (its own kind): cfg as for the UNet it is paired with (in_channels = 4, bf16 only: fp8 is
 * refused by name; no IP-Adapter fields); cond_embed_channels: diffusers' conditioning_embedding_out_channels, the four
 * widths of ControlNetConditioningEmbedding's conv chain (16, 32, 96, 256 for the published SD-1.5 ControlNets; multiples
 * of 8).  Parameters under diffusers' names -- time_embedding.*,
 * conv_in.*, down_blocks.*, mid_block.* as in the UNet, controlnet_cond_embedding.{conv_in, blocks.0..5, conv_out}.{weight,
 * bias}, controlnet_down_blocks.N.{weight [C, C, 1, 1], bias}, controlnet_mid_block.{weight, bias} -- are enumerated / loaded /
 * finalised through the sd_unet_* calls; sd_unet_workspace_bytes_hw sizes its workspace (cache_branch_id = -1),
 * sd_unet_set_context_hw stores its prompt and sd_unet_set_timestep_cond its LCM condition.
 *
 * Residual buffer (caller-owned, 256-byte aligned, sd_controlnet_residual_bytes_hw bytes; the same function serves a UNet
 * handle of the same widths): bf16, channel-last, one segment [unet_batch][h_i * w_i][C_i] per residual in diffusers' order --
 * conv_in's output, then per level its layers_per_block block outputs followed by its downsampler's output (none at the last
 * level), then the mid block: 12 + 1 segments for SD-1.5, with (C, side divisor) = (c0, 1) x 3, (c0, 2), (c1, 2) x 2,
 * (c1, 4), (c2, 4) x 2, (c2, 8), (c3, 8) x 2 and the mid (c3, 8).  Segment i starts where segment i - 1 ends, rounded up to
 * 256 bytes.  The residuals are stored UNSCALED: conditioning_scale is applied where they are consumed. */
int sd_controlnet_create(const sd_unet_config* cfg, const int cond_embed_channels[4], sd_unet** out);
long long sd_controlnet_residual_bytes_hw(const sd_unet* u, int unet_batch, int latent_h, int latent_w);
/* The step-invariant conditioning embedding, once per call: cond_image = device fp32 [batch, 3, 8 latent_h, 8 latent_w] in
 * [0, 1] (rgb, not normalised), 16-byte aligned.  Eight convs (3x3, pad 1; SiLU after all but the last; stride 2 on blocks
 * 1, 3, 5) on the general implicit-GEMM conv kernel leave [batch][latent_h * latent_w][block_out_channels[0]] bf16 on the
 * handle; every later forward at that latent size adds it inside conv_in, reading sample b's row from b % batch (unet_batch
 * must be a multiple of batch).  Scratch is owned by the handle.  cond_image = NULL clears it. */
int sd_controlnet_set_cond_hw(sd_unet* u, void* stream, const float* cond_image, int batch, int latent_h, int latent_w);
/* residuals = ControlNet(latents, t, prompt, cond): the UNet's time embedding, conv_in (+ the stored embedding, in the same
 * launch), down path and mid block, then one 1x1 GEMM per residual into `residuals` (layout above).  latents / latent_batch /
 * unet_batch as for sd_unet_forward_hw (a CFG pair runs its prompt-independent prefix once). */
int sd_controlnet_forward_hw(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch, int latent_h,
                             int latent_w, float timestep, void* residuals, void* workspace, long long workspace_bytes);
/* UNet side: while residuals are set, every forward of the handle runs the "control" plan variant -- today's ops, then after
 * the mid block ONE launch (profile kind 23) that does x <- bf16(float(x) + scale * float(r)) in place on the twelve skip
 * tensors and the mid output (every reader of the unmodified tensors has run by then), and up-block GroupNorms that compute
 * their own statistics where the plain plan took them from the producer of a tensor this variant modifies.  `residuals`: a
 * buffer in the layout above for (unet_batch, latent_h, latent_w), borrowed until cleared or replaced; a forward at another
 * batch or size, or with a DeepCache mode, fails and says so.  residuals = NULL clears: the handle runs the plain plans again,
 * bit for bit.  fp8 handles refuse.  A handle builds and sizes the control variants only from its first call of this function on:
 * sd_unet_workspace_bytes_hw covers them from then on, so query it again after the first call (the context tensors keep their
 * offsets, so a larger workspace may be filled by copying the old one); a forward whose workspace is too small fails and says so. */
int sd_unet_set_control_residuals_hw(sd_unet* u, const void* residuals, float scale, int unet_batch, int latent_h, int latent_w);

/* Token Merging around the self-attention of the transformer blocks whose level is at most max_downsample (1 or 2) times
 * coarser than the latent: each merges r = min(num_src, int(tokens * ratio)) src tokens (0 < ratio <= 0.75).  The setting is
 * part of the plan key; ratio 0 = off = the plans, workspace sizes and results of a handle that never saw it.  After a change
 * call sd_unet_workspace_bytes_hw and sd_unet_set_context_hw again.  bf16 UNet handles only.
 * set_tome_choice: the dst choice (one byte 0..3 per 2x2 cell) of all merging blocks at this latent size, concatenated in plan
 * order (block_info: each block's token grid, r and offset), copied asynchronously on the stream from host or device memory;
 * shared by all samples; zero until set.
 * tome_matching: reads back what the last forward matched in one block (synchronises the stream): kept [B][num_src - r],
 * merged [B][r], dst_idx [B][r], tok [h w] into host buffers (any may be NULL), *batch = B (half the UNet batch for the first
 * block of a classifier-free-guidance pair, which runs once per latent). */
int sd_unet_set_tome(sd_unet* u, double ratio, int max_downsample);
int sd_unet_tome_block_count_hw(sd_unet* u, int latent_h, int latent_w);
int sd_unet_tome_block_info_hw(sd_unet* u, int block, int latent_h, int latent_w, int* h, int* w, int* r, long long* choice_off);
int sd_unet_set_tome_choice_hw(sd_unet* u, void* stream, const unsigned char* choice, long long n, int latent_h, int latent_w);
int sd_unet_tome_matching_hw(sd_unet* u, void* stream, int block, int unet_batch, int cache_branch_id, void* workspace, int* kept,
                             int* merged, int* dst_idx, int* tok, int* r, int* batch);

/* FreeU (Si et al.; diffusers enable_freeu(s1, s2, b1, b2)): while set, every forward of the handle runs the "freeu" plan variant --
 * in up blocks 0 and 1, in front of each of the three resnets, ONE launch (profile kind 31; csrc/freeu.hip) writes new tensors
 * hidden' = hidden with its first half of the channels times b and skip' = fourier_filter(skip, threshold 1, scale s), and the
 * resnet reads [hidden' | skip']; (b, s) = (b1, s1) in block 0 and (b2, s2) in block 1.  The GroupNorms of those resnets compute
 * their own statistics.  The four factors live on the handle and are read at launch: changing them builds no plan; switching
 * FreeU on or off selects other plans, so call sd_unet_workspace_bytes_hw and sd_unet_set_context_hw again.  On a DeepCache skip
 * step whose branch reaches into those blocks the op runs on the cached feature each time it is consumed; the cached feature
 * itself stays raw.  With ControlNet residuals the filter sees the skips after the residual add.  All four factors must be
 * finite and > 0 (diffusers switches FreeU off silently when one is 0; here that is an error).  fp8 handles refuse: their
 * calibrated activation scales do not describe the scaled tensors.  disable_freeu: the plans, workspace sizes and results of a
 * handle that never saw it, bit for bit. */
int sd_unet_set_freeu(sd_unet* u, float s1, float s2, float b1, float b2);
int sd_unet_disable_freeu(sd_unet* u);
/* T-GATE (Zhang et al. 2024): temporal gating of the prompt cross-attention.  The handle has three states.
 * mode 1, capture: forwards run today's plan for their batch with every cross-attention form computed WITHOUT its residual
 * operand (the one-launch fused form reads a zeroed residual tensor) and one launch behind it (profile kind 24; csrc/tgate.hip)
 * that writes h2 = h1 + y and the block's slice of `cache`: y itself when the UNet batch equals latent_batch, the mean of the
 * [uncond | cond] pair's two rows (summed in fp32, stored as bf16) when it is twice that.  mode 2, reuse: forwards run at UNet
 * batch = latent_batch on plans without norm2, attn2 and any context tensor -- sd_unet_set_context_hw is not needed and is
 * refused -- where one launch per block (profile kind 25) writes h2 = h1 + slice.  Both launches deliver the row partials that
 * keep norm3 folded into the GEGLU projection.  mode 0 with cache = NULL clears: the plans, workspace sizes and results of a
 * handle that never saw it, bit for bit.
 * `cache` is the CALLER's device buffer (256-byte aligned, at least sd_unet_tgate_bytes_hw bytes), borrowed until the next call:
 * one [latent_batch * tokens][C] bf16 slice per transformer block in plan order (down, mid, up; sd_unet_tgate_block_info_hw:
 * offset, rows and channels of one block, returns the block count, also for block < 0).  The capture and the reuse plans are
 * other plans than the plain ones: call sd_unet_workspace_bytes_hw for each mode and batch that will run.  Reuse before a capture
 * into the same buffer for the same latent batch and size fails and says so, at this call and at the forward.  Refused by name:
 * fp8 handles, 9-channel inpainting UNets, UNets with an IP-Adapter, ControlNet residuals, DeepCache (its cached features are
 * stored at the CFG batch). */
long long sd_unet_tgate_bytes_hw(sd_unet* u, int latent_batch, int latent_h, int latent_w);
int sd_unet_tgate_block_info_hw(sd_unet* u, int block, int latent_batch, int latent_h, int latent_w, long long* offset, long long* rows,
                                int* channels);
int sd_unet_set_tgate_hw(sd_unet* u, int mode, void* cache, long long bytes, int latent_batch, int latent_h, int latent_w);
/* How many execution plans the handle has built so far (one per batch, DeepCache branch, latent size and variant); < 0 on a
 * null handle.  For tests of "this setting builds no new plan". */
int sd_unet_plan_count(const sd_unet* u);
/* The options of a UNet and the pairs of them that are not built together: ONE table behind every setter, the forward and
 * the workspace sizing, which all refuse a pair by the names of both.  sd_unet_option_name: the name of option i (0 .. count - 1),
 * NULL past the end.  sd_unet_option_conflict: why options a and b are refused together, NULL when the pair is built (symmetric
 * in a, b).  The Python layers hold the same rows (options.py); a test compares the two. */
const char* sd_unet_option_name(int i);
const char* sd_unet_option_conflict(int a, int b);

/* HyperTile (tfernd/HyperTile, swap_size = 1): tiled self-attention.  tile_tokens = the tile side T in tokens (tile_size / 8), 8 or
 * more; max_depth 0..3; tile_tokens 0 = off = the plans, workspace sizes and results of a handle that never saw it.  A transformer
 * block on rh x rw tokens at depth d = log2(latent_h / rh) <= max_depth is cut into nh x nw tiles of th x tw tokens, th = the smallest
 * divisor of rh that is >= min(T, rh) (tw likewise); it is tiled when nh nw > 1.  A tiled block gathers its input into tile order
 * (profile kind 9), runs WHOLE in that order with every fold of the plain plan -- only attn1 changes, to batch * nh nw samples of
 * th tw keys -- and scatters the exit GEMM's output back (kind 10).  The setting is part of the plan key; after a change call
 * sd_unet_workspace_bytes_hw and sd_unet_set_context_hw again.  bf16 UNet handles only, not together with Token Merging.
 * block_count / block_info: the tiled blocks at a latent size in plan order (down, mid, up) with their token grid and tile counts.
 * They report the FULL plan: which blocks tile depends on the latent size and the setting alone, and a DeepCache skip step runs
 * the subset of these blocks its branch keeps, tiled the same way (there is no per-branch view). */
int sd_unet_set_hypertile(sd_unet* u, int tile_tokens, int max_depth);
int sd_unet_hypertile_block_count_hw(sd_unet* u, int latent_h, int latent_w);
int sd_unet_hypertile_block_info_hw(sd_unet* u, int block, int latent_h, int latent_w, int* rh, int* rw, int* nh, int* nw);

/* Perturbed-attention guidance (Ahn et al. 2024; diffusers' PAGMixin).  layer_mask: bit i = transformer block i in
 * plan order (down, mid, up -- the order of the T-GATE cache slices; sd_unet_pag_block_count of them) is perturbed; 0 = off = the
 * plans, workspace sizes and results of a handle that never saw it.  With a mask set, a forward runs a UNet batch of 3 or 2 times
 * the latent batch -- [uncond | cond | perturbed] or [cond | perturbed] over the SAME latents -- and in a perturbed block attn1 of
 * the LAST latent_batch samples is to_out(to_v(norm1(h))): the attention kernel runs on the other samples and one identity launch
 * (profile kind 11) fills the perturbed rows of its output, so to_out stays one GEMM.  The prompt-independent prefix ends at the
 * entry of the first transformer block when that block is perturbed, else where the plain plan ends it.  The mask is part of the
 * plan key; after a change call sd_unet_workspace_bytes_hw and sd_unet_set_context_hw again.  bf16 4-channel UNet handles without
 * an IP-Adapter only; a forward with Token Merging, T-GATE, DeepCache or ControlNet residuals is refused by name. */
int sd_unet_set_pag(sd_unet* u, long long layer_mask);
int sd_unet_pag_block_count(const sd_unet* u);

/* Self-attention guidance (Hong et al. 2023; diffusers' StableDiffusionSAGPipeline): capture of the attention mass.
 * on != 0: the mid block's transformer block runs one more launch behind its q | k | v projection, which writes
 *   mass[b][k] = (1 / heads) * sum_h sum_q softmax_k(Q_h K_h^T / sqrt(d))[q][k]     fp32 [unet_batch][mh * mw], mh x mw the mid grid
 * of attn1 for every sample of the forward into the buffer sd_unet_set_sag_buffer names (the caller owns it; at least
 * unet_batch * mh * mw floats, else the forward refuses; it must stay valid until the forward has run).  Nothing else in the plan
 * changes: the forward's output is the output without capture bit for bit.  Capture is part of the plan key; off = the plans,
 * workspace sizes and results of a handle that never saw it.  bf16 4-channel UNet handles without an IP-Adapter whose mid grid has
 * 4 .. 16 tokens per side and head dim 64, 80 or 160; refused by name: PAG, Token Merging, T-GATE, DeepCache, ControlNet
 * residuals, an IP-Adapter image prompt, fp8, and HyperTile settings that tile the mid block. */
int sd_unet_set_sag(sd_unet* u, int on);
int sd_unet_set_sag_buffer(sd_unet* u, float* mass, long long floats);

enum { SD_CACHE_OFF = 0, SD_CACHE_FULL_AND_STORE = 1, SD_CACHE_SKIP = 2 };

/* eps = UNet(latent_model_input, t, encoder_hidden_states)  (src/models.py:217-235).
 * `latents` is fp32 NCHW [latent_batch,4,H,W]; with unet_batch = 2*latent_batch the CFG
 * duplication `torch.cat([latents]*2)` (src/models.py:217) is fused: the two halves of the batch then see the same latents
 * and timestep, so everything before the first prompt cross-attention (conv_in, down_blocks.0.resnets.0,
 * attentions.0 up to attn1.to_out) is computed once per latent and copied to both halves -- the results are those of
 * the duplicated batch (SD_CFG_DEDUP=0 in the environment computes the prefix twice instead).
 * `eps_out` is fp32 NCHW [unet_batch,4,H,W].  cache_mode selects the DeepCache plan
 * (full step that refreshes the cache / skip step that reuses it). */
int sd_unet_forward(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                    float timestep, float* eps_out, void* workspace, long long workspace_bytes, int cache_mode,
                    int cache_branch_id);
/* The same at latent [latent_batch, 4, latent_h, latent_w] (eps_out [unet_batch, 4, latent_h, latent_w]). */
int sd_unet_forward_hw(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch, int latent_h,
                       int latent_w, float timestep, float* eps_out, void* workspace, long long workspace_bytes,
                       int cache_mode, int cache_branch_id);

/* ---- AutoencoderKL decoder: replaces `self.vae.decode(latents / scaling_factor)`
 * (src/models.py:287-302).  `sd_vae` IS the `sd_unet` handle type: parameters are enumerated / loaded /
 * finalised and the workspace is sized through the sd_unet_* functions above (diffusers AutoencoderKL
 * names: post_quant_conv.*, decoder.*); cfg: sample_size = latent size, block_out_channels =
 * 128,256,512,512, layers_per_block = 2, in_channels = 4, out_channels = 3, norm_num_groups = 32.
 * decode: fp32 NCHW latents [batch,4,h,w] * latent_scale -> fp32 NCHW images [batch,3,8h,8w]. */
typedef struct sd_unet sd_vae;
int sd_vae_create(const sd_unet_config* cfg, sd_vae** out);
int sd_vae_decode(sd_vae* v, void* stream, const float* latents, int batch, float latent_scale, float* images_out,
                  void* workspace, long long workspace_bytes);
/* latents [batch, 4, latent_h, latent_w] -> images [batch, 3, 8 latent_h, 8 latent_w].  Beyond 4096 latent pixels the
 * mid-block attention runs its query rows in chunks of 2048 with a long-row softmax (scores stay <= 64 MiB). */
int sd_vae_decode_hw(sd_vae* v, void* stream, const float* latents, int batch, int latent_h, int latent_w, float latent_scale,
                     float* images_out, void* workspace, long long workspace_bytes);

/* ---- AutoencoderKL encoder: `vae.encode(image)` of diffusers 0.32.1 (AutoencoderKL.encode, as
 * StableDiffusionImg2ImgPipeline.prepare_latents calls it; upstream-recall).  Additions under ABI 3: resolve them by name.
 * The handle is again an `sd_unet`: parameters (diffusers names encoder.* and quant_conv.*) are enumerated / loaded /
 * finalised and the workspace is sized through the sd_unet_* functions (sd_unet_workspace_bytes_hw with cache_branch_id = -1
 * and the LATENT size).  cfg as for sd_vae_create: sample_size = latent size, in_channels = 4 (latent), out_channels = 3
 * (image), four levels.
 * encode: fp32 NCHW images [batch,3,8h,8w] in [0,1] -> 2 x - 1 -> encoder -> quant_conv -> fp32 NCHW moments [batch,8,h,w] =
 * [mean | logvar]; latent sides are multiples of 8 in [8, 128].  conv_in runs in fp32 on the fp32 image, conv_out
 * contracts bf16 operands into fp32 and quant_conv is applied to those sums in fp32 by the same kernel. */
int sd_vae_encoder_create(const sd_unet_config* cfg, sd_vae** out);
int sd_vae_encode_hw(sd_vae* v, void* stream, const float* images, int batch, int latent_h, int latent_w, float* moments_out,
                     void* workspace, long long workspace_bytes);
/* DiagonalGaussianDistribution of the moments [batch,8,hw]: latents_out [batch,4,hw] =
 * scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), or scale * mean when noise is NULL (mode()).  One launch. */
int sd_vae_posterior_sample(void* stream, const float* moments, const float* noise_or_null, float scale, float* latents_out,
                            int batch, long long hw);

/* ---- AutoencoderTiny (TAESD; diffusers 0.32 AutoencoderTiny, upstream-recall).  Additions under ABI 3: resolve them by name.
 * The structure is fixed (all widths 64, num_encoder_blocks 1,3,3,3, num_decoder_blocks 3,3,3,1, relu, nearest, 4 latent
 * channels), so the create calls take no config.  The handle is again an `sd_unet`: parameters (diffusers names
 * decoder.layers.N.* / encoder.layers.N.*, blocks as <layer>.conv.{0,2,4}.{weight,bias}) are enumerated / loaded / finalised
 * through the sd_unet_* functions, and the workspace is sized with sd_unet_workspace_bytes_hw (cache_branch_id = -1, the
 * LATENT size).  Latent sides are multiples of 8 in [8, 128].  Either half is a flat list of 35 launches: entry, 10 blocks of
 * three 64-channel convs, three up- / down-sampling convs, exit.
 * decode: fp32 NCHW latents [batch,4,h,w] (the UNet's scaled latents as they are: scaling_factor is 1) -> tanh(z / 3) * 3 ->
 *   decoder -> fp32 NCHW images [batch,3,8h,8w]; out_mode 0: y * 2 - 1 in [-1, 1], 1: clamp(y, 0, 1).
 * encode: fp32 NCHW images [batch,3,8h,8w] in [0,1] -> encoder -> fp32 NCHW latents [batch,4,h,w] (no posterior). */
typedef struct sd_unet sd_taesd;
int sd_taesd_decoder_create(sd_taesd** out);
int sd_taesd_encoder_create(sd_taesd** out);
int sd_taesd_decode_hw(sd_taesd* v, void* stream, const float* latents, int batch, int latent_h, int latent_w, int out_mode,
                       float* images_out, void* workspace, long long workspace_bytes);
int sd_taesd_encode_hw(sd_taesd* v, void* stream, const float* images01, int batch, int latent_h, int latent_w, float* latents_out,
                       void* workspace, long long workspace_bytes);
/* The tiny autoencoder's kernels one by one (parity tests, tools).  sd_op_conv64: 3x3 conv at 64 -> 64 channels on bf16 NHWC
 * X [B,Hin,Win,64] with the weights packed by sd_op_conv64_pack (host; OIHW fp32 [64][64][3][3] -> 73,728 bytes, which it
 * returns; out NULL: the size only); bias [64] fp32 or NULL; R [B,Hout,Wout,64] or NULL, added before the ReLU; mode 0: pad 1,
 * 1: nearest-2x upsample first, 2: stride 2 with pad 1 on all sides.  sd_op_taesd_entry: fp32 NCHW [B,Cin,H,W] -> conv3x3 in
 * fp32 (Wt [Cin*9][64] fp32) -> bf16 NHWC; decoder (Cin 4): tanh(x / 3) * 3 in the load, ReLU; encoder (Cin 3): neither.
 * sd_op_taesd_exit: bf16 NHWC -> conv3x3 64 -> Cout <= 4 (Wp [Cout][9][64] bf16) -> fp32 NCHW; out_mode 0: y * 2 - 1,
 * 1: clamp(y, 0, 1), 2: y. */
int sd_op_conv64(void* stream, const void* X, const void* Wpacked, const float* bias, const void* R, void* Y, int B, int Hin,
                 int Win, int mode, int relu);
long long sd_op_conv64_pack(const float* w_oihw, void* out);
int sd_op_taesd_entry(void* stream, const float* x, const float* Wt, const float* bias, void* y, int B, int H, int W, int Cin,
                      int decoder);
int sd_op_taesd_exit(void* stream, const void* x, const void* Wp, const float* bias, float* y, int B, int H, int W, int Cout,
                     int out_mode);

/* ---- CLIP text encoder: replaces `self.text_encoder(text_input_ids)[0]` inside
 * `encode_prompt` (src/models.py:139-155; transformers CLIPTextModel, quick_gelu, causal mask).  `sd_clip` IS the
 * `sd_unet` handle type: parameters (transformers names, `text_model.` prefix: embeddings.token_embedding.weight,
 * encoder.layers.N.self_attn.{q,k,v,out}_proj.*, layer_norm1/2.*, mlp.fc1/fc2.*, final_layer_norm.*) are
 * enumerated / loaded / finalised and the workspace is sized (unet_batch = prompts, cache_branch_id = -1) through the
 * sd_unet_* functions.  encode: device int32 token ids [batch, max_positions] -> device fp32
 * last_hidden_state [batch, max_positions, hidden_size] (what `prompt_embeds` is, src/models.py:139-150).
 * Tokenisation (CLIP BPE) is host-side text processing and stays in the host language. */
typedef struct sd_clip_config {
    int vocab_size;          /* 49408 */
    int hidden_size;         /* 768 */
    int num_layers;          /* 12 */
    int num_heads;           /* 12 */
    int intermediate_size;   /* 3072 */
    int max_positions;       /* 77 */
    float layer_norm_eps;    /* 1e-5 */
    /* MLP activation: SD_ACT_QUICK_GELU (0: OpenAI CLIP ViT-L/14, SD-1.5) or SD_ACT_GELU (exact, erf: the OpenCLIP ViT-H text
     * tower of Stable Diffusion 2.x, hidden 1024 / 16 heads / 23 layers).  (Appended: zero-initialise the struct.) */
    int hidden_act;
} sd_clip_config;
typedef struct sd_unet sd_clip;
int sd_clip_create(const sd_clip_config* cfg, sd_clip** out);
int sd_clip_encode(sd_clip* c, void* stream, const int* input_ids, int batch, float* hidden_out, void* workspace,
                   long long workspace_bytes);

/* ---- CLIP score: the reference's quality metric (quality_metrics.clip_score; torchmetrics CLIPScore over
 * transformers CLIPModel.get_image_features / get_text_features).
 * Text side: a kind-2 handle created with a projection also takes `text_projection.weight` [projection_dim, hidden_size];
 * sd_clip_text_embeds runs the text tower on int32 ids [batch, max_positions], takes the row at the EOS position (the first
 * position holding eos_token_id; eos_token_id < 0: the argmax of the ids, transformers' rule for configs whose
 * eos_token_id is 2), applies final_layer_norm and the projection -> fp32 [batch, projection_dim].
 * Vision side: `sd_clip_vision` is again the sd_unet handle type (kind 3), parameters under transformers'
 * CLIPVisionModelWithProjection names (vision_model.embeddings.{class_embedding, patch_embedding.weight,
 * position_embedding.weight}, vision_model.pre_layrnorm.*, vision_model.encoder.layers.N.*, vision_model.post_layernorm.*,
 * visual_projection.weight), enumerated / loaded / finalised through the sd_unet_* calls.  encode: device uint8 images
 * [batch, 3, height, width] (any size) -> CLIPImageProcessor (shortest edge -> image_size with Pillow's bicubic, bit-exact;
 * centre crop; OpenAI CLIP mean / std) -> ViT (non-causal attention, head dim 64 or 80, <= 320 tokens) -> post_layernorm of the
 * class token -> visual_projection: fp32 image_embeds [batch, projection_dim].  One plan per (batch, height, width).
 * sd_clip_score: raw[b] = 100 cos(image_embeds[b], text_embeds[b]) and score[b] = max(raw[b], 0) (either may be NULL). */
typedef struct sd_clip_vision_config {
    int hidden_size;         /* 768 (ViT-B/16) */
    int num_layers;          /* 12 */
    int num_heads;           /* 12 (head dim 64) */
    int intermediate_size;   /* 3072 */
    int image_size;          /* 224: resize shortest edge and centre crop */
    int patch_size;          /* 16 */
    int projection_dim;      /* 512 */
    float layer_norm_eps;    /* 1e-5 */
    /* MLP activation: SD_ACT_QUICK_GELU (x sigmoid(1.702 x): OpenAI CLIP) or SD_ACT_GELU (exact, erf: the OpenCLIP ViT-H/14 that
     * IP-Adapters use as image encoder, hidden 1280 / 16 heads = head dim 80).  (Appended: zero-initialise the struct.) */
    int hidden_act;
} sd_clip_vision_config;
enum { SD_ACT_QUICK_GELU = 0, SD_ACT_GELU = 1 };
typedef struct sd_unet sd_clip_vision;
int sd_clip_create_projected(const sd_clip_config* cfg, int projection_dim, int eos_token_id, sd_clip** out);
long long sd_clip_text_embeds_workspace_bytes(sd_clip* c, int batch);
int sd_clip_text_embeds(sd_clip* c, void* stream, const int* input_ids, int batch, float* text_embeds, void* workspace,
                        long long workspace_bytes);
int sd_clip_vision_create(const sd_clip_vision_config* cfg, sd_clip_vision** out);
long long sd_clip_vision_workspace_bytes(sd_clip_vision* v, int batch, int height, int width);
int sd_clip_vision_encode(sd_clip_vision* v, void* stream, const unsigned char* images, int batch, int height, int width,
                          float* image_embeds, void* workspace, long long workspace_bytes);
int sd_clip_score(void* stream, const float* image_embeds, const float* text_embeds, int batch, int dim, float* raw,
                  float* score);
/* ---- ImageReward (reference src/metrics/metrics.py:44-95, quality_metrics.image_reward: the ImageReward-v1.0 reward model) ----
 * A kind-6 sd_unet handle: BLIP's ViT (timm layout: fused attn.qkv, a patch-embedding bias, no pre-LayerNorm, the final `norm`
 * over all tokens, exact gelu), BLIP's BERT text encoder (post-LN layers: masked self-attention, cross-attention over the image
 * tokens, gelu MLP) and the reward head (five Linears with no activation between them, folded into one vector at finalize).
 * Parameters are enumerated / loaded / finalised through the sd_unet_* calls under these names:
 *   visual_encoder.{cls_token [H], pos_embed [tokens, H], patch_embed.proj.{weight,bias}, blocks.N.{norm1,attn.qkv,attn.proj,
 *   norm2,mlp.fc1,mlp.fc2}.{weight,bias}, norm.{weight,bias}};
 *   text_encoder.embeddings.{word_embeddings,position_embeddings}.weight, text_encoder.embeddings.LayerNorm.*,
 *   text_encoder.encoder.layer.N.{attention.self.{query,key,value}, attention.output.{dense,LayerNorm},
 *   crossattention.self.{query,key,value}, crossattention.output.{dense,LayerNorm}, intermediate.dense,
 *   output.{dense,LayerNorm}}.*;  mlp.layers.{0,2,4,6,7}.{weight,bias} (hidden -> 1024 -> 128 -> 64 -> 16 -> 1).
 * sd_image_reward_score: device uint8 images [B,3,h,w] (any size; CLIP preprocessing to image_size), device int32 ids and key
 * mask [B, L] (1 <= L <= max_text_len; mask 1 = token, 0 = padding; every row needs a valid key: the call copies the mask to
 * the host to check, which synchronises the stream) -> device fp32 rewards [B] = (head(last_hidden_state[:, 0]) - mean) / std
 * and, when features is not NULL, the fp32 class-token rows [B, hidden_size].  One plan per (B, L, h, w);
 * sd_image_reward_workspace_bytes sizes the L = max_text_len plan. */
typedef struct sd_image_reward_config {
    int vision_hidden_size;        /* 1024 (ViT-L/16); also the text encoder's encoder_width */
    int vision_num_layers;         /* 24 */
    int vision_num_heads;          /* 16 (head dim 64) */
    int vision_intermediate_size;  /* 4096 */
    int image_size;                /* 224 */
    int patch_size;                /* 16 */
    float vision_layer_norm_eps;   /* 1e-6 */
    int vocab_size;                /* 30524 */
    int hidden_size;               /* 768 */
    int num_layers;                /* 12 */
    int num_heads;                 /* 12 (head dim 64) */
    int intermediate_size;         /* 3072 */
    int max_positions;             /* 512 */
    float layer_norm_eps;          /* 1e-12 */
    int hidden_act;                /* SD_ACT_GELU only */
    int position_embedding_absolute; /* 1 only */
    int max_text_len;              /* 35; at most 64 */
    float reward_mean, reward_std; /* 0.16717362830052426, 1.0333394966054072 */
} sd_image_reward_config;
typedef struct sd_unet sd_image_reward;
int sd_image_reward_create(const sd_image_reward_config* cfg, sd_image_reward** out);
long long sd_image_reward_workspace_bytes(sd_image_reward* m, int batch, int height, int width);
int sd_image_reward_score(sd_image_reward* m, void* stream, const unsigned char* images, const int* input_ids,
                          const int* attention_mask, int batch, int text_len, int height, int width, float* rewards,
                          float* features_or_null, void* workspace, long long workspace_bytes);
/* Host only: Pillow's bicubic tap table (precompute_coeffs + normalize_coeffs_8bpc, 22 fractional bits) for a resize of
 * in_size -> out_size, output positions [first, first + count).  Returns the tap stride ksize; with non-NULL arrays also
 * writes xmin[count], xcnt[count] and coeffs[count][ksize]. */
int sd_clip_resize_taps(int in_size, int out_size, int first, int count, int* xmin, int* xcnt, int* coeffs);

/* ---- FID (reference src/metrics/metrics.py:98-112: torchmetrics FrechetInceptionDistance over torch-fidelity's
 * FeatureExtractorInceptionV3, "pt_inception-2015-12-05") ----
 * The handle owns the 94 conv blocks of the FID Inception-v3 with BatchNorm (eps 1e-3, running statistics) folded into
 * weight and bias by the caller: sd_inception_conv_info enumerates them in forward order (name = the module's state-dict
 * prefix, e.g. "Mixed_6c.branch7x7dbl_3"; shape = [Cout, Cin, kh, kw]), sd_inception_load_conv takes the folded fp32 OIHW
 * weight and the folded bias from the HOST, sd_inception_finalize uploads them (bf16 OHWI weights, fp32 biases).
 * sd_inception_features: uint8 images [batch, 3, height, width] (any size) -> TensorFlow-1 legacy bilinear resize to 299 x 299
 * (src = dst * in / out, no half-pixel offset; lerp along x, then y) -> (x - 128) / 128 -> the network as deep as `tap` needs
 * -> fp32 features [batch, tap], the global spatial mean of: 64 = first max pool, 192 = second max pool, 768 = Mixed_6e,
 * 2048 = Mixed_7c.  Activations are bf16 NHWC; every conv runs on one implicit-GEMM MFMA kernel whose epilogue writes the
 * branch's channel slice of the block output.  The workspace (256-byte aligned) depends on (batch, tap) only.
 * sd_fid_accumulate: sum[dim] += sum_b f_b, cov_sum[dim][dim] += sum_b f_b f_b^T, count += batch, all fp64 / int64 on the
 * device, in one launch -- the state torchmetrics keeps (features.double()). */
typedef struct sd_inception sd_inception;
int sd_inception_create(sd_inception** out);
void sd_inception_destroy(sd_inception* h);
int sd_inception_num_convs(const sd_inception* h);
int sd_inception_conv_info(const sd_inception* h, int index, char* name, int name_cap, long long shape[4]);
int sd_inception_load_conv(sd_inception* h, const char* name, const float* weight_oihw, long long weight_numel,
                           const float* bias, int cout);
int sd_inception_finalize(sd_inception* h);
long long sd_inception_workspace_bytes(sd_inception* h, int batch, int tap);
int sd_inception_features(sd_inception* h, void* stream, const unsigned char* images, int batch, int height, int width,
                          int tap, float* features, void* workspace, long long workspace_bytes);
int sd_fid_accumulate(void* stream, const float* features, int batch, int dim, double* sum, double* cov_sum,
                      long long* count);
/* operator level: Y[.., coff : coff + Cout] of rows of ldy channels = relu?(conv(X NHWC bf16, W bf16 [Cout][kh][kw][Cin],
 * stride, padding (pad_h, pad_w)) + bias); any Cin / Cout (no padding of tensors asked of the caller).  relu = 2: SiLU
 * instead (the ControlNet's conditioning embedding runs on this kernel) */
int sd_op_inception_conv(void* stream, const void* X, const void* W, const float* bias, void* Y, int B, int Hin, int Win,
                         int Cin, int Cout, int kh, int kw, int stride, int pad_h, int pad_w, int ldy, int coff, int relu);
/* 3x3 pools on NHWC bf16 into a channel slice: max with (stride, pad) = (2, 0) or (1, 1), padding never wins; average with
 * stride 1, pad 1 dividing by the number of in-bounds taps (count_include_pad=False) */
int sd_op_maxpool3x3(void* stream, const void* X, void* Y, int B, int H, int W, int C, int stride, int pad, int ldy, int coff);
int sd_op_avgpool3x3(void* stream, const void* X, void* Y, int B, int H, int W, int C, int ldy, int coff);
/* out fp32 [B][C] = mean over the HW pixels of X bf16 [B][HW][C] */
int sd_op_global_mean(void* stream, const void* X, float* out, int B, int HW, int C);
/* the preprocessing of sd_inception_features alone: uint8 [B][3][H][W] -> [B][299][299][3], bf16 or (out_fp32) fp32 */
int sd_op_inception_resize(void* stream, const unsigned char* images, int B, int H, int W, void* out, int out_fp32);

/* Measurement hook for bench.py: the same forward with a hipEvent pair around every launch.  Per
 * op kind (0 sinusoid, 1 gemv, 2 conv_in, 3 groupnorm, 4 conv3x3, 5 gemm, 6 layernorm,
 * 7 attention, 8 conv_out; 16 conv3x3 with fp8 operands, 17 gemm with fp8 operands, 18 fused prompt cross-attention,
 * 22 IP-Adapter image branch, 23 ControlNet residual add, 24 T-GATE capture, 25 T-GATE apply, 26 the zero fill of a T-GATE
 * capture plan's fused cross-attention residual) it returns summed
 * milliseconds, launch count, algorithmic FLOPs and algorithmic HBM bytes in arrays of SD_PROFILE_KINDS = 32
 * entries.  Synchronises the stream; never used inside a timed region. */
#define SD_PROFILE_KINDS 32
int sd_unet_forward_profiled(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                             float timestep, float* eps_out, void* workspace, long long workspace_bytes, int cache_mode,
                             int cache_branch_id, double kind_ms[SD_PROFILE_KINDS], long long kind_launches[SD_PROFILE_KINDS],
                             double kind_flops[SD_PROFILE_KINDS], double kind_bytes[SD_PROFILE_KINDS]);

/* The same measurement, one text line per launch: "op-index kind M N K milliseconds GFLOP MB" (kinds as above before the
 * 16+ regrouping; development: which shapes carry a group's time).  Returns the bytes written to `text`, < 0 on error. */
long long sd_unet_forward_op_times(sd_unet* u, void* stream, const float* latents, int latent_batch, int unet_batch,
                                   float timestep, float* eps_out, void* workspace, long long workspace_bytes, int cache_mode,
                                   int cache_branch_id, char* text, long long cap);

/* Debug/parity hook: copy a named intermediate (bf16 NHWC) of the LAST full forward into `out`
 * as fp32; names: "conv_in", "down0".."down3", "mid", "up0".."up3".  Synchronises the stream. */
int sd_unet_debug_tensor(sd_unet* u, void* stream, const char* name, float* host_out, long long numel,
                         void* workspace, int unet_batch, int cache_branch_id);

/* ---- fused CFG combine + scheduler.step (src/models.py:238-261; src/schedulers.py:98-187) ----
 *   eps   = cfg ? eps[0:n] + guidance*(eps[n:2n]-eps[0:n]) : eps[0:n]
 *   prev  = coef[0]*x + coef[1]*eps + coef[2]*m1 + coef[3]*m2 + coef[9]*m3 + coef[4]*noise
 *   y2    = coef[5]*x + coef[6]*eps      (x0_pred / LCM "denoised"), optional
 *   m_out = coef[7]*x + coef[8]*eps      (multistep history entry), optional
 * One launch serves DDIM, DPM-Solver / DPM-Solver++ (orders 1-3), LCM and PNDM/PLMS (4 history
 * terms); the host computes the scalar coefficients from its sigma tables, so the kernel needs no
 * host sync.  m1..m3, noise, y2, m_out may be NULL. */
int sd_sched_step(void* stream, const float* eps, int cfg, float guidance, const float* x, const float* m1,
                  const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                  const float coef[10], long long n);

/* ---- rescaled classifier-free guidance (guidance_rescale; diffusers' rescale_noise_cfg) ----
 * eps holds [u: batch samples | c: batch samples] of n_per_sample fp32 elements each.  Per sample b, with
 * g = u + guidance*(c - u) formed as sd_sched_step forms it:
 *   k_out[b] = rescale * std(c_b) / std(g_b) + (1 - rescale)      (torch.std: unbiased, no epsilon)
 * Deterministic: k_out[b] depends on sample b's elements and n_per_sample only -- one workgroup per sample, a fixed
 * thread/element assignment, double partials summed in a fixed order (mean, then the centred sum of squares).
 * n_per_sample: a positive multiple of 4; batch <= 65535. */
int sd_cfg_rescale_factors(void* stream, const float* eps, int batch, long long n_per_sample, float guidance,
                           float rescale, float* k_out);
/* sd_sched_step with the (CFG-combined) prediction of sample b = i / n_per_sample scaled by k[b] before every use:
 * e := k[b]*e in prev, y2 and m_out.  Same operands and coefficients as sd_sched_step. */
int sd_sched_step_rescaled(void* stream, const float* eps, int cfg, float guidance, const float* x, const float* m1,
                           const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                           const float coef[10], long long n, const float* k, long long n_per_sample);

/* ---- inpainting (diffusers' StableDiffusionInpaintPipeline) ----
 * sd_sched_step_inpaint: sd_sched_step (k = NULL) or sd_sched_step_rescaled (k given) with the latent blend of a 4-channel
 * UNet's inpainting loop in the SAME launch:
 *   prev = mask ? step : a*init + s*blend_noise
 * mask [n / n_per_sample][hw] fp32 (>= 0.5: repaint, take the step), broadcast over the n_per_sample / hw channels of its
 * sample; init / blend_noise: n fp32 elements like x (the clean image latents and the call's forward noise); (a, s) =
 * (sqrt(alpha_bar), sqrt(1 - alpha_bar)) of the NEXT timestep, (1, 0) after the last step.  s == 0 skips the noise term
 * (blend_noise may then be NULL), so a = 1 returns init bit for bit.  The step side is the expression of the unmasked kernels
 * in their order: where the mask is set, prev is bit-identical to theirs; y2 and m_out do not see the mask.  hw and
 * n_per_sample / hw: hw a positive multiple of 4 dividing n_per_sample. */
int sd_sched_step_inpaint(void* stream, const float* eps, int cfg, float guidance, const float* x, const float* m1,
                          const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                          const float coef[10], long long n, const float* k, long long n_per_sample, const float* init,
                          const float* blend_noise, const float* mask, float a, float s, long long hw);

/* ---- UniPC (Zhao et al. 2023; diffusers' UniPCMultistepScheduler): corrector + predictor of one step in ONE launch ----
 * Per element, with coef = [cm0 cm1 | cy0 cy1 | cc0 cc1 cc2 cc3 cc4 | cp0 cp1 cp2 cp3]:
 *   e     = cfg ? u + guidance*(c - u) : eps[0:n]      formed exactly as sd_sched_step forms it
 *   e     = k[b] * e                                   only when k != NULL (b = i / n_per_sample; as sd_sched_step_rescaled)
 *   m_t   = cm[0]*x + cm[1]*e                          history entry (x0 when predict_x0, else eps)
 *   y2    = cy[0]*x + cy[1]*e                          x0 prediction, optional output
 *   xc    = cc[0]*x_last + cc[1]*h1 + cc[2]*h2 + cc[3]*h3 + cc[4]*m_t     corrector
 *           (x_last == NULL: no corrector, xc = x bit for bit; nothing of cc is read)
 *   prev  = cp[0]*xc + cp[1]*m_t + cp[2]*h1 + cp[3]*h2                    predictor
 *   prev  = mask ? prev : a*init + s*blend_noise       only when init != NULL; same rule, operands and argument checks
 *                                                      as sd_sched_step_inpaint
 *   outputs: prev, x_corr (= xc, optional), y2 (optional), m_out (= m_t, optional)
 * h1, h2, h3: the history entries BEFORE this step's shift, newest first; the corrector of order o reads h1..h_o and m_t, the
 * predictor of order o reads m_t and h1..h_(o-1).  Sums run left to right in fp32; a NULL history entry is skipped and must
 * have zero coefficients (refused otherwise).  Refused before any launch: null eps / x / prev / coef; n not a positive multiple
 * of 4; n_per_sample not a positive multiple of 4 dividing n; with init: a null mask, s != 0 without blend_noise, hw not a
 * positive multiple of 4 dividing n_per_sample; a coefficient (or guidance, a, s) that is not finite; an output that overlaps
 * an input or another output (named in the message).  x_corr, y2 and m_out do not see the mask. */
int sd_sched_step_pc(void* stream, const float* eps, int cfg, float guidance, const float* x, const float* x_last,
                     const float* h1, const float* h2, const float* h3, float* prev, float* x_corr, float* y2, float* m_out,
                     const float coef[13], long long n, const float* k, long long n_per_sample, const float* init,
                     const float* blend_noise, const float* mask, float a, float s, long long hw);

/* ---- perturbed-attention guidance (PAG; Ahn et al. 2024, diffusers' PAGMixin) ----
 * The guidance modes of the PAG steps.  SD_GUIDE_CFG_PAG: eps = [u | c | p] (3 n elements), e = (u + guidance*(c - u)) +
 * pag_scale*(c - p); SD_GUIDE_PAG: eps = [c | p] (2 n elements), e = c + pag_scale*(c - p).  Per element in fp32, the CFG
 * part formed exactly as sd_sched_step forms it, the PAG term added to it.  p is the UNet output of the perturbed samples
 * (sd_unet_set_pag).
 * sd_sched_step_pag: sd_sched_step_inpaint with that e -- k and init may each be NULL (no rescale / no blend; with neither,
 * n_per_sample is not read).  sd_sched_step_pc_pag: sd_sched_step_pc with that e.  Same operands, coefficients and argument
 * checks as those two; besides, mode must be one of the two, and guidance and pag_scale finite.  pag_scale = 0 in
 * SD_GUIDE_CFG_PAG gives the bits of the plain CFG step for finite eps.
 * sd_cfg_rescale_factors_pag: sd_cfg_rescale_factors over eps = [u | c | p] with g = (u + guidance*(c - u)) +
 * pag_scale*(c - p), the value the SD_GUIDE_CFG_PAG step scales (CFG mode only: guidance_rescale needs CFG). */
enum { SD_GUIDE_CFG_PAG = 2, SD_GUIDE_PAG = 3 };
int sd_sched_step_pag(void* stream, const float* eps, int mode, float guidance, float pag_scale, const float* x, const float* m1,
                      const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                      const float coef[10], long long n, const float* k, long long n_per_sample, const float* init,
                      const float* blend_noise, const float* mask, float a, float s, long long hw);
int sd_sched_step_pc_pag(void* stream, const float* eps, int mode, float guidance, float pag_scale, const float* x,
                         const float* x_last, const float* h1, const float* h2, const float* h3, float* prev, float* x_corr,
                         float* y2, float* m_out, const float coef[13], long long n, const float* k, long long n_per_sample,
                         const float* init, const float* blend_noise, const float* mask, float a, float s, long long hw);
int sd_cfg_rescale_factors_pag(void* stream, const float* eps, int batch, long long n_per_sample, float guidance,
                               float pag_scale, float rescale, float* k_out);

/* ---- self-attention guidance (SAG) ----
 * SD_GUIDE_CFG_SAG: eps = [u | c | d] (3 n elements), e = (u + guidance*(c - u)) + sag_scale*(u - d); SD_GUIDE_SAG: eps = [c | d]
 * (2 n elements), e = c + sag_scale*(c - d).  d is the UNet output on the degraded latents (sd_op_sag_degrade).  Per element in
 * fp32, the CFG part formed exactly as sd_sched_step forms it.  Operands, coefficients and argument checks of the _pag twins;
 * mode must be one of the two, guidance and sag_scale finite.  sag_scale = 0 in SD_GUIDE_CFG_SAG gives the bits of the plain CFG
 * step for finite eps. */
enum { SD_GUIDE_CFG_SAG = 4, SD_GUIDE_SAG = 5 };
int sd_sched_step_sag(void* stream, const float* eps, int mode, float guidance, float sag_scale, const float* x, const float* m1,
                      const float* m2, const float* m3, const float* noise, float* prev, float* y2, float* m_out,
                      const float coef[10], long long n, const float* k, long long n_per_sample, const float* init,
                      const float* blend_noise, const float* mask, float a, float s, long long hw);
int sd_sched_step_pc_sag(void* stream, const float* eps, int mode, float guidance, float sag_scale, const float* x,
                         const float* x_last, const float* h1, const float* h2, const float* h3, float* prev, float* x_corr,
                         float* y2, float* m_out, const float coef[13], long long n, const float* k, long long n_per_sample,
                         const float* init, const float* blend_noise, const float* mask, float a, float s, long long hw);

/* One launch: image [batch,3,height,width] fp32 in [0,1] and mask [batch,1,height,width] fp32 ->
 *   masked_image [batch,3,height,width] = mask >= 0.5 ? 0.5 : image   (the encoder's input domain: 2 * 0.5 - 1 is exactly 0,
 *                                                                      upstream's (2 image - 1) * (mask < 0.5))
 *   latent_mask  [batch,1,height/8,width/8] = mask(8i, 8j) >= 0.5 as fp32 0 / 1   (binarise, then nearest resize)
 * height and width: positive multiples of 8. */
int sd_inpaint_prepare(void* stream, const float* image, const float* mask, float* masked_image, float* latent_mask,
                       int batch, int height, int width);

/* ---- operator-level entry points (each is one hot kernel; used by the parity tests) ----------- */
/* C[M,N] = [X|X2][M,K] . W[N,K]^T + bias + bias2 + R ; epi=1: GEGLU on interleaved W (N -> N/2) */
int sd_op_gemm(void* stream, const void* X, long long ldx, const void* X2, long long ldx2, int K1, const void* W,
               const float* bias, const float* bias2, const void* R, long long ldr, void* C, long long ldc, int M,
               int N, int K, int epi);
/* Which variant of the general GEMM kernel the plain (epi = 0) entry points run a problem on; no device work (additions
 * under ABI 3: resolve them by name).  sd_op_gemm_tile_rows: the rows of the bf16 output tile, 64 or 128 (tiles are 160
 * columns wide).  sd_op_gemm_splitk: the split-K factor (1 = none) sd_op_gemm picks (dtype 0, bf16) or sd_op_gemm_fp8 picks
 * (dtype 1, K in e4m3 elements; always on the 128-row tile).  Split s of S covers the 64-element (fp8: 128-element) K tiles
 * [KT s / S, KT (s + 1) / S) of the KT the problem has. */
int sd_op_gemm_tile_rows(int M, int N, int K);
int sd_op_gemm_splitk(int M, int N, int K, int dtype);
/* Same GEMM with a PER-SAMPLE weight matrix: rows [b*rows_per_batch, (b+1)*rows_per_batch) use W + b*w_batch_stride
 * (elements; rows_per_batch a multiple of 128).  epi=2: row softmax over the first sm_valid of every 80 output
 * columns, the rest written as 0.  The two halves of the folded prompt cross-attention
 * (Y = R + sum_h softmax_77(X A_h) B_h, src/models.py:227 -> diffusers Attention with 77 keys) are these two calls. */
int sd_op_gemm_batched(void* stream, const void* X, long long ldx, const void* W, long long w_batch_stride,
                       int rows_per_batch, const float* bias, const void* R, long long ldr, void* C, long long ldc,
                       int M, int N, int K, int epi, int sm_valid);
/* The softmax form (epi 2) with the block's norm2 folded in -- the first GEMM of the two-GEMM prompt cross-attention at the
 * 16x16 level: X = un-normalised rows, W = per-sample operands scaled by gamma, c1 / c2 = per-sample [N] fp32 vectors (row
 * sums of the rounded W; beta term), rowstats [parts][M][2] = (sum, sum of squares) partials of X's rows:
 * P = softmax over every 80-column group of  rstd_m * (X W^T - mean_m * c1) + c2. */
int sd_op_gemm_batched_softmax_ln(void* stream, const void* X, long long ldx, const void* W, long long w_batch_stride,
                                  int rows_per_batch, void* C, long long ldc, int M, int N, int K, int sm_valid,
                                  const float* rowstats, int parts, const float* c1, const float* c2, float eps);
/* NHWC 3x3 conv, pad 1, stride 1|2, optional fused nearest-2x upsample; W is bf16
 * [Cout][Cin/64][3*3][64] (K runs over 64-channel slice, tap, channel) */
int sd_op_conv3x3(void* stream, const void* X, const void* W, const float* bias, const float* bias2, const void* R,
                  void* Y, int B, int Hin, int Win, int Cin, int Cout, int stride, int upsample);
/* Which kernel a 3x3 conv of this shape runs on: 0 = implicit GEMM, 1 = halo kernel (9 taps), 2 = halo kernel's 4-tap
 * mode.  M = output rows (B Hout Wout; for upsample = 2, the sub-pixel form, 4 B Hin Win); upsample 1 = fused nearest-2x;
 * dtype 0 = bf16, 1 = fp8 e4m3 (Cin padded to 128).  No device work. */
/* A ResNet block's conv2 with its 1x1 conv_shortcut folded into the same launch (the halo kernel's shortcut phase):
 *   Y = conv3x3(X, W) + [Xs1 | Xs2] Wsc^T + bias,   stride 1, pad 1, bf16.
 * X = [B, H, W, Cin] and W as for sd_op_conv3x3; Xs1 = [B, H, W, Cs1], Xs2 = [B, H, W, Cs2] (NULL with Cs2 = 0): the
 * shortcut's input as a virtual channel concat, Cs1 and Cs2 multiples of 64; Wsc = bf16 [Cout][Cs1 + Cs2]; bias = fp32
 * [Cout], the SUM of the two convs' biases.  The 1x1 product is accumulated in fp32 on the conv's accumulators (no bf16
 * rounding of the shortcut on its own).  Returns an error where the conv does not run on the halo kernel's 9-tap mode. */
int sd_op_conv3x3_shortcut(void* stream, const void* X, const void* W, const float* bias, const void* Xs1, int Cs1,
                           const void* Xs2, int Cs2, const void* Wsc, void* Y, int B, int H, int Wd, int Cin, int Cout);
/* The same launch feeding GroupNorm(+SiLU) from its epilogue's block statistics, as sd_op_conv3x3_groupnorm does for the
 * plain conv (H * W a multiple of 64, images the single-launch GroupNorm does not take): Y = conv output, Yn = normalised. */
int sd_op_conv3x3_shortcut_groupnorm(void* stream, const void* X, const void* W, const float* bias, const void* Xs1, int Cs1,
                                     const void* Xs2, int Cs2, const void* Wsc, void* Y, int B, int H, int Wd, int Cin,
                                     int Cout, const float* gamma, const float* beta, void* Yn, int groups, float eps, int silu);
/* The 3x3 stride-2 conv padded on the right and the bottom only: F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride = 2), the
 * AutoencoderKL encoder's downsampler.  W as for sd_op_conv3x3; Hin and Win even; Y = [B, Hin / 2, Win / 2, Cout]. */
int sd_op_conv3x3_down_asym(void* stream, const void* X, const void* W, const float* bias, void* Y, int B, int Hin, int Win,
                            int Cin, int Cout);
int sd_op_conv3x3_kernel(int M, int N, int Cin, int Hin, int Win, int stride, int upsample, int dtype);
/* In-place softmax(scale * row) of bf16 S [rows, cols], cols a multiple of 8: the VAE mid-block attention's softmax
 * (one wave per row up to 4096 columns; beyond, a workgroup per row with an online max / sum over the row). */
int sd_op_softmax_rows(void* stream, void* S, long long rows, int cols, float scale);
/* Upsample2D (nearest 2x, then 3x3 conv; diffusers resnet.py, the UNet's three upsamplers) as four 2x2 convs on the
 * LOW-RES input -- one per output sub-pixel phase -- with the 3x3 taps that read the same low-res pixel summed: 4/9 of
 * the multiply-adds, the same linear map.  W4 = bf16 [4 phases (py, px)][Cout][Cin/64][4 taps (dy, dx)][64];
 * needs Hin * Win % 128 == 0.  Y = [B, 2 Hin, 2 Win, Cout]. */
int sd_op_conv3x3_upsample_subpixel(void* stream, const void* X, const void* W4, const float* bias, void* Y, int B, int Hin,
                                    int Win, int Cin, int Cout);
/* The same followed by the GroupNorm(+SiLU) of the next resnet, as the plan runs the pair: the conv epilogue delivers the
 * per-64-row-block channel statistics (row order (sample, phase, low-res pixel)) and the GroupNorm skips its statistics pass.
 * Where (pixel tiles x 4 phases x channel tiles) >= 256 the conv runs on the halo kernel's 4-tap mode (csrc/conv_halo.hip,
 * SD_SUBPIX_HALO=0: the implicit-GEMM kernel; bit-identical).  Y: conv output, Yn: normalised output. */
int sd_op_conv3x3_upsample_subpixel_groupnorm(void* stream, const void* X, const void* W4, const float* bias, void* Y, int B,
                                              int Hin, int Win, int Cin, int Cout, const float* gamma, const float* beta,
                                              void* Yn, int groups, float eps, int silu);
int sd_op_groupnorm(void* stream, const void* x1, int C1, const void* x2, int C2, const float* gamma,
                    const float* beta, void* y, int B, int HW, int groups, float eps, int silu);
/* conv3x3 (stride 1) -> GroupNorm(+SiLU) the way the forward plan runs every resnet's conv -> norm pair
 * (diffusers ResnetBlock2D, reached from src/models.py:227): the conv's epilogue leaves per-64-pixel-block channel sums
 * and the GroupNorm takes its statistics from them instead of re-reading Y.  Y = conv output, Yn = normalised output. */
int sd_op_conv3x3_groupnorm(void* stream, const void* X, const void* W, const float* bias, const float* bias2,
                            const void* R, void* Y, int B, int Hin, int Win, int Cin, int Cout, const float* gamma,
                            const float* beta, void* Yn, int groups, float eps, int silu);
/* Small images (the single-launch GroupNorm: <= 256 pixels and <= 10240 values per group) take the same entry point: a
 * split-K conv then leaves its fp32 partial slabs to the GroupNorm kernel, which finishes the reduce (+ bias + bias2 + R, in
 * splitk_reduce's order of additions), stores Y and normalises it in ONE launch (SD_GN_SLAB=0: conv + reduce, then the
 * GroupNorm; bit-identical).  sd_op_conv3x3_splitk: the split factor the library picks for a 3x3 conv (1 = none). */
int sd_op_conv3x3_splitk(int M, int Cout, int Cin, int Hin, int Win, int stride, int upsample);
int sd_op_layernorm(void* stream, const void* x, const float* gamma, const float* beta, void* y, int rows, int C,
                    float eps);
/* Token Merging for Stable Diffusion (tomesd; csrc/tome.hip), kernel by kernel.  A level of h x w tokens (even
 * sides, at most 16384 tokens) is cut into 2x2 cells; choice [h/2 * w/2] bytes names the dst token of each cell (0..3, row-major
 * in the cell), the other three are src tokens: num_dst = h w / 4, num_src = 3 num_dst.  dst slots are numbered by cell, src
 * slots by ascending token index; every index list below holds slot numbers.  C: a multiple of 64 up to 1536.
 * match: x [B][h w][C] bf16 -> per src slot the largest cosine similarity to a dst token (node_max fp32 [B][num_src]) and that
 *   dst slot (node_idx; ties: the lowest slot), on MFMAs over the raw rows, scaled by the fp32 inverse norms afterwards
 *   (|error| <= 4 C 2^-24; a zero row scores 0).  Also writes tok [h w]: the token index of every src slot, then of every dst slot.
 * select: the r largest of num_src (<= 12288) scores per sample, radix select, ties at the cut to the lowest slot ->
 *   kept [B][num_src - r] and merged [B][r] (ascending slots), dst_idx [B][r] = node_idx of the merged.
 * merge: out [B][h w - r] rows of pitch ldo = the kept src rows, then every dst row averaged with the src rows merged into it
 *   (fp32, ascending src slot, one rounding).
 * unmerge: out [B][h w][C] = y[row of the token] + residual (NULL: no residual); y [B][h w - r] rows of pitch ldy; a merged
 *   src token reads its dst's row.
 * All four are deterministic. */
int sd_op_tome_match(void* stream, const void* x, const unsigned char* choice, int B, int h, int w, int C, float* node_max,
                     int* node_idx, int* tok);
int sd_op_tome_select(void* stream, const float* node_max, const int* node_idx, int B, int num_src, int r, int* kept, int* merged,
                      int* dst_idx);
int sd_op_tome_merge(void* stream, const void* x, const int* tok, const int* kept, const int* merged, const int* dst_idx, void* out,
                     long long ldo, int B, int h, int w, int C, int r);
int sd_op_tome_unmerge(void* stream, const void* y, long long ldy, const void* residual, const int* tok, const int* kept,
                       const int* merged, const int* dst_idx, void* out, int B, int h, int w, int C, int r);
/* FreeU on the inputs of one resnet (csrc/freeu.hip), one launch on bf16 NHWC tensors: skip_out [B][H][W][C_skip] =
 * fourier_filter(skip, threshold = 1, scale = s) -- per (sample, channel) plane the Fourier modes {-1, 0} x {-1, 0} times s, real
 * part, as the closed form  y[n] = x[n] + (s - 1) / (H W) (S0 + sum_k C_k cos a_k(n) + S_k sin a_k(n)),  k in {(1,0), (0,1), (1,1)}
 * in fp32 with one rounding -- and hidden_out [B][H][W][C_hidden] = hidden with channels [0, C_hidden / 2) times b (one rounding),
 * the others copied.  The outputs must be new tensors.  H, W in [2, 128]; C_hidden, C_skip multiples of 32; b, s finite and > 0.
 * Deterministic. */
/* T-GATE's two kernels (csrc/tgate.hip) on bf16 rows of C channels, C a multiple of 8, any row count; fp32 sums rounded
 * once to bf16.  capture: y, res [pair * rows][C] -> h2 = res + y for every row and cache [rows][C] = (y[m] + y[rows + m]) / 2
 * (pair 2: a CFG pair) or y (pair 1).  apply: h2 [rows][C] = h1 + cache.  rowstats (NULL = off): [2][rows of h2][2] fp32, the (sum, sum
 * of squares) of the stored h2 row's first ceil(C / 16) 16-byte vectors and of the rest (the LayerNorm-fold partials of
 * sd_op_gemm_ln).  The outputs are new tensors; anything else is refused by name and nothing is written. */
int sd_op_tgate_capture(void* stream, const void* y, const void* res, void* h2, void* cache, float* rowstats, long long rows, int C,
                        int pair);
int sd_op_tgate_apply(void* stream, const void* h1, const void* cache, void* h2, float* rowstats, long long rows, int C);
int sd_op_freeu(void* stream, const void* hidden, const void* skip, void* hidden_out, void* skip_out, int B, int H, int W,
                int C_hidden, int C_skip, float b, float s);
/* HyperTile's copy kernel on its own (csrc/hypertile.hip).  Raster order: [B][rh][rw] rows of C bf16 channels with a row
 * pitch of `pitch` elements; tile order: [B][nh][nw][rh / nh][rw / nw] dense rows of C -- tile (i, j) holds the tokens
 * (i th + y, j tw + x), row-major inside the tile, the tiles row-major in the sample.  gather: raster x -> tile-order out; scatter:
 * tile-order y -> raster out.  16-byte accesses and 64-bit offsets; bit-exact copies.
 * sd_hypertile_check: the shape rule of both (and of the plan builder), no GPU work: 1 <= B <= 65535, sides in 1..256, nh | rh and
 * nw | rw, C a multiple of 8 up to 16384, pitch a multiple of 8, >= C and <= 2^30 (so that no element offset leaves 63 bits).  What it refuses the ops refuse by name, writing nothing;
 * they also want 16-byte-aligned pointers. */
int sd_hypertile_check(int B, int rh, int rw, int C, int nh, int nw, long long pitch);
int sd_op_hypertile_gather(void* stream, const void* x, long long pitch, void* out, int B, int rh, int rw, int C, int nh, int nw);
int sd_op_hypertile_scatter(void* stream, const void* y, void* out, long long pitch, int B, int rh, int rw, int C, int nh, int nw);
/* PAG's identity self-attention on its own (csrc/pag.hip): the attention output of a perturbed sample is V.  Writes
 * out[r][h * D + d] = V(r, h, d), D = C / heads, for the rows [row0, row0 + rows) of a token-major [rows_total][C] bf16 output and
 * nothing else.  tok == 0: V token-major, row r at V + r * ldv (the q | k | v projection: V = qkv + 2 C, ldv = 3 C); tok > 0: V
 * head-major [rows_total / tok][heads][tok][D] dense (ldv not read), sample = r / tok.  A bit-exact copy, 16-byte accesses, 64-bit
 * offsets.  sd_pag_identity_check: the shape rule (and the plan builder's), no GPU work: rows_total in 1 .. 2^31, the row range
 * inside it, D a multiple of 8, C <= 16384, token-major: ldv a multiple of 8 in C .. 2^30; head-major: tok divides rows_total,
 * row0 and rows.  What it refuses the op refuses by name, writing nothing; the op also wants 16-byte-aligned pointers. */
int sd_pag_identity_check(long long rows_total, long long row0, long long rows, int C, int heads, long long ldv, int tok);
int sd_op_pag_identity(void* stream, const void* V, long long ldv, int tok, void* out, long long rows_total, long long row0,
                       long long rows, int C, int heads);
/* SAG's kernels on their own (csrc/sag.hip).
 * sd_op_sag_attn_mass: mass[b][k] = (1 / heads) * sum_h sum_q softmax_k(Q_h K_h^T)[q][k], fp32 [B][N]; Q and K token-major bf16,
 * sample b's row t at Q + (b N + t) ld (the q | k | v projection: K = Q + C, ld = 3 C, C = heads * D).  Q carries the softmax
 * scale already: exp2_units = 0: 1 / sqrt(D), the softmax is the natural one; 1: log2(e) / sqrt(D), as attn1's packed W_q gives
 * it, and the kernel exponentiates to base 2.  Exact two-pass fp32 softmax, fixed summation order, no atomics: the same bits on
 * every run.  sd_sag_mass_check: the shape rule (and the plan builder's), no GPU work: B in 1 .. 65535, N in 16 .. 256, D 64, 80
 * or 160, heads 1 .. 64, ld a multiple of 8 in 2 C .. 2^30, head_major must be 0 (head-major K is refused by name).
 * sd_op_sag_degrade: x and m fp32 [LB][4][H][W] (latents and the model output on them), mass fp32 [>= LB][mh * mw] ->
 *   x0 = coef[0] x + coef[1] m (pred_type 2: m),  eps = coef[2] x + coef[3] m (pred_type 0: m),
 *   blur = 9x9 Gaussian of x0, sigma 1, reflect padding, separable (rows, then columns; each acc = fma(w_i, v_i, acc), i = -4 .. 4),
 *   deg = mass[b][y / 8][x / 8] > 1 ? blur : x0,   out = coef[4] deg + coef[5] eps.
 * pred_type 0 epsilon, 1 v_prediction, 2 sample; coef derived in fp64 by the caller from alphas_cumprod[t] (schedulers.py::
 * sag_degrade_coef).  H, W multiples of 8 in 32 .. 128, mh = H / 8, mw = W / 8; out must not alias x or m. */
int sd_sag_mass_check(int B, int heads, int N, int D, long long ld, int head_major);
int sd_op_sag_attn_mass(void* stream, const void* Q, const void* K, long long ld, float* mass, int B, int heads, int N, int D,
                        int exp2_units);
int sd_op_sag_degrade(void* stream, const float* x, const float* m, const float* mass, int mh, int mw, int pred_type,
                      const float coef[6], float* out, int LB, int H, int W);
/* flash-style attention on token-major [B, N, heads * D] views; D = 40, 64, 80 or 160 (64: Stable Diffusion 2.x), any Nq / Nk */
int sd_op_attention(void* stream, const void* Q, long long ldq, const void* K, long long ldk, const void* V,
                    long long ldv, void* O, long long ldo, int B, int heads, int Nq, int Nk, int D, float scale);
/* the same with HEAD-MAJOR K / V, [B][heads][Nk][D] contiguous (how the plan's fused q|k|v projection stores K and V at
 * the 64x64 level: a 64-key tile of one head is one contiguous 5 KiB block for the LDS-DMA); d = 40, Nk % 64 == 0 */
int sd_op_gemm_qkv_headmajor(void* stream, const void* X, long long ldx, const void* W, void* Q, void* KV, int M, int C,
                             int tokens, int K);   /* the producer: Q [M][C], KV [2][M/tokens][C/40][tokens][40] */
int sd_op_attention_headmajor(void* stream, const void* Q, long long ldq, const void* K, const void* V, void* O,
                              long long ldo, int B, int heads, int Nq, int Nk, int D, float scale);
/* causal self-attention of the CLIP text tower (transformers CLIPAttention, reached from src/models.py:139-155) on the fused
 * projection output qkv [B * L][3 H] (q | k | v, bf16) -> out [B * L][H]; 1 <= L <= 128, head dim 64 (16 in the reduced tests),
 * B <= 65535, out 4-byte aligned */
int sd_op_clip_attention(void* stream, const void* qkv, void* out, int B, int L, int H, int heads);
/* non-causal ViT self-attention on the fused projection output qkv [B * L][3 H] -> out [B * L][H]; head dim 64, L <= 320 */
int sd_op_vit_attention(void* stream, const void* qkv, void* out, int B, int L, int H, int heads);
/* the text tower's embedding: out [rows][H] bf16 = tok [vocab][H] row ids[r] + pos [L][H] row r % L (fp32 sum, one rounding);
 * ids int32 [rows], rows = B * L, H even.  An id outside [0, vocab) is CLAMPED to row 0 / vocab - 1 (the Python wrapper
 * refuses such ids before the call). */
int sd_op_clip_embed(void* stream, const int* ids, const void* tok, const void* pos, void* out, int rows, int L, int H,
                     int vocab);
/* the towers' MLP activation in place on n bf16 values (n even): kind SD_ACT_QUICK_GELU (x sigmoid(1.702 x)) or SD_ACT_GELU
 * (x Phi(x), within 1.3e-5 |x| before the output rounding); any other kind is refused */
int sd_op_activation(void* stream, void* x, long long n, int kind);
/* dst [B][H] = src [B * L][H] row b * L + p_b (bf16, copied): ids NULL -> p_b = 0 (the class token); ids int32 [B][L] with
 * eos_id >= 0 -> the first position holding eos_id (0 when there is none), eos_id < 0 -> the first maximum of ids[b]
 * (transformers' two pooling rules of CLIPTextModel) */
int sd_op_pool_rows(void* stream, const void* src, const int* ids, int B, int L, int H, int eos_id, void* dst);
/* the vision tower's embedding: out [B][Np + 1][H] bf16; row 0 = cls [H] (fp32) + pos row 0, row 1 + p = patch_rows
 * [B * Np][H] row b * Np + p + pos [Np + 1][H] row 1 + p (fp32 sum, one rounding) */
int sd_op_vit_embed(void* stream, const void* patch_rows, const float* cls, const void* pos, void* out, int B, int Np, int H);
/* masked attention of a short query block (the BLIP text encoder's self- and cross-attention), head dim 64: q [B * Lq][ldq],
 * k and v [B * Lk][ldkv] (bf16; each pointer at its own column offset, 16-byte aligned, pitches multiples of 8), key mask int32
 * [B][Lk] or NULL (all valid) -> out [B * Lq][ldo]; 1 <= Lq <= 64, 1 <= Lk <= 320.  A masked key is excluded by select: whatever
 * finite value its K / V rows hold does not reach the output.  Copies the mask to the host and refuses a sample without a valid
 * key (synchronises the stream). */
int sd_op_bert_attention(void* stream, const void* q, long long ldq, const void* k, const void* v, long long ldkv,
                         const int* mask, void* out, long long ldo, int B, int heads, int Lq, int Lk);
/* rewards[b] = (w . x_b + bias[0] - mean) / std over the fp32 of the bf16 row hidden[b * row_stride .. + H); features
 * (or NULL) fp32 [B][H] = x_b */
int sd_op_reward_head(void* stream, const void* hidden, long long row_stride, const float* w, const float* bias, float mean,
                      float std, int B, int H, float* rewards, float* features);
/* the CLIP preprocessing of sd_clip_vision_encode on its own: uint8 [B][3][H][W] -> uint8 crop [B][3][S][S] and bf16 patch
 * rows [B (S/P)^2][Kp], Kp = 3 P^2 rounded up to a multiple of 64 (zero columns past 3 P^2).  Synchronises the stream. */
int sd_op_clip_preprocess(void* stream, const unsigned char* images, int B, int H, int W, int S, int P, unsigned char* crop,
                          void* patches);
int sd_op_conv_in(void* stream, const float* x, int Bsrc, const float* Wt, const float* bias, void* y, int B, int H,
                  int W, int Cin, int Cout);
/* conv_in of an inpainting UNet: x [Bsrc,4,H,W] and cond [Bcond,5,H,W] fp32 (batch indices modulo their source batch), Wt
 * [81][Cout] fp32 (k = ic*9 + tap over the 9 concatenated channels) -> y NHWC bf16 [B,H,W,Cout]; one launch, Cout <= 1024 */
int sd_op_conv_in_cond(void* stream, const float* x, int Bsrc, const float* cond, int Bcond, const float* Wt,
                       const float* bias, void* y, int B, int H, int W, int Cout);
/* conv_in of a ControlNet: y = bf16(conv_in(x) + float(addend)), x [Bsrc,4,H,W] fp32, addend NHWC bf16 [Badd,H,W,Cout] (batch
 * indices modulo their source batch), fp32 accumulation, ONE rounding, 16-byte stores; Cout a multiple of 8, <= 2048 */
int sd_op_conv_in_add(void* stream, const float* x, int Bsrc, const void* addend, int Badd, const float* Wt, const float* bias,
                      void* y, int B, int H, int W, int Cout);
/* x[dst_off[i] + j] <- bf16(float(x[dst_off[i] + j]) + scale * float(r[src_off[i] + j])), j < count[i], for nseg <= 16 segments
 * in ONE launch (bf16 element offsets, multiples of 8; any count; x and r 16-byte aligned; host arrays) */
int sd_op_residual_add(void* stream, void* x, const long long* dst_off, const void* r, const long long* src_off,
                       const long long* count, int nseg, float scale);
int sd_op_conv_out(void* stream, const void* x, const void* Wp, const float* bias, float* y, int B, int H, int W,
                   int Cin, int Cout);
int sd_op_time_embedding(void* stream, float t, const void* W1, const float* b1, const void* W2, const float* b2,
                         float* scratch, float* temb, int dim_in, int dim);
/* the two kernels of a conditioned time embedding: row = Wc . cond (Wc bf16 [dim][cond_dim], cond fp32 [cond_dim], 16-byte
 * aligned, cond_dim a multiple of 8), then emb = [cos(t f_k) | sin(t f_k)] + row (fp32 [dim], dim even) */
int sd_op_timestep_cond(void* stream, float t, const float* cond, const void* Wc, float* row, float* emb, int cond_dim,
                        int dim);

/* Fused prompt cross-attention of one transformer block (src/models.py:227-235 -> diffusers Attention over the 77 prompt
 * keys): Y = R + sum_h softmax_L(X A_h) B_h + b_o in ONE launch, probabilities kept in registers.  8 heads x 80 key
 * slots.  A^T row (head, slot) = scale * K_h[slot] . W_q,h over the C channels (zero rows for slots >= L); Bw row =
 * output channel, columns (head, slot) with bits 2 and 3 of the slot index swapped inside every group of 16 (the order in
 * which an MFMA accumulator tile is consumed as the next product's operand).  Both are passed TILED so that every
 * LDS-DMA piece of the kernel is one contiguous KiB: At [samples][C/32][640][32], Bw [samples][C/32][20][32][32] (bf16).
 * sd_unet_set_context builds both from the prompt.  M tokens, rows_per_sample tokens per sample (multiple of 128). */
/* LayerNorm folded into the GEMM that consumes it (BasicTransformerBlock norm1 -> attn1 q|k|v, norm3 -> ff GEGLU; diffusers
 * attention.py, reached from src/models.py:227).  The producer of the residual stream leaves per-row (sum, sum of squares)
 * partials of its stored bf16 output, [parts][M][2] fp32 (sd_op_ln_partials: kind 0 = a GEMM with N columns, kind 1 = the
 * fused cross-attention of M rows x N channels); the consumer runs on the UN-normalised rows with Wg = bf16(W * gamma),
 * c1[n] = sum_k Wg[n][k], c2[n] = sum_k W[n][k] beta[k] + b[n] and finishes  rstd_m (acc - mean_m c1[n]) + c2[n]. */
int sd_op_ln_partials(int kind, int M, int N);
int sd_op_gemm_rowstats(void* stream, const void* X, long long ldx, const void* W, const float* bias, const void* R,
                        long long ldr, void* C, long long ldc, int M, int N, int K, float* rowstats);
int sd_op_gemm_ln(void* stream, const void* X, long long ldx, const void* Wg, const float* c1, const float* c2,
                  const float* rowstats, int parts, float eps, void* C, long long ldc, int M, int N, int K, int epi);
/* the std-epilogue GEMM with every side input / output the UNet plan combines on it (second K segment, bias + bias2, residual,
 * LayerNorm row partials [2 N/160][M][2] and GroupNorm block statistics [M/64][N][2] of the stored output, the LayerNorm
 * fold, head-major K / V) -- the entry through which tests compare the lean projection kernel (csrc/gemm_lean.hip) with
 * the general one bit for bit (environment SD_GEMM_LEAN=0 selects the general kernel; results are identical) */
int sd_op_gemm_plan(void* stream, const void* X, long long ldx, const void* X2, long long ldx2, int K1, const void* W,
                    const float* bias, const float* bias2, const void* R, long long ldr, void* C, long long ldc, int M, int N,
                    int K, float* rowstats, float* stats, const float* ln_rs, int ln_parts, const float* ln_c1, float ln_eps,
                    void* KV, int hm_tokens);
int sd_op_xattn_fused_rowstats(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                               const float* bias, int M, int C, int rows_per_sample, int L, float* rowstats);
/* The IP-Adapter image branch as one launch (what sd_unet_set_ip_adapter_hw's plan variant runs in front of every prompt
 * cross-attention):  Rout[m] = R[m] + sum_h softmax_T( LN(R[m]) . A_h[s]^T ) . B_h[s],  s = m / rows_per_sample.
 * R, Rout: bf16 [M][C], Rout != R.  A: bf16 [samples][32][C], row head * (32 / heads) + t = the folded key t of that head
 * (softmax scale included), every other row zero.  Bt: bf16 [samples][C][32], the folded values in the same slots (adapter
 * scale included).  gamma / beta: fp32 [C], the LayerNorm the kernel applies from each row's own statistics; the normalised
 * row is rounded to bf16 before the first product, the probabilities before the second; sums, softmax and the residual add
 * are fp32 with one bf16 rounding on store.  C % 32 == 0 (at most 2048), heads in {1, 2, 4, 8}, T = 4, any
 * rows_per_sample >= 1 (a tile of 32 rows never spans two samples), M a multiple of rows_per_sample; 16-byte aligned. */
int sd_op_ip_xattn(void* stream, const void* R, void* Rout, const void* A, const void* Bt, const float* gamma, const float* beta,
                   float eps, long long M, int C, int rows_per_sample, int heads, int T);
/* The builders of the prompt-side operands of cross-attention on their own (what sd_unet_set_context_hw and
 * sd_unet_set_ip_adapter_hw run per layer; all tensors bf16 unless said otherwise).
 * sd_op_xattn_expand: out [B * heads * slots][C], row (b, h, j) = scale * kv [b * L + j][col_off + c] (fp32
 *   product, one rounding) for j < L and c in head h, +0 elsewhere.  kv rows are 2 C wide (K | V): col_off 0 or C.  1 <= L <=
 *   slots, heads divides C, C / heads even.
 * sd_op_transpose_bf16: dst [b][c][r'] = src [b][r][c] (B <= 65535); perm16: r' = r with bits 2 and 3 swapped
 *   ((r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1), R % 16 == 0), else r' = r.
 * sd_op_retile32: dst [b][R / RT][K / 32][RT][32] = src [b][R][K]; K % 32 == 0, R % RT == 0, 16-byte aligned. */
int sd_op_xattn_expand(void* stream, const void* kv, void* out, int B, int L, int C, int heads, int slots, int col_off, float scale);
int sd_op_transpose_bf16(void* stream, const void* src, void* dst, int B, int R, int Cc, int perm16);
int sd_op_retile32(void* stream, const void* src, void* dst, int B, int R, int K, int RT);
/* sd_op_xattn_fold: every operand of one folded prompt cross-attention layer.  kv [UB * L][2 C] = the projected prompt (K | V),
 *   wqT [C][C] = to_q transposed ([in][out]; with norm2 folded: gamma-scaled and centred over the input channel), wo [C][C] =
 *   to_out.  NP = heads * 80 key slots, slot h * 80 + j = key j of head h, slots j >= L are zero rows.
 *   at = rows of (K_h / sqrt d) . W_q,h, bw = columns of V_h . W_o,h^T.  perm = 1: the layouts sd_op_xattn_fused reads (at
 *   [UB][C / 32][NP][32], bw [UB][C / 32][NP / 32][32][32] with the slot permutation of sd_op_transpose_bf16); perm = 0: at
 *   [UB][NP][C], bw [UB][C][NP] (sd_op_gemm_batched's per-sample W).  c2 [UB][NP] fp32 = (K_h / sqrt d) . lnu (lnu fp32 [C]; both
 *   null or neither), c1 [UB][NP] fp32 = ones . the stored rows of at (perm = 0 only; ones fp32 [C]; both null or neither).
 *   scratch: 3 * UB * NP * C bf16; afterwards its first third holds bw before the transpose ([UB * NP][C]), the second the V
 *   expansion.  1 <= L <= 80, C % 64 == 0, C / heads even.
 * sd_op_ip_fold: the same for one IP-Adapter block over 32 key slots (32 / heads per head, T <= 32 / heads image tokens): ip_kv
 *   [UB * T][2 C] -> at [UB][32][C], bt [UB][C][32] (sd_op_ip_xattn's A and Bt; V is multiplied by scale before its rounding).
 *   scratch: 3 * UB * 32 * C bf16: the K expansion, the V expansion, bt before the transpose. */
int sd_op_xattn_fold(void* stream, const void* kv, const void* wqT, const void* wo, const float* lnu, const float* ones, void* at,
                     void* bw, float* c1, float* c2, void* scratch, int UB, int L, int C, int heads, int perm);
int sd_op_ip_fold(void* stream, const void* ip_kv, const void* wqT, const void* wo, void* at, void* bt, void* scratch, int UB, int T,
                  int C, int heads, float scale);
int sd_op_xattn_fused(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                      const float* bias, int M, int C, int rows_per_sample, int L);
/* The same with the block's norm2 folded in (how the plan runs it at the 64x64 / 32x32 levels): X holds the UN-normalised rows
 * (normally X == R), ln_rowstats [ln_parts][ln_rows][2] their (sum, sum of squares) partials (row m reads row m % ln_rows),
 * At = tiled rows of scale K_h W_q,h diag(gamma) centred over the channel, c2 [samples][640] fp32 the beta term of every key
 * slot: score = rstd_m (X . At)[m][n] + c2[n].  rowstats: optional partials of Y as in sd_op_xattn_fused_rowstats. */
int sd_op_xattn_fused_ln(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                         const float* bias, int M, int C, int rows_per_sample, int L, const float* ln_rowstats, int ln_parts,
                         long long ln_rows, const float* c2, float eps, float* rowstats);
/* diagnostic twin (tools/xattn_stamps.py; no reference counterpart): same result, and the kernel stores 8 s_memtime
 * stamps per workgroup to `stamps` (caller-owned device memory, 8 * (M / 128) * slices 64-bit words) */
/* timing ablations of the dominant kernel (the stride-1 3x3 conv with the LDS-resident halo); results are WRONG by design
 * and Y is scratch: ablate 0 = the product kernel, 1 = no LDS-DMA waits, 2 = no LDS-DMA, 4 = no tap barrier either, 8 = no
 * fragment reads either (the bare MFMA stream: the rate the matrix pipe sustains at the clock the chip holds under load).
 * + 256 (with 0 or 8): the 4-wave layout of the kernel -- 128 x 80 outputs per wave, one wave per SIMD; with 0 it is a
 * CORRECT kernel, bit-identical to the product layout, measured 12 % slower (profiles/round3_notes.md) and kept for A/B.
 * Every mode but 0 exists ONLY in the SD_ABLATE build of these sources (libsdhip_ablate.so, a second library next to
 * libsdhip.so): the product library carries none of the ablation kernels and returns an error for them. */
int sd_op_conv3x3_ablate(void* stream, const void* X, const void* W, void* Y, int B, int Hin, int Win, int Cin, int Cout,
                         int ablate);
int sd_op_xattn_fused_stamps(void* stream, const void* X, const void* R, void* Y, const void* At, const void* Bw,
                             const float* bias, int M, int C, int rows_per_sample, int L, unsigned long long* stamps);

/* ---- fp8-e4m3 operand path (SD_DTYPE_FP8_E4M3), operator level ------------------------------------------------
 * X, W hold OCP e4m3 bytes; K / Cin count fp8 elements and are multiples of 128 (zero padded); wscale [N] fp32 is the
 * per-output-channel weight scale, xscale the static activation scale: C = (X_fp8 . W_fp8^T) * wscale[n] / xscale
 * + bias + bias2 + R.  epi = 1: GEGLU on interleaved W; with out_fp8 the result is stored as e4m3 bytes of
 * sat(out * oscale) (ldc in bytes) -- the input of the next fp8 GEMM. */
int sd_op_gemm_fp8(void* stream, const void* X, long long ldx, const void* W, const float* wscale, float xscale,
                   const float* bias, const void* R, long long ldr, void* C, long long ldc, int M, int N, int K, int epi,
                   int out_fp8, float oscale);
/* W is e4m3 [Cout][Cin/128][3*3][128] */
int sd_op_conv3x3_fp8(void* stream, const void* X, const void* W, const float* wscale, float xscale, const float* bias,
                      const float* bias2, const void* R, void* Y, int B, int Hin, int Win, int Cin, int Cout, int stride,
                      int upsample);
/* producers: GroupNorm(+SiLU) / LayerNorm writing e4m3 rows of Cpad = roundup(C, 128) bytes (pad zero), and a plain
 * bf16 -> e4m3 conversion */
int sd_op_groupnorm_fp8(void* stream, const void* x1, int C1, const void* x2, int C2, const float* gamma,
                        const float* beta, void* y, int B, int HW, int groups, float eps, int silu, int Cpad, float oscale);
int sd_op_layernorm_fp8(void* stream, const void* x, const float* gamma, const float* beta, void* y, int rows, int C,
                        int Cpad, float eps, float oscale);
int sd_op_quantize_fp8(void* stream, const void* x_bf16, void* y_fp8, long long rows, int C, int Cpad, float scale);
/* the measurement of sd_unet_calibrate_fp8: *out_code (a device word, zeroed here) = the largest magnitude code
 * (byte & 0x7f) among `nbytes` e4m3 bytes; codes 16-byte aligned, nbytes a multiple of 16 */
int sd_op_amax_e4m3(void* stream, const void* codes, long long nbytes, unsigned* out_code);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_H */
