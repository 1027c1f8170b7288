// libsdhip host side: parameter enumeration (the state_dict names of the seven handle kinds) and the weight packer.  Pure host
// code: it runs on a box without a GPU too.
#include "model.h"

#include <stdlib.h>

#include <chrono>
#include <thread>

namespace sdhip {

// ---------------------------------------------------------------------------------------------
// parameter enumeration (diffusers state_dict names)
// ---------------------------------------------------------------------------------------------
namespace {
struct Enum {
    sd_unet* u;
    void add(const std::string& n, std::vector<long long> shape) {
        ParamSpec p;
        p.name = n;
        p.shape = std::move(shape);
        u->pindex[n] = (int)u->params.size();
        u->params.push_back(std::move(p));
    }
    void resnet(const std::string& p, int cin, int cout, int temb) {      // temb 0: the AutoencoderKL's blocks (no time embedding)
        add(p + "norm1.weight", {cin});
        add(p + "norm1.bias", {cin});
        add(p + "conv1.weight", {cout, cin, 3, 3});
        add(p + "conv1.bias", {cout});
        if (temb) {
            add(p + "time_emb_proj.weight", {cout, temb});
            add(p + "time_emb_proj.bias", {cout});
        }
        add(p + "norm2.weight", {cout});
        add(p + "norm2.bias", {cout});
        add(p + "conv2.weight", {cout, cout, 3, 3});
        add(p + "conv2.bias", {cout});
        if (cin != cout) {
            add(p + "conv_shortcut.weight", {cout, cin, 1, 1});
            add(p + "conv_shortcut.bias", {cout});
        }
    }
    void transformer(const std::string& p, int c, int ctx) {
        add(p + "norm.weight", {c});
        add(p + "norm.bias", {c});
        add(p + "proj_in.weight", {c, c, 1, 1});
        add(p + "proj_in.bias", {c});
        const std::string t = p + "transformer_blocks.0.";
        for (int i = 1; i <= 3; ++i) {
            add(t + "norm" + std::to_string(i) + ".weight", {c});
            add(t + "norm" + std::to_string(i) + ".bias", {c});
        }
        add(t + "attn1.to_q.weight", {c, c});
        add(t + "attn1.to_k.weight", {c, c});
        add(t + "attn1.to_v.weight", {c, c});
        add(t + "attn1.to_out.0.weight", {c, c});
        add(t + "attn1.to_out.0.bias", {c});
        add(t + "attn2.to_q.weight", {c, c});
        add(t + "attn2.to_k.weight", {c, ctx});
        add(t + "attn2.to_v.weight", {c, ctx});
        add(t + "attn2.to_out.0.weight", {c, c});
        add(t + "attn2.to_out.0.bias", {c});
        if (u->cfg.ip_adapter_tokens > 0) {      // IPAdapterAttnProcessor2_0 of one adapter (diffusers' names)
            add(t + "attn2.processor.to_k_ip.0.weight", {c, ctx});
            add(t + "attn2.processor.to_v_ip.0.weight", {c, ctx});
        }
        add(t + "ff.net.0.proj.weight", {8 * c, c});
        add(t + "ff.net.0.proj.bias", {8 * c});
        add(t + "ff.net.2.weight", {c, 4 * c});
        add(t + "ff.net.2.bias", {c});
        add(p + "proj_out.weight", {c, c, 1, 1});
        add(p + "proj_out.bias", {c});
    }
    void vae_attention(const std::string& a, int top) {
        add(a + "group_norm.weight", {top}); add(a + "group_norm.bias", {top});
        for (const char* n : {"to_q", "to_k", "to_v", "to_out.0"}) {
            add(a + n + ".weight", {top, top});
            add(a + n + ".bias", {top});
        }
    }
    void clip_encoder_layer(const std::string& p, int H, int I) {      // (both CLIP towers)
        for (const char* n : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
            add(p + "self_attn." + n + ".weight", {H, H});
            add(p + "self_attn." + n + ".bias", {H});
        }
        add(p + "layer_norm1.weight", {H}); add(p + "layer_norm1.bias", {H});
        add(p + "mlp.fc1.weight", {I, H}); add(p + "mlp.fc1.bias", {I});
        add(p + "mlp.fc2.weight", {H, I}); add(p + "mlp.fc2.bias", {H});
        add(p + "layer_norm2.weight", {H}); add(p + "layer_norm2.bias", {H});
    }
};
}  // namespace

// ControlNetConditioningEmbedding (diffusers controlnet.py): conv_in 3 -> e0, blocks.2i e_i -> e_i, blocks.2i+1 e_i -> e_(i+1)
// with stride 2, conv_out e3 -> block_out_channels[0]; all 3x3, pad 1
int cond_embed_convs(const sd_unet* u, std::string names[8], int cin[8], int cout[8], int stride[8]) {
    const std::string p = "controlnet_cond_embedding.";
    const sd_unet_config& c = u->cfg;
    const int* e = u->cond_embed;
    names[0] = p + "conv_in."; cin[0] = 3; cout[0] = e[0]; stride[0] = 1;
    for (int i = 0; i < 3; ++i) {
        names[1 + 2 * i] = p + "blocks." + std::to_string(2 * i) + "."; cin[1 + 2 * i] = e[i]; cout[1 + 2 * i] = e[i]; stride[1 + 2 * i] = 1;
        names[2 + 2 * i] = p + "blocks." + std::to_string(2 * i + 1) + "."; cin[2 + 2 * i] = e[i]; cout[2 + 2 * i] = e[i + 1]; stride[2 + 2 * i] = 2;
    }
    names[7] = p + "conv_out."; cin[7] = e[3]; cout[7] = c.block_out_channels[0]; stride[7] = 1;
    return 8;
}

void enumerate_params(sd_unet* u) {
    const sd_unet_config& c = u->cfg;
    Enum e{u};
    const bool cnet = u->kind == 5;       // a ControlNet: the UNet's encoder half under the same names, then its own convs
    const int c0 = c.block_out_channels[0], temb = 4 * c0, nl = c.num_levels;
    e.add("time_embedding.linear_1.weight", {temb, c0});
    e.add("time_embedding.linear_1.bias", {temb});
    if (c.time_cond_proj_dim > 0) e.add("time_embedding.cond_proj.weight", {c0, c.time_cond_proj_dim});
    e.add("time_embedding.linear_2.weight", {temb, temb});
    e.add("time_embedding.linear_2.bias", {temb});
    e.add("conv_in.weight", {c0, c.in_channels, 3, 3});
    e.add("conv_in.bias", {c0});
    int ch = c0;
    std::vector<int> skip_ch{c0};
    for (int i = 0; i < nl; ++i) {
        const int co = c.block_out_channels[i];
        const std::string bp = "down_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block; ++j) {
            e.resnet(bp + "resnets." + std::to_string(j) + ".", ch, co, temb);
            ch = co;
            if (c.attn_levels[i]) e.transformer(bp + "attentions." + std::to_string(j) + ".", co, c.cross_attention_dim);
            skip_ch.push_back(co);
        }
        if (i < nl - 1) {
            e.add(bp + "downsamplers.0.conv.weight", {co, co, 3, 3});
            e.add(bp + "downsamplers.0.conv.bias", {co});
            skip_ch.push_back(co);
        }
    }
    e.resnet("mid_block.resnets.0.", ch, ch, temb);
    e.transformer("mid_block.attentions.0.", ch, c.cross_attention_dim);
    e.resnet("mid_block.resnets.1.", ch, ch, temb);
    if (cnet) {
        std::string names[8];
        int cin[8], cout[8], stride[8];
        cond_embed_convs(u, names, cin, cout, stride);
        for (int i = 0; i < 8; ++i) {
            e.add(names[i] + "weight", {cout[i], cin[i], 3, 3});
            e.add(names[i] + "bias", {cout[i]});
        }
        for (size_t i = 0; i < skip_ch.size(); ++i) {
            e.add("controlnet_down_blocks." + std::to_string(i) + ".weight", {skip_ch[i], skip_ch[i], 1, 1});
            e.add("controlnet_down_blocks." + std::to_string(i) + ".bias", {skip_ch[i]});
        }
        e.add("controlnet_mid_block.weight", {ch, ch, 1, 1});
        e.add("controlnet_mid_block.bias", {ch});
        return;
    }
    for (int i = 0; i < nl; ++i) {
        const int lev = nl - 1 - i, co = c.block_out_channels[lev];
        const std::string bp = "up_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            const int sc = skip_ch.back();
            skip_ch.pop_back();
            e.resnet(bp + "resnets." + std::to_string(j) + ".", ch + sc, co, temb);
            ch = co;
            if (c.attn_levels[lev]) e.transformer(bp + "attentions." + std::to_string(j) + ".", co, c.cross_attention_dim);
        }
        if (i < nl - 1) {
            e.add(bp + "upsamplers.0.conv.weight", {co, co, 3, 3});
            e.add(bp + "upsamplers.0.conv.bias", {co});
        }
    }
    e.add("conv_norm_out.weight", {c0});
    e.add("conv_norm_out.bias", {c0});
    e.add("conv_out.weight", {c.out_channels, c0, 3, 3});
    e.add("conv_out.bias", {c.out_channels});
    if (c.ip_adapter_tokens > 0) {      // ImageProjection of the IP-Adapter (diffusers: unet.encoder_hid_proj)
        const std::string p = "encoder_hid_proj.image_projection_layers.0.";
        e.add(p + "image_embeds.weight", {c.ip_adapter_tokens * c.cross_attention_dim, c.ip_adapter_embed_dim});
        e.add(p + "image_embeds.bias", {c.ip_adapter_tokens * c.cross_attention_dim});
        e.add(p + "norm.weight", {c.cross_attention_dim});
        e.add(p + "norm.bias", {c.cross_attention_dim});
    }
}

void enumerate_params_clip(sd_unet* u) {
    const sd_clip_config& c = u->clip;
    Enum e{u};
    const int H = c.hidden_size, I = c.intermediate_size;
    e.add("text_model.embeddings.token_embedding.weight", {c.vocab_size, H});
    e.add("text_model.embeddings.position_embedding.weight", {c.max_positions, H});
    for (int i = 0; i < c.num_layers; ++i) e.clip_encoder_layer(clip_layer(i), H, I);
    e.add("text_model.final_layer_norm.weight", {H});
    e.add("text_model.final_layer_norm.bias", {H});
    if (u->text_proj) e.add("text_projection.weight", {u->text_proj, H});
}

void enumerate_params_vit(sd_unet* u) {
    const sd_clip_vision_config& c = u->vis;
    Enum e{u};
    const int H = c.hidden_size, I = c.intermediate_size, G = c.image_size / c.patch_size;
    e.add("vision_model.embeddings.class_embedding", {H});
    e.add("vision_model.embeddings.patch_embedding.weight", {H, 3, c.patch_size, c.patch_size});
    e.add("vision_model.embeddings.position_embedding.weight", {G * G + 1, H});
    e.add("vision_model.pre_layrnorm.weight", {H}); e.add("vision_model.pre_layrnorm.bias", {H});
    for (int i = 0; i < c.num_layers; ++i) e.clip_encoder_layer(vit_layer(i), H, I);
    e.add("vision_model.post_layernorm.weight", {H}); e.add("vision_model.post_layernorm.bias", {H});
    e.add("visual_projection.weight", {c.projection_dim, H});
}

// ImageReward: BLIP ViT (timm names), BLIP text encoder (BERT names with crossattention), the reward head's five Linears
void enumerate_params_image_reward(sd_unet* u) {
    const sd_image_reward_config& c = u->ir;
    Enum e{u};
    auto lin = [&](const std::string& n, int out, int in) { e.add(n + ".weight", {out, in}); e.add(n + ".bias", {out}); };
    auto norm = [&](const std::string& n, int h) { e.add(n + ".weight", {h}); e.add(n + ".bias", {h}); };
    const int VH = c.vision_hidden_size, VI = c.vision_intermediate_size, G = c.image_size / c.patch_size;
    e.add("visual_encoder.cls_token", {VH});
    e.add("visual_encoder.pos_embed", {G * G + 1, VH});
    e.add("visual_encoder.patch_embed.proj.weight", {VH, 3, c.patch_size, c.patch_size});
    e.add("visual_encoder.patch_embed.proj.bias", {VH});
    for (int i = 0; i < c.vision_num_layers; ++i) {
        const std::string p = blip_block(i);
        norm(p + "norm1", VH); lin(p + "attn.qkv", 3 * VH, VH); lin(p + "attn.proj", VH, VH);
        norm(p + "norm2", VH); lin(p + "mlp.fc1", VI, VH); lin(p + "mlp.fc2", VH, VI);
    }
    norm("visual_encoder.norm", VH);
    const int H = c.hidden_size, I = c.intermediate_size;
    e.add("text_encoder.embeddings.word_embeddings.weight", {c.vocab_size, H});
    e.add("text_encoder.embeddings.position_embeddings.weight", {c.max_positions, H});
    norm("text_encoder.embeddings.LayerNorm", H);
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = blip_text_layer(i);
        for (const char* n : {"query", "key", "value"}) lin(p + "attention.self." + n, H, H);
        lin(p + "attention.output.dense", H, H); norm(p + "attention.output.LayerNorm", H);
        lin(p + "crossattention.self.query", H, H);
        lin(p + "crossattention.self.key", H, VH); lin(p + "crossattention.self.value", H, VH);
        lin(p + "crossattention.output.dense", H, H); norm(p + "crossattention.output.LayerNorm", H);
        lin(p + "intermediate.dense", I, H); lin(p + "output.dense", H, I); norm(p + "output.LayerNorm", H);
    }
    int in = H;
    for (int k = 0; k < 5; ++k) {
        lin("mlp.layers." + std::to_string(kRewardHeadLayers[k]), kRewardHeadDims[k], in);
        in = kRewardHeadDims[k];
    }
}

// AutoencoderKL decoder (diffusers names): post_quant_conv + decoder.*  
void enumerate_params_vae(sd_unet* u) {
    const sd_unet_config& c = u->cfg;
    Enum e{u};
    const int nl = c.num_levels, top = c.block_out_channels[nl - 1];
    auto resnet = [&](const std::string& p, int cin, int cout) { e.resnet(p, cin, cout, 0); };
    e.add("post_quant_conv.weight", {c.in_channels, c.in_channels, 1, 1});
    e.add("post_quant_conv.bias", {c.in_channels});
    e.add("decoder.conv_in.weight", {top, c.in_channels, 3, 3});
    e.add("decoder.conv_in.bias", {top});
    resnet("decoder.mid_block.resnets.0.", top, top);
    e.vae_attention("decoder.mid_block.attentions.0.", top);
    resnet("decoder.mid_block.resnets.1.", top, top);
    int ch = top;
    for (int i = 0; i < nl; ++i) {
        const int co = c.block_out_channels[nl - 1 - i];
        const std::string bp = "decoder.up_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            resnet(bp + "resnets." + std::to_string(j) + ".", ch, co);
            ch = co;
        }
        if (i < nl - 1) {
            e.add(bp + "upsamplers.0.conv.weight", {co, co, 3, 3});
            e.add(bp + "upsamplers.0.conv.bias", {co});
        }
    }
    e.add("decoder.conv_norm_out.weight", {ch}); e.add("decoder.conv_norm_out.bias", {ch});
    e.add("decoder.conv_out.weight", {c.out_channels, ch, 3, 3});
    e.add("decoder.conv_out.bias", {c.out_channels});
}

// AutoencoderKL encoder (diffusers 0.32.1 names): encoder.* + quant_conv.  cfg.out_channels = image channels (3),
// cfg.in_channels = latent channels (4): the moments carry 2 * in_channels = 8.
void enumerate_params_vae_encoder(sd_unet* u) {
    const sd_unet_config& c = u->cfg;
    Enum e{u};
    const int nl = c.num_levels, top = c.block_out_channels[nl - 1], c0 = c.block_out_channels[0], zc = 2 * c.in_channels;
    auto resnet = [&](const std::string& p, int cin, int cout) { e.resnet(p, cin, cout, 0); };
    e.add("encoder.conv_in.weight", {c0, c.out_channels, 3, 3});
    e.add("encoder.conv_in.bias", {c0});
    int ch = c0;
    for (int i = 0; i < nl; ++i) {
        const int co = c.block_out_channels[i];
        const std::string bp = "encoder.down_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block; ++j) {
            resnet(bp + "resnets." + std::to_string(j) + ".", ch, co);
            ch = co;
        }
        if (i < nl - 1) {
            e.add(bp + "downsamplers.0.conv.weight", {co, co, 3, 3});
            e.add(bp + "downsamplers.0.conv.bias", {co});
        }
    }
    resnet("encoder.mid_block.resnets.0.", top, top);
    e.vae_attention("encoder.mid_block.attentions.0.", top);
    resnet("encoder.mid_block.resnets.1.", top, top);
    e.add("encoder.conv_norm_out.weight", {top}); e.add("encoder.conv_norm_out.bias", {top});
    e.add("encoder.conv_out.weight", {zc, top, 3, 3});
    e.add("encoder.conv_out.bias", {zc});
    e.add("quant_conv.weight", {zc, zc, 1, 1});
    e.add("quant_conv.bias", {zc});
}

// ---------------------------------------------------------------------------------------------
// weight packing (host)
// ---------------------------------------------------------------------------------------------
namespace {

inline unsigned short f32_to_bf16_host(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    u = u + 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// f32 -> OCP e4m3fn byte, round to nearest even, saturating at +-448 (no infinities; 0x7f = NaN)
inline unsigned char f32_to_e4m3_host(float f) {
    if (f != f) return 0x7f;
    const unsigned char sign = std::signbit(f) ? 0x80 : 0;
    const float a = fabsf(f);
    if (a >= 448.f) return sign | 0x7e;
    if (a < 0.015625f) {                                  // subnormal range: multiples of 2^-9
        const int q = (int)nearbyintf(a * 512.f);         // 0..8 (8 = the smallest normal)
        return sign | (unsigned char)q;
    }
    int e;
    const float m = frexpf(a, &e);                        // a = m * 2^e, m in [0.5, 1)
    int ex = e - 1;
    int q = (int)nearbyintf((m * 2.f - 1.f) * 8.f);       // 0..8
    if (q == 8) { q = 0; ++ex; }
    const int biased = ex + 7;
    if (biased > 15 || (biased == 15 && q == 7)) return sign | 0x7e;
    return sign | (unsigned char)((biased << 3) | q);
}

// host-side packing runs over up to 8 threads (0.86 G parameters: the single-threaded pack took ~20 s) -- of this RANK's
// share of the host cores: under a launcher every rank of the node packs its own replica at the same time
// (LOCAL_WORLD_SIZE ranks; 8 ranks x 8 threads on shared cores was round 3's start-up), SD_AMD_PACK_THREADS overrides
static int pack_threads() {
    static const int nt = [] {
        if (const char* e = getenv("SD_AMD_PACK_THREADS")) return std::max(1, std::min(64, atoi(e)));
        int ranks = 1;
        if (const char* e = getenv("LOCAL_WORLD_SIZE")) ranks = std::max(1, atoi(e));
        else if (const char* e2 = getenv("WORLD_SIZE")) ranks = std::max(1, atoi(e2));
        const int cores = (int)std::max(1u, std::thread::hardware_concurrency());
        return std::max(1, std::min(8, cores / ranks));
    }();
    return nt;
}
template <class F>
static void parallel_for(long n, F&& body) {
    const int nt = (int)std::max(1l, std::min<long>(pack_threads(), n));
    if (nt == 1) { body(0l, n); return; }
    std::vector<std::thread> th;
    const long per = (n + nt - 1) / nt;
    for (int t = 1; t < nt; ++t) th.emplace_back([&, t] { body(std::min(n, t * per), std::min(n, (t + 1) * per)); });
    body(0l, std::min(n, per));
    for (auto& x : th) x.join();
}
// dst[i][k] += a[i] * row[k] for NB rows (the inner kernel of Packer::ff_out_merge); the AVX2 + FMA clone is picked at run
// time (the library is built for the generic x86-64 baseline)
template <int NB>
__attribute__((target("avx2,fma"))) static void axpy_rows_avx2(float* const* dst, const float* a, const float* __restrict__ row, int K) {
    for (int i = 0; i < NB; ++i) {
        float* __restrict__ d = dst[i];
        const float ai = a[i];
#pragma clang loop vectorize(enable) interleave(enable)
        for (int k = 0; k < K; ++k) d[k] += ai * row[k];
    }
}
template <int NB>
static void axpy_rows_base(float* const* dst, const float* a, const float* __restrict__ row, int K) {
    for (int i = 0; i < NB; ++i) {
        float* __restrict__ d = dst[i];
        const float ai = a[i];
#pragma clang loop vectorize(enable) interleave(enable)
        for (int k = 0; k < K; ++k) d[k] += ai * row[k];
    }
}

double g_alloc_s = 0;
struct Packer {
    sd_unet* u;
    // rows [N][K] fp32 -> e4m3 [N][Kp] (K zero padded to Kp) + one fp32 scale per row (amax / 448)
    void quant_rows(const std::string& key, const float* w, int N, int K, int Kp) {
        size_t off = alloc(key + ".fp8", (size_t)N * Kp);
        size_t soff = alloc(key + ".scale", (size_t)N * 4);
        unsigned char* o = u->hblob.data() + off;
        float* sc = (float*)(u->hblob.data() + soff);
        for (int n = 0; n < N; ++n) {
            float amax = 0.f;
            for (int k = 0; k < K; ++k) amax = std::max(amax, fabsf(w[(size_t)n * K + k]));
            const float scale = amax > 0.f ? amax / 448.f : 1.f;
            sc[n] = scale;
            const float inv = 1.f / scale;
            for (int k = 0; k < K; ++k) o[(size_t)n * Kp + k] = f32_to_e4m3_host(w[(size_t)n * K + k] * inv);
            for (int k = K; k < Kp; ++k) o[(size_t)n * Kp + k] = 0;
        }
    }
    void fp8_same(const std::string& n, int N, int K) { quant_rows(n, P(n).data(), N, K, (K + 127) / 128 * 128); }
    // scale0: factor on the rows of the FIRST matrix (the self-attention's to_q carries softmax scale * log2 e, see qscale())
    void fp8_concat_rows(const std::string& key, const std::vector<std::string>& names, int K, float scale0 = 1.f) {
        std::vector<float> all;
        for (auto& n : names) all.insert(all.end(), P(n).begin(), P(n).end());
        for (size_t i = 0; i < P(names[0]).size(); ++i) all[i] *= scale0;
        quant_rows(key, all.data(), (int)(all.size() / K), K, (K + 127) / 128 * 128);
    }
    // OIHW -> e4m3 [O][Ip/128][tap][128] (Ip = I padded to 128) + per-output-channel scale
    void conv3_fp8(const std::string& n, int O, int I) {
        const auto& d = P(n);
        const int Ip = (I + 127) / 128 * 128;
        size_t off = alloc(n + ".fp8", (size_t)O * 9 * Ip);
        size_t soff = alloc(n + ".scale", (size_t)O * 4);
        unsigned char* o = u->hblob.data() + off;
        float* sc = (float*)(u->hblob.data() + soff);
        memset(o, 0, (size_t)O * 9 * Ip);
        for (int oc = 0; oc < O; ++oc) {
            float amax = 0.f;
            for (int k = 0; k < I * 9; ++k) amax = std::max(amax, fabsf(d[(size_t)oc * I * 9 + k]));
            const float scale = amax > 0.f ? amax / 448.f : 1.f, inv = 1.f / scale;
            sc[oc] = scale;
            for (int ic = 0; ic < I; ++ic)
                for (int t = 0; t < 9; ++t)
                    o[(((size_t)oc * (Ip / 128) + ic / 128) * 9 + t) * 128 + (ic % 128)] =
                        f32_to_e4m3_host(d[((size_t)oc * I + ic) * 9 + t] * inv);
        }
    }
    const std::vector<float>& P(const std::string& n) { return u->params[u->pindex.at(n)].data; }
    size_t alloc(const std::string& key, size_t bytes) {
        size_t off = (u->hblob.size() + 255) / 256 * 256;
        const auto t0 = std::chrono::steady_clock::now();
        u->hblob.resize(off + bytes);
        g_alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        u->woff[key] = off;
        return off;
    }
    void f32(const std::string& n) {
        const auto& d = P(n);
        size_t off = alloc(n, d.size() * 4);
        memcpy(u->hblob.data() + off, d.data(), d.size() * 4);
    }
    void bf16_same(const std::string& n) {
        const auto& d = P(n);
        size_t off = alloc(n, d.size() * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        const float* src = d.data();
        parallel_for((long)d.size(), [=](long b, long e) { for (long i = b; i < e; ++i) o[i] = f32_to_bf16_host(src[i]); });
    }
    // OIHW -> [O][I/64][tap][64]: K index = (64-channel slice, tap, channel) as the conv kernel walks it
    void conv3(const std::string& n, int O, int I) {
        const auto& d = P(n);
        size_t off = alloc(n, d.size() * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        const float* src = d.data();
        parallel_for(O, [=](long b, long e) {
            for (long oc = b; oc < e; ++oc)
                for (int ic = 0; ic < I; ++ic)
                    for (int t = 0; t < 9; ++t)
                        o[(((size_t)oc * (I / 64) + ic / 64) * 9 + t) * 64 + (ic % 64)] =
                            f32_to_bf16_host(src[((size_t)oc * I + ic) * 9 + t]);
        });
    }
    // nearest-2x upsample + 3x3 conv == four 2x2 convs on the low-res input (GemmArgs::subpix): phase (py, px) of the output
    // reads low-res rows {y - 1 + py, y + py}; the 3x3 taps that land on the same low-res pixel are summed (in fp32):
    //   py = 0: row 0 <- tap row 0, row 1 <- tap rows 1 + 2;   py = 1: row 0 <- tap rows 0 + 1, row 1 <- tap row 2
    // OIHW -> [4 phases][O][I/64][4 taps (dy, dx)][64]
    void conv3_subpixel(const std::string& n, int O, int I) {
        const auto& d = P(n);
        const size_t per = (size_t)O * I * 4;
        size_t off = alloc(n + ".sub", 4 * per * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        auto lo = [](int p, int t) { return p == 0 ? (t == 0 ? 0 : 1) : (t == 0 ? 0 : 2); };      // first 3x3 tap of 2x2 tap t
        auto hi = [](int p, int t) { return p == 0 ? (t == 0 ? 0 : 2) : (t == 0 ? 1 : 2); };      // last one
        for (int ph = 0; ph < 4; ++ph)
            for (int oc = 0; oc < O; ++oc)
                for (int ic = 0; ic < I; ++ic)
                    for (int t = 0; t < 4; ++t) {
                        const int py = ph >> 1, px = ph & 1, dy = t >> 1, dx = t & 1;
                        float acc = 0.f;
                        for (int ty = lo(py, dy); ty <= hi(py, dy); ++ty)
                            for (int tx = lo(px, dx); tx <= hi(px, dx); ++tx) acc += d[((size_t)oc * I + ic) * 9 + ty * 3 + tx];
                        o[ph * per + (((size_t)oc * (I / 64) + ic / 64) * 4 + t) * 64 + (ic % 64)] = f32_to_bf16_host(acc);
                    }
    }
    void conv3_ohwi(const std::string& n, int O, int I) {  // OIHW -> [O][tap][I] (conv_out kernel)
        const auto& d = P(n);
        size_t off = alloc(n, d.size() * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        for (int oc = 0; oc < O; ++oc)
            for (int ic = 0; ic < I; ++ic)
                for (int t = 0; t < 9; ++t)
                    o[((size_t)oc * 9 + t) * I + ic] = f32_to_bf16_host(d[((size_t)oc * I + ic) * 9 + t]);
    }
    void concat_rows(const std::string& key, const std::vector<std::string>& names, float scale0 = 1.f) {
        size_t total = 0;
        for (auto& n : names) total += P(n).size();
        size_t off = alloc(key, total * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        for (auto& n : names)
            for (float v : P(n)) *o++ = f32_to_bf16_host(&n == &names[0] ? v * scale0 : v);
    }
    // LayerNorm folded into the GEMM that consumes it (GemmArgs::ln_rs): rows [N][K] fp32 -> key.ln = bf16(W * gamma),
    // key.c1[n] = sum_k of the ROUNDED row (what the kernel's raw sums contain per unit of the row mean),
    // key.c2[n] = sum_k W[n][k] beta[k] + bias[n]
    void ln_fold(const std::string& key, const float* w, int N, int K, const std::vector<float>& gamma,
                 const std::vector<float>& beta, const float* bias) {
        const size_t woff = alloc(key + ".ln", (size_t)N * K * 2);
        const size_t c1off = alloc(key + ".c1", (size_t)N * 4);
        const size_t c2off = alloc(key + ".c2", (size_t)N * 4);
        unsigned short* o = (unsigned short*)(u->hblob.data() + woff);
        float* c1 = (float*)(u->hblob.data() + c1off);
        float* c2 = (float*)(u->hblob.data() + c2off);
        for (int n = 0; n < N; ++n) {
            double s1 = 0.0, s2 = bias ? (double)bias[n] : 0.0;
            for (int k = 0; k < K; ++k) {
                const float wv = w[(size_t)n * K + k];
                const unsigned short r = f32_to_bf16_host(wv * gamma[k]);
                o[(size_t)n * K + k] = r;
                const unsigned bits = (unsigned)r << 16;
                float rf;
                memcpy(&rf, &bits, 4);
                s1 += rf;
                s2 += (double)wv * beta[k];
            }
            c1[n] = (float)s1;
            c2[n] = (float)s2;
        }
    }
    // ff.net.2 and proj_out are two linear maps with only a residual add between them:
    //   out = (ff W2^T + b2 + h2) Wpo^T + bpo + x  =  [ff | h2] . [Wpo W2 | Wpo]^T + (Wpo b2 + bpo) + x
    // -> ONE GEMM with a two-segment K (4C + C) instead of two launches and the h3 round trip.  The product Wpo W2 is
    // formed here once, in fp32 from the fp32 parameters, and rounded to bf16 like every other weight.
    void ff_out_merge(const std::string& p, const std::string& t, int C) {
        const auto& w2 = P(t + "ff.net.2.weight");      // [C][4C]
        const auto& b2 = P(t + "ff.net.2.bias");
        const auto& wpo = P(p + "proj_out.weight");     // [C][C]
        const auto& bpo = P(p + "proj_out.bias");
        const int K4 = 4 * C, KT = 5 * C;
        std::vector<float> prod((size_t)C * K4, 0.f);
        const int nthreads = pack_threads();
        const bool avx2 = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
        auto work = [&](int tid) {
            constexpr int NB = 8;                        // output rows per pass over W2 (C is a multiple of 8)
            for (int n0 = tid * NB; n0 + NB <= C; n0 += nthreads * NB) {
                float* dst[NB];
                float a[NB];
                for (int i = 0; i < NB; ++i) dst[i] = &prod[(size_t)(n0 + i) * K4];
                for (int c = 0; c < C; ++c) {
                    for (int i = 0; i < NB; ++i) a[i] = wpo[(size_t)(n0 + i) * C + c];
                    if (avx2) axpy_rows_avx2<NB>(dst, a, &w2[(size_t)c * K4], K4);
                    else axpy_rows_base<NB>(dst, a, &w2[(size_t)c * K4], K4);
                }
            }
        };
        std::vector<std::thread> th;
        for (int i = 1; i < nthreads; ++i) th.emplace_back(work, i);
        work(0);
        for (auto& x : th) x.join();
        const size_t woff = alloc(p + "ff_out.weight", (size_t)C * KT * 2);
        const size_t boff = alloc(p + "ff_out.bias", (size_t)C * 4);
        unsigned short* o = (unsigned short*)(u->hblob.data() + woff);
        float* bo = (float*)(u->hblob.data() + boff);
        for (int n = 0; n < C; ++n) {
            for (int k = 0; k < K4; ++k) o[(size_t)n * KT + k] = f32_to_bf16_host(prod[(size_t)n * K4 + k]);
            for (int c = 0; c < C; ++c) o[(size_t)n * KT + K4 + c] = f32_to_bf16_host(wpo[(size_t)n * C + c]);
            double acc = bpo[n];
            for (int c = 0; c < C; ++c) acc += (double)wpo[(size_t)n * C + c] * b2[c];
            bo[n] = (float)acc;
        }
    }
    void geglu(const std::string& t, int C) {  // rows: every 32 = [16 value | 16 gate]
        const auto& w = P(t + "ff.net.0.proj.weight");
        const auto& b = P(t + "ff.net.0.proj.bias");
        const int H = 4 * C;
        std::vector<float> pw((size_t)2 * H * C), pb(2 * H);      // rows and biases in the packed order
        for (int r = 0; r < 2 * H; ++r) {
            const int grp = r / 32, within = r % 32;
            const int src = within < 16 ? grp * 16 + within : H + grp * 16 + (within - 16);
            memcpy(&pw[(size_t)r * C], &w[(size_t)src * C], (size_t)C * 4);
            pb[r] = b[src];
        }
        const size_t boff = alloc(t + "ff.geglu.bias", pb.size() * 4);
        memcpy(u->hblob.data() + boff, pb.data(), pb.size() * 4);
        if (u->fp8) { quant_rows(t + "ff.geglu.weight", pw.data(), 2 * H, C, (C + 127) / 128 * 128); return; }
        const size_t woff = alloc(t + "ff.geglu.weight", pw.size() * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + woff);
        for (size_t i = 0; i < pw.size(); ++i) o[i] = f32_to_bf16_host(pw[i]);
        // norm3 folded in: same packed row order
        ln_fold(t + "ff.geglu.weight", pw.data(), 2 * H, C, P(t + "norm3.weight"), P(t + "norm3.bias"), pb.data());
    }
    void conv_in(const std::string& n, int O, int I) {      // [O][I][3][3] -> Wt[k = ic*9+tap][O] fp32 (the entry convs run in fp32), + bias
        const auto& d = P(n + "weight");
        size_t off = alloc(n + "weight", d.size() * 4);
        float* o = (float*)(u->hblob.data() + off);
        for (int oc = 0; oc < O; ++oc)
            for (int k = 0; k < I * 9; ++k) o[(size_t)k * O + oc] = d[(size_t)oc * I * 9 + k];
        f32(n + "bias");
    }
    void vae_attention(const std::string& a, int top) {      // q | k fused (S = Q K^T reads both from one tensor), v and to_out plain
        f32(a + "group_norm.weight"); f32(a + "group_norm.bias");
        concat_rows(a + "qk.weight", {a + "to_q.weight", a + "to_k.weight"});
        size_t off = alloc(a + "qk.bias", (size_t)2 * top * 4);
        float* o = (float*)(u->hblob.data() + off);
        for (const char* n : {"to_q.bias", "to_k.bias"})
            for (float v : P(a + n)) *o++ = v;
        bf16_same(a + "to_v.weight"); f32(a + "to_v.bias");
        bf16_same(a + "to_out.0.weight"); f32(a + "to_out.0.bias");
    }
    void resnet(const std::string& p, int cin, int cout) {
        f32(p + "norm1.weight"); f32(p + "norm1.bias");
        f32(p + "conv1.bias");
        f32(p + "norm2.weight"); f32(p + "norm2.bias");
        f32(p + "conv2.bias");
        if (u->fp8) { conv3_fp8(p + "conv1.weight", cout, cin); conv3_fp8(p + "conv2.weight", cout, cout); }
        else { conv3(p + "conv1.weight", cout, cin); conv3(p + "conv2.weight", cout, cout); }
        if (cin != cout) {
            bf16_same(p + "conv_shortcut.weight"); f32(p + "conv_shortcut.bias");
            // conv2 with the shortcut folded in (Builder::resnet) adds ONE vector: the two biases summed in fp32
            const auto& b2 = P(p + "conv2.bias");
            const auto& bs = P(p + "conv_shortcut.bias");
            const size_t off = alloc(p + "conv2.bias+shortcut", b2.size() * 4);
            float* o = (float*)(u->hblob.data() + off);
            for (size_t i = 0; i < b2.size(); ++i) o[i] = b2[i] + bs[i];
        }
    }
    void transformer(const std::string& p, int c) {
        f32(p + "norm.weight"); f32(p + "norm.bias");
        f32(p + "proj_in.bias");
        const std::string t = p + "transformer_blocks.0.";
        for (int i = 1; i <= 3; ++i) { f32(t + "norm" + std::to_string(i) + ".weight"); f32(t + "norm" + std::to_string(i) + ".bias"); }
        // The self-attention's softmax scale and the exp -> exp2 factor live in W_q (fp32, before the one rounding every weight
        // gets): S = (c W_q x) . k comes out of the attention kernels' QK^T product in exp2 units (AttnArgs::q_prescaled)
        const float qs = 1.4426950408889634f / sqrtf((float)(c / block_heads(u->cfg, p)));
        if (u->fp8) {
            fp8_same(p + "proj_in.weight", c, c);
            fp8_concat_rows(t + "attn1.qkv.weight", {t + "attn1.to_q.weight", t + "attn1.to_k.weight", t + "attn1.to_v.weight"}, c, qs);
            fp8_same(t + "ff.net.2.weight", c, 4 * c);
        } else {
            bf16_same(p + "proj_in.weight");
            concat_rows(t + "attn1.qkv.weight", {t + "attn1.to_q.weight", t + "attn1.to_k.weight", t + "attn1.to_v.weight"}, qs);
            {   // norm1 folded into the q|k|v projection
                std::vector<float> all;
                for (const char* n : {"attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight"})
                    all.insert(all.end(), P(t + n).begin(), P(t + n).end());
                for (size_t i = 0; i < (size_t)c * c; ++i) all[i] *= qs;
                ln_fold(t + "attn1.qkv.weight", all.data(), 3 * c, c, P(t + "norm1.weight"), P(t + "norm1.bias"), nullptr);
            }
            bf16_same(t + "ff.net.2.weight");
        }
        bf16_same(t + "attn1.to_out.0.weight"); f32(t + "attn1.to_out.0.bias");
        bf16_same(t + "attn2.to_q.weight");
        {   // to_q transposed ([in][out]): the W operand of A^T = (scale K_h) . W_q,h of the folded cross-attention
            const auto& d = P(t + "attn2.to_q.weight");
            size_t off = alloc(t + "attn2.to_q.weight.T", d.size() * 2);
            unsigned short* o = (unsigned short*)(u->hblob.data() + off);
            for (int r = 0; r < c; ++r)
                for (int k = 0; k < c; ++k) o[(size_t)r * c + k] = f32_to_bf16_host(d[(size_t)k * c + r]);
        }
        if (!u->fp8) {
            // norm2 folded into the fused cross-attention (XattnArgs::ln_rs): A^T = (scale K_h) . W with
            //   W[c][j] = W_q[j][c] gamma[c] - (1 / C) sum_c' W_q[j][c'] gamma[c']      (rows c of the ".T" layout, CENTRED over c:
            //   sum_c (x_c - mean) w_c = sum_c x_c (w_c - mean_c w), so the kernel never needs the row mean), and
            //   u[j] = sum_c W_q[j][c] beta[c]: the beta term of key slot n is  (scale K_h[n]) . u  (set_context, fp32)
            const auto& d = P(t + "attn2.to_q.weight");
            const auto& gm = P(t + "norm2.weight");
            const auto& bt = P(t + "norm2.bias");
            size_t off = alloc(t + "attn2.to_q.weight.T.ln", d.size() * 2);
            size_t uoff = alloc(t + "attn2.to_q.lnu", (size_t)c * 4);
            size_t ooff = alloc(t + "attn2.to_q.ones", (size_t)c * 4);      // (x of the GEMV that sums the rounded rows of A^T: c1)
            for (int j = 0; j < c; ++j) ((float*)(u->hblob.data() + ooff))[j] = 1.0f;
            unsigned short* o = (unsigned short*)(u->hblob.data() + off);
            float* uu = (float*)(u->hblob.data() + uoff);
            for (int j = 0; j < c; ++j) {
                double m = 0.0, ub = 0.0;
                for (int cc = 0; cc < c; ++cc) {
                    m += (double)d[(size_t)j * c + cc] * gm[cc];
                    ub += (double)d[(size_t)j * c + cc] * bt[cc];
                }
                m /= c;
                uu[j] = (float)ub;
                for (int cc = 0; cc < c; ++cc) o[(size_t)cc * c + j] = f32_to_bf16_host((float)((double)d[(size_t)j * c + cc] * gm[cc] - m));
            }
        }
        if (!u->fp8)      // ... and into the plain to_q GEMM of the levels that run the 77-key flash kernel (the 8x8 level at UNet batch 16)
            ln_fold(t + "attn2.to_q.weight", P(t + "attn2.to_q.weight").data(), c, c, P(t + "norm2.weight"), P(t + "norm2.bias"), nullptr);
        concat_rows(t + "attn2.kv.weight", {t + "attn2.to_k.weight", t + "attn2.to_v.weight"});
        bf16_same(t + "attn2.to_out.0.weight"); f32(t + "attn2.to_out.0.bias");
        if (u->cfg.ip_adapter_tokens > 0)      // to_k_ip | to_v_ip as one projection of the image tokens, like attn2.kv
            concat_rows(t + "attn2.kv_ip.weight", {t + "attn2.processor.to_k_ip.0.weight", t + "attn2.processor.to_v_ip.0.weight"});
        geglu(t, c);
        f32(t + "ff.net.2.bias");
        bf16_same(p + "proj_out.weight"); f32(p + "proj_out.bias");
        if (!u->fp8) ff_out_merge(p, t, c);
    }
};

// walks the architecture once; F gets (kind, prefix, cin, cout/c) callbacks in forward order
template <class FR, class FT>
void walk_blocks(const sd_unet_config& c, FR&& on_resnet, FT&& on_transformer, bool up = true) {
    const int nl = c.num_levels;
    int ch = c.block_out_channels[0];
    std::vector<int> skip_ch{ch};
    for (int i = 0; i < nl; ++i) {
        const int co = c.block_out_channels[i];
        const std::string bp = "down_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block; ++j) {
            on_resnet(bp + "resnets." + std::to_string(j) + ".", ch, co);
            ch = co;
            if (c.attn_levels[i]) on_transformer(bp + "attentions." + std::to_string(j) + ".", co);
            skip_ch.push_back(co);
        }
        if (i < nl - 1) skip_ch.push_back(co);
    }
    on_resnet("mid_block.resnets.0.", ch, ch);
    on_transformer("mid_block.attentions.0.", ch);
    on_resnet("mid_block.resnets.1.", ch, ch);
    if (!up) return;       // (a ControlNet ends here)
    for (int i = 0; i < nl; ++i) {
        const int lev = nl - 1 - i, co = c.block_out_channels[lev];
        const std::string bp = "up_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            const int sc = skip_ch.back();
            skip_ch.pop_back();
            on_resnet(bp + "resnets." + std::to_string(j) + ".", ch + sc, co);
            ch = co;
            if (c.attn_levels[lev]) on_transformer(bp + "attentions." + std::to_string(j) + ".", co);
        }
    }
}

int pack_vae(sd_unet* u) {
    const sd_unet_config& c = u->cfg;
    Packer pk{u};
    const int nl = c.num_levels, top = c.block_out_channels[nl - 1];
    pk.f32("post_quant_conv.weight"); pk.f32("post_quant_conv.bias");
    pk.conv_in("decoder.conv_in.", top, c.in_channels);
    pk.resnet("decoder.mid_block.resnets.0.", top, top);
    pk.vae_attention("decoder.mid_block.attentions.0.", top);
    pk.resnet("decoder.mid_block.resnets.1.", top, top);
    int ch = top;
    for (int i = 0; i < nl; ++i) {
        const int co = c.block_out_channels[nl - 1 - i];
        const std::string bp = "decoder.up_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            pk.resnet(bp + "resnets." + std::to_string(j) + ".", ch, co);
            ch = co;
        }
        if (i < nl - 1) { pk.conv3(bp + "upsamplers.0.conv.weight", co, co); pk.f32(bp + "upsamplers.0.conv.bias"); }
    }
    pk.f32("decoder.conv_norm_out.weight"); pk.f32("decoder.conv_norm_out.bias");
    pk.conv3_ohwi("decoder.conv_out.weight", c.out_channels, ch); pk.f32("decoder.conv_out.bias");
    return 0;
}

int pack_vae_encoder(sd_unet* u) {
    const sd_unet_config& c = u->cfg;
    Packer pk{u};
    const int nl = c.num_levels, top = c.block_out_channels[nl - 1], c0 = c.block_out_channels[0];
    pk.conv_in("encoder.conv_in.", c0, c.out_channels);      // (on the fp32 image)
    int ch = c0;
    for (int i = 0; i < nl; ++i) {
        const int co = c.block_out_channels[i];
        const std::string bp = "encoder.down_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < c.layers_per_block; ++j) {
            pk.resnet(bp + "resnets." + std::to_string(j) + ".", ch, co);
            ch = co;
        }
        if (i < nl - 1) { pk.conv3(bp + "downsamplers.0.conv.weight", co, co); pk.f32(bp + "downsamplers.0.conv.bias"); }
    }
    pk.resnet("encoder.mid_block.resnets.0.", top, top);
    pk.vae_attention("encoder.mid_block.attentions.0.", top);
    pk.resnet("encoder.mid_block.resnets.1.", top, top);
    pk.f32("encoder.conv_norm_out.weight"); pk.f32("encoder.conv_norm_out.bias");
    pk.conv3_ohwi("encoder.conv_out.weight", 2 * c.in_channels, top); pk.f32("encoder.conv_out.bias");
    pk.f32("quant_conv.weight"); pk.f32("quant_conv.bias");       // applied in fp32 by the exit kernel
    return 0;
}

// the encoder layers of both CLIP towers: fused q | k | v rows and biases, bf16 GEMM weights, fp32 vectors
void pack_clip_layer(Packer& pk, const std::string& p, int H) {
    const std::string a = p + "self_attn.";
    pk.concat_rows(a + "qkv.weight", {a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight"});
    {
        size_t off = pk.alloc(a + "qkv.bias", (size_t)3 * H * 4);
        float* o = (float*)(pk.u->hblob.data() + off);
        for (const char* n : {"q_proj.bias", "k_proj.bias", "v_proj.bias"})
            for (float v : pk.P(a + n)) *o++ = v;
    }
    pk.bf16_same(a + "out_proj.weight"); pk.f32(a + "out_proj.bias");
    pk.f32(p + "layer_norm1.weight"); pk.f32(p + "layer_norm1.bias");
    pk.bf16_same(p + "mlp.fc1.weight"); pk.f32(p + "mlp.fc1.bias");
    pk.bf16_same(p + "mlp.fc2.weight"); pk.f32(p + "mlp.fc2.bias");
    pk.f32(p + "layer_norm2.weight"); pk.f32(p + "layer_norm2.bias");
}

int pack_clip(sd_unet* u) {
    const sd_clip_config& c = u->clip;
    Packer pk{u};
    pk.bf16_same("text_model.embeddings.token_embedding.weight");
    pk.bf16_same("text_model.embeddings.position_embedding.weight");
    for (int i = 0; i < c.num_layers; ++i) pack_clip_layer(pk, clip_layer(i), c.hidden_size);
    pk.f32("text_model.final_layer_norm.weight"); pk.f32("text_model.final_layer_norm.bias");
    if (u->text_proj) pk.bf16_same("text_projection.weight");
    return 0;
}

int pack_vit(sd_unet* u) {
    const sd_clip_vision_config& c = u->vis;
    Packer pk{u};
    const int H = c.hidden_size, K = 3 * c.patch_size * c.patch_size, Kp = vit_kp(c);
    pk.f32("vision_model.embeddings.class_embedding");
    {   // [H][3][P][P] -> bf16 rows [H][Kp], columns (c, kh, kw) as the patch rows of the preprocessing, zero past K
        const auto& d = pk.P("vision_model.embeddings.patch_embedding.weight");
        size_t off = pk.alloc("vision_model.embeddings.patch_embedding.weight", (size_t)H * Kp * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        for (int n = 0; n < H; ++n)
            for (int k = 0; k < Kp; ++k) o[(size_t)n * Kp + k] = k < K ? f32_to_bf16_host(d[(size_t)n * K + k]) : 0;
    }
    pk.bf16_same("vision_model.embeddings.position_embedding.weight");
    pk.f32("vision_model.pre_layrnorm.weight"); pk.f32("vision_model.pre_layrnorm.bias");
    for (int i = 0; i < c.num_layers; ++i) pack_clip_layer(pk, vit_layer(i), H);
    pk.f32("vision_model.post_layernorm.weight"); pk.f32("vision_model.post_layernorm.bias");
    pk.bf16_same("visual_projection.weight");
    return 0;
}

// ImageReward.  Vision: the fused attn.qkv rows as given; the patch-embedding bias folded into position rows 1..N (in fp32,
// before the bf16 cast: the embedding kernel adds a position row to every patch row anyway).  Text: self-attention q | k | v
// fused per layer; the cross-attention key | value weights of ALL layers concatenated ([layers][k | v] rows over the encoder
// width), because every layer projects the same image tokens: one GEMM.  Head: the five Linears are a linear chain (no
// activation, dropout is identity in eval), folded here in fp64 into one vector and one bias.
int pack_image_reward(sd_unet* u) {
    const sd_image_reward_config& c = u->ir;
    Packer pk{u};
    auto lin = [&](const std::string& n) { pk.bf16_same(n + ".weight"); pk.f32(n + ".bias"); };
    auto norm = [&](const std::string& n) { pk.f32(n + ".weight"); pk.f32(n + ".bias"); };
    auto cat_bias = [&](const std::string& key, const std::vector<std::string>& names) {
        size_t total = 0;
        for (auto& n : names) total += pk.P(n).size();
        size_t off = pk.alloc(key, total * 4);
        float* o = (float*)(u->hblob.data() + off);
        for (auto& n : names)
            for (float v : pk.P(n)) *o++ = v;
    };
    const int VH = c.vision_hidden_size, K = 3 * c.patch_size * c.patch_size, Kp = blip_kp(c);
    const int G = c.image_size / c.patch_size, Np = G * G;
    pk.f32("visual_encoder.cls_token");
    {
        const auto& d = pk.P("visual_encoder.patch_embed.proj.weight");
        size_t off = pk.alloc("visual_encoder.patch_embed.proj.weight", (size_t)VH * Kp * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        for (int n = 0; n < VH; ++n)
            for (int k = 0; k < Kp; ++k) o[(size_t)n * Kp + k] = k < K ? f32_to_bf16_host(d[(size_t)n * K + k]) : 0;
    }
    {
        const auto& pos = pk.P("visual_encoder.pos_embed");
        const auto& pb = pk.P("visual_encoder.patch_embed.proj.bias");
        size_t off = pk.alloc("visual_encoder.pos_embed", (size_t)(Np + 1) * VH * 2);
        unsigned short* o = (unsigned short*)(u->hblob.data() + off);
        for (int t = 0; t <= Np; ++t)
            for (int k = 0; k < VH; ++k) o[(size_t)t * VH + k] = f32_to_bf16_host(pos[(size_t)t * VH + k] + (t ? pb[k] : 0.f));
    }
    for (int i = 0; i < c.vision_num_layers; ++i) {
        const std::string p = blip_block(i);
        norm(p + "norm1"); lin(p + "attn.qkv"); lin(p + "attn.proj"); norm(p + "norm2"); lin(p + "mlp.fc1"); lin(p + "mlp.fc2");
    }
    norm("visual_encoder.norm");
    pk.bf16_same("text_encoder.embeddings.word_embeddings.weight");
    pk.bf16_same("text_encoder.embeddings.position_embeddings.weight");
    norm("text_encoder.embeddings.LayerNorm");
    std::vector<std::string> kvw, kvb;
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = blip_text_layer(i), a = p + "attention.self.", x = p + "crossattention.self.";
        pk.concat_rows(a + "qkv.weight", {a + "query.weight", a + "key.weight", a + "value.weight"});
        cat_bias(a + "qkv.bias", {a + "query.bias", a + "key.bias", a + "value.bias"});
        lin(p + "attention.output.dense"); norm(p + "attention.output.LayerNorm");
        lin(x + "query");
        kvw.push_back(x + "key.weight"); kvw.push_back(x + "value.weight");
        kvb.push_back(x + "key.bias"); kvb.push_back(x + "value.bias");
        lin(p + "crossattention.output.dense"); norm(p + "crossattention.output.LayerNorm");
        lin(p + "intermediate.dense"); lin(p + "output.dense"); norm(p + "output.LayerNorm");
    }
    pk.concat_rows("text_encoder.cross_kv.weight", kvw);
    cat_bias("text_encoder.cross_kv.bias", kvb);
    {   // r = W7 (W6 (W4 (W2 (W0 x + b0) + b2) + b4) + b6) + b7 = w . x + b: row vector times matrix, last layer first
        const int H = c.hidden_size;
        std::vector<double> w{1.0};      // [1][out of the layer below]
        double b = 0.0;
        for (int k = 4; k >= 0; --k) {
            const std::string n = "mlp.layers." + std::to_string(kRewardHeadLayers[k]);
            const auto& W = pk.P(n + ".weight");
            const auto& B = pk.P(n + ".bias");
            const int out = kRewardHeadDims[k], in = k ? kRewardHeadDims[k - 1] : H;
            std::vector<double> nw((size_t)in, 0.0);
            for (int o = 0; o < out; ++o) {
                b += w[o] * (double)B[o];
                for (int i = 0; i < in; ++i) nw[i] += w[o] * (double)W[(size_t)o * in + i];
            }
            w.swap(nw);
        }
        size_t off = pk.alloc("reward_head.weight", (size_t)H * 4);
        float* o = (float*)(u->hblob.data() + off);
        for (int i = 0; i < H; ++i) o[i] = (float)w[i];
        off = pk.alloc("reward_head.bias", 4);
        *(float*)(u->hblob.data() + off) = (float)b;
    }
    return 0;
}

}  // namespace

double pack_alloc_seconds() { return g_alloc_s; }

int pack_all(sd_unet* u) {
    g_alloc_s = 0;
    if (u->kind == 1) return pack_vae(u);
    if (u->kind == 2) return pack_clip(u);
    if (u->kind == 3) return pack_vit(u);
    if (u->kind == 4) return pack_vae_encoder(u);
    if (u->kind == 6) return pack_image_reward(u);
    if (u->kind == 7 || u->kind == 8) return pack_taesd(u);
    const sd_unet_config& c = u->cfg;
    Packer pk{u};
    const int c0 = c.block_out_channels[0], nl = c.num_levels;
    pk.bf16_same("time_embedding.linear_1.weight"); pk.f32("time_embedding.linear_1.bias");
    pk.bf16_same("time_embedding.linear_2.weight"); pk.f32("time_embedding.linear_2.bias");
    if (c.time_cond_proj_dim > 0) pk.bf16_same("time_embedding.cond_proj.weight");     // (gemv_kernel operand, like linear_1)
    pk.conv_in("conv_in.", c0, c.in_channels);
    std::vector<std::string> tw, tb;
    long toff = 0;
    walk_blocks(c,
        [&](const std::string& p, int cin, int cout) {
            pk.resnet(p, cin, cout);
            tw.push_back(p + "time_emb_proj.weight");
            tb.push_back(p + "time_emb_proj.bias");
            u->tproj_off[p] = toff;
            toff += cout;
        },
        [&](const std::string& p, int cc) { pk.transformer(p, cc); }, u->kind != 5);
    u->tproj_total = toff;
    pk.concat_rows("tproj.weight", tw);
    {
        size_t off = pk.alloc("tproj.bias", (size_t)toff * 4);
        float* o = (float*)(u->hblob.data() + off);
        for (auto& n : tb)
            for (float v : pk.P(n)) *o++ = v;
    }
    for (int i = 0; i < nl - 1; ++i) {
        const int co = c.block_out_channels[i];
        const std::string d = "down_blocks." + std::to_string(i) + ".downsamplers.0.conv.";
        pk.conv3(d + "weight", co, co); pk.f32(d + "bias");
        if (u->kind == 5) continue;
        const int lev = nl - 1 - i, cu = c.block_out_channels[lev];
        const std::string up = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv.";
        pk.conv3(up + "weight", cu, cu); pk.f32(up + "bias");
        pk.conv3_subpixel(up + "weight", cu, cu);
    }
    if (u->kind == 5) {     // the conditioning embedding's convs as the general conv kernel reads them ([O][tap][I]), the zero convs as GEMM rows
        std::string names[8];
        int cin[8], cout[8], stride[8];
        cond_embed_convs(u, names, cin, cout, stride);
        for (int i = 0; i < 8; ++i) { pk.conv3_ohwi(names[i] + "weight", cout[i], cin[i]); pk.f32(names[i] + "bias"); }
        for (int i = 0; u->pindex.count("controlnet_down_blocks." + std::to_string(i) + ".weight"); ++i) {
            pk.bf16_same("controlnet_down_blocks." + std::to_string(i) + ".weight"); pk.f32("controlnet_down_blocks." + std::to_string(i) + ".bias");
        }
        pk.bf16_same("controlnet_mid_block.weight"); pk.f32("controlnet_mid_block.bias");
        return 0;
    }
    pk.f32("conv_norm_out.weight"); pk.f32("conv_norm_out.bias");
    pk.conv3_ohwi("conv_out.weight", c.out_channels, c0); pk.f32("conv_out.bias");
    if (c.ip_adapter_tokens > 0) {
        const std::string p = "encoder_hid_proj.image_projection_layers.0.";
        pk.bf16_same(p + "image_embeds.weight"); pk.f32(p + "image_embeds.bias");
        pk.f32(p + "norm.weight"); pk.f32(p + "norm.bias");
    }
    return 0;
}

}  // namespace sdhip
