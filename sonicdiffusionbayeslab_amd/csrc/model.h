// libsdhip host side, internal: the data model shared by the host units -- pack.hip (parameter enumeration, weight packer),
// plan.hip (plan builder, workspace assignment), unet.hip (run_op, the handle ABI) and ops.hip (operator entry points) -- and
// the few functions that cross between them.
#pragma once
#include "../../include/sd_hip.h"
#include "common.h"
#include "kernels.h"

#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <map>
#include <new>
#include <set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

namespace sdhip {

constexpr size_t NOFF = (size_t)-1;
constexpr int T_LATENTS = -2, T_EPS = -3;       // T_EPS: the call's output buffer (a ControlNet's residual GEMMs write it at Op::coff)
constexpr int MAX_CONTROL_RES = SD_MAX_RES_SEGMENTS;      // residual segments of a ControlNet (12 + 1 for SD-1.5): one add launch

struct ParamSpec {
    std::string name;
    std::vector<long long> shape;
    std::vector<float> data;
    bool loaded = false;
    long long numel() const {
        long long n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

struct Wrap {  // one DeepCache-wrapped module enclosing an op
    int type;  // 0 down, 1 mid, 2 up
    int block_i, layer_i;
};

enum OpKind { OP_SINUSOID, OP_GEMV, OP_CONV_IN, OP_GN, OP_CONV3, OP_GEMM, OP_LN, OP_ATTN, OP_CONV_OUT, OP_SOFTMAX, OP_PQCONV,
              OP_CLIP_EMBED, OP_CLIP_ATTN, OP_QGELU, OP_TO_F32, OP_XATTN, OP_REPLICATE,
              OP_VIT_PREP, OP_VIT_EMBED, OP_VIT_ATTN, OP_POOL, OP_CONV_IN_IMG, OP_ENC_OUT, OP_IP_XATTN, OP_RES_ADD,
              OP_BERT_ATTN, OP_REWARD_HEAD,
              OP_TOME_MATCH, OP_TOME_SELECT, OP_TOME_MERGE, OP_TOME_UNMERGE,
              OP_FREEU,
              OP_TGATE_CAPTURE, OP_TGATE_APPLY, OP_TGATE_ZERO,
              OP_HT_GATHER, OP_HT_SCATTER,
              OP_PAG_IDENTITY,
              OP_SAG_MASS };

constexpr int TGATE_OFF = 0, TGATE_CAPTURE = 1, TGATE_REUSE = 2;      // sd_unet_set_tgate_hw modes

constexpr int REP_TEXT_POOLED = 2;       // Plan::rep of a CLIP text handle's sd_clip_text_embeds plan

// ---- UNet options and the pairs of them that are not built ------------------------------------------------------------------
// ONE table for the setters, the forward, get_plan and the workspace sizing (options.py holds the same rows for the Python
// layers; tests/test_options_cpu.py compares the two through sd_unet_option_name / sd_unet_option_conflict).  The first three
// are properties of a handle, DEEPCACHE / IP_PROMPT / CONTROL belong to a forward (or to what is set for the next one), the
// rest are settings of the handle.
enum UnetOption { OPT_FP8, OPT_INPAINT9, OPT_IP_MODEL, OPT_DEEPCACHE, OPT_IP_PROMPT, OPT_CONTROL, OPT_TOME, OPT_HYPERTILE, OPT_FREEU,
                  OPT_TGATE, OPT_PAG, OPT_SAG, OPT_COUNT };
constexpr unsigned opt_bit(int o) { return 1u << o; }

inline const char* option_name(int i) {
    static const char* const names[OPT_COUNT] = {"fp8", "9-channel UNet", "UNet with IP-Adapter weights", "DeepCache",
                                                 "IP-Adapter image prompt", "ControlNet residuals", "Token Merging", "HyperTile",
                                                 "FreeU", "T-GATE", "PAG", "SAG"};
    return i >= 0 && i < OPT_COUNT ? names[i] : nullptr;
}

// the reason a pair is refused, null = the pair is built (symmetric)
inline const char* option_conflict(int a, int b) {
    static const struct { int a, b; const char* why; } refused[] = {
        {OPT_FP8, OPT_CONTROL, "the calibrated activation scales do not describe the skip tensors with residuals added"},
        {OPT_FP8, OPT_TOME, "the merge and unmerge kernels take bf16 tokens"},
        {OPT_FP8, OPT_HYPERTILE, "the tile gather and scatter take bf16 tokens"},
        {OPT_FP8, OPT_FREEU, "the calibrated activation scales do not describe the scaled tensors"},
        {OPT_FP8, OPT_TGATE, "the calibrated activation scales do not describe the gated tensors"},
        {OPT_FP8, OPT_PAG, "the identity kernel takes bf16 tokens"},
        {OPT_FP8, OPT_SAG, "the attention-mass kernel takes bf16 q | k"},
        {OPT_INPAINT9, OPT_TGATE, "an inpainting UNet is not gated"},
        {OPT_INPAINT9, OPT_PAG, "an inpainting UNet has no perturbed branch"},
        {OPT_INPAINT9, OPT_SAG, "the degraded latents have no mask channels"},
        {OPT_IP_MODEL, OPT_TGATE, "the image branch of the cross-attention is not cached"},
        {OPT_IP_MODEL, OPT_PAG, "the image prompt has no third branch"},
        {OPT_IP_MODEL, OPT_SAG, "the image prompt has no branch on the degraded latents"},
        {OPT_TOME, OPT_HYPERTILE, "merged tokens have no tile grid"},
        {OPT_TOME, OPT_PAG, "merged tokens have no identity attention"},
        {OPT_TOME, OPT_SAG, "merged tokens have no attention mass"},
        {OPT_TGATE, OPT_DEEPCACHE, "the cached features are stored at the CFG batch"},
        {OPT_TGATE, OPT_IP_PROMPT, "the image branch of the cross-attention is not cached"},
        {OPT_TGATE, OPT_CONTROL, "the residuals are computed for the CFG batch"},
        {OPT_TGATE, OPT_PAG, "behind the gate the UNet runs at the latent batch alone"},
        {OPT_TGATE, OPT_SAG, "behind the gate the step has no pair to degrade from"},
        {OPT_PAG, OPT_DEEPCACHE, "the cached features are stored at the CFG batch"},
        {OPT_PAG, OPT_IP_PROMPT, "the image prompt has no third branch"},
        {OPT_PAG, OPT_CONTROL, "the residuals are computed for the CFG batch"},
        {OPT_PAG, OPT_SAG, "one extra guidance branch per step is built"},
        {OPT_SAG, OPT_DEEPCACHE, "a skip step does not run the mid block"},
        {OPT_SAG, OPT_IP_PROMPT, "the image prompt has no branch on the degraded latents"},
        {OPT_SAG, OPT_CONTROL, "the residuals are computed for the first forward alone"},
        {OPT_CONTROL, OPT_DEEPCACHE, "a skip step does not run the blocks the residuals are added in"},
    };
    for (const auto& p : refused)
        if ((p.a == a && p.b == b) || (p.a == b && p.b == a)) return p.why;
    return nullptr;
}

// fails (sd_set_error, -1) on the first refused pair among the options in `mask`
inline int check_options(const char* who, unsigned mask) {
    for (int a = 0; a < OPT_COUNT; ++a)
        for (int b = a + 1; b < OPT_COUNT; ++b)
            if ((mask & opt_bit(a)) && (mask & opt_bit(b)) && option_conflict(a, b)) {
                sd_set_error("%s: %s with %s is not built (%s)", who, option_name(a), option_name(b), option_conflict(a, b));
                return -1;
            }
    return 0;
}

// What names a plan of a handle, field by field (the key of sd_unet::plans, kept in the plan as Plan::v).  UNet (kind 0): rep
// 2 = the prompt-independent prefix runs once per latent (CFG pair), see Builder::build; with a PAG mask rep = the copies of
// the latent batch, 3 or 2.  CLIP text (kind 2): REP_TEXT_POOLED = the pooled + projected variant of sd_clip_text_embeds.
// ip / cn: the IP-Adapter and the "control" variant; tome_bits: the bits of the merging ratio, with tome_max_downsample 0 = off;
// freeu, sag: on / off; tgate: TGATE_OFF / CAPTURE / REUSE; tg_pair: y rows per cache row of a capture, 2 for a CFG pair, else
// 1; ht_tokens / ht_max_depth: HyperTile's tile side in tokens and depth, 0 = off; pag_mask: the PAG layer mask, 0 = off.
struct PlanVariant {
    int UB = 0, branch = -1, rep = 1;
    int lh = 0, lw = 0;
    int ip = 0, cn = 0;
    long long tome_bits = 0;
    int tome_max_downsample = 0;
    int freeu = 0, tgate = TGATE_OFF, tg_pair = 1;
    int ht_tokens = 0, ht_max_depth = 0;
    long long pag_mask = 0;
    int sag = 0;
    auto tied() const {
        return std::tie(UB, branch, rep, lh, lw, ip, cn, tome_bits, tome_max_downsample, freeu, tgate, tg_pair, ht_tokens, ht_max_depth,
                        pag_mask, sag);
    }
    bool operator<(const PlanVariant& o) const { return tied() < o.tied(); }
};

struct Op {
    int kind = 0;
    int x1 = -1, x2 = -1, r = -1, out = -1, aux = -1, b2t = -1;
    size_t w = NOFF, b = NOFF, g = NOFF, be = NOFF;
    long b2idx = 0;
    int M = 0, N = 0, K = 0, K1 = 0, epi = 0;
    int B = 0, Hin = 0, Win = 0, Cin = 0, Hout = 0, Wout = 0, stride = 1, up = 0;
    int C1 = 0, C2 = 0, HW = 0, silu = 0, nsplit = 0;
    float eps = 0.f;
    int heads = 0, D = 0, Nq = 0, Nk = 0;
    long ldq = 0, ldk = 0, ldv = 0, ldo = 0, qoff = 0, koff = 0, voff = 0;
    int silu_in = 0, splitk = 1;
    int pool_by_ids = 0;          // OP_POOL: the row is the EOS position of the call's token ids (0: row 0, the class token)
    int key_mask = 0;             // OP_BERT_ATTN: the keys carry the call's attention mask (self-attention; 0: all valid)
    // split-K producer + single-launch GroupNorm as ONE reduce (fuse_deferred_reduce): the producer (CONV3 / GEMM) sets `defer`
    // and launches no splitk_reduce_kernel; the GroupNorm reads the producer's slabs (slab_t, slab_k of them) with its bias /
    // time-embedding row / residual and writes the producer's output tensor on the way (GroupNormArgs::slab)
    int defer = 0, slab_t = -1, slab_k = 0, slab_r = -1, slab_b2t = -1;
    size_t slab_b = NOFF;
    long slab_b2idx = 0;
    // generalised GEMM operands (VAE attention): W operand taken from an activation tensor, X taken
    // from the weight blob, element offsets into tensors and explicit row strides
    int wt = -1;
    size_t wx = NOFF;
    long xoff = 0, woff_el = 0, coff = 0, ldx_o = 0, ldw_o = 0, ldc_o = 0;
    float scale = 0.f;
    long wbs = 0;                 // per-sample W: batch stride (elements), rows per sample, softmax width
    int rpb = 0, sm_valid = 0;
    // fp8-e4m3 operands (SD_DTYPE_FP8_E4M3): this op's X and W are e4m3 (K / Cin padded to 128), wsc = offset of
    // the per-output-channel weight scales, xs = activation scale of its input; out_fp8: the op WRITES e4m3
    // (rows of Cpad bytes) with scale os.  Kalg: unpadded contraction length (algorithmic FLOPs).
    int dt = 0, out_fp8 = 0, Cpad = 0, Kalg = 0;
    int sname = -1;                   // fp8 producer: index into sd_unet::act_names of the tensor it writes (its scale = os)
    // GroupNorm statistics from the producer's epilogue: `stats` = tensor this op writes ([M/64][N][2] fp32),
    // s1 / s2 = the statistics tensors of a GroupNorm's sources (it then skips its statistics pass)
    int stats = -1, s1 = -1, s2 = -1;
    // LayerNorm fold: rs = row partials this op writes ([np][M][2] fp32); lnrs / lnnp / c1 = partials and column sums
    // this GEMM normalises with (its x1 is the un-normalised tensor, its weights carry gamma, its bias W beta + b)
    int subpix = 0;                   // CONV3 with up: four 2x2 convs on the low-res input (GemmArgs::subpix)
    int asym = 0;                     // CONV3 stride 2 padded right / bottom only (GemmArgs::asym: the VAE encoder's downsamplers)
    int hm = 0;                       // GEMM: q|k|v with head-major K / V (HW = tokens per sample); ATTN: K / V are head-major
    int qps = 0;                      // ATTN: Q arrives multiplied by scale * log2 e (folded into W_q at pack time)
    int rs = -1, lnrs = -1, lnnp = 0;
    size_t c1 = NOFF;
    size_t wsc = NOFF;
    float xs = 1.f, os = 1.f;
    // CONV3 with the resnet's 1x1 shortcut folded in (GemmArgs::Xs1 ...): shortcut sources [scx1 | scx2] of scc1 + scc2
    // channels, scw = the packed conv_shortcut weight; `b` is then the summed bias vector and Kalg counts the shortcut channels
    int scx1 = -1, scx2 = -1, scc1 = 0, scc2 = 0;
    size_t scw = NOFF;
    // OP_RES_ADD (the "control" plan variant): the tensors the ControlNet residuals are added to, in segment order
    int nres = 0;
    int res_t[MAX_CONTROL_RES];
    int nwrap = 0;
    Wrap wraps[3];
};

// Host staging buffer of the packed weights: ONE anonymous mapping reserved up front and populated by the kernel in bulk
// (MAP_POPULATE, transparent huge pages where available).  A std::vector paid ~20 us per 4 KiB first-touch fault here:
// 11-19 s of a 22 s finalize for the 2.3 GB UNet blob.
struct HostBlob {
    unsigned char* p = nullptr;
    size_t n = 0, cap = 0;
    unsigned char* data() { return p; }
    const unsigned char* data() const { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    bool reserve(size_t bytes) {
        if (bytes <= cap) return true;
        void* q = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_POPULATE, -1, 0);
        if (q == MAP_FAILED) return false;
        (void)madvise(q, bytes, MADV_HUGEPAGE);
        if (p) { memcpy(q, p, n); munmap(p, cap); }
        p = (unsigned char*)q; cap = bytes;
        return true;
    }
    void resize(size_t bytes) {             // (new bytes are zero: fresh anonymous pages)
        // a failed mapping surfaces as an error of sd_unet_finalize (which catches this), never as an abort of the host process
        if (bytes > cap && !reserve(std::max(bytes, cap * 2))) throw std::bad_alloc();
        n = bytes;
    }
    void release() { if (p) munmap(p, cap); p = nullptr; n = cap = 0; }
    ~HostBlob() { release(); }
    HostBlob() = default;
    HostBlob(const HostBlob&) = delete;
    HostBlob& operator=(const HostBlob&) = delete;
};

struct Tn {
    size_t bytes = 0;
    int def = -1, last = -1;
    bool persistent = false;
    bool ctx = false;            // written by sd_unet_set_context: same offset in every plan variant of a (batch, branch)
    bool ctx_ip = false;         // ctx tensor of the IP-Adapter variant (sd_unet_set_ip_adapter_hw): laid out BEHIND the others
    size_t off = NOFF;
};

struct Plan {
    PlanVariant v;                        // what the plan was built for (its key)
    // IP-Adapter variant (v.ip): one OP_IP_XATTN in front of every block's prompt cross-attention, whose
    // residual operand becomes that op's output.  ip_fold: per block the folded operands A [UB][32][C] and Bt [UB][C][32]
    // (ip_xattn.hip) with the packed weights they are folded from; ip_e / ip_proj / ip_tok / ip_kv: what
    // sd_unet_set_ip_adapter_hw computes on the way (bf16: embeds [UB][E], projection [UB][T * CD], tokens [UB * T][CD], and one
    // block's K_ip | V_ip [UB * T][2 C]).
    struct IpFold { int at, bt, C; size_t wqT, wo, wkv; int heads; };
    std::vector<IpFold> ip_fold;
    int ip_e = -1, ip_proj = -1, ip_tok = -1, ip_kv = -1;
    // "control" variant (v.cn): one OP_RES_ADD after the mid block adds the ControlNet residuals in place to the
    // twelve skip tensors and the mid output; up-block GroupNorms of those tensors compute their own statistics
    std::vector<size_t> cn_off;           // UNet / ControlNet plans: the residual segments' byte offsets and bf16 element
    std::vector<long> cn_count;           // counts for this batch and size (control_segments)
    // Token Merging variant (v.tome_bits): the merging blocks in plan order.  Each owns its
    // index tensors (persistent: readable after the forward, sd_unet_tome_matching_hw) and a slice of the handle's choice array.
    struct TomeBlock { int tok, kept, merged, dst_idx, B, h, w, r; long choice_off; };
    std::vector<TomeBlock> tome;
    long tome_choice_bytes = 0;
    // HyperTile variant (v.ht_tokens): the tiled transformer blocks in plan order, each with its
    // token grid and tile counts (sd_unet_hypertile_block_info_hw)
    struct HtBlock { int rh, rw, nh, nw; };
    std::vector<HtBlock> hypertile;
    // PAG variant (v.pag_mask, pag.hip): pag_lb() > 0 = the LAST pag_lb() samples of the batch are the perturbed ones (v.rep = UB /
    // pag_lb() is 3 or 2; rep 1: the plan sd_unet_set_context_hw lays the prompt tensors out with); in the blocks the mask names
    // attn1 runs on the other samples and one OP_PAG_IDENTITY fills the perturbed rows of its output.  pag_blocks: the
    // transformer blocks the builder has seen so far.
    int pag_lb() const { return v.pag_mask && v.rep > 1 ? v.UB / v.rep : 0; }
    int pag_blocks = 0;
    // SAG capture variant (v.sag, sag.hip): one OP_SAG_MASS behind the q | k | v projection of the mid block's
    // transformer block writes the attention mass of every sample into the buffer the handle names; nothing else changes
    // FreeU variant (v.freeu): one OP_FREEU in front of every resnet of up blocks 0 and 1 (x1 = hidden, x2 = skip ->
    // out = the scaled hidden, aux = the filtered skip, epi = the up block: which pair of the handle's factors the launch reads)
    // T-GATE variant (v.tgate; tgate.hip): TGATE_CAPTURE = every prompt cross-attention form runs WITHOUT its residual
    // operand and one OP_TGATE_CAPTURE behind it writes h2 = h1 + y and the block's slice of the handle's cache (v.tg_pair = rows of
    // y per cache row: 2 for a CFG pair [uncond | cond]); TGATE_REUSE = norm2, attn2 and every context tensor are gone and one
    // OP_TGATE_APPLY writes h2 = h1 + slice.  tg_off / tg_rows / tg_ch: the slices in plan order (tgate_segments), for tg_batch
    // latents; Op::b2idx of the two ops = the block's index.
    int tg_batch = 0;
    std::vector<size_t> tg_off;
    std::vector<long> tg_rows;
    std::vector<int> tg_ch;
    int tg_blocks = 0;                    // blocks the builder has wired so far
    std::vector<Tn> tensors;
    std::vector<Op> ops;
    std::vector<char> skipped;            // per op: skipped on a DeepCache skip step
    std::vector<int> ctx_kv;              // tensor id of the [UB*L, 2C] K|V cache per cross-attn layer
    std::vector<size_t> ctx_w;            // packed [2C, 768] weight offset per layer
    std::vector<int> ctx_c;               // C per layer
    int ctx_bf16 = -1;                    // bf16 copy of encoder_hidden_states
    // folded prompt cross-attention (per layer): A^T [UB][heads*80][C] and B [UB][C][heads*80], see transformer()
    struct Fold { int kv, at, bw, C, heads; size_t wqT, wo; bool perm; int c2 = -1; size_t lnu = NOFF; int c1 = -1; size_t ones = NOFF; };   // perm: Bw in the fused kernel's k order; c2 >= 0: norm2 folded (wqT = the .ln weights, c2 = tensor of the beta terms)
    std::vector<Fold> ctx_fold;
    int ctx_fold_scratch = -1;            // masked K / V expansions [3][UB][max over levels of heads*80*C]
    std::map<std::string, int> taps;
    size_t total_bytes = 0;
    // CLIP vision plans (kind 3): preprocessing geometry of the plan's input size and its tap tables (host copy while the plan
    // is built; the device copy belongs to the handle, one per input size)
    ClipPrepGeom geom;
    std::vector<int> prep_tab;
    const int* dtab = nullptr;
};

}  // namespace sdhip

struct sd_unet {
    // 0 = UNet2DConditionModel, 1 = AutoencoderKL decoder, 2 = CLIP text encoder, 3 = CLIP vision tower, 4 = AutoencoderKL encoder,
    // 5 = ControlNetModel (the UNet's time embedding, conv_in, down path and mid block + the zero convs),
    // 6 = ImageReward (BLIP ViT + BLIP text encoder + reward head),
    // 7 / 8 = AutoencoderTiny decoder / encoder (taesd.hip: flat launch lists, no Plan)
    int kind = 0;
    sd_unet_config cfg;
    sd_clip_config clip;
    sd_clip_vision_config vis;
    sd_image_reward_config ir;         // kind 6
    // kind 6: the text operands and the optional feature output of the call in flight (sd_image_reward_score sets them, the
    // plan's embedding / attention / head ops read them; the images travel as the plan's input, the rewards as its output)
    const int* ir_ids = nullptr;
    const int* ir_mask = nullptr;
    float* ir_features = nullptr;
    int text_proj = 0;                 // kind 2 with text_projection.weight [text_proj, hidden] (sd_clip_create_projected)
    int eos_id = -1;                   // pooled text row: first position of this id; < 0: argmax of the ids
    std::map<std::pair<int, int>, int*> prep_tabs;     // kind 3: device tap tables per input (H, W)
    std::vector<sdhip::ParamSpec> params;
    std::unordered_map<std::string, int> pindex;
    std::unordered_map<std::string, size_t> woff;  // packed item -> byte offset into dweights
    sdhip::HostBlob hblob;                                // host staging of the packed blob
    char* dweights = nullptr;
    bool finalized = false;
    bool debug_taps = false;
    bool fp8 = false;                  // cfg.weight_dtype == SD_DTYPE_FP8_E4M3
    float s_norm = 8.f, s_ff = 2.f;    // fp8 activation scales (GroupNorm / LayerNorm outputs, GEGLU outputs): the DEFAULTS
    // per-tensor activation scales (sd_unet_calibrate_fp8 / sd_unet_set_fp8_scale): every e4m3 activation tensor is named
    // after the module that writes it ("<resnet>.norm1", "<attn>.norm", "<block>.norm1|3", "<block>.ff.net.0"); a tensor
    // without an entry uses the default of its kind.  act_amax: largest |value| calibration has seen (0 = never calibrated).
    std::vector<std::string> act_names;
    std::unordered_map<std::string, int> act_index;
    std::vector<float> act_scale, act_amax;
    int act_id(const std::string& name, float dflt) {
        auto it = act_index.find(name);
        if (it != act_index.end()) return it->second;
        act_index[name] = (int)act_names.size();
        act_names.push_back(name); act_scale.push_back(dflt); act_amax.push_back(0.f);
        return (int)act_names.size() - 1;
    }
    std::map<sdhip::PlanVariant, sdhip::Plan> plans;
    sdhip::PlanVariant last;           // variant of the last forward (sd_unet_debug_tensor, sd_unet_tome_matching_hw); lh 0 = none yet
    std::unordered_map<std::string, long> tproj_off;  // resnet prefix -> float index into tproj vector
    long tproj_total = 0;
    // LCM-distilled UNets (cfg.time_cond_proj_dim > 0): cond_proj . condition, [c0] fp32, written by sd_unet_set_timestep_cond.
    // Owned by the handle (not the workspace) so that it outlives plans, sizes and DeepCache branches; while cond_set, every
    // forward's OP_SINUSOID adds it to the sinusoid.
    float* dcond = nullptr;
    bool cond_set = false;
    // inpainting UNets (cfg.in_channels == 9): the five constant input channels of a call, [inpaint_b][5][h][w] fp32 =
    // [mask | masked-image latents], written by sd_unet_set_inpaint_cond_hw.  Owned by the handle like dcond; OP_CONV_IN reads
    // channels 4..8 from it (batch index modulo inpaint_b), so no concatenated input is built per forward.
    float* dinpaint = nullptr;
    size_t inpaint_cap = 0;
    int inpaint_b = 0, inpaint_h = 0, inpaint_w = 0;
    // IP-Adapter (cfg.ip_adapter_tokens > 0): the (UNet batch, DeepCache branch, latent H, W) whose workspace holds folded image
    // operands (sd_unet_set_ip_adapter_hw).  While the set is not empty every forward runs the "IP on" plan variant and must find
    // its own key here; empty = the plans of a handle without an adapter.
    std::set<std::tuple<int, int, int, int>> ip_keys;
    // ControlNet residuals of a UNet (sd_unet_set_control_residuals_hw): the caller's buffer, borrowed, with the scale and the
    // (UNet batch, latent H, W) it is laid out for.  Null = the plain plans.
    const char* ctrl_res = nullptr;
    float ctrl_scale = 0.f;
    int ctrl_ub = 0, ctrl_h = 0, ctrl_w = 0;
    // set by the first sd_unet_set_control_residuals_hw: from then on sd_unet_workspace_bytes_hw covers the control plan variants
    // (a handle that never sees a ControlNet builds and sizes only today's plans)
    bool ctrl_enabled = false;
    // ControlNet handle (kind 5): the conditioning embedding [cn_b][cn_h * cn_w][c0] bf16 of the call and the scratch its conv
    // chain runs in (sd_controlnet_set_cond_hw), owned by the handle like dinpaint; conv_in adds it (batch index modulo cn_b)
    bf16_t* cn_embed = nullptr;
    char* cn_scratch = nullptr;
    size_t cn_embed_cap = 0, cn_scratch_cap = 0;
    int cn_b = 0, cn_h = 0, cn_w = 0;
    int cond_embed[4] = {0, 0, 0, 0};       // conditioning_embedding_out_channels
    // Token Merging (sd_unet_set_tome; kind 0, bf16): ratio 0 = off = the plans of a handle that never saw it.  The dst choice of
    // every merging block (one byte per 2x2 cell, blocks concatenated in plan order) is owned by the handle like dinpaint and
    // zero (position 0 of every cell) until sd_unet_set_tome_choice_hw writes it.
    double tome_ratio = 0.0;
    int tome_max_downsample = 0;
    unsigned char* tome_choice = nullptr;
    size_t tome_choice_cap = 0;
    long tome_choice_n = 0;
    // HyperTile (sd_unet_set_hypertile; kind 0, bf16): the tile side in tokens, 0 = off = the plans of a handle that never saw it
    int ht_tokens = 0, ht_max_depth = 0;
    // PAG (sd_unet_set_pag; kind 0, bf16): bit i = transformer block i in plan order (down, mid, up) has identity attn1 for the
    // perturbed samples; 0 = off = the plans of a handle that never saw it
    long long pag_mask = 0;
    // SAG (sd_unet_set_sag; kind 0, bf16): capture of the mid block's attention mass into sag_mass (the caller's buffer of
    // sag_mass_floats floats, sd_unet_set_sag_buffer); off = the plans of a handle that never saw it
    bool sag_on = false;
    float* sag_mass = nullptr;
    long long sag_mass_floats = 0;
    // FreeU (sd_unet_set_freeu; kind 0, bf16): on = the "freeu" plan variants; the factors are read when OP_FREEU is launched
    bool freeu_on = false;
    float freeu_s[2] = {1.f, 1.f}, freeu_b[2] = {1.f, 1.f};       // (s1, s2), (b1, b2): up block 0, up block 1
    // T-GATE (sd_unet_set_tgate_hw; kind 0, bf16): mode off = the plans of a handle that never saw it.  The cache is the caller's
    // buffer, borrowed like ctrl_res (the capture plan at the CFG batch and the reuse plan at the latent batch share it), laid out
    // for tg_b latents at tg_h x tg_w; tg_captured: a capture forward has filled it for exactly that layout.
    int tg_mode = 0;
    char* tg_cache = nullptr;
    long long tg_bytes = 0;
    int tg_b = 0, tg_h = 0, tg_w = 0;
    bool tg_captured = false;
    bool unet_like() const { return kind == 0 || kind == 5; }      // runs the UNet's encoder ops (plan.hip Builder::build)
};

namespace sdhip {

// Head count of the transformer blocks at a resolution level (sd_unet_config::num_heads_per_level; all zeros = num_heads at
// every level), and of a block by its prefix: down_blocks.i sits on level i, up_blocks.i on level num_levels - 1 - i, the mid
// block on the last level.
inline int level_heads(const sd_unet_config& c, int level) {
    return c.num_heads_per_level[level] > 0 ? c.num_heads_per_level[level] : c.num_heads;
}
inline int block_heads(const sd_unet_config& c, const std::string& p) {
    if (p.compare(0, 12, "down_blocks.") == 0) return level_heads(c, atoi(p.c_str() + 12));
    if (p.compare(0, 10, "up_blocks.") == 0) return level_heads(c, c.num_levels - 1 - atoi(p.c_str() + 10));
    return level_heads(c, c.num_levels - 1);
}

// pack.hip
void enumerate_params(sd_unet* u);
void enumerate_params_vae(sd_unet* u);
void enumerate_params_vae_encoder(sd_unet* u);
void enumerate_params_clip(sd_unet* u);
void enumerate_params_vit(sd_unet* u);
void enumerate_params_image_reward(sd_unet* u);
int cond_embed_convs(const sd_unet* u, std::string names[8], int cin[8], int cout[8], int stride[8]);     // ControlNetConditioningEmbedding's chain
int pack_all(sd_unet* u);
double pack_alloc_seconds();      // staging-blob growth inside the last pack_all (SD_PACK_TIMING)
// transformers CLIPTextModel state_dict names (4.48.0 layout, `text_model.` prefix)
inline std::string clip_layer(int i) { return "text_model.encoder.layers." + std::to_string(i) + "."; }
// transformers CLIPVisionModelWithProjection names (`vision_model.` prefix; `pre_layrnorm` is transformers' spelling)
inline std::string vit_layer(int i) { return "vision_model.encoder.layers." + std::to_string(i) + "."; }
// ImageReward (kind 6) names: BLIP's own, without the checkpoint's `blip.` prefix
inline std::string blip_block(int i) { return "visual_encoder.blocks." + std::to_string(i) + "."; }
inline std::string blip_text_layer(int i) { return "text_encoder.encoder.layer." + std::to_string(i) + "."; }
constexpr int kRewardHeadDims[5] = {1024, 128, 64, 16, 1};       // mlp.layers.{0,2,4,6,7}: hidden -> ... -> 1
constexpr int kRewardHeadLayers[5] = {0, 2, 4, 6, 7};
inline int blip_kp(const sd_image_reward_config& c) { return (3 * c.patch_size * c.patch_size + 63) / 64 * 64; }
inline int vit_kp(const sd_clip_vision_config& c) { return (3 * c.patch_size * c.patch_size + 63) / 64 * 64; }

// taesd.hip (handle kinds 7 / 8)
void enumerate_params_taesd(sd_unet* u);
int pack_taesd(sd_unet* u);
long long taesd_workspace_bytes(const sd_unet* u, int batch, int lh, int lw);

// plan.hip
int plan_rep(const sd_unet* u, int latent_batch, int unet_batch);
int check_latent_size(const sd_unet* u, int lh, int lw, const char* who);
// the variant of (UB, branch, latent size) under the handle's option state: rep 1, no image prompt, no residuals (a call site
// that runs another one sets the field).  lh / lw < 0: the handle's sample_size; branch < 0: -1; kinds other than 0 have no options
PlanVariant plan_variant(const sd_unet* u, int UB, int branch = -1, int lh = -1, int lw = -1);
unsigned variant_options(const sd_unet* u, const PlanVariant& v);     // the options a plan of this variant runs with (check_options)
unsigned active_options(const sd_unet* u);        // ... and those on the handle now, residuals and image prompts that are set included
int get_plan(sd_unet* u, const PlanVariant& v, Plan** out);
int transformer_block_count(const sd_unet_config& c);      // transformer blocks of a UNet in plan order (down, mid, up)
bool ip_active(const sd_unet* u, int UB, int branch, int lh, int lw);     // is this forward's IP-Adapter key set?
// the ControlNet residual segments of a (UNet batch, latent size), in order: byte offset into the residual buffer and bf16
// element count of each (include/sd_hip.h: the layout); returns the buffer's bytes
size_t control_segments(const sd_unet_config& c, int UB, int lh, int lw, std::vector<size_t>* off, std::vector<long>* count);
// the T-GATE cache slices of `batch` latents at a latent size, one per transformer block in plan order (down, mid, up): byte
// offset into the cache buffer, rows (batch * tokens) and channels of each; returns the buffer's bytes
size_t tgate_segments(const sd_unet_config& c, int batch, int lh, int lw, std::vector<size_t>* off, std::vector<long>* rows, std::vector<int>* ch);

// unet.hip
int ensure_zero_page();
const void* zero_page();          // (null until ensure_zero_page has run)
int check_image_size(int H, int W, const char* who);
int run_op(sd_unet* u, const Plan& pl, const Op& o, char* ws, const float* latents, int latent_batch, float* eps_out,
           float timestep, hipStream_t stream);

// ops.hip
void* op_scratch(size_t bytes);

}  // namespace sdhip
