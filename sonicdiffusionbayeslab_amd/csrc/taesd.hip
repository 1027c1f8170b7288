// libsdhip host side: the tiny autoencoder (diffusers 0.32 AutoencoderTiny = TAESD, upstream-recall): parameter names, weight
// packing, and the two flat launch lists (decoder: 35 launches, encoder: 35 launches) on conv64.hip's kernels.
//
//   Block(x) = relu(conv(x) + x),  conv = C3(64,64)+b, ReLU, C3(64,64)+b, ReLU, C3(64,64)+b   (keys <layer>.conv.{0,2,4}.*; the
//   skip is an identity without parameters).
//   decoder.layers:  0 C3(4,64)+b | 1 ReLU | 2-4 Block | 5 nearest x2 | 6 C3(64,64) no bias | 7-9 Block | 10 x2 | 11 C3 | 12-14 Block |
//                    15 x2 | 16 C3 | 17 Block | 18 C3(64,3)+b;  input tanh(z / 3) * 3, output y * 2 - 1
//   encoder.layers:  0 C3(3,64)+b | 1 Block | 2 C3(64,64) stride 2 no bias | 3-5 Block | 6 s2 | 7-9 Block | 10 s2 | 11-13 Block |
//                    14 C3(64,4)+b;  input (x + 1) / 2 of a [-1, 1] image = the [0, 1] image
//
// Launches: entry (1) + 10 Blocks x 3 + 3 up / down convs + exit (1) = 35 for either half.  A Block keeps its input alive for
// the residual while conv 2 reads conv 1's output, so the activations rotate through THREE buffers of the largest level's
// size ([batch, 8 h, 8 w, 64] bf16 each); the upsample is fused into the conv that follows it (conv64 mode 1).
#include "model.h"

namespace sdhip {

namespace {

enum TinyKind { T_ENTRY, T_BLOCK, T_UP, T_DOWN, T_EXIT };
struct TinyLayer { int kind, layer; };
// THE table: structure and key numbering of both halves (enumeration, packing and the launch lists all walk it)
const TinyLayer kDecoder[] = {{T_ENTRY, 0}, {T_BLOCK, 2}, {T_BLOCK, 3}, {T_BLOCK, 4}, {T_UP, 6}, {T_BLOCK, 7}, {T_BLOCK, 8}, {T_BLOCK, 9},
                              {T_UP, 11}, {T_BLOCK, 12}, {T_BLOCK, 13}, {T_BLOCK, 14}, {T_UP, 16}, {T_BLOCK, 17}, {T_EXIT, 18}};
const TinyLayer kEncoder[] = {{T_ENTRY, 0}, {T_BLOCK, 1}, {T_DOWN, 2}, {T_BLOCK, 3}, {T_BLOCK, 4}, {T_BLOCK, 5}, {T_DOWN, 6}, {T_BLOCK, 7},
                              {T_BLOCK, 8}, {T_BLOCK, 9}, {T_DOWN, 10}, {T_BLOCK, 11}, {T_BLOCK, 12}, {T_BLOCK, 13}, {T_EXIT, 14}};
constexpr int kTinyLayers = 15;
constexpr int TC = 64;        // every hidden width

const TinyLayer* table(const sd_unet* u) { return u->kind == 7 ? kDecoder : kEncoder; }
std::string lname(const sd_unet* u, int layer) { return std::string(u->kind == 7 ? "decoder" : "encoder") + ".layers." + std::to_string(layer) + "."; }
int entry_cin(const sd_unet* u) { return u->kind == 7 ? 4 : 3; }
int exit_cout(const sd_unet* u) { return u->kind == 7 ? 3 : 4; }

inline unsigned short bf16_host(float f) {
    unsigned v;
    memcpy(&v, &f, 4);
    v = v + 0x7FFFu + ((v >> 16) & 1u);
    return (unsigned short)(v >> 16);
}

size_t blob_alloc(sd_unet* u, const std::string& key, size_t bytes) {
    const size_t off = (u->hblob.size() + 255) / 256 * 256;
    u->hblob.resize(off + bytes);
    u->woff[key] = off;
    return off;
}
const std::vector<float>& P(const sd_unet* u, const std::string& n) { return u->params[u->pindex.at(n)].data; }
void put_f32(sd_unet* u, const std::string& n) {
    const auto& d = P(u, n);
    const size_t off = blob_alloc(u, n, d.size() * 4);
    memcpy(u->hblob.data() + off, d.data(), d.size() * 4);
}
void put_conv64(sd_unet* u, const std::string& n) {
    const size_t off = blob_alloc(u, n, SD_CONV64_PACKED_BYTES);
    sd_conv64_pack(P(u, n).data(), (bf16_t*)(u->hblob.data() + off));
}

int check_size(int lh, int lw, const char* who) {
    SD_REQUIRE(lh >= 8 && lw >= 8 && lh <= 128 && lw <= 128 && lh % 8 == 0 && lw % 8 == 0,
               "%s: latent %dx%d (the tiny autoencoder takes sides that are multiples of 8 in [8, 128])", who, lh, lw);
    return 0;
}

size_t buffer_bytes(int batch, int lh, int lw) { return ((size_t)batch * 64 * lh * lw * TC * 2 + 255) / 256 * 256; }

}  // namespace

void enumerate_params_taesd(sd_unet* u) {
    auto add = [&](const std::string& n, std::vector<long long> shape) {
        ParamSpec p;
        p.name = n;
        p.shape = std::move(shape);
        u->pindex[n] = (int)u->params.size();
        u->params.push_back(std::move(p));
    };
    const TinyLayer* t = table(u);
    for (int i = 0; i < kTinyLayers; ++i) {
        const std::string p = lname(u, t[i].layer);
        switch (t[i].kind) {
        case T_ENTRY: add(p + "weight", {TC, entry_cin(u), 3, 3}); add(p + "bias", {TC}); break;
        case T_BLOCK:
            for (int k : {0, 2, 4}) {
                add(p + "conv." + std::to_string(k) + ".weight", {TC, TC, 3, 3});
                add(p + "conv." + std::to_string(k) + ".bias", {TC});
            }
            break;
        case T_UP: case T_DOWN: add(p + "weight", {TC, TC, 3, 3}); break;
        case T_EXIT: add(p + "weight", {exit_cout(u), TC, 3, 3}); add(p + "bias", {exit_cout(u)}); break;
        }
    }
}

int pack_taesd(sd_unet* u) {
    const TinyLayer* t = table(u);
    for (int i = 0; i < kTinyLayers; ++i) {
        const std::string p = lname(u, t[i].layer);
        switch (t[i].kind) {
        case T_ENTRY: {      // OIHW -> [Cin * 9][64] fp32: the entry conv runs in fp32 on the fp32 input
            const int ci = entry_cin(u);
            const auto& d = P(u, p + "weight");
            float* o = (float*)(u->hblob.data() + blob_alloc(u, p + "weight", d.size() * 4));
            for (int oc = 0; oc < TC; ++oc)
                for (int c = 0; c < ci; ++c)
                    for (int tap = 0; tap < 9; ++tap) o[(c * 9 + tap) * TC + oc] = d[((size_t)oc * ci + c) * 9 + tap];
            put_f32(u, p + "bias");
            break;
        }
        case T_BLOCK:
            for (int k : {0, 2, 4}) {
                put_conv64(u, p + "conv." + std::to_string(k) + ".weight");
                put_f32(u, p + "conv." + std::to_string(k) + ".bias");
            }
            break;
        case T_UP: case T_DOWN: put_conv64(u, p + "weight"); break;
        case T_EXIT: {       // OIHW -> [Cout][tap][64] bf16
            const int co = exit_cout(u);
            const auto& d = P(u, p + "weight");
            unsigned short* o = (unsigned short*)(u->hblob.data() + blob_alloc(u, p + "weight", d.size() * 2));
            for (int oc = 0; oc < co; ++oc)
                for (int c = 0; c < TC; ++c)
                    for (int tap = 0; tap < 9; ++tap) o[((size_t)oc * 9 + tap) * TC + c] = bf16_host(d[((size_t)oc * TC + c) * 9 + tap]);
            put_f32(u, p + "bias");
            break;
        }
        }
    }
    return 0;
}

long long taesd_workspace_bytes(const sd_unet* u, int batch, int lh, int lw) {
    SD_REQUIRE(batch > 0 && batch <= 4096, "taesd: bad batch %d", batch);
    if (check_size(lh, lw, "workspace_bytes")) return -1;
    return (long long)(3 * buffer_bytes(batch, lh, lw));
}

// One half, as a flat list of launches.  `in`: latents [batch, 4, lh, lw] (decoder) or images in [0, 1] [batch, 3, 8 lh, 8 lw]
// (encoder); `out`: images [batch, 3, 8 lh, 8 lw] or latents [batch, 4, lh, lw].
static int run_taesd(sd_unet* u, hipStream_t stream, const float* in, int batch, int lh, int lw, int out_mode, float* out, void* ws,
                     long long ws_bytes, const char* who) {
    SD_REQUIRE(u->finalized, "%s: parameters not finalized", who);
    SD_REQUIRE(in && out && ws && batch > 0, "%s: null argument", who);
    if (check_size(lh, lw, who)) return -1;
    const long long need = taesd_workspace_bytes(u, batch, lh, lw);
    if (need < 0) return -1;
    SD_REQUIRE(ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, ws_bytes, need);
    SD_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    const size_t bb = buffer_bytes(batch, lh, lw);
    bf16_t* buf[3] = {(bf16_t*)ws, (bf16_t*)((char*)ws + bb), (bf16_t*)((char*)ws + 2 * bb)};
    auto W = [&](const std::string& key) -> const char* { return u->dweights + u->woff.at(key); };
    int cur = 0, H = u->kind == 7 ? lh : 8 * lh, Wd = u->kind == 7 ? lw : 8 * lw;
    auto conv = [&](const std::string& wkey, const char* bias, int src, int res, int dst, int mode, int relu) -> int {
        Conv64Args a;
        a.X = buf[src]; a.Wp = (const bf16_t*)W(wkey); a.bias = (const float*)bias; a.R = res >= 0 ? buf[res] : nullptr; a.Y = buf[dst];
        a.B = batch; a.Hin = H; a.Win = Wd; a.mode = mode; a.relu = relu;
        return sd_launch_conv64(a, stream);
    };
    const TinyLayer* t = table(u);
    for (int i = 0; i < kTinyLayers; ++i) {
        const std::string p = lname(u, t[i].layer);
        int rc = 0;
        switch (t[i].kind) {
        case T_ENTRY:
            rc = sd_launch_taesd_entry(in, (const float*)W(p + "weight"), (const float*)W(p + "bias"), buf[cur], batch, H, Wd, entry_cin(u),
                                       u->kind == 7, stream);
            break;
        case T_BLOCK: {
            const int t1 = (cur + 1) % 3, t2 = (cur + 2) % 3;
            rc = conv(p + "conv.0.weight", W(p + "conv.0.bias"), cur, -1, t1, 0, 1);
            if (!rc) rc = conv(p + "conv.2.weight", W(p + "conv.2.bias"), t1, -1, t2, 0, 1);
            if (!rc) rc = conv(p + "conv.4.weight", W(p + "conv.4.bias"), t2, cur, t1, 0, 1);      // relu(conv + b + x)
            cur = t1;
            break;
        }
        case T_UP: case T_DOWN: {
            const int mode = t[i].kind == T_UP ? 1 : 2, dst = (cur + 1) % 3;
            rc = conv(p + "weight", nullptr, cur, -1, dst, mode, 0);
            H = sd_conv64_out_size(H, mode); Wd = sd_conv64_out_size(Wd, mode);
            cur = dst;
            break;
        }
        case T_EXIT:
            rc = sd_launch_taesd_exit(buf[cur], (const bf16_t*)W(p + "weight"), (const float*)W(p + "bias"), out, batch, H, Wd, exit_cout(u),
                                      out_mode, stream);
            break;
        }
        if (rc) return rc;
    }
    return 0;
}

}  // namespace sdhip

using namespace sdhip;

static int taesd_create(int kind, sd_unet** out, const char* who) {
    SD_REQUIRE(out, "%s: null argument", who);
    sd_unet* u = new sd_unet();      // no device work here: parameter enumeration also runs on a CPU-only box
    u->kind = kind;
    memset(&u->cfg, 0, sizeof(u->cfg));
    u->cfg.num_levels = 4;
    u->cfg.sample_size = 64;
    u->cfg.in_channels = 4;
    u->cfg.out_channels = 3;
    for (int i = 0; i < 4; ++i) u->cfg.block_out_channels[i] = 64;
    enumerate_params_taesd(u);
    *out = u;
    return 0;
}

extern "C" int sd_taesd_decoder_create(sd_unet** out) { return taesd_create(7, out, "sd_taesd_decoder_create"); }
extern "C" int sd_taesd_encoder_create(sd_unet** out) { return taesd_create(8, out, "sd_taesd_encoder_create"); }

extern "C" int sd_taesd_decode_hw(sd_unet* v, void* stream, const float* latents, int batch, int latent_h, int latent_w, int out_mode,
                                  float* images_out, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(v && v->kind == 7, "taesd_decode: not a tiny-autoencoder decoder handle");
    SD_REQUIRE(out_mode == 0 || out_mode == 1, "taesd_decode: out_mode %d (0: images in [-1, 1], 1: clamped to [0, 1])", out_mode);
    return run_taesd(v, (hipStream_t)stream, latents, batch, latent_h, latent_w, out_mode, images_out, workspace, workspace_bytes,
                     "taesd_decode");
}

extern "C" int sd_taesd_encode_hw(sd_unet* v, void* stream, const float* images01, int batch, int latent_h, int latent_w,
                                  float* latents_out, void* workspace, long long workspace_bytes) {
    SD_REQUIRE(v && v->kind == 8, "taesd_encode: not a tiny-autoencoder encoder handle");
    return run_taesd(v, (hipStream_t)stream, images01, batch, latent_h, latent_w, 2, latents_out, workspace, workspace_bytes, "taesd_encode");
}
