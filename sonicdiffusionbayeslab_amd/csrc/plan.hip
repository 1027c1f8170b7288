// libsdhip host side: the execution plan of a handle -- Builder (one op list per model kind), the deferred split-K reduce
// fusion, lifetime-based workspace assignment with DeepCache plan filtering, and the per-handle plan cache.
#include "model.h"

#include <stdlib.h>

namespace sdhip {

namespace {

// ---------------------------------------------------------------------------------------------
// plan builder
// ---------------------------------------------------------------------------------------------
struct Builder {
    sd_unet* u;
    Plan& pl;
    int UB;
    std::vector<Wrap> wrapstack;
    std::map<int, int> stats_of;      // activation tensor -> statistics tensor written by its producer
    std::map<int, float> tscale;      // e4m3 activation tensor -> the scale its producer wrote it with
    static std::string stem(const std::string& key) {      // "....norm1.weight" -> "....norm1"
        const size_t n = key.rfind(".weight");
        return n == std::string::npos ? key : key.substr(0, n);
    }
    // the first inconsistency found while building (a C-ABI library reports it as an error code, it never aborts the host
    // process): the builder carries on with harmless values and get_plan refuses the plan
    std::string error;
    float xscale(int t) {
        auto it = tscale.find(t);
        if (it == tscale.end()) {
            if (error.empty()) error = "fp8 consumer of a tensor without a scale";
            return 1.0f;
        }
        return it->second;
    }
    // SD_GN_PRODUCER_STATS=0: every GroupNorm runs its own statistics pass (round-1 behaviour)
    bool producer_stats = !(getenv("SD_GN_PRODUCER_STATS") && atoi(getenv("SD_GN_PRODUCER_STATS")) == 0);
    void want_stats(Op& o, int M, int N) {      // called for producers whose output feeds a GroupNorm
        if (!producer_stats || !u->unet_like() || o.splitk > 1 || M % 64 != 0 || o.epi != 0 || o.rpb != 0) return;
        o.stats = tensor((size_t)(M / 64) * N * 2 * 4);
        stats_of[o.out] = o.stats;
    }

    // CFG de-duplication (Plan::rep == 2: the UNet batch is [uncond | cond] over the SAME latents and timestep): every op
    // before the first prompt cross-attention -- conv_in, down_blocks.0.resnets.0 and attentions.0 up to attn1.to_out --
    // sees identical inputs in both halves, so it runs once per latent (UB / 2) and its three outputs that live on
    // (conv_in's skip, the block input = proj_out's residual, h1) are copied to both halves.  prefix_rep > 1 while the
    // builder is inside that prefix.
    int prefix_rep = 1;
    int replicate(int t, size_t bytes, int r) {
        Op o; o.kind = OP_REPLICATE; o.x1 = t; o.M = (int)(bytes / 16); o.N = r; o.out = tensor(bytes * r);
        push(o);
        return o.out;
    }
    // T-GATE capture: a zeroed tensor of at least `bytes`, the residual operand of the fused cross-attention form (filled by an
    // op of its own in front of its first reader; a later, larger request gets a new one)
    int tg_zero = -1;
    int tgate_zero(size_t bytes) {
        if (tg_zero < 0 || pl.tensors[tg_zero].bytes < bytes) {
            Op o; o.kind = OP_TGATE_ZERO; o.out = tg_zero = tensor(bytes); push(o);
        }
        return tg_zero;
    }
    // SD_LN_FOLD=0: every LayerNorm is its own launch (round-1 behaviour)
    bool ln_fold = !(getenv("SD_LN_FOLD") && atoi(getenv("SD_LN_FOLD")) == 0);
    // Ask the op that produced a residual-stream tensor for per-row LayerNorm partials; returns the partial count (0 =
    // this producer cannot deliver them: split-K, fp8 output, ...) and the tensor in `rs`.
    int want_rowstats(Op& o, int M, int C, int& rs) {
        int np = 0;
        if (o.kind == OP_GEMM && o.epi == 0 && o.splitk == 1 && !o.out_fp8 && o.N == C && o.M == M && o.ldc_o == 0) np = (C + 159) / 160 * 2;
        else if (o.kind == OP_XATTN && o.N == C && o.M == M) np = 2 * sd_xattn_slices(M, C);
        else if ((o.kind == OP_TGATE_CAPTURE || o.kind == OP_TGATE_APPLY) && o.N == C && o.M == M) np = SD_TGATE_PARTS;
        // the consumer's preconditions (gemm_conv.hip::check_ln): K = C >= 128 (two K tiles: with one, the c1 | c2 LDS-DMA is
        // never waited for), at most 16 partials per row, 128-row tiles -- otherwise the plan keeps the separate LayerNorm
        static const bool big_tiles = getenv("SD_GEMM_BIG") != nullptr;
        if (!ln_fold || np == 0 || np > 16 || C < 128 || big_tiles) return 0;
        o.rs = rs = tensor((size_t)np * M * 2 * 4);
        return np;
    }
    // GEMM over the un-normalised rows x with the LayerNorm folded in (weights key.ln / key.c1 / key.c2 of the packer)
    int gemm_ln(int x, int rs, int np, int M, int N, int C, const std::string& w, int epi) {
        Op o; o.kind = OP_GEMM; o.x1 = x; o.K1 = o.K = o.Kalg = C; o.M = M; o.N = N; o.epi = epi; o.splitk = 1;
        o.w = W(w + ".ln"); o.c1 = W(w + ".c1"); o.b = W(w + ".c2"); o.lnrs = rs; o.lnnp = np;
        o.out = tensor((size_t)M * (epi ? N / 2 : N) * 2);
        push(o);
        return o.out;
    }

    int ctx_tensor(size_t bytes) {       // persistent and written by sd_unet_set_context
        const int id = tensor(bytes, true);
        pl.tensors[id].ctx = true;
        return id;
    }
    int ctx_ip_tensor(size_t bytes) {    // ... by sd_unet_set_ip_adapter_hw (laid out behind the others: see assign_memory)
        const int id = ctx_tensor(bytes);
        pl.tensors[id].ctx_ip = true;
        return id;
    }
    int tensor(size_t bytes, bool persistent = false) {
        Tn t;
        t.bytes = (bytes + 255) / 256 * 256;
        t.persistent = persistent;
        pl.tensors.push_back(t);
        return (int)pl.tensors.size() - 1;
    }
    size_t W(const std::string& k) {
        auto it = u->woff.find(k);
        if (it == u->woff.end()) {
            if (error.empty()) error = "missing packed weight " + k;
            return 0;
        }
        return it->second;
    }
    Op& push(Op op) {
        op.nwrap = (int)wrapstack.size();
        for (int i = 0; i < op.nwrap; ++i) op.wraps[i] = wrapstack[i];
        pl.ops.push_back(op);
        return pl.ops.back();
    }
    static int pad128(int c) { return (c + 127) / 128 * 128; }
    // fq: the output feeds an fp8 contraction -> e4m3 rows of pad128(C) bytes, scaled by the handle's norm scale
    int gn(int x1, int c1, int x2, int c2, int hw, const std::string& g, const std::string& b, float eps, int silu,
           bool fq = false) {
        Op o; o.kind = OP_GN; o.x1 = x1; o.C1 = c1; o.x2 = x2; o.C2 = c2; o.HW = hw; o.B = UB;
        o.g = W(g); o.be = W(b); o.eps = eps; o.silu = silu;
        o.nsplit = sd_groupnorm_nsplit(UB, hw);
        o.aux = tensor(sd_groupnorm_scratch_bytes(UB, hw, u->cfg.norm_num_groups));
        if (hw % 64 == 0 && !sd_groupnorm_uses_small(UB, hw, c1, c2, u->cfg.norm_num_groups) && stats_of.count(x1) &&
            (x2 < 0 || stats_of.count(x2))) {
            o.s1 = stats_of[x1];
            o.s2 = x2 >= 0 ? stats_of[x2] : -1;
        }
        if (fq) {
            o.out_fp8 = 1; o.Cpad = pad128(c1 + c2); o.sname = u->act_id(stem(g), u->s_norm); o.os = u->act_scale[o.sname];
            o.out = tensor((size_t)UB * hw * o.Cpad); tscale[o.out] = o.os;
        } else o.out = tensor((size_t)UB * hw * (c1 + c2) * 2);
        push(o);
        return o.out;
    }
    // fq: x is an e4m3 tensor of pad128(cin) channels written with activation scale xs
    int conv3(int x, int hin, int win, int cin, int cout, int stride, int up, const std::string& w, const std::string& b,
              long b2idx, int b2t, int r, bool fq = false) {
        Op o; o.kind = OP_CONV3; o.x1 = x; o.B = UB; o.Hin = hin; o.Win = win; o.Cin = cin; o.N = cout;
        o.stride = stride; o.up = up;
        o.Hout = ((hin << up) + 2 - 3) / stride + 1;
        o.Wout = ((win << up) + 2 - 3) / stride + 1;
        o.M = UB * o.Hout * o.Wout; o.K = 9 * cin; o.Kalg = o.K;
        o.b = W(b); o.b2t = b2t; o.b2idx = b2idx; o.r = r;
        if (fq) { o.dt = 1; o.Cin = pad128(cin); o.K = 9 * o.Cin; o.w = W(w + ".fp8"); o.wsc = W(w + ".scale"); o.xs = xscale(x); }
        else o.w = W(w);
        // upsampler: nearest-2x + 3x3 as four 2x2 convs on the low-res input, 4/9 of the multiply-adds (SD_CONV_SUBPIXEL=0: off)
        static const bool subpix_off = getenv("SD_CONV_SUBPIXEL") && atoi(getenv("SD_CONV_SUBPIXEL")) == 0;
        if (up && !fq && !subpix_off && u->kind == 0 && stride == 1 && r < 0 && b2t < 0 && (hin * win) % 64 == 0 &&
            u->woff.count(w + ".sub")) {
            o.subpix = 1; o.K = 4 * cin; o.Kalg = 4 * cin;        // (Kalg: the EXECUTED multiply-adds, 4/9 of the 3x3 form)
            o.w = W(w + ".sub"); o.splitk = 1;
            o.out = tensor((size_t)o.M * cout * 2);
            if ((hin * win) % 128 == 0) want_stats(o, o.M, cout);     // (8x8 inputs run on 64-row tiles: no block statistics)
            push(o);
            return o.out;
        }
        o.splitk = sd_conv3x3_splitk(o.M, o.N, o.Cin, hin, win, stride, up, o.dt);
        if (o.splitk > 1) o.aux = tensor((size_t)o.splitk * o.M * o.N * 4);
        o.out = tensor((size_t)o.M * cout * 2);
        // every 3x3 conv of the UNet feeds a GroupNorm (directly or as a skip); the halo kernel's geometry mode delivers no
        // block statistics (its tiles are not 64-row aligned): that GroupNorm runs its own statistics pass
        GemmArgs g;
        g.M = o.M; g.N = o.N; g.Cin = o.Cin; g.K = o.K; g.ldw = o.K; g.Hin = hin; g.Win = win; g.Hout = o.Hout; g.Wout = o.Wout;
        g.stride = stride; g.up = up; g.dt = o.dt;
        if (sd_conv_halo_mode(g) != 2) want_stats(o, o.M, cout);
        push(o);
        return o.out;
    }
    // fq: x1 is an e4m3 tensor (its scale comes from its producer); oname: name of the e4m3 tensor this GEMM WRITES (GEGLU
    // epilogue only; empty = bf16 output)
    int gemm(int x1, int k1, int x2, int k2, int M, int N, const std::string& w, const std::string& b, int r, int epi,
             bool fq = false, const std::string& oname = "") {
        Op o; o.kind = OP_GEMM; o.x1 = x1; o.x2 = x2; o.K1 = k1; o.K = k1 + k2; o.Kalg = o.K; o.M = M; o.N = N; o.epi = epi;
        o.b = b.empty() ? NOFF : W(b); o.r = r;
        if (fq) { o.dt = 1; o.K = o.K1 = pad128(k1); o.w = W(w + ".fp8"); o.wsc = W(w + ".scale"); o.xs = xscale(x1); }
        else o.w = W(w);
        o.splitk = epi ? 1 : sd_gemm_splitk(M, N, o.dt ? o.K / 2 : o.K, o.dt ? 128 : 0);     // the heuristic counts 128-byte K tiles
        if (o.splitk > 1) o.aux = tensor((size_t)o.splitk * M * N * 4);
        if (!oname.empty()) {
            o.out_fp8 = 1; o.sname = u->act_id(oname, u->s_ff); o.os = u->act_scale[o.sname]; o.Cpad = pad128(N / 2);
            o.out = tensor((size_t)M * o.Cpad); tscale[o.out] = o.os;
        } else o.out = tensor((size_t)M * (epi ? N / 2 : N) * 2);
        push(o);
        return o.out;
    }
    int ln(int x, int M, int C, const std::string& g, const std::string& b, bool fq = false, float eps = 1e-5f) {
        Op o; o.kind = OP_LN; o.x1 = x; o.M = M; o.N = C; o.g = W(g); o.be = W(b); o.eps = eps;
        if (fq) {
            o.out_fp8 = 1; o.Cpad = pad128(C); o.sname = u->act_id(stem(g), u->s_norm); o.os = u->act_scale[o.sname];
            o.out = tensor((size_t)M * o.Cpad); tscale[o.out] = o.os;
        } else o.out = tensor((size_t)M * C * 2);
        push(o);
        return o.out;
    }
    // B: the samples the kernel sees (UB, or UB x tiles for the self-attention of a HyperTile block)
    int attn(int q, long qoff, long ldq, int kv, long koff, long voff, long ldkv, int nq, int nk, int C, int heads, int B) {
        Op o; o.kind = OP_ATTN; o.x1 = q; o.x2 = kv; o.qoff = qoff; o.koff = koff; o.voff = voff;
        o.ldq = ldq; o.ldk = o.ldv = ldkv; o.ldo = C; o.B = B; o.heads = heads; o.D = C / heads;
        o.Nq = nq; o.Nk = nk;
        o.out = tensor((size_t)B * nq * C * 2);
        push(o);
        return o.out;
    }
    // SD_SHORTCUT_FUSE=0: the conv_shortcut of a resnet stays a GEMM of its own (read when a plan is built: two handles of one
    // process can differ)
    bool shortcut_fuse = !(getenv("SD_SHORTCUT_FUSE") && atoi(getenv("SD_SHORTCUT_FUSE")) == 0);
    // ResnetBlock2D (A.3); input may be a virtual channel concat [x1 | x2]
    int resnet(const std::string& p, int x1, int c1, int x2, int c2, int cout, int rh, int rw, int tproj_t) {
        const int hw = rh * rw, cin = c1 + c2, M = UB * hw;
        const bool fq = u->fp8;          // GroupNorm+SiLU writes e4m3, both 3x3 convs contract in fp8
        int t1 = gn(x1, c1, x2, c2, hw, p + "norm1.weight", p + "norm1.bias", u->cfg.norm_eps, 1, fq);
        int t2 = conv3(t1, rh, rw, cin, cout, 1, 0, p + "conv1.weight", p + "conv1.bias", u->tproj_off.at(p), tproj_t, -1, fq);
        int t3 = gn(t2, cout, -1, 0, hw, p + "norm2.weight", p + "norm2.bias", u->cfg.norm_eps, 1, fq);
        int sc = x1;
        if (cin != cout) {
            // The 1x1 shortcut rides on conv2's halo-kernel launch where it can (UNet, bf16): conv2 owns the same output tile in
            // fp32 accumulators, so the GEMM's launch, its rounded output and conv2's residual read all go (conv_halo.hip SC).
            GemmArgs g;
            g.M = M; g.N = cout; g.Cin = cout; g.K = 9 * cout; g.ldw = g.K; g.Hin = g.Hout = rh; g.Win = g.Wout = rw;
            g.Csc1 = c1; g.Csc2 = x2 >= 0 ? c2 : 0;
            if (shortcut_fuse && !fq && u->unet_like() && u->woff.count(p + "conv2.bias+shortcut") && sd_conv_halo_shortcut_applicable(g)) {
                const int out = conv3(t3, rh, rw, cout, cout, 1, 0, p + "conv2.weight", p + "conv2.bias+shortcut", 0, -1, -1, fq);
                Op& o = pl.ops.back();
                o.scx1 = x1; o.scc1 = c1; o.scx2 = x2; o.scc2 = g.Csc2; o.scw = W(p + "conv_shortcut.weight");
                o.Kalg += cin;          // the launch's algorithmic work includes the shortcut's K
                return out;
            }
            sc = gemm(x1, c1, x2, c2, M, cout, p + "conv_shortcut.weight", p + "conv_shortcut.bias", -1, 0);
        }
        return conv3(t3, rh, rw, cout, cout, 1, 0, p + "conv2.weight", p + "conv2.bias", 0, -1, sc, fq);
    }
    // Token Merging: how many src tokens a block on a level of rh x rw tokens merges; 0 = the block does not merge (the setting
    // is off, or the level is past max_downsample).  r = min(num_src, int(N ratio)) as tomesd computes it.
    int tome_r(int rh, int rw, int C) {
        if (u->kind != 0 || u->fp8 || !(u->tome_ratio > 0.0) || rh <= 0 || pl.v.lh / rh > u->tome_max_downsample) return 0;
        const int N = rh * rw;
        if (rh % 2 || rw % 2 || N > 16384 || C % 64 || C > 1536) {
            if (error.empty()) error = "Token Merging needs even token-grid sides, at most 16384 tokens and C a multiple of 64 up to 1536 on "
                                       "every merging level (" + std::to_string(rh) + "x" + std::to_string(rw) + ", C = " + std::to_string(C) + ")";
            return 0;
        }
        return std::min(N - N / 4, (int)((double)N * u->tome_ratio));
    }
    // HyperTile: the tile counts (nh, nw) of a block on rh x rw tokens; 1 x 1 = the block is not tiled (the setting is off, the
    // level is deeper than max_depth, or no divisor gives more than one tile).  The tile side th is the smallest divisor of rh
    // that is >= min(T, rh) -- upstream's first option, what swap_size = 1 selects -- and tw likewise.  UNet handles only (a
    // ControlNet's own handle never tiles).
    static int ht_tile_side(int r, int T) {
        for (int d = std::min(T, r); d <= r; ++d)
            if (r % d == 0) return d;
        return r;
    }
    void hypertile_tiles(int rh, int rw, int* nh, int* nw) {
        *nh = *nw = 1;
        if (u->kind != 0 || u->fp8 || u->ht_tokens <= 0 || rh <= 0 || rw <= 0 || pl.v.lh / rh > (1 << u->ht_max_depth)) return;
        *nh = rh / ht_tile_side(rh, u->ht_tokens);
        *nw = rw / ht_tile_side(rw, u->ht_tokens);
    }
    // Transformer2DModel with one BasicTransformerBlock (A.4).  A HyperTile block (hypertile.hip): ONE gather of the block input
    // into tile order, the whole block on it exactly as the plain plan runs it on x -- every op but attn1 is row-wise or per
    // sample, and the tile order permutes rows inside a sample -- and ONE scatter of the exit GEMM's output (which carries the
    // gathered residual).  The producers' GroupNorm statistics are per 64-row block, summed per sample: they describe a
    // permuted tensor as well as the original, so the entry GroupNorm keeps x's statistics and the next resnet's GroupNorm
    // gets the exit GEMM's.
    // A PAG block (pag.hip; Plan::pag_lb > 0 and the handle's mask names the block): attn1 of the last pag_lb samples is the
    // identity, see transformer_block.  The prompt-independent prefix must end before the first perturbed attn1: when the first
    // transformer block is perturbed the prefix ends at the block's ENTRY -- its input is replicated and the whole block runs at
    // the full batch -- instead of behind attn1.to_out (the rows of attn1 then differ between the samples of one latent).
    int n_transformers = 0;
    int transformer(const std::string& p, int x, int C, int rh, int rw) {
        const int blk = pl.pag_blocks++;
        const bool pert = pl.pag_lb() > 0 && ((u->pag_mask >> blk) & 1);
        if (pert && prefix_rep > 1) {
            x = replicate(x, (size_t)UB * rh * rw * C * 2, prefix_rep);
            UB *= prefix_rep;
            prefix_rep = 1;
        }
        int ht_nh, ht_nw;
        hypertile_tiles(rh, rw, &ht_nh, &ht_nw);
        if (ht_nh * ht_nw == 1) return transformer_block(p, x, C, rh, rw, 1, pert);
        if (u->tome_ratio > 0.0) { if (error.empty()) error = "HyperTile and Token Merging together are not built"; return x; }
        if (sd_hypertile_shape_ok(UB, rh, rw, C, ht_nh, ht_nw, C, "HyperTile")) { if (error.empty()) error = sd_last_error(); return x; }
        pl.hypertile.push_back(Plan::HtBlock{rh, rw, ht_nh, ht_nw});
        int xp;
        { Op o; o.kind = OP_HT_GATHER; o.x1 = x; o.B = UB; o.Hin = rh; o.Win = rw; o.N = C; o.K = ht_nh; o.K1 = ht_nw;
          o.out = xp = tensor((size_t)UB * rh * rw * C * 2); push(o); }
        if (stats_of.count(x)) stats_of[xp] = stats_of[x];
        const int yp = transformer_block(p, xp, C, rh, rw, ht_nh * ht_nw, pert);
        // (UB here: the block may have ended the CFG prefix and doubled it)
        Op o; o.kind = OP_HT_SCATTER; o.x1 = yp; o.B = UB; o.Hin = rh; o.Win = rw; o.N = C; o.K = ht_nh; o.K1 = ht_nw;
        o.out = tensor((size_t)UB * rh * rw * C * 2); push(o);
        if (stats_of.count(yp)) stats_of[o.out] = stats_of[yp];
        return o.out;
    }
    // nt: the tiles per sample (1 = not tiled): attn1 sees UB * nt samples of hw / nt tokens.  pert: a PAG block -- the attention
    // kernel sees the (UB - pag_lb) * nt samples in front, OP_PAG_IDENTITY copies V into the rows of the pag_lb samples behind them
    // (tile order permutes rows inside a sample, so they stay the last pag_lb * hw rows), and to_out runs over all rows as ever
    int transformer_block(const std::string& p, int x, int C, int rh, int rw, int nt, bool pert) {
        const int hw = rh * rw, L = u->cfg.context_len;
        const int NH = block_heads(u->cfg, p), NP = NH * 80;      // heads of the level the block sits on
        int M = UB * hw;
        const std::string t = p + "transformer_blocks.0.";
        const bool fq = u->fp8;
        int g = gn(x, C, -1, 0, hw, p + "norm.weight", p + "norm.bias", 1e-6f, 0, fq);
        int h0 = gemm(g, C, -1, 0, M, C, p + "proj_in.weight", p + "proj_in.bias", -1, 0, fq);
        // Token Merging (tome.hip): norm1 as its own launch, the matching on h0, the merge of norm1's rows; attn1 then runs on
        // Nm = hw - r rows per sample and the unmerge below writes h1 = attn1 output (copied to every member) + h0
        const int tr = tome_r(rh, rw, C);
        const int Nm = hw - tr, Mm = UB * Nm;
        int tome_i = -1;
        int qkv, rs = -1, np = 0;
        if (tr > 0) {
            const int num_dst = hw / 4, num_src = hw - num_dst;
            Plan::TomeBlock tb;
            tb.B = UB; tb.h = rh; tb.w = rw; tb.r = tr; tb.choice_off = pl.tome_choice_bytes;
            pl.tome_choice_bytes += num_dst;
            tb.tok = tensor((size_t)hw * 4, true);
            tb.kept = tensor((size_t)UB * std::max(num_src - tr, 1) * 4, true);
            tb.merged = tensor((size_t)UB * tr * 4, true);
            tb.dst_idx = tensor((size_t)UB * tr * 4, true);
            int n1 = ln(h0, M, C, t + "norm1.weight", t + "norm1.bias");
            int nmax, nidx;
            { Op o; o.kind = OP_TOME_MATCH; o.x1 = h0; o.B = UB; o.Hin = rh; o.Win = rw; o.N = C; o.b2idx = tb.choice_off;
              o.out = nmax = tensor((size_t)UB * num_src * 4); o.aux = nidx = tensor((size_t)UB * num_src * 4);
              o.stats = tb.tok; o.rs = tensor((size_t)UB * hw * 4); push(o); }
            { Op o; o.kind = OP_TOME_SELECT; o.x1 = nmax; o.x2 = nidx; o.B = UB; o.M = num_src; o.K = tr;
              o.out = tb.kept; o.aux = tb.merged; o.stats = tb.dst_idx; push(o); }
            int m;
            { Op o; o.kind = OP_TOME_MERGE; o.x1 = n1; o.x2 = tb.tok; o.r = tb.kept; o.wt = tb.merged; o.s1 = tb.dst_idx;
              o.B = UB; o.Hin = rh; o.Win = rw; o.N = C; o.K = tr; o.out = m = tensor((size_t)Mm * C * 2); push(o); }
            tome_i = (int)pl.tome.size();
            pl.tome.push_back(tb);
            qkv = gemm(m, C, -1, 0, Mm, 3 * C, t + "attn1.qkv.weight", "", -1, 0);
        } else if (!fq && (np = want_rowstats(pl.ops.back(), M, C, rs)) > 0) {       // norm1 folded into the projection
            qkv = gemm_ln(h0, rs, np, M, 3 * C, C, t + "attn1.qkv.weight", 0);
        } else {
            int n1 = ln(h0, M, C, t + "norm1.weight", t + "norm1.bias", fq);
            qkv = gemm(n1, C, -1, 0, M, 3 * C, t + "attn1.qkv.weight", "", -1, 0, fq);
        }
        // 64x64 level (head dim 40): the projection stores K and V head-major, [which][sample][head][token][40] behind the
        // token-major Q block, so that the self-attention's LDS-DMA pieces are contiguous (SD_ATTN_HEADMAJOR=0: off)
        static const bool hm_off = (getenv("SD_ATTN_HEADMAJOR") && atoi(getenv("SD_ATTN_HEADMAJOR")) == 0) ||
                                   getenv("SD_ATTN_NO_PIPE") || getenv("SD_ATTN_NO_DMA") || getenv("SD_GEMM_BIG");
        // (a merging block: the same conditions on its Nm tokens per sample)
        // (a HyperTile block: on the tokens of one tile -- tr == 0 there, so Nm = hw and Na = hw / nt)
        const int Na = Nm / nt;
        const bool hm = !hm_off && C / NH == 40 && C % 160 == 0 && Na % 128 == 0 && Na >= 256 &&
                        sd_gemm_tile_rows(Mm, 3 * C) == 128 && pl.ops.back().splitk == 1;
        if (pert && (tr > 0 || fq || pl.pag_lb() >= UB)) {
            if (error.empty()) error = "PAG with Token Merging or fp8, or a batch without unperturbed samples, is not built";
            return x;
        }
        const int Ba = (pert ? UB - pl.pag_lb() : UB) * nt;      // the samples the attention kernel sees
        const int qkv_op = (int)pl.ops.size() - 1;             // the q | k | v projection (an OP_SAG_MASS may follow it)
        // SAG capture (sag.hip): the mid block's attention mass of all UB samples, from Q and K as the projection left them
        // (token-major, pitch 3 C; W_q carries scale * log2 e).  Reads qkv, writes the handle's buffer: no plan tensor changes.
        if (pl.v.sag && p == "mid_block.attentions.0.") {
            if (nt != 1) { if (error.empty()) error = "SAG with a HyperTile setting that tiles the mid block is not built"; return x; }
            if (tr > 0 || fq || pert) { if (error.empty()) error = "SAG with Token Merging, fp8 or PAG is not built"; return x; }
            if (rh < 4 || rh > 16 || rw < 4 || rw > 16) {
                if (error.empty()) error = "SAG: the mid grid is " + std::to_string(rh) + "x" + std::to_string(rw) + " (4 .. 16 tokens per side)";
                return x;
            }
            if (sd_sag_mass_shape_ok(UB, NH, hw, C / NH, 3 * C, hm ? 1 : 0, "SAG")) { if (error.empty()) error = sd_last_error(); return x; }
            Op o; o.kind = OP_SAG_MASS; o.x1 = qkv; o.B = UB; o.heads = NH; o.D = C / NH; o.Nk = hw; o.Hin = rh; o.Win = rw;
            o.koff = C; o.ldk = 3 * C;
            push(o);
        }
        int a1;
        if (hm) {
            pl.ops[qkv_op].hm = 1;
            pl.ops[qkv_op].HW = Na;
            a1 = attn(qkv, 0, C, qkv, (long)Mm * C, 2l * Mm * C, C, Na, Na, C, NH, Ba);
            pl.ops.back().hm = 1;
        } else {
            a1 = attn(qkv, 0, 3 * C, qkv, C, 2 * C, 3 * C, Na, Na, C, NH, Ba);
        }
        pl.ops.back().qps = 1;          // W_q of attn1 carries the scale (Packer::transformer)
        if (pert) {
            const long row0 = (long)(UB - pl.pag_lb()) * hw, rows = (long)pl.pag_lb() * hw;
            if (sd_pag_identity_shape_ok(Mm, row0, rows, C, NH, 3 * C, hm ? Na : 0, "PAG")) { if (error.empty()) error = sd_last_error(); return x; }
            pl.tensors[a1].bytes = ((size_t)Mm * C * 2 + 255) / 256 * 256;      // (the attention op sized it for its own samples)
            Op o; o.kind = OP_PAG_IDENTITY; o.x1 = qkv; o.out = a1; o.M = Mm; o.N = C; o.heads = NH; o.qoff = row0; o.koff = rows;
            o.hm = hm ? 1 : 0; o.HW = hm ? Na : 0; o.voff = hm ? 2l * Mm * C : 2 * C; o.ldv = 3 * C;
            push(o);
        }
        int h1 = gemm(a1, C, -1, 0, Mm, C, t + "attn1.to_out.0.weight", t + "attn1.to_out.0.bias", tr > 0 ? -1 : h0, 0);
        const int to_out_op = (int)pl.ops.size() - 1;
        if (tr > 0) {
            const Plan::TomeBlock& tb = pl.tome[tome_i];
            Op o; o.kind = OP_TOME_UNMERGE; o.x1 = h1; o.r = h0; o.x2 = tb.tok; o.wt = tb.kept; o.s1 = tb.merged; o.s2 = tb.dst_idx;
            o.B = UB; o.Hin = rh; o.Win = rw; o.N = C; o.K = tr; o.out = tensor((size_t)M * C * 2); push(o);
            h1 = o.out;
        }
        if (prefix_rep > 1) {        // end of the prompt-independent prefix: both CFG halves continue from copies
            x = replicate(x, (size_t)M * C * 2, prefix_rep);
            h1 = replicate(h1, (size_t)M * C * 2, prefix_rep);
            UB *= prefix_rep;
            M = UB * hw;
            prefix_rep = 1;
        }
        // Prompt cross-attention.  The prompt is step-invariant, so per sample and head
        //   A_h = scale * W_q,h^T K_h^T  [C x 77]   and   B_h = V_h W_o,h^T  [77 x C]
        // are computed once per sampling run (sd_unet_set_context; 80 key slots per head, 3 of them padding).
        //  * SD_XATTN_FUSED (levels with >= n tokens, default 1024 = 64x64 and 32x32; 0 = never): ONE launch,
        //    Y = h1 + sum_h softmax_77(X A_h) B_h + b_o with the probabilities kept in registers (xattn.hip);
        //  * SD_XATTN_FOLD (levels with <= n tokens, default 1024; heads * 80 a multiple of 64: 8 or 20 heads, not 5 or 10): two GEMMs with per-sample weights,
        //    P = softmax_77(X A) in the GEMM epilogue and h2 = h1 + P B + b_o;
        //  * otherwise to_q GEMM, the 77-key flash-attention kernel and the to_out GEMM.
        // norm2 (round 5): folded into the first kernel of whichever form runs -- rstd from the row partials attn1.to_out's
        // epilogue delivers, gamma in the operand (A^T centred over the channel: the row mean drops out; the plain to_q weights
        // with the c1 correction), beta as a constant per key slot / output column.  SD_XATTN_LN=0: the separate LayerNorm launch.
        // T-GATE (tgate.hip).  Reuse: norm2, attn2 and their context tensors are gone -- h2 = h1 + the block's cache slice, one
        // launch, which also delivers the row partials norm3's fold reads.  Capture (below): whichever form runs, runs WITHOUT
        // its residual operand, so that its output is y = to_out(attention) + b_o alone, and OP_TGATE_CAPTURE adds the residual.
        const int tg_i = pl.v.tgate ? pl.tg_blocks++ : -1;
        if (pl.v.tgate && (tg_i >= (int)pl.tg_rows.size() || pl.tg_rows[tg_i] != (long)(M / pl.v.tg_pair) || pl.tg_ch[tg_i] != C)) {
            if (error.empty()) error = "T-GATE cache layout (block " + std::to_string(tg_i) + ")";
            return x;
        }
        if (pl.v.tgate == TGATE_REUSE) {
            Op o; o.kind = OP_TGATE_APPLY; o.x1 = h1; o.M = M; o.N = C; o.b2idx = tg_i;
            o.out = tensor((size_t)M * C * 2); push(o);
            return transformer_ff(p, t, x, o.out, M, C, fq);
        }
        static const int fused_min_hw = getenv("SD_XATTN_FUSED") ? atoi(getenv("SD_XATTN_FUSED")) : 1024;
        static const int fold_max_hw = getenv("SD_XATTN_FOLD") ? atoi(getenv("SD_XATTN_FOLD")) : 1024;
        static const bool xln_off = getenv("SD_XATTN_LN") && atoi(getenv("SD_XATTN_LN")) == 0;
        const int xmode = (fused_min_hw > 0 && hw >= fused_min_hw && sd_xattn_fused_applicable(hw, C, NH, L)) ? 0
                          : (hw <= fold_max_hw && hw % 128 == 0 && L <= 80 && NP % 64 == 0) ? 1 : 2;      // (NP is the second GEMM's K: heads % 4 == 0)
        int rs2 = -1, np2 = 0;
        const long rs2_rows = (long)pl.ops[to_out_op].M;     // (< M when the CFG pair was replicated after attn1.to_out ran)
        // (the set_context plan and the forward plan must agree on every operand it writes: the CFG-pair variant replicates the
        // rows after attn1.to_out of the FIRST transformer only -- the fused kernel reads its partials modulo their rows, the
        // GEMM consumers do not, so in the two GEMM forms that block keeps its LayerNorm in EVERY plan variant)
        const bool first_tf = n_transformers++ == 0;
        // (a merging block keeps norm2 as the separate LayerNorm launch: its rows come from the unmerge, not from a GEMM epilogue)
        if (!fq && !xln_off && tr == 0 && (xmode == 0 || (!first_tf && rs2_rows == M)) &&
            u->woff.count(t + (xmode == 2 ? "attn2.to_q.weight.ln" : "attn2.to_q.weight.T.ln"))) {
            if (first_tf) pl.ops[to_out_op].splitk = 1;      // (its row count differs between the plan variants: the split heuristic must not)
            np2 = want_rowstats(pl.ops[to_out_op], (int)rs2_rows, C, rs2);
        }
        int n2 = np2 > 0 ? h1 : ln(h1, M, C, t + "norm2.weight", t + "norm2.bias");
        // K|V of the prompt: projected once per sampling run by sd_unet_set_context
        int kv = ctx_tensor((size_t)UB * L * 2 * C * 2);
        pl.ctx_kv.push_back(kv);
        pl.ctx_w.push_back(W(t + "attn2.kv.weight"));
        pl.ctx_c.push_back(C);
        // IP-Adapter variant: the image branch runs first and writes R' = h1 + sum_h softmax_T(LN(h1) A_ip,h^T) B_ip,h (ip_xattn.hip:
        // its own LayerNorm from the row itself, whatever form and fold the text attention below uses); R' then is the RESIDUAL
        // operand of that form, whose other operands stay as they are:  h2 = h1 + scale to_out(image) + to_out(text) + b_o
        int res = h1;
        if (pl.v.ip) {
            const int at = ctx_ip_tensor((size_t)UB * 32 * C * 2), bt = ctx_ip_tensor((size_t)UB * C * 32 * 2);
            pl.ip_fold.push_back(Plan::IpFold{at, bt, C, W(t + "attn2.to_q.weight.T"), W(t + "attn2.to_out.0.weight"), W(t + "attn2.kv_ip.weight"), NH});
            Op o; o.kind = OP_IP_XATTN; o.x1 = h1; o.wt = at; o.x2 = bt; o.M = M; o.N = C; o.rpb = hw; o.heads = NH;
            o.g = W(t + "norm2.weight"); o.be = W(t + "norm2.bias"); o.eps = 1e-5f;
            o.out = tensor((size_t)M * C * 2); push(o); res = o.out;
        }
        const bool tg_cap = pl.v.tgate == TGATE_CAPTURE;
        int h2;
        if (xmode == 0) {
            int at = ctx_tensor((size_t)UB * NP * C * 2), bw = ctx_tensor((size_t)UB * C * NP * 2);
            Plan::Fold fd{kv, at, bw, C, NH, W(t + (np2 > 0 ? "attn2.to_q.weight.T.ln" : "attn2.to_q.weight.T")), W(t + "attn2.to_out.0.weight"), true};
            if (np2 > 0) { fd.c2 = ctx_tensor((size_t)UB * NP * 4); fd.lnu = W(t + "attn2.to_q.lnu"); }
            pl.ctx_fold.push_back(fd);
            // (the fused kernel always adds a residual tensor: under a T-GATE capture it reads a zeroed one, OP_TGATE_ZERO)
            Op o; o.kind = OP_XATTN; o.x1 = n2; o.r = tg_cap ? tgate_zero((size_t)M * C * 2) : res; o.wt = at; o.x2 = bw; o.M = M; o.N = C; o.K = NP; o.rpb = hw;
            o.sm_valid = L; o.b = W(t + "attn2.to_out.0.bias"); o.heads = NH;
            if (np2 > 0) { o.lnrs = rs2; o.lnnp = np2; o.s1 = fd.c2; o.ldx_o = rs2_rows; }   // (s1: the c2 tensor; ldx_o: rows of the partials)
            o.out = tensor((size_t)M * C * 2); push(o); h2 = o.out;
        } else if (xmode == 1) {
            int at = ctx_tensor((size_t)UB * NP * C * 2), bw = ctx_tensor((size_t)UB * C * NP * 2);
            Plan::Fold fd{kv, at, bw, C, NH, W(t + (np2 > 0 ? "attn2.to_q.weight.T.ln" : "attn2.to_q.weight.T")), W(t + "attn2.to_out.0.weight"), false};
            if (np2 > 0) {      // c1 = row sums of the ROUNDED centred operand (what is left of the mean term), c2 = the beta term
                fd.c2 = ctx_tensor((size_t)UB * NP * 4); fd.lnu = W(t + "attn2.to_q.lnu");
                fd.c1 = ctx_tensor((size_t)UB * NP * 4); fd.ones = W(t + "attn2.to_q.ones");
            }
            pl.ctx_fold.push_back(fd);
            int pr;
            { Op o; o.kind = OP_GEMM; o.x1 = n2; o.K1 = C; o.K = C; o.M = M; o.N = NP; o.epi = 2; o.sm_valid = L;
              o.wt = at; o.wbs = (long)NP * C; o.rpb = hw;
              if (np2 > 0) { o.lnrs = rs2; o.lnnp = np2; o.s1 = fd.c1; o.s2 = fd.c2; }          // (s1 / s2: the per-sample c1 / c2 tensors)
              o.out = tensor((size_t)M * NP * 2); push(o); pr = o.out; }
            { Op o; o.kind = OP_GEMM; o.x1 = pr; o.K1 = NP; o.K = NP; o.M = M; o.N = C; o.epi = 0;
              o.wt = bw; o.wbs = (long)C * NP; o.rpb = hw; o.b = W(t + "attn2.to_out.0.bias"); o.r = tg_cap ? -1 : res;
              o.out = tensor((size_t)M * C * 2); push(o); h2 = o.out; }
        } else {
            int q2 = np2 > 0 ? gemm_ln(h1, rs2, np2, M, C, C, t + "attn2.to_q.weight", 0)
                             : gemm(n2, C, -1, 0, M, C, t + "attn2.to_q.weight", "", -1, 0);
            int a2 = attn(q2, 0, C, kv, 0, C, 2 * C, hw, L, C, NH, UB);
            h2 = gemm(a2, C, -1, 0, M, C, t + "attn2.to_out.0.weight", t + "attn2.to_out.0.bias", tg_cap ? -1 : res, 0);
        }
        if (tg_cap) {
            Op o; o.kind = OP_TGATE_CAPTURE; o.x1 = h2; o.r = res; o.M = M; o.N = C; o.K = pl.v.tg_pair; o.b2idx = tg_i;
            o.out = tensor((size_t)M * C * 2); push(o); h2 = o.out;
        }
        return transformer_ff(p, t, x, h2, M, C, fq);
    }
    // the feed-forward half of a BasicTransformerBlock and the Transformer2DModel's exit (h2 = the residual stream after attn2,
    // produced by the op pushed last; x = the block's input)
    int transformer_ff(const std::string& p, const std::string& t, int x, int h2, int M, int C, bool fq) {
        int rs = -1, np = 0;
        int ff;
        if (!fq && (np = want_rowstats(pl.ops.back(), M, C, rs)) > 0) {       // norm3 folded into the GEGLU projection
            ff = gemm_ln(h2, rs, np, M, 8 * C, C, t + "ff.geglu.weight", 1);
        } else {
            int n3 = ln(h2, M, C, t + "norm3.weight", t + "norm3.bias", fq);
            ff = gemm(n3, C, -1, 0, M, 8 * C, t + "ff.geglu.weight", t + "ff.geglu.bias", -1, 1, fq, fq ? t + "ff.net.0" : std::string());
        }
        // ff.net.2 + residual + proj_out + residual as ONE GEMM over [ff | h2] (Packer::ff_out_merge; SD_FF_MERGE=0: two)
        static const bool merge_off = getenv("SD_FF_MERGE") && atoi(getenv("SD_FF_MERGE")) == 0;
        int out;
        if (!fq && !merge_off) {
            out = gemm(ff, 4 * C, h2, C, M, C, p + "ff_out.weight", p + "ff_out.bias", x, 0);
        } else {
            int h3 = gemm(ff, 4 * C, -1, 0, M, C, t + "ff.net.2.weight", t + "ff.net.2.bias", h2, 0, fq);
            out = gemm(h3, C, -1, 0, M, C, p + "proj_out.weight", p + "proj_out.bias", x, 0);
        }
        // the block's output feeds the next resnet's GroupNorm (not at the small levels: their GroupNorms are single-launch or
        // fall back to their own pass, and the statistics epilogue would keep this GEMM on 128-row tiles)
        if (pl.ops.back().splitk == 1 && sd_gemm_tile_rows(M, C, pl.ops.back().K) == 128) want_stats(pl.ops.back(), M, C);
        return out;
    }
    // ---- AutoencoderKL decoder: latents/scale -> post_quant_conv -> decoder -> image ----
    int vae_resnet(const std::string& p, int x, int cin, int cout, int rh, int rw) {
        const int hw = rh * rw, M = UB * hw;
        int t1 = gn(x, cin, -1, 0, hw, p + "norm1.weight", p + "norm1.bias", 1e-6f, 1);
        int t2 = conv3(t1, rh, rw, cin, cout, 1, 0, p + "conv1.weight", p + "conv1.bias", 0, -1, -1);
        int t3 = gn(t2, cout, -1, 0, hw, p + "norm2.weight", p + "norm2.bias", 1e-6f, 1);
        int sc = x;
        if (cin != cout) sc = gemm(x, cin, -1, 0, M, cout, p + "conv_shortcut.weight", p + "conv_shortcut.bias", -1, 0);
        return conv3(t3, rh, rw, cout, cout, 1, 0, p + "conv2.weight", p + "conv2.bias", 0, -1, sc);
    }
    // single-head attention with head dim C (512): too wide for the flash kernel's register tile, so it
    // is three GEMMs per image (S = Q K^T, row softmax, O = P V with V^T produced directly by a GEMM).
    // Up to 4096 tokens S holds all query rows of an image; beyond that the query rows go in chunks of
    // 2048 (S <= 2048 x 16384 bf16 = 64 MiB at a 128x128 latent) and the softmax is the long-row kernel.
    int vae_attention(const std::string& p, int x, int C, int rh, int rw) {
        const int hw = rh * rw, M = UB * hw;
        const int qc = hw <= 4096 ? hw : 2048;      // query rows per S chunk
        int g = gn(x, C, -1, 0, hw, p + "group_norm.weight", p + "group_norm.bias", 1e-6f, 0);
        int qk = gemm(g, C, -1, 0, M, 2 * C, p + "qk.weight", p + "qk.bias", -1, 0);
        const int vT = tensor((size_t)UB * C * hw * 2), S = tensor((size_t)qc * hw * 2), O = tensor((size_t)M * C * 2);
        for (int img = 0; img < UB; ++img) {
            {   // V^T[C, hw] = Wv[C, C] . g_img[hw, C]^T   (bias of V is added to O: rows of P sum to 1)
                Op o; o.kind = OP_GEMM; o.wx = W(p + "to_v.weight"); o.ldx_o = C; o.K1 = C; o.K = C; o.M = C; o.N = hw;
                o.wt = g; o.woff_el = (long)img * hw * C; o.ldw_o = C;
                o.out = vT; o.coff = (long)img * C * hw; o.ldc_o = hw;
                push(o);
            }
            for (int q0 = 0; q0 < hw; q0 += qc) {
                const int rows = std::min(qc, hw - q0);
                {   // S[rows, hw] = Q_img[q0 : q0 + rows] . K_img^T
                    Op o; o.kind = OP_GEMM; o.x1 = qk; o.xoff = ((long)img * hw + q0) * 2 * C; o.ldx_o = 2 * C; o.K1 = C; o.K = C;
                    o.M = rows; o.N = hw; o.wt = qk; o.woff_el = (long)img * hw * 2 * C + C; o.ldw_o = 2 * C;
                    o.out = S; o.ldc_o = hw;
                    push(o);
                }
                { Op o; o.kind = OP_SOFTMAX; o.x1 = S; o.out = S; o.M = rows; o.N = hw; o.scale = 1.0f / sqrtf((float)C); push(o); }
                {   // O_img[q0 : q0 + rows, C] = P . V + b_v
                    Op o; o.kind = OP_GEMM; o.x1 = S; o.ldx_o = hw; o.K1 = hw; o.K = hw; o.M = rows; o.N = C;
                    o.wt = vT; o.woff_el = (long)img * C * hw; o.ldw_o = hw; o.b = W(p + "to_v.bias");
                    o.out = O; o.coff = ((long)img * hw + q0) * C; o.ldc_o = C;
                    push(o);
                }
            }
        }
        return gemm(O, C, -1, 0, M, C, p + "to_out.0.weight", p + "to_out.0.bias", x, 0);
    }
    void build_vae() {
        const sd_unet_config& c = u->cfg;
        const int nl = c.num_levels, top = c.block_out_channels[nl - 1];
        int rh = pl.v.lh, rw = pl.v.lw;
        int t_pq = tensor((size_t)UB * c.in_channels * rh * rw * 4);
        { Op o; o.kind = OP_PQCONV; o.x1 = T_LATENTS; o.out = t_pq; o.B = UB; o.HW = rh * rw;
          o.w = W("post_quant_conv.weight"); o.b = W("post_quant_conv.bias"); push(o); }
        int h;
        { Op o; o.kind = OP_CONV_IN; o.x1 = t_pq; o.B = UB; o.Hin = rh; o.Win = rw; o.Cin = c.in_channels; o.N = top;
          o.w = W("decoder.conv_in.weight"); o.b = W("decoder.conv_in.bias"); o.out = tensor((size_t)UB * rh * rw * top * 2);
          push(o); h = o.out; }
        pl.taps["conv_in"] = h;
        h = vae_resnet("decoder.mid_block.resnets.0.", h, top, top, rh, rw);
        h = vae_attention("decoder.mid_block.attentions.0.", h, top, rh, rw);
        h = vae_resnet("decoder.mid_block.resnets.1.", h, top, top, rh, rw);
        pl.taps["mid"] = h;
        int ch = top;
        for (int i = 0; i < nl; ++i) {
            const int co = c.block_out_channels[nl - 1 - i];
            const std::string bp = "decoder.up_blocks." + std::to_string(i) + ".";
            for (int j = 0; j < c.layers_per_block + 1; ++j) {
                h = vae_resnet(bp + "resnets." + std::to_string(j) + ".", h, ch, co, rh, rw);
                ch = co;
            }
            if (i < nl - 1) {
                h = conv3(h, rh, rw, co, co, 1, 1, bp + "upsamplers.0.conv.weight", bp + "upsamplers.0.conv.bias", 0, -1, -1);
                rh *= 2; rw *= 2;
            }
            pl.taps["up" + std::to_string(i)] = h;
        }
        int g = gn(h, ch, -1, 0, rh * rw, "decoder.conv_norm_out.weight", "decoder.conv_norm_out.bias", 1e-6f, 1);
        { Op o; o.kind = OP_CONV_OUT; o.x1 = g; o.out = T_EPS; o.B = UB; o.Hin = rh; o.Win = rw; o.Cin = ch; o.N = c.out_channels;
          o.w = W("decoder.conv_out.weight"); o.b = W("decoder.conv_out.bias"); push(o); }
    }

    // ---- AutoencoderKL encoder (diffusers 0.32.1 AutoencoderKL.encode, upstream-recall): image -> moments [mean | logvar] ----
    // The plan's (lh, lw) is the LATENT size; the image is 2^(levels - 1) times that.  Entry and exit are kernels of their
    // own (small.hip); everything between runs on the decoder's ops, with the downsamplers on the conv's asymmetric mode.
    void build_vae_encoder() {
        const sd_unet_config& c = u->cfg;
        const int nl = c.num_levels, top = c.block_out_channels[nl - 1], c0 = c.block_out_channels[0];
        int rh = pl.v.lh << (nl - 1), rw = pl.v.lw << (nl - 1);
        int h;
        { Op o; o.kind = OP_CONV_IN_IMG; o.x1 = T_LATENTS; o.B = UB; o.Hin = rh; o.Win = rw; o.Cin = c.out_channels; o.N = c0;
          o.w = W("encoder.conv_in.weight"); o.b = W("encoder.conv_in.bias"); o.out = tensor((size_t)UB * rh * rw * c0 * 2);
          push(o); h = o.out; }
        pl.taps["conv_in"] = h;
        int ch = c0;
        for (int i = 0; i < nl; ++i) {
            const int co = c.block_out_channels[i];
            const std::string bp = "encoder.down_blocks." + std::to_string(i) + ".";
            for (int j = 0; j < c.layers_per_block; ++j) {
                h = vae_resnet(bp + "resnets." + std::to_string(j) + ".", h, ch, co, rh, rw);
                ch = co;
            }
            if (i < nl - 1) {
                h = conv3(h, rh, rw, co, co, 2, 0, bp + "downsamplers.0.conv.weight", bp + "downsamplers.0.conv.bias", 0, -1, -1);
                pl.ops.back().asym = 1;
                rh /= 2; rw /= 2;
            }
            pl.taps["down" + std::to_string(i)] = h;
        }
        h = vae_resnet("encoder.mid_block.resnets.0.", h, top, top, rh, rw);
        h = vae_attention("encoder.mid_block.attentions.0.", h, top, rh, rw);
        h = vae_resnet("encoder.mid_block.resnets.1.", h, top, top, rh, rw);
        pl.taps["mid"] = h;
        int g = gn(h, top, -1, 0, rh * rw, "encoder.conv_norm_out.weight", "encoder.conv_norm_out.bias", 1e-6f, 1);
        { Op o; o.kind = OP_ENC_OUT; o.x1 = g; o.out = T_EPS; o.B = UB; o.Hin = rh; o.Win = rw; o.Cin = top; o.N = 2 * c.in_channels;
          o.w = W("encoder.conv_out.weight"); o.b = W("encoder.conv_out.bias");
          o.g = W("quant_conv.weight"); o.be = W("quant_conv.bias"); push(o); }
    }

    // one pre-LN encoder layer of either CLIP tower (p = the layer's prefix, t = the residual stream [M][H]); `attn_kind` =
    // OP_CLIP_ATTN (causal) or OP_VIT_ATTN, over L tokens per sample; gelu: the exact (erf) GELU instead of quick_gelu.  A
    // vision tower with head dim 80 (ViT-H/14) runs its non-causal attention on the general attention kernels, reading q | k | v
    // in place from the strided projection output
    int clip_encoder_layer(const std::string& p, int t, int M, int L, int H, int I, int heads, int attn_kind, bool gelu = false) {
        const std::string a = p + "self_attn.";
        int n1 = ln(t, M, H, p + "layer_norm1.weight", p + "layer_norm1.bias");
        int qkv = gemm(n1, H, -1, 0, M, 3 * H, a + "qkv.weight", a + "qkv.bias", -1, 0);
        int at;
        if (attn_kind == OP_VIT_ATTN && H / heads == 80) {
            Op o; o.kind = OP_ATTN; o.x1 = qkv; o.x2 = qkv; o.qoff = 0; o.koff = H; o.voff = 2 * H; o.ldq = o.ldk = o.ldv = 3 * H;
            o.ldo = H; o.B = UB; o.heads = heads; o.D = 80; o.Nq = L; o.Nk = L;
            o.out = tensor((size_t)M * H * 2); push(o); at = o.out;
        } else {
            Op o; o.kind = attn_kind; o.x1 = qkv; o.B = UB; o.Nq = L; o.N = H; o.heads = heads;
            o.out = tensor((size_t)M * H * 2); push(o); at = o.out;
        }
        t = gemm(at, H, -1, 0, M, H, a + "out_proj.weight", a + "out_proj.bias", t, 0);
        int n2 = ln(t, M, H, p + "layer_norm2.weight", p + "layer_norm2.bias");
        int f = gemm(n2, H, -1, 0, M, I, p + "mlp.fc1.weight", p + "mlp.fc1.bias", -1, 0);
        { Op o; o.kind = OP_QGELU; o.x1 = f; o.out = f; o.M = M; o.N = I; o.epi = gelu ? 1 : 0; push(o); }      // (epi 1: exact GELU)
        return gemm(f, I, -1, 0, M, H, p + "mlp.fc2.weight", p + "mlp.fc2.bias", t, 0);
    }

    // CLIPTextTransformer (transformers 4.48.0 modeling_clip.py): token + position embedding,
    // pre-LN layers with causal self-attention and a quick_gelu (or, sd_clip_config::hidden_act, exact gelu) MLP, final
    // LayerNorm -> last_hidden_state
    void build_clip() {
        const sd_clip_config& c = u->clip;
        const int L = c.max_positions, H = c.hidden_size, I = c.intermediate_size, M = UB * L;
        int t;
        { Op o; o.kind = OP_CLIP_EMBED; o.x1 = T_LATENTS; o.M = M; o.N = H; o.Nk = L;
          o.w = W("text_model.embeddings.token_embedding.weight"); o.g = W("text_model.embeddings.position_embedding.weight");
          o.out = tensor((size_t)M * H * 2); push(o); t = o.out; }
        for (int i = 0; i < c.num_layers; ++i) {
            t = clip_encoder_layer(clip_layer(i), t, M, L, H, I, c.num_heads, OP_CLIP_ATTN, c.hidden_act == SD_ACT_GELU);
            pl.taps["layer" + std::to_string(i)] = t;
        }
        if (pl.v.rep == REP_TEXT_POOLED) {      // pooled + projected variant (sd_clip_text_embeds): the EOS row, final LayerNorm, text_projection
            int pr;
            { Op o; o.kind = OP_POOL; o.x1 = t; o.pool_by_ids = 1; o.B = UB; o.Nq = L; o.N = H; o.out = tensor((size_t)UB * H * 2); push(o); pr = o.out; }
            int f = ln(pr, UB, H, "text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias");
            int e = gemm(f, H, -1, 0, UB, u->text_proj, "text_projection.weight", "", -1, 0);
            { Op o; o.kind = OP_TO_F32; o.x1 = e; o.out = T_EPS; o.M = UB; o.N = u->text_proj; push(o); }
            return;
        }
        int f = ln(t, M, H, "text_model.final_layer_norm.weight", "text_model.final_layer_norm.bias");
        { Op o; o.kind = OP_TO_F32; o.x1 = f; o.out = T_EPS; o.M = M; o.N = H; push(o); }
    }

    // CLIPVisionModelWithProjection (transformers modeling_clip.py): CLIPImageProcessor on the uint8 input (OP_VIT_PREP), patch
    // embedding as a GEMM over the patch rows (no bias), class token + position embedding, pre_layrnorm, the pre-LN encoder
    // layers with NON-causal attention, post_layernorm of the class-token row, visual_projection (no bias) -> image_embeds
    void build_vit() {
        const sd_clip_vision_config& c = u->vis;
        const int S = c.image_size, P = c.patch_size, G = S / P, Np = G * G, L = Np + 1;
        const int H = c.hidden_size, I = c.intermediate_size, Kp = vit_kp(c), M = UB * L;
        if (sd_clip_prep_tables(pl.v.lh, pl.v.lw, S, pl.prep_tab, pl.geom)) { error = sd_last_error(); return; }
        int patches;
        { Op o; o.kind = OP_VIT_PREP; o.x1 = T_LATENTS; o.B = UB; o.K = Kp; o.Cin = P;
          o.aux = tensor((size_t)UB * 3 * pl.geom.R * S); o.out = tensor((size_t)UB * Np * Kp * 2); push(o); patches = o.out; }
        int pe = gemm(patches, Kp, -1, 0, UB * Np, H, "vision_model.embeddings.patch_embedding.weight", "", -1, 0);
        int t;
        { Op o; o.kind = OP_VIT_EMBED; o.x1 = pe; o.B = UB; o.Nq = Np; o.N = H;
          o.b = W("vision_model.embeddings.class_embedding"); o.g = W("vision_model.embeddings.position_embedding.weight");
          o.out = tensor((size_t)M * H * 2); push(o); t = o.out; }
        t = ln(t, M, H, "vision_model.pre_layrnorm.weight", "vision_model.pre_layrnorm.bias");
        for (int i = 0; i < c.num_layers; ++i) {
            t = clip_encoder_layer(vit_layer(i), t, M, L, H, I, c.num_heads, OP_VIT_ATTN, c.hidden_act == SD_ACT_GELU);
            pl.taps["layer" + std::to_string(i)] = t;
        }
        int pr;
        { Op o; o.kind = OP_POOL; o.x1 = t; o.B = UB; o.Nq = L; o.N = H; o.out = tensor((size_t)UB * H * 2); push(o); pr = o.out; }
        int f = ln(pr, UB, H, "vision_model.post_layernorm.weight", "vision_model.post_layernorm.bias");
        int e = gemm(f, H, -1, 0, UB, c.projection_dim, "visual_projection.weight", "", -1, 0);
        { Op o; o.kind = OP_TO_F32; o.x1 = e; o.out = T_EPS; o.M = UB; o.N = c.projection_dim; push(o); }
    }

    // ---- ImageReward (kind 6): both towers in ONE plan per (batch, text length, image H, W) ----
    // BLIP's ViT (timm VisionTransformer as BLIP's vit.py builds it): the patch embedding as a GEMM over the patch rows (its bias
    // rides in the position rows, Packer), class token + position embedding, NO pre-LayerNorm, pre-LN blocks with the fused
    // attn.qkv as given and the exact GELU, the final `norm` over ALL rows.  Returns the image tokens [UB * L][H], bf16.
    int ln_eps(int x, int M, int C, const std::string& n, float eps) { return ln(x, M, C, n + ".weight", n + ".bias", false, eps); }
    int lin(int x, int K, int M, int N, const std::string& n, int r = -1) { return gemm(x, K, -1, 0, M, N, n + ".weight", n + ".bias", r, 0); }
    int build_blip_vision(int* tokens) {
        const sd_image_reward_config& c = u->ir;
        const int S = c.image_size, P = c.patch_size, G = S / P, Np = G * G, L = Np + 1;
        const int H = c.vision_hidden_size, I = c.vision_intermediate_size, Kp = blip_kp(c), M = UB * L;
        const float eps = c.vision_layer_norm_eps;
        *tokens = L;
        if (sd_clip_prep_tables(pl.v.lh, pl.v.lw, S, pl.prep_tab, pl.geom)) { error = sd_last_error(); return -1; }
        int patches;
        { Op o; o.kind = OP_VIT_PREP; o.x1 = T_LATENTS; o.B = UB; o.K = Kp; o.Cin = P;
          o.aux = tensor((size_t)UB * 3 * pl.geom.R * S); o.out = tensor((size_t)UB * Np * Kp * 2); push(o); patches = o.out; }
        int pe = gemm(patches, Kp, -1, 0, UB * Np, H, "visual_encoder.patch_embed.proj.weight", "", -1, 0);
        int t;
        { Op o; o.kind = OP_VIT_EMBED; o.x1 = pe; o.B = UB; o.Nq = Np; o.N = H;
          o.b = W("visual_encoder.cls_token"); o.g = W("visual_encoder.pos_embed");
          o.out = tensor((size_t)M * H * 2); push(o); t = o.out; }
        for (int i = 0; i < c.vision_num_layers; ++i) {
            const std::string p = blip_block(i);
            int n1 = ln_eps(t, M, H, p + "norm1", eps);
            int qkv = lin(n1, H, M, 3 * H, p + "attn.qkv");
            int at;
            { Op o; o.kind = OP_VIT_ATTN; o.x1 = qkv; o.B = UB; o.Nq = L; o.N = H; o.heads = c.vision_num_heads;
              o.out = tensor((size_t)M * H * 2); push(o); at = o.out; }
            t = lin(at, H, M, H, p + "attn.proj", t);
            int n2 = ln_eps(t, M, H, p + "norm2", eps);
            int f = lin(n2, H, M, I, p + "mlp.fc1");
            { Op o; o.kind = OP_QGELU; o.x1 = f; o.out = f; o.M = M; o.N = I; o.epi = 1; push(o); }
            t = lin(f, I, M, H, p + "mlp.fc2", t);
        }
        return ln_eps(t, M, H, "visual_encoder.norm", eps);
    }
    // masked attention of the text encoder (bert.hip): q at column qoff of tensor q (pitch ldq), k / v at columns koff / voff
    // of tensor kv (pitch ldkv); mask: the keys carry the call's attention mask
    int bert_attn(int q, long qoff, long ldq, int kv, long koff, long voff, long ldkv, int nq, int nk, int H, int heads, int mask) {
        Op o; o.kind = OP_BERT_ATTN; o.x1 = q; o.x2 = kv; o.qoff = qoff; o.koff = koff; o.voff = voff;
        o.ldq = ldq; o.ldk = o.ldv = ldkv; o.ldo = H; o.B = UB; o.heads = heads; o.D = H / heads; o.Nq = nq; o.Nk = nk;
        o.key_mask = mask;
        o.out = tensor((size_t)UB * nq * H * 2);
        push(o);
        return o.out;
    }
    // BLIP's text encoder (its med.py BertModel in multimodal mode) over Lt = Plan::rep tokens per prompt: word + position
    // embedding and LayerNorm, then post-LN layers -- self-attention under the key-padding mask, cross-attention over the image
    // tokens (no mask), GELU MLP -- and the reward head on the class-token rows.  The image tokens are the same for every layer,
    // so K | V of ALL layers' cross-attentions come from one GEMM (N = layers * 2 * H, K = encoder width) and each layer's
    // attention reads its slice through the column offset.
    void build_blip_text(int img, int Lv) {
        const sd_image_reward_config& c = u->ir;
        const int Lt = pl.v.rep, H = c.hidden_size, I = c.intermediate_size, EW = c.vision_hidden_size, M = UB * Lt, NL = c.num_layers;
        const float eps = c.layer_norm_eps;
        const long ldkv = (long)NL * 2 * H;
        int kvall = lin(img, EW, UB * Lv, NL * 2 * H, "text_encoder.cross_kv");
        int h;
        { Op o; o.kind = OP_CLIP_EMBED; o.x1 = T_LATENTS; o.M = M; o.N = H; o.Nk = Lt;
          o.w = W("text_encoder.embeddings.word_embeddings.weight"); o.g = W("text_encoder.embeddings.position_embeddings.weight");
          o.out = tensor((size_t)M * H * 2); push(o); h = o.out; }
        h = ln_eps(h, M, H, "text_encoder.embeddings.LayerNorm", eps);
        for (int i = 0; i < NL; ++i) {
            const std::string p = blip_text_layer(i);
            int qkv = lin(h, H, M, 3 * H, p + "attention.self.qkv");
            int a1 = bert_attn(qkv, 0, 3 * H, qkv, H, 2 * H, 3 * H, Lt, Lt, H, c.num_heads, 1);
            h = ln_eps(lin(a1, H, M, H, p + "attention.output.dense", h), M, H, p + "attention.output.LayerNorm", eps);
            int q2 = lin(h, H, M, H, p + "crossattention.self.query");
            int a2 = bert_attn(q2, 0, H, kvall, (long)i * 2 * H, (long)i * 2 * H + H, ldkv, Lt, Lv, H, c.num_heads, 0);
            h = ln_eps(lin(a2, H, M, H, p + "crossattention.output.dense", h), M, H, p + "crossattention.output.LayerNorm", eps);
            int f = lin(h, H, M, I, p + "intermediate.dense");
            { Op o; o.kind = OP_QGELU; o.x1 = f; o.out = f; o.M = M; o.N = I; o.epi = 1; push(o); }
            h = ln_eps(lin(f, I, M, H, p + "output.dense", h), M, H, p + "output.LayerNorm", eps);
            pl.taps["text_layer" + std::to_string(i)] = h;
        }
        { Op o; o.kind = OP_REWARD_HEAD; o.x1 = h; o.out = T_EPS; o.B = UB; o.N = H; o.Nq = Lt;
          o.w = W("reward_head.weight"); o.b = W("reward_head.bias"); push(o); }
    }
    void build_image_reward() {
        int Lv = 0;
        const int img = build_blip_vision(&Lv);
        if (img < 0) return;
        pl.taps["image_tokens"] = img;
        build_blip_text(img, Lv);
    }

    void build() {
        if (u->kind == 6) { build_image_reward(); return; }
        if (u->kind == 1) { build_vae(); return; }
        if (u->kind == 2) { build_clip(); return; }
        if (u->kind == 3) { build_vit(); return; }
        if (u->kind == 4) { build_vae_encoder(); return; }
        const sd_unet_config& c = u->cfg;
        const int nl = c.num_levels, c0 = c.block_out_channels[0], temb = 4 * c0;
        const int L = c.context_len;
        if (pl.v.tgate) {
            pl.tg_batch = UB / pl.v.tg_pair;
            tgate_segments(c, pl.tg_batch, pl.v.lh, pl.v.lw, &pl.tg_off, &pl.tg_rows, &pl.tg_ch);
        }
        // (a T-GATE reuse plan has no prompt cross-attention: no context tensor at all, sd_unet_set_context_hw is not needed for it)
        if (pl.v.tgate != TGATE_REUSE) pl.ctx_bf16 = ctx_tensor((size_t)UB * L * c.cross_attention_dim * 2);
        // masked K / V expansions used by sd_unet_set_context for the folded cross-attention: sized for the level with the most
        // (head, key slot) rows x channels (the mid block sits on the last level)
        size_t fold_max = 0;
        for (int i = 0; i < nl; ++i)
            if (c.attn_levels[i] || i == nl - 1) fold_max = std::max(fold_max, (size_t)level_heads(c, i) * 80 * c.block_out_channels[i]);
        if (pl.v.tgate != TGATE_REUSE) pl.ctx_fold_scratch = ctx_tensor((size_t)3 * UB * fold_max * 2);
        if (pl.v.ip) {      // what sd_unet_set_ip_adapter_hw computes on the way to the folded operands (its expansions reuse the scratch above)
            const int T = c.ip_adapter_tokens, CD = c.cross_attention_dim;
            int cmax = 0;
            for (int i = 0; i < nl; ++i) cmax = std::max(cmax, c.block_out_channels[i]);
            pl.ip_e = ctx_ip_tensor((size_t)UB * c.ip_adapter_embed_dim * 2);
            pl.ip_proj = ctx_ip_tensor((size_t)UB * T * CD * 2);
            pl.ip_tok = ctx_ip_tensor((size_t)UB * T * CD * 2);
            pl.ip_kv = ctx_ip_tensor((size_t)UB * T * 2 * cmax * 2);
        }
        // ---- time embedding (M = 1: the reference passes one scalar t per call) ----
        int t_sin = tensor((size_t)c0 * 4), t_h1 = tensor((size_t)temb * 4), t_emb = tensor((size_t)temb * 4);
        int t_proj = tensor((size_t)u->tproj_total * 4);
        { Op o; o.kind = OP_SINUSOID; o.out = t_sin; o.N = c0; push(o); }
        { Op o; o.kind = OP_GEMV; o.x1 = t_sin; o.out = t_h1; o.N = temb; o.K = c0; o.w = W("time_embedding.linear_1.weight"); o.b = W("time_embedding.linear_1.bias"); push(o); }
        { Op o; o.kind = OP_GEMV; o.x1 = t_h1; o.out = t_emb; o.N = temb; o.K = temb; o.silu_in = 1; o.w = W("time_embedding.linear_2.weight"); o.b = W("time_embedding.linear_2.bias"); push(o); }
        { Op o; o.kind = OP_GEMV; o.x1 = t_emb; o.out = t_proj; o.N = (int)u->tproj_total; o.K = temb; o.silu_in = 1; o.w = W("tproj.weight"); o.b = W("tproj.bias"); push(o); }
        // ---- conv_in ----
        int rh = pl.v.lh, rw = pl.v.lw;
        int h;
        // (restored by the first transformer block; a PAG plan of a UNet without one on its first level runs without the prefix)
        if (pl.v.rep > 1 && (!pl.pag_lb() || c.attn_levels[0])) { prefix_rep = pl.v.rep; UB /= pl.v.rep; }
        { Op o; o.kind = OP_CONV_IN; o.x1 = T_LATENTS; o.B = UB; o.Hin = rh; o.Win = rw; o.Cin = c.in_channels; o.N = c0;
          o.w = W("conv_in.weight"); o.b = W("conv_in.bias"); o.out = tensor((size_t)UB * rh * rw * c0 * 2); push(o); h = o.out; }
        const int h_skip = prefix_rep > 1 ? replicate(h, (size_t)UB * rh * rw * c0 * 2, prefix_rep) : h;
        pl.taps["conv_in"] = h_skip;
        int ch = c0;
        std::vector<int> skips{h_skip}, skip_ch{c0}, skip_hw{rh * rw};
        // ---- down ----
        for (int i = 0; i < nl; ++i) {
            const int co = c.block_out_channels[i];
            const std::string bp = "down_blocks." + std::to_string(i) + ".";
            wrapstack.push_back(Wrap{0, i, 0});
            for (int j = 0; j < c.layers_per_block; ++j) {
                wrapstack.push_back(Wrap{0, i, j});
                h = resnet(bp + "resnets." + std::to_string(j) + ".", h, ch, -1, 0, co, rh, rw, t_proj);
                ch = co;
                if (c.attn_levels[i]) h = transformer(bp + "attentions." + std::to_string(j) + ".", h, co, rh, rw);
                wrapstack.pop_back();
                skips.push_back(h); skip_ch.push_back(co); skip_hw.push_back(rh * rw);
            }
            if (i < nl - 1) {
                wrapstack.push_back(Wrap{0, i, c.layers_per_block});
                const std::string d = bp + "downsamplers.0.conv.";
                h = conv3(h, rh, rw, co, co, 2, 0, d + "weight", d + "bias", 0, -1, -1);
                wrapstack.pop_back();
                rh /= 2; rw /= 2;
                skips.push_back(h); skip_ch.push_back(co); skip_hw.push_back(rh * rw);
            }
            wrapstack.pop_back();
            pl.taps["down" + std::to_string(i)] = h;
        }
        // ---- mid ----
        wrapstack.push_back(Wrap{1, 0, 0});
        h = resnet("mid_block.resnets.0.", h, ch, -1, 0, ch, rh, rw, t_proj);
        h = transformer("mid_block.attentions.0.", h, ch, rh, rw);
        h = resnet("mid_block.resnets.1.", h, ch, -1, 0, ch, rh, rw, t_proj);
        wrapstack.pop_back();
        pl.taps["mid"] = h;
        skips.push_back(h); skip_ch.push_back(ch); skip_hw.push_back(rh * rw);       // (the mid output: the thirteenth residual)
        if ((int)skips.size() > MAX_CONTROL_RES && (u->kind == 5 || pl.v.cn)) { error = "more than 16 ControlNet residuals"; return; }
        control_segments(c, UB, pl.v.lh, pl.v.lw, &pl.cn_off, &pl.cn_count);
        if (u->kind == 5) {
            // ---- ControlNet: the zero convs, one 1x1 GEMM per residual straight into the caller's buffer (T_EPS at the segment's
            // offset, unscaled: conditioning_scale is applied where the residuals are consumed) ----
            for (size_t i = 0; i < skips.size(); ++i) {
                const bool mid = i + 1 == skips.size();
                const std::string w = mid ? "controlnet_mid_block." : "controlnet_down_blocks." + std::to_string(i) + ".";
                const int C = skip_ch[i], M = UB * skip_hw[i];
                if ((long)M * C != pl.cn_count[i]) { error = "ControlNet residual layout"; return; }
                Op o; o.kind = OP_GEMM; o.x1 = skips[i]; o.K1 = o.K = o.Kalg = C; o.M = M; o.N = C;
                o.w = W(w + "weight"); o.b = W(w + "bias");
                o.splitk = sd_gemm_splitk(M, C, C, 0);
                if (o.splitk > 1) o.aux = tensor((size_t)o.splitk * M * C * 4);
                o.out = T_EPS; o.coff = (long)(pl.cn_off[i] / 2);
                push(o);
            }
            return;
        }
        if (pl.v.cn) {
            // ---- "control" variant: x <- x + scale * r on the twelve skips (conv_in's is the replicated tensor under rep == 2)
            // and the mid output, in place, ONE launch.  Every reader of the unmodified tensors -- the down path and the mid
            // block, including a GroupNorm that finishes a producer's deferred split-K reduce -- has run (op_tensors lists the
            // tensors as this op's inputs, so fuse_deferred_reduce never defers a reduce across it).  The producers' epilogue
            // statistics of these tensors are stale from here on: the up-block GroupNorms run their own statistics pass.
            Op o; o.kind = OP_RES_ADD; o.nres = (int)skips.size(); o.B = UB;
            for (size_t i = 0; i < skips.size(); ++i) {
                if ((long)UB * skip_hw[i] * skip_ch[i] != pl.cn_count[i]) { error = "ControlNet residual layout"; return; }
                o.res_t[i] = skips[i];
                o.M += (int)pl.cn_count[i];
                stats_of.erase(skips[i]);
            }
            push(o);
        }
        skips.pop_back(); skip_ch.pop_back(); skip_hw.pop_back();
        // ---- up ----
        const int nres = c.layers_per_block + 1;
        for (int i = 0; i < nl; ++i) {
            const int lev = nl - 1 - i, co = c.block_out_channels[lev], rb = nl - 1 - i;
            const std::string bp = "up_blocks." + std::to_string(i) + ".";
            wrapstack.push_back(Wrap{2, rb, 0});
            for (int j = 0; j < nres; ++j) {
                const int s = skips.back(), sc = skip_ch.back();
                skips.pop_back(); skip_ch.pop_back();
                const int rl = nres - 1 - j;
                wrapstack.push_back(Wrap{2, rb, rl});
                int hin = h, sin = s;
                if (pl.v.freeu && i < 2) {
                    // FreeU (freeu.hip) inside the resnet's own Wrap: it runs whenever the resnet runs, on new tensors -- a DeepCache
                    // skip step reads the cached feature through it and leaves the feature raw.  The new tensors have no entry in
                    // stats_of: the producers' statistics do not describe them, norm1 runs its own pass.
                    if (sd_freeu_check(UB, rh, rw, ch, sc, "FreeU")) { if (error.empty()) error = sd_last_error(); }
                    Op o; o.kind = OP_FREEU; o.x1 = h; o.x2 = s; o.B = UB; o.Hin = rh; o.Win = rw; o.C1 = ch; o.C2 = sc; o.epi = i;
                    o.out = hin = tensor((size_t)UB * rh * rw * ch * 2); o.aux = sin = tensor((size_t)UB * rh * rw * sc * 2);
                    push(o);
                }
                h = resnet(bp + "resnets." + std::to_string(j) + ".", hin, ch, sin, sc, co, rh, rw, t_proj);
                ch = co;
                if (c.attn_levels[lev]) h = transformer(bp + "attentions." + std::to_string(j) + ".", h, co, rh, rw);
                wrapstack.pop_back();
            }
            if (i < nl - 1) {
                wrapstack.push_back(Wrap{2, rb, 0});
                const std::string up = bp + "upsamplers.0.conv.";
                h = conv3(h, rh, rw, co, co, 1, 1, up + "weight", up + "bias", 0, -1, -1);
                wrapstack.pop_back();
                rh *= 2; rw *= 2;
            }
            wrapstack.pop_back();
            pl.taps["up" + std::to_string(i)] = h;
        }
        if (pl.v.tgate && pl.tg_blocks != (int)pl.tg_rows.size() && error.empty()) error = "T-GATE cache layout (block count)";
        // ---- out ----
        int g = gn(h, ch, -1, 0, rh * rw, "conv_norm_out.weight", "conv_norm_out.bias", c.norm_eps, 1);
        { Op o; o.kind = OP_CONV_OUT; o.x1 = g; o.out = T_EPS; o.B = UB; o.Hin = rh; o.Win = rw; o.Cin = ch; o.N = c.out_channels;
          o.w = W("conv_out.weight"); o.b = W("conv_out.bias"); push(o); }
    }
};

bool wrap_skipped(const Wrap& w, int branch) {
    const int cache_layer_id = branch % 3, cache_block_id = branch / 3;
    if (w.block_i > cache_block_id || w.type == 1) return true;
    if (w.block_i < cache_block_id) return false;
    return w.type == 0 ? w.layer_i >= cache_layer_id : w.layer_i > cache_layer_id;
}

void op_tensors(const Op& o, int ins[32], int& nin) {
    nin = 0;
    for (int t : {o.x1, o.x2, o.r, o.b2t, o.wt, o.s1, o.s2, o.lnrs, o.slab_t, o.slab_r, o.slab_b2t, o.scx1, o.scx2})
        if (t >= 0) ins[nin++] = t;
    for (int k = 0; k < o.nres; ++k) ins[nin++] = o.res_t[k];      // (OP_RES_ADD reads and rewrites them in place)
}

// A split-K conv / GEMM whose output is first read by a single-launch GroupNorm (the 8x8 and 16x16 levels: every resnet conv,
// the downsamplers, proj_out) hands its partial slabs to that GroupNorm instead of launching splitk_reduce_kernel: the
// reduce was a 42 MB pass at the launch floor (8-11 us) followed by a 6-10 us GroupNorm over 2.6 MB (27 pairs per forward at
// UNet batch 16).  Bit-identical to the two launches (same sums in the same order; SD_GN_SLAB=0: off).  Conditions: bf16,
// plain [M][N] output, no reader of the output between the two ops, both on the same side of the DeepCache boundary.
void fuse_deferred_reduce(sd_unet* u, Plan& pl) {
    if (getenv("SD_GN_SLAB") && atoi(getenv("SD_GN_SLAB")) == 0) return;       // (read when a plan is built: tests build both)
    const int nops = (int)pl.ops.size();
    auto skipped = [&](const Op& o) {
        if (pl.v.branch < 0) return false;
        for (int k = 0; k < o.nwrap; ++k)
            if (wrap_skipped(o.wraps[k], pl.v.branch)) return true;
        return false;
    };
    std::vector<int> producer(pl.tensors.size(), -1);
    for (int i = 0; i < nops; ++i)
        if (pl.ops[i].out >= 0) producer[pl.ops[i].out] = i;
    for (int g = 0; g < nops; ++g) {
        Op& G = pl.ops[g];
        if (G.kind != OP_GN || G.out_fp8 || G.x1 < 0 || !sd_groupnorm_slab_ok(G.B, G.HW, G.C1, G.C2, u->cfg.norm_num_groups)) continue;
        const int p = producer[G.x1];
        if (p < 0 || p >= g) continue;
        Op& P = pl.ops[p];
        if (P.kind != OP_CONV3 && !(P.kind == OP_GEMM && P.epi == 0)) continue;
        if (P.splitk <= 1 || P.splitk > 64 || P.aux < 0 || P.dt || P.out_fp8 || P.defer || P.subpix) continue;
        if (P.kind == OP_GEMM && (P.coff || P.ldc_o || P.hm || P.rs >= 0 || P.lnrs >= 0)) continue;
        if ((long)G.B * G.HW != P.M || G.C1 != P.N || skipped(P) != skipped(G)) continue;
        bool first_reader = true;
        for (int i = p + 1; i < g && first_reader; ++i) {
            int ins[32], nin;
            op_tensors(pl.ops[i], ins, nin);
            for (int k = 0; k < nin; ++k)
                if (ins[k] == P.out) first_reader = false;
        }
        if (!first_reader) continue;
        P.defer = 1;
        G.slab_t = P.aux; G.slab_k = P.splitk; G.slab_b = P.b; G.slab_r = P.r;
        G.slab_b2t = P.kind == OP_CONV3 ? P.b2t : -1; G.slab_b2idx = P.b2idx;
    }
}

void assign_memory(sd_unet* u, Plan& pl) {
    const int nops = (int)pl.ops.size();
    // DeepCache: which ops are skipped on skip steps, and which tensors they leave behind for running ops
    pl.skipped.assign(nops, 0);
    if (pl.v.branch >= 0) {
        for (int i = 0; i < nops; ++i)
            for (int k = 0; k < pl.ops[i].nwrap; ++k)
                if (wrap_skipped(pl.ops[i].wraps[k], pl.v.branch)) pl.skipped[i] = 1;
        std::vector<int> producer(pl.tensors.size(), -1);
        for (int i = 0; i < nops; ++i) {
            if (pl.ops[i].out >= 0) producer[pl.ops[i].out] = i;
            if (pl.ops[i].stats >= 0) producer[pl.ops[i].stats] = i;
            if (pl.ops[i].rs >= 0) producer[pl.ops[i].rs] = i;
        }
        for (int i = 0; i < nops; ++i) {
            if (pl.skipped[i]) continue;
            int ins[32], nin;
            op_tensors(pl.ops[i], ins, nin);
            for (int k = 0; k < nin; ++k) {
                const int p = producer[ins[k]];
                if (p >= 0 && pl.skipped[p]) pl.tensors[ins[k]].persistent = true;
            }
        }
    }
    if (u->debug_taps)
        for (auto& kv : pl.taps) pl.tensors[kv.second].persistent = true;
    // lifetimes over the full plan
    for (int i = 0; i < nops; ++i) {
        const Op& o = pl.ops[i];
        int ins[32], nin;
        op_tensors(o, ins, nin);
        for (int k = 0; k < nin; ++k) pl.tensors[ins[k]].last = std::max(pl.tensors[ins[k]].last, i);
        for (int t : {o.out, o.aux, o.stats, o.rs})
            if (t >= 0) {
                if (pl.tensors[t].def < 0) pl.tensors[t].def = i;
                pl.tensors[t].last = std::max(pl.tensors[t].last, i);
            }
    }
    // persistent region
    size_t off = 0;
    for (auto& t : pl.tensors)               // what sd_unet_set_context writes: first, so every variant agrees on it
        if (t.ctx && !t.ctx_ip) { t.off = off; off += t.bytes; }
    for (auto& t : pl.tensors)               // ... then what sd_unet_set_ip_adapter_hw writes: the prompt's tensors sit where the
        if (t.ctx_ip) { t.off = off; off += t.bytes; }      // plans without an image prompt have them
    for (auto& t : pl.tensors)
        if (t.persistent && !t.ctx) { t.off = off; off += t.bytes; }
    const size_t arena0 = off;
    // arena: first-fit over live intervals
    struct Live { size_t off, bytes; int last; };
    std::vector<Live> live;
    size_t high = arena0;
    std::vector<std::vector<int>> def_at(nops);
    for (int t = 0; t < (int)pl.tensors.size(); ++t)
        if (!pl.tensors[t].persistent && pl.tensors[t].def >= 0) def_at[pl.tensors[t].def].push_back(t);
    for (int i = 0; i < nops; ++i) {
        for (int t : def_at[i]) {
            std::sort(live.begin(), live.end(), [](const Live& a, const Live& b) { return a.off < b.off; });
            size_t cur = arena0;
            for (const Live& l : live) {
                if (l.off >= cur + pl.tensors[t].bytes) break;
                cur = std::max(cur, l.off + l.bytes);
            }
            pl.tensors[t].off = cur;
            live.push_back(Live{cur, pl.tensors[t].bytes, pl.tensors[t].last});
            high = std::max(high, cur + pl.tensors[t].bytes);
        }
        live.erase(std::remove_if(live.begin(), live.end(), [i](const Live& l) { return l.last <= i; }), live.end());
    }
    pl.total_bytes = high + 4096;
}

}  // namespace

int transformer_block_count(const sd_unet_config& c) {
    int n = 1;      // (the mid block's)
    for (int i = 0; i < c.num_levels; ++i)
        if (c.attn_levels[i]) n += 2 * c.layers_per_block + 1;
    return n;
}

// CFG de-duplication applies to a forward whose UNet batch is exactly two copies of the latent batch (SD_CFG_DEDUP=0: off).
// A handle with a PAG mask: the copies of the latent batch in the UNet batch, 3 or 2 (the forward refuses any other batch).
int plan_rep(const sd_unet* u, int latent_batch, int unet_batch) {
    if (u->kind == 0 && u->pag_mask)
        return (latent_batch > 0 && (unet_batch == 3 * latent_batch || unet_batch == 2 * latent_batch)) ? unet_batch / latent_batch : 1;
    static const bool off = getenv("SD_CFG_DEDUP") && atoi(getenv("SD_CFG_DEDUP")) == 0;
    return (!off && u->unet_like() && u->cfg.attn_levels[0] && latent_batch > 0 && unet_batch == 2 * latent_batch) ? 2 : 1;
}

// Latent sizes a handle takes per call (the _hw entry points).  UNet: both sides divisible by 2^(num_levels - 1), so that
// every downsampler halves them exactly; VAE decoder: sides that are multiples of 8 (the mid-block attention's token count
// HW = h * w then stays a multiple of 64) up to 128.  The handle's sample_size is the default and always accepted.
int check_latent_size(const sd_unet* u, int lh, int lw, const char* who) {
    if (u->kind == 1 || u->kind == 4) {
        SD_REQUIRE(lh >= 8 && lw >= 8 && lh <= 128 && lw <= 128 && lh % 8 == 0 && lw % 8 == 0,
                   "%s: latent %dx%d (the VAE %s takes sides that are multiples of 8 in [8, 128])", who, lh, lw,
                   u->kind == 1 ? "decoder" : "encoder");
    } else if (u->unet_like()) {
        const int d = 1 << (u->cfg.num_levels - 1);
        SD_REQUIRE(lh >= d && lw >= d && lh <= 256 && lw <= 256 && lh % d == 0 && lw % d == 0,
                   "%s: latent %dx%d (both sides must be multiples of %d, at most 256)", who, lh, lw, d);
    }
    return 0;
}

size_t control_segments(const sd_unet_config& c, int UB, int lh, int lw, std::vector<size_t>* off, std::vector<long>* count) {
    off->clear(); count->clear();
    size_t bytes = 0;
    auto seg = [&](int C, int h, int w) {
        const long n = (long)UB * h * w * C;
        off->push_back(bytes); count->push_back(n);
        bytes = (bytes + (size_t)n * 2 + 255) / 256 * 256;
    };
    int h = lh, w = lw;
    seg(c.block_out_channels[0], h, w);
    for (int i = 0; i < c.num_levels; ++i) {
        for (int j = 0; j < c.layers_per_block; ++j) seg(c.block_out_channels[i], h, w);
        if (i < c.num_levels - 1) { h /= 2; w /= 2; seg(c.block_out_channels[i], h, w); }
    }
    seg(c.block_out_channels[c.num_levels - 1], h, w);
    return bytes;
}

size_t tgate_segments(const sd_unet_config& c, int batch, int lh, int lw, std::vector<size_t>* off, std::vector<long>* rows, std::vector<int>* ch) {
    off->clear(); rows->clear(); ch->clear();
    size_t bytes = 0;
    auto seg = [&](int C, int h, int w) {
        const long m = (long)batch * h * w;
        off->push_back(bytes); rows->push_back(m); ch->push_back(C);
        bytes = (bytes + (size_t)m * C * 2 + 255) / 256 * 256;
    };
    const int nl = c.num_levels;
    int h = lh, w = lw;
    for (int i = 0; i < nl; ++i) {
        for (int j = 0; j < c.layers_per_block; ++j)
            if (c.attn_levels[i]) seg(c.block_out_channels[i], h, w);
        if (i < nl - 1) { h /= 2; w /= 2; }
    }
    seg(c.block_out_channels[nl - 1], h, w);
    for (int i = 0; i < nl; ++i) {
        const int lev = nl - 1 - i;
        for (int j = 0; j < c.layers_per_block + 1; ++j)
            if (c.attn_levels[lev]) seg(c.block_out_channels[lev], h, w);
        if (i < nl - 1) { h *= 2; w *= 2; }
    }
    return bytes;
}

bool ip_active(const sd_unet* u, int UB, int branch, int lh, int lw) {
    return u->ip_keys.count(std::make_tuple(UB, branch < 0 ? -1 : branch, lh, lw)) != 0;
}

PlanVariant plan_variant(const sd_unet* u, int UB, int branch, int lh, int lw) {
    PlanVariant v;
    v.UB = UB;
    v.branch = branch < 0 ? -1 : branch;
    v.lh = lh < 0 ? u->cfg.sample_size : lh;
    v.lw = lw < 0 ? u->cfg.sample_size : lw;
    if (u->kind != 0) return v;
    if (u->tome_ratio > 0.0) {
        memcpy(&v.tome_bits, &u->tome_ratio, sizeof(v.tome_bits));
        v.tome_max_downsample = u->tome_max_downsample;
    }
    v.freeu = u->freeu_on ? 1 : 0;
    v.tgate = u->tg_mode;
    // y rows per cache row of a capture: 2 for a CFG pair (the forward's batch is twice the batch the cache was laid out for)
    v.tg_pair = v.tgate == TGATE_CAPTURE && UB == 2 * u->tg_b ? 2 : 1;
    v.ht_tokens = u->ht_tokens;
    v.ht_max_depth = u->ht_tokens ? u->ht_max_depth : 0;
    v.pag_mask = u->pag_mask;
    v.sag = u->sag_on ? 1 : 0;
    return v;
}

unsigned variant_options(const sd_unet* u, const PlanVariant& v) {
    unsigned m = 0;
    if (u->kind != 0) return m;
    if (u->fp8) m |= opt_bit(OPT_FP8);
    if (u->cfg.in_channels == 9) m |= opt_bit(OPT_INPAINT9);
    if (u->cfg.ip_adapter_tokens > 0) m |= opt_bit(OPT_IP_MODEL);
    if (v.branch >= 0) m |= opt_bit(OPT_DEEPCACHE);
    if (v.ip) m |= opt_bit(OPT_IP_PROMPT);
    if (v.cn) m |= opt_bit(OPT_CONTROL);
    if (v.tome_bits) m |= opt_bit(OPT_TOME);
    if (v.ht_tokens) m |= opt_bit(OPT_HYPERTILE);
    if (v.freeu) m |= opt_bit(OPT_FREEU);
    if (v.tgate) m |= opt_bit(OPT_TGATE);
    if (v.pag_mask) m |= opt_bit(OPT_PAG);
    if (v.sag) m |= opt_bit(OPT_SAG);
    return m;
}

unsigned active_options(const sd_unet* u) {
    PlanVariant v = plan_variant(u, 1);
    v.ip = u->ip_keys.empty() ? 0 : 1;
    v.cn = u->ctrl_res ? 1 : 0;
    return variant_options(u, v);
}

int get_plan(sd_unet* u, const PlanVariant& v, Plan** out) {
    SD_REQUIRE(u && u->finalized, "unet: parameters not finalized");
    SD_REQUIRE(v.UB > 0 && v.UB <= 4096, "unet: bad batch %d", v.UB);
    SD_REQUIRE(v.branch < 3 * u->cfg.num_levels, "unet: cache_branch_id %d out of range", v.branch);
    if (check_options("unet", variant_options(u, v))) return -1;
    const int UB = v.UB, lh = v.lh, lw = v.lw;
    SD_REQUIRE(v.tg_pair == 1 || UB % 2 == 0, "unet: a T-GATE capture of a CFG pair needs an even batch (%d)", UB);
    SD_REQUIRE(!v.pag_mask || v.rep == 1 || ((v.rep == 2 || v.rep == 3) && UB % v.rep == 0),
               "unet: a PAG forward runs 2 or 3 copies of the latent batch (%d of batch %d)", v.rep, UB);
    auto it = u->plans.find(v);
    if (it == u->plans.end()) {
        if (lh != u->cfg.sample_size || lw != u->cfg.sample_size)
            if (check_latent_size(u, lh, lw, "unet")) return -1;
        Plan pl;
        pl.v = v;
        Builder b{u, pl, UB, {}};
        b.build();
        SD_REQUIRE(b.error.empty(), "unet: cannot build the plan for batch %d (cache branch %d, latent %dx%d): %s", UB, v.branch, lh, lw,
                   b.error.c_str());
        fuse_deferred_reduce(u, pl);
        assign_memory(u, pl);
        if (u->kind == 3 || u->kind == 6) {     // tap tables of this input size: uploaded once, owned by the handle
            int*& d = u->prep_tabs[std::make_pair(lh, lw)];
            if (!d) {
                SD_CHECK_HIP(hipMalloc((void**)&d, pl.prep_tab.size() * sizeof(int)));
                SD_CHECK_HIP(hipMemcpy(d, pl.prep_tab.data(), pl.prep_tab.size() * sizeof(int), hipMemcpyHostToDevice));
            }
            pl.dtab = d;
            std::vector<int>().swap(pl.prep_tab);
        }
        it = u->plans.emplace(v, std::move(pl)).first;
    }
    *out = &it->second;
    return 0;
}

}  // namespace sdhip
