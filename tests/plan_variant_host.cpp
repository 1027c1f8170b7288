// Stand-alone host program for tests/test_options_cpu.py: the ordering of PlanVariant (csrc/model.h) field by field, and that
// plan_variant fills equal keys from equal handle state.  No GPU call is made.  Prints "ok" and exits 0, or names what failed.
#include "../sonicdiffusionbayeslab_amd/csrc/model.h"

#include <cstdio>
#include <functional>
#include <vector>

using sdhip::PlanVariant;

static int fail(const char* what, int i = -1, int j = -1) {
    printf("FAILED: %s (%d, %d)\n", what, i, j);
    return 1;
}

int main() {
    // one setter per field, in the order of the comparison
    const std::vector<std::function<void(PlanVariant&, long long)>> bump = {
        [](PlanVariant& v, long long d) { v.UB += (int)d; },           [](PlanVariant& v, long long d) { v.branch += (int)d; },
        [](PlanVariant& v, long long d) { v.rep += (int)d; },          [](PlanVariant& v, long long d) { v.lh += (int)d; },
        [](PlanVariant& v, long long d) { v.lw += (int)d; },           [](PlanVariant& v, long long d) { v.ip += (int)d; },
        [](PlanVariant& v, long long d) { v.cn += (int)d; },           [](PlanVariant& v, long long d) { v.tome_bits += d << 40; },
        [](PlanVariant& v, long long d) { v.tome_max_downsample += (int)d; }, [](PlanVariant& v, long long d) { v.freeu += (int)d; },
        [](PlanVariant& v, long long d) { v.tgate += (int)d; },        [](PlanVariant& v, long long d) { v.tg_pair += (int)d; },
        [](PlanVariant& v, long long d) { v.ht_tokens += (int)d; },    [](PlanVariant& v, long long d) { v.ht_max_depth += (int)d; },
        [](PlanVariant& v, long long d) { v.pag_mask += d << 40; },    [](PlanVariant& v, long long d) { v.sag += (int)d; }};
    if (bump.size() != 16) return fail("sixteen fields");
    PlanVariant base;
    base.UB = 2; base.lh = base.lw = 16;
    if (base < base) return fail("a key orders before itself");
    for (int i = 0; i < 16; ++i) {
        PlanVariant hi = base;
        bump[i](hi, 1);
        if (!(base < hi) || hi < base) return fail("flipping a field gives a distinct, later key", i);
        for (int j = i + 1; j < 16; ++j) {          // ... and a later field that is smaller does not outweigh it
            PlanVariant lo = hi;
            bump[j](lo, -1);
            if (!(base < lo) || lo < base) return fail("the fields compare in their order", i, j);
        }
    }
    // two handles in equal state give equal keys; each setting gives a key of its own; off gives the plain key back
    sd_unet a, b;
    for (sd_unet* u : {&a, &b}) { u->kind = 0; u->cfg.sample_size = 16; u->cfg.in_channels = 4; }
    auto key = [](const sd_unet& u) { return sdhip::plan_variant(&u, 2); };
    auto same = [](const PlanVariant& x, const PlanVariant& y) { return !(x < y) && !(y < x); };
    const PlanVariant plain = key(a);
    if (!same(plain, base) || !same(plain, key(b))) return fail("the plain key");
    if (sdhip::plan_variant(&a, 3, 4, 24, 8).branch != 4 || sdhip::plan_variant(&a, 3, -7, 24, 8).branch != -1 ||
        sdhip::plan_variant(&a, 3, 4, 24, 8).lh != 24 || sdhip::plan_variant(&a, 3, 4, 24, 8).lw != 8) return fail("batch, branch, size");
    const std::vector<std::function<void(sd_unet&, bool)>> settings = {
        [](sd_unet& u, bool on) { u.tome_ratio = on ? 0.5 : 0.0; u.tome_max_downsample = on ? 2 : 0; },
        [](sd_unet& u, bool on) { u.tome_ratio = on ? 0.25 : 0.0; u.tome_max_downsample = on ? 2 : 0; },
        [](sd_unet& u, bool on) { u.tome_ratio = on ? 0.5 : 0.0; u.tome_max_downsample = on ? 1 : 0; },
        [](sd_unet& u, bool on) { u.ht_tokens = on ? 8 : 0; u.ht_max_depth = on ? 1 : 0; },
        [](sd_unet& u, bool on) { u.ht_tokens = on ? 8 : 0; u.ht_max_depth = 0; },
        [](sd_unet& u, bool on) { u.freeu_on = on; },
        [](sd_unet& u, bool on) { u.tg_mode = on ? sdhip::TGATE_CAPTURE : 0; u.tg_b = on ? 1 : 0; },
        [](sd_unet& u, bool on) { u.tg_mode = on ? sdhip::TGATE_CAPTURE : 0; u.tg_b = on ? 2 : 0; },
        [](sd_unet& u, bool on) { u.tg_mode = on ? sdhip::TGATE_REUSE : 0; },
        [](sd_unet& u, bool on) { u.pag_mask = on ? 1ll << 6 : 0; },
        [](sd_unet& u, bool on) { u.pag_mask = on ? 3ll << 6 : 0; },
        [](sd_unet& u, bool on) { u.sag_on = on; }};
    std::vector<PlanVariant> seen = {plain};
    for (int i = 0; i < (int)settings.size(); ++i) {
        settings[i](a, true); settings[i](b, true);
        const PlanVariant v = key(a);
        if (!same(v, key(b))) return fail("equal state, equal keys", i);
        for (const PlanVariant& s : seen)
            if (same(v, s)) return fail("a setting's key is its own", i);
        seen.push_back(v);
        settings[i](a, false); settings[i](b, false);
        if (!same(key(a), plain)) return fail("off gives the plain key back", i);
    }
    a.kind = 1; a.pag_mask = 1; a.sag_on = true;           // handle kinds other than 0 have no options
    if (!same(key(a), plain)) return fail("kinds other than 0");
    printf("ok\n");
    return 0;
}
