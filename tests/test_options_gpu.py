"""The option table on a live UNet handle: every pair the wrapper can reach through its setters is refused in both orders, and
a refusal leaves nothing behind -- with the option that was on cleared, the handle has the plans, the workspace size and the
output bits it had before.

One handle of the SAG tests' ``sd15`` environment at a 32x32 latent (the smallest SAG takes: a 4x4 mid grid), UNet batch 2.  The
fp8, 9-channel and IP-Adapter-weights rows are properties of a handle: tests/test_options_cpu.py and the suites of those
features cover them.  Nothing here runs but setters that refuse and plain forwards.

"As it was" is the fresh handle's plan count, workspace size and output bits -- with one exception that is the handle's own and
older than the table: setting ControlNet residuals builds the control plans of the live workspace's batch and keeps them in
the sizing for good, so the four cases that have residuals ON are held to the plan count of the handle after one such switch
without a refusal (4 here, against the fresh handle's 2); their workspace size and output bits are the fresh handle's too."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import options as O
from tests import sag_oracle as so

H = W = 32
UB = 2


def _switches(net):
    """option -> (on, off) through the wrapper's setters.  T-GATE goes on in capture mode with a cache laid out for another
    latent size than the live workspace's, so that switching it on sizes nothing; ControlNet residuals go on as a zero buffer."""
    from sonicdiffusionbayeslab_amd.controlnet import new_residual_buffer, residual_layout
    res = new_residual_buffer(residual_layout(net.config, UB, H, W)[1], net.device).zero_()
    mass = torch.zeros(UB, (H // 8) * (W // 8), device=net.device)
    return {O.DEEPCACHE: (lambda: net.set_deepcache(0), lambda: net.set_deepcache(-1)),
            O.CONTROL: (lambda: net.set_control_residuals(res, 1.0, UB, H, W), net.clear_control_residuals),
            O.TOME: (lambda: net.set_tome(0.5), lambda: net.set_tome(0.0)),
            O.HYPERTILE: (lambda: net.set_hypertile(8, 0), lambda: net.set_hypertile(0)),
            O.TGATE: (lambda: net.set_tgate(net.TGATE_CAPTURE, 1, 16, 16), lambda: net.set_tgate(net.TGATE_OFF)),
            O.PAG: (lambda: net.set_pag(1 << 6), lambda: net.set_pag(0)),
            O.SAG: (lambda: net.set_sag(True, mass), net.clear_sag)}


def test_every_reachable_pair_is_refused_in_both_orders_and_leaves_the_handle_as_it_was():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd, _, _ = so.env("sd15")
    lat, pe, ne = so.unet_inputs(cfg, H, W, 1)
    ctx, lat = torch.cat([ne, pe]).cuda(), lat.cuda()
    net = HipUNet2DConditionModel(cfg, sd)

    def plain():
        net.set_context(ctx, H, W)
        return net.forward_latents(lat, UB, 501.0).clone()
    recorded = plain()
    plans, nbytes = net.plan_count(), net._workspace_bytes(UB, -1, H, W)
    sw = _switches(net)
    pairs = [tuple(p) for p in map(sorted, map(tuple, map(frozenset, O.HANDLE_PAIRS))) if all(o in sw for o in p)]
    assert len(pairs) == 13                 # tome x {hypertile, pag, sag}, tgate x 4, pag x 3 more, sag x 2 more, control x deepcache
    # Residuals that were set once stay in the handle's workspace sizing (sd_unet_set_control_residuals_hw: "from then on
    # sd_unet_workspace_bytes_hw covers the control plan variants"), and setting them sizes the live workspace at once: the switch
    # itself builds the two control plans of this batch (plan_count 2 -> 4, measured; the workspace stays at 78 581 248 bytes).
    # That is the handle's behaviour of before, not the refusal's, so the four cases that switch residuals ON run last, behind one
    # on / off cycle without any refusal that moves the plan count by what the switch builds; from there on they are held to
    # the same figures as every other case.  No other case lets residuals reach the handle.
    cases = sorted([(a, b) for a, b in pairs] + [(b, a) for a, b in pairs], key=lambda c: c[0] == O.CONTROL)
    assert [c[0] for c in cases].count(O.CONTROL) == 4 and all(c[0] == O.CONTROL for c in cases[-4:])
    for i, (on, asked) in enumerate(cases):
        if i == len(cases) - 4:
            sw[O.CONTROL][0]()
            sw[O.CONTROL][1]()
            assert net._workspace_bytes(UB, -1, H, W) == nbytes and torch.equal(plain(), recorded)
            print(f"ControlNet residuals on and off: plans {net.plan_count()} (fresh {plans})")
            plans = net.plan_count()
        sw[on][0]()
        try:
            before = net.plan_count()
            with pytest.raises(NotImplementedError) as e:
                sw[asked][0]()
            assert on in str(e.value) and asked in str(e.value), str(e.value)
            assert asked not in net.options_on() and net.plan_count() == before       # the refusal itself built nothing
        finally:
            sw[on][1]()
        assert net.options_on() == []
        figures = (net.plan_count(), net._workspace_bytes(UB, -1, H, W))
        print(f"{on} on, {asked} asked: plans {figures[0]} (fresh {plans}), workspace {figures[1]} (fresh {nbytes})")
        assert figures == (plans, nbytes), (on, asked)
        assert torch.equal(plain(), recorded), (on, asked)
