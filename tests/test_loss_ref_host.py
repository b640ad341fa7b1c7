"""tests/loss_ref.py is pinned, and its tolerance rule bites (CPU only).

The GPU tests of tests/test_gpu_loss_edges.py hold the HIP loss kernels to float64 through ``loss_ref.hold``.  Here the
same function is given (1) an honest float32 implementation that is NOT the reference's arithmetic -- a separable filter,
row pass then column pass, with the window built the way ``make_window()`` of gfl_ssim.hip builds it -- which must pass in
every cell, and (2) that implementation with one defect at a time, which must fail in the cell named next to it."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import loss_oracle as LO
from tests import loss_ref as R


# ------------------------------------------------------------------ pinning
PIN_CELLS = [R.cell("noisy", 48, 70), R.cell("noisy", 48, 70, "disc"), R.cell("smooth1e-3", 21, 27, "disc"),
             R.cell("noisy", 21, 27, "checker", (0.3, 1.0), (0.9, 0.2))]


@pytest.mark.parametrize("c", PIN_CELLS, ids=lambda c: c.id)
def test_float32_run_reproduces_the_loss_oracle(c):
    inp = R.cell_inputs(c, 3)
    got = R.run_ref(c, inp, torch.float32)
    rc = inp["render4"][:3].clone().requires_grad_(True)
    dc = inp["render4"][3:].clone().requires_grad_(True)
    ab = torch.tensor(c.ab, requires_grad=True)
    move = None if inp["keep"] is None else inp["keep"] == 0
    l_rgb, err = LO.rgb_loss(rc, inp["gt_rgb"], move)
    l_dep = LO.depth_loss(dc, inp["gt_depth"].unsqueeze(-1), ab[0], ab[1], move)
    (c.lam_rgb * l_rgb + c.lam_depth * l_dep).backward()
    n = c.H * c.W
    assert abs((got["sums"][0] / n + 1 - got["sums"][1] / (3 * n)).item() - l_rgb.item()) < 2e-6
    assert abs(got["sums"][2].item() / n - l_dep.item()) < 2e-6
    np.testing.assert_allclose(got["err_px"].numpy(), err.detach().numpy(), rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(got["d_render"].numpy(), torch.cat([rc.grad, dc.grad]).numpy(), rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(got["d_ab"].numpy(), ab.grad.numpy(), rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(got["sums"][3:].numpy(), ab.grad.numpy(), rtol=1e-4, atol=1e-8)


def test_float32_run_reproduces_the_ssim_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "ssim_small.npz"))
    for a, b, val, grad in (("img1", "img2", "value", "grad1"), ("img3", "img4", "value34", "grad3")):
        x, y = torch.from_numpy(g[a])[0], torch.from_numpy(g[b])[0]
        H, W = x.shape[1:]
        got = R.loss_ref(torch.cat([x, torch.zeros(1, H, W)]), y.permute(1, 2, 0), None, None, None, 1.0, 0.0, dtype=torch.float32)
        assert abs(got["S"].mean().item() - float(g[val])) < 2e-6
        d_ssim = 2 * (x.double() - y.double()) / x.numel() - got["d_render"][:3].double()     # dL/dx = d mse/dx - d ssim/dx
        np.testing.assert_allclose(d_ssim.numpy(), g[grad][0], rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("c", [R.cell("noisy", 48, 70, "disc"), R.cell("smooth1e-3", 33, 17), R.cell("noisy", 1, 40)],
                         ids=lambda c: c.id)
def test_tile_sums_add_up_to_the_totals(c):
    r = R.rule(c).r64[0]
    T = ((c.H + 15) // 16) * ((c.W + 15) // 16)
    assert r["p_ssim"].shape == (3 * T,) and r["p_grad"].shape == (T, 4)
    torch.testing.assert_close(r["p_ssim"].sum(), r["sums"][1], rtol=1e-12, atol=0)
    torch.testing.assert_close(r["p_grad"].sum(dim=0), r["sums"][[0, 2, 3, 4]], rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(r["p_ssim"].reshape(3, T).sum(dim=0)[0], r["S"][:, :16, :16].sum(), rtol=1e-12, atol=0)
    torch.testing.assert_close(r["d_ab"], r["sums"][3:], rtol=0, atol=0)


def test_flat_images_give_the_closed_form_in_the_centre_tile():
    """48 x 48, render 0.7, target 0.6: the centre tile is 16 pixels from every border, the variances are zero and
    S = (2ab + C1) / (a^2 + b^2 + C1) there -- no oracle involved."""
    c = R.KNOWN_CELLS[-1]
    assert c.regime == "flat" and (c.H, c.W) == (48, 48)
    a, b = float(np.float32(R.FLAT_A)), float(np.float32(R.FLAT_B))
    want = 256 * (2 * a * b + R.SSIM_C1) / (a * a + b * b + R.SSIM_C1)
    # the float32 window sums to q = 1 + 7e-8, not to 1: mu = a q, E[x^2] = a^2 q, so the "variances" are (q - q^2) times
    # the squares -- the closed form with q in it is what float64 must give to rounding, the one with q = 1 under the rule
    w1 = LO.ssim_window(11, 1.5, torch.float32)
    q = (w1.unsqueeze(1) @ w1.unsqueeze(0)).double().sum().item()
    v = q - q * q
    exact = 256 * ((2 * a * b * q * q + R.SSIM_C1) * (2 * a * b * v + R.SSIM_C2)) / (
        ((a * a + b * b) * q * q + R.SSIM_C1) * ((a * a + b * b) * v + R.SSIM_C2))
    ru = R.rule(c)
    r = ru.r64[0]
    for ch in range(3):
        got = r["p_ssim"][ch * 9 + 4].item()
        assert abs(got - exact) < 1e-11 * exact
        assert abs(got - want) <= R.FACTOR * ru.E32["p_ssim"][ch * 9 + 4].item()


# ------------------------------------------------------------------ another implementation, honest and not
def make_window():
    """As make_window() of gfl_ssim.hip: exp in double cast to float32, float32 running sum, divide."""
    w = np.array([math.exp(-((i - 5) ** 2) / (2.0 * 1.5 * 1.5)) for i in range(11)]).astype(np.float32)
    s = np.float32(0)
    for v in w:
        s = np.float32(s + v)
    return torch.from_numpy((w / s).astype(np.float32))


def separable(win=None, pad="zero"):
    w = make_window() if win is None else win

    def blur(x, dtype):
        k = w.to(dtype)
        p = 5
        if pad == "replicate":
            x, p = F.pad(x, (5, 5, 5, 5), mode="replicate"), 0
        h = F.conv2d(x, k.view(1, 1, 1, 11).expand(3, 1, 1, 11).contiguous(), padding=(0, p), groups=3)        # row pass
        return F.conv2d(h, k.view(1, 1, 11, 1).expand(3, 1, 11, 1).contiguous(), padding=(p, 0), groups=3)     # column pass
    return blur


def _no_outer_taps():
    w = make_window().clone()
    w[0] = w[10] = 0
    return w / w.sum()


def _transposed_tiles(r):
    T = r["p_ssim"].numel() // 3
    r = dict(r)
    r["p_ssim"] = r["p_ssim"].reshape(3, T).T.reshape(-1)           # tile * 3 + c
    return r


def restate(c, variant=None, post=None):
    out = []
    for inp in R.rule(c).inputs:
        r = R.run_ref(c, inp, torch.float32, **(variant or dict(blur=separable())))
        out.append(post(r) if post else r)
    return out


@pytest.mark.parametrize("c", R.CELLS, ids=lambda c: c.id)
def test_rule_passes_a_separable_float32_restatement(c):
    R.hold(c, restate(c), "separable-f32")


# defect -> (variant of loss_ref, post-processing, the cell that catches it)
DEFECTS = {
    "outermost_taps_dropped_and_renormalised": (dict(blur=separable(_no_outer_taps())), None, R.cell("noisy", 21, 27)),
    "edge_replication_for_zero_padding": (dict(blur=separable(pad="replicate")), None, R.cell("noisy", 16, 16)),
    "mask_on_the_render_only": (dict(blur=separable(), mask_target=False), None, R.cell("noisy", 21, 27, "disc")),
    "c2_is_0.03_not_its_square": (dict(blur=separable(), c2=0.03), None, R.cell("smooth1e-3", 21, 27)),
    "tile_order_transposed": (None, _transposed_tiles, R.cell("noisy", 21, 27)),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_rule_rejects_a_defect(name, capsys):
    variant, post, c = DEFECTS[name]
    assert c in R.CELLS, "the catching cell must be one the GPU tests run"
    R.hold(c, restate(c), "honest")                                   # the same cell passes without the defect
    with pytest.raises(AssertionError, match="outside 4 x E32"):
        R.hold(c, restate(c, variant, post), name)


@pytest.mark.parametrize("name,regimes", [
    ("outermost_taps_dropped_and_renormalised", ("smooth1e-2", "smooth1e-3")),
    ("edge_replication_for_zero_padding", ("smooth1e-3",)),
    ("mask_on_the_render_only", ("smooth1e-3",)),
    ("c2_is_0.03_not_its_square", ("noisy",)),
    ("tile_order_transposed", ("smooth1e-3",)),
])
def test_defects_are_caught_in_the_other_regimes_too(name, regimes):
    """Not only where the bound is tightest: the smooth cells of the same shape and mask see each defect as well."""
    variant, post, c = DEFECTS[name]
    for regime in regimes:
        c2 = c._replace(regime=regime)
        assert c2 in R.CELLS
        with pytest.raises(AssertionError, match="outside 4 x E32"):
            R.hold(c2, restate(c2, variant, post), name)
