"""Parity per opacity regime (``-m gpu``): alpha at the cap (o G > 0.99: alpha = 0.99, straight-through gradient,
1 / (1 - alpha) = 100 in the backward's reconstruction of T), opacity at the visibility threshold (1/255 <= o < 1.05/255: the
fused path's no-culling branch of alpha_cutoff), invisible rows (o < 1/255: in no list) and saturated activations
(sigmoid(10 x) == 1.0f).  Every other scene of the suite keeps o G inside [0.02, 0.99].

The scenes, the row sets and the reference's own error are those of tests/test_opacity_regimes_host.py (checked there on the
CPU); the reference is the float32 oracle.  A regime's rows are compared on their OWN norm and their own largest entry: in
the regime scene the threshold rows carry 1e-4 of the d_xyz norm and the whole-tensor bounds do not see them."""
import numpy as np
import pytest
import torch

from oracle import fit_oracle as FO
from oracle import loss_oracle as LO
from oracle import msplat_oracle as MO
from tests.scenes import (ATTRS, REGIME_LAMBDAS, known_answer_inputs, opacity_known_answers, oracle_front_end, reference_fit,
                          regime_rows)
from tests.test_gpu_fused import _copy_engine_state, _engine, _lists, _reserved_on
from tests.test_gpu_parity import close_frac, observe, subset_check
from tests.test_gpu_render_op import NAMES, _loss, _weights
from tests.test_opacity_regimes_host import POSE, REGIMES, _case

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCENES = ["regimes", "pile"]


def _ms():
    import gflow_amd.msplat as ms
    return ms


def _regime_check(got, ref, sets, name, what, rel_bound, rtol, atol_scale, bad_frac, skip=()):
    """The whole tensor's bounds once more over each regime's rows minus the fragile ones -- relative L2 of the rows' own norm,
    atol from the rows' own largest entry.  Rows whose reference is all zero must be all zero."""
    got, ref = torch.as_tensor(got).detach().cpu(), ref.detach()
    for regime in REGIMES[name]:
        if regime in skip:
            continue
        rows = regime_rows(sets, regime)
        if float(ref[rows].abs().max()) == 0.0:
            assert float(got[rows].abs().max()) == 0.0, f"{what}, {regime} rows: the reference is zero, the device is not"
            observe(f"{what}, {regime} rows: zero in both")
            continue
        subset_check(got, ref, rows, f"{what}, {regime} rows", rel_bound=rel_bound,
                     frac=(rtol, atol_scale * ref[rows].abs().max().item(), bad_frac))


# ------------------------------------------------------------------------------------------------ fused forward
@pytest.mark.parametrize("name", SCENES)
def test_fused_forward_per_regime(name):
    """The fused forward at the bounds of test_gpu_fused._check_fused_forward; no invisible row in the lists, every
    threshold row in every tile of its rectangle (no disc culling on the 3e38 branch), never more pairs than the oracle."""
    sc, img, dep, sets, _ = _case(name)
    n = sc["raw"]["xyz"].shape[0]
    eng = _engine(sc["raw"], sc, img, dep, pose=POSE, bg=0.2)
    eng.forward()
    eng.check_overflow()
    fe = oracle_front_end(sc, POSE, torch.float32)
    feat = torch.cat([fe["rgb"], fe["depth"]], dim=1)
    ref4 = MO.alpha_blending(fe["uv"], fe["conic"], fe["opacity"], feat, fe["ids"], fe["tile_range"], 0.2, sc["W"], sc["H"])
    close_frac(eng.render, ref4, 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=f"[{name}] fused render vs oracle")
    close_frac(eng.uv, fe["uv"], 1e-5, 1e-3, what=f"[{name}] uv")
    close_frac(eng.depth, fe["depth"], 1e-6, 1e-6, what=f"[{name}] depth")
    tiles = fe["tiles"].reshape(-1).long()
    K = eng.K
    assert 0 < K <= int(tiles.sum())
    count = torch.bincount(eng.ids[:K].long().cpu(), minlength=n)
    assert int(count[sets["invisible"]].sum()) == 0, "an invisible row (o < 1/255) is in a list"
    thr = sets["threshold"]
    assert torch.equal(count[thr], tiles[thr]), "a threshold row was culled from a tile of its rectangle"
    if name == "pile":
        tr = eng.tile_range[sc["pile_tile"]].cpu()
        assert int(tr[1] - tr[0]) > max(448, 3 * 192), f"the pile's list has {int(tr[1] - tr[0])} entries"
    r1 = eng.render.clone()
    eng.forward()
    assert torch.equal(r1, eng.render)


# ------------------------------------------------------------------------------------------------ fused gradients
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_fused_gradients_per_regime(name, deterministic):
    """One iteration from a zero Adam state (g = m / 0.1), at the whole-tensor bounds of test_gpu_fused._check_fused_gradients
    and then per regime at the same bounds on the regime's own scale; pose and depth-affine gradients; invisible rows get
    nothing and do not move; saturated rows have no opacity gradient; rows the reference gives nothing get nothing."""
    from gflow_amd.fused import COLS
    sc, img, dep, sets, _ = _case(name)
    ref = reference_fit(sc, POSE, img, dep, torch.float32)
    n = sc["raw"]["xyz"].shape[0]
    eng = _engine(sc["raw"], sc, img, dep, pose=POSE, lr=1e-3, lr_camera=1e-3, total_iters=100, **REGIME_LAMBDAS)
    eng.deterministic = deterministic
    before = eng.params[:n, :14].clone()
    eng.iteration()
    eng.check_overflow()
    tag = f"[{name}{', deterministic' if deterministic else ''}] fused: "
    l_rgb, l_depth = eng.loss_terms()
    assert abs(l_rgb.item() - ref["l_rgb"]) <= 1e-4 * abs(ref["l_rgb"])
    assert abs(l_depth.item() - ref["l_depth"]) <= 1e-4 * abs(ref["l_depth"])
    g_all = (eng.adam_m[:n] / (1.0 - 0.9)).cpu()
    for k, (a, b) in COLS.items():
        want = ref["grads"][k]
        got = g_all[:, a:b]
        rel = ((got - want).norm() / want.norm()).item()
        observe(f"{tag}d_{k}: relative L2 {rel:.2e} (bound 0.002)")
        assert rel < 2e-3, f"{tag}d_{k}: relative L2 error {rel:.2e}"
        close_frac(got, want, 5e-3, 5e-4 * want.abs().max().item(), bad_frac=1e-2, what=f"{tag}d_{k}")
        _regime_check(got, want, sets, name, f"{tag}d_{k}", 2e-3, 5e-3, 5e-4, 1e-2,
                      skip=("saturated",) if k == "opacity" else ())
    gp = (eng.pose_m / 0.1).cpu()
    rel = ((gp - ref["d_pose"]).norm() / ref["d_pose"].norm()).item()
    observe(f"{tag}d_pose: relative L2 {rel:.2e} (bound 0.002)")
    assert rel < 2e-3, f"{tag}d_pose: relative L2 error {rel:.2e}  {gp} vs {ref['d_pose']}"
    np.testing.assert_allclose((eng.ab_m / 0.1).cpu().numpy(), ref["d_ab"].numpy(), rtol=2e-3)
    # invisible rows: nothing arrives, nothing moves
    inv = sets["invisible"]
    after = eng.params[:n, :14].cpu()
    if bool(inv.any()):
        for k in ("xyz", "rotate", "opacity", "rgb"):
            a, b = COLS[k]
            assert float(g_all[inv][:, a:b].abs().max()) == 0.0, f"{tag}d_{k} of an invisible row is not zero"
        assert torch.equal(after[inv], before.cpu()[inv]), f"{tag}an invisible row moved"
    # saturated rows: sigmoid(10 x) == 1.0f, the chain rule's 10 o (1 - o) is zero
    a, b = COLS["opacity"]
    d_op = g_all[:, a:b]
    worst = float(d_op[sets["saturated"]].abs().max()) / float(d_op.abs().max())
    observe(f"{tag}largest |d_opacity| of a saturated row / largest of all: {worst:.2e} (bound 1e-06)")
    assert worst <= 1e-6
    # the pile: rows the reference gives no gradient at all (behind the stop) -- the device writes nothing for them
    if name == "pile":
        none = torch.cat([ref["grads"][k] for k in ATTRS], dim=1).abs().sum(dim=1) == 0
        assert float(none[:sc["n_pile"]].double().mean()) >= 0.9
        assert float(g_all[none][:, :14].abs().max()) == 0.0, f"{tag}a row without a reference gradient got one"
        assert torch.equal(after[none], before.cpu()[none]), f"{tag}a row without a gradient moved"
    assert int(eng.step.item()) == 1


# ------------------------------------------------------------------------------------------------ reserved regions
def test_reserved_tile_regions_on_the_regime_scene():
    """The second iteration bins into reserved tile regions in ONE launch (the cutoff -- 3e38 for the threshold rows, -1 for
    the invisible ones -- stays in registers between the preprocess and the scatter); against a copy of the engine that bins
    exactly: records, every tile's list, render, T and contributor counts bit for bit."""
    sc, img, dep, sets, _ = _case("regimes")
    # (lr: Adam moves a raw opacity by lr whatever its gradient, and 4e-3 there is 4 % of o -- most of the threshold branch's width)
    hyper = dict(lr=2e-4, lr_camera=0.0, total_iters=100, **REGIME_LAMBDAS)
    a = _engine(sc["raw"], sc, img, dep, pose=POSE, **hyper)
    b = _engine(sc["raw"], sc, img, dep, pose=POSE, **hyper)
    if not _reserved_on(a):
        pytest.skip("reserved tile regions are switched off (GFL_RESERVED=0)")
    a.iteration()
    assert a._reserved_flag() == a.GFL_ITER_RESERVED
    _copy_engine_state(a, b)
    b.iteration(reserved=False)
    a.iteration()
    a.check_overflow(); b.check_overflow()
    assert a.K == b.K > 0
    assert torch.equal(a.rec[:a.N], b.rec[:b.N])
    la, lb = _lists(a), _lists(b)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert int(a.tile_range[:, 1].max()) > a.K                       # (regions: gaps between the lists)
    assert torch.equal(a.render, b.render) and torch.equal(a.final_T, b.final_T) and torch.equal(a.n_contrib, b.n_contrib)
    n = a.N
    count = torch.bincount(torch.cat(la).long(), minlength=n)
    assert int(count[sets["invisible"]].sum()) == 0
    # ... and that iteration had rows on both special returns of alpha_cutoff (rec column 10 is the cutoff)
    cutoff = a.rec[:n, 10].cpu()
    live = a.rec[:n, 9].cpu() > 0
    assert int((live & (cutoff > 1e38)).sum()) >= 100 and int((live & (cutoff < 0)).sum()) >= 100


# ------------------------------------------------------------------------------------------------ the blend's modes, long tile
def test_forward_modes_agree_on_the_long_tile_walk():
    """The pile's tile is long enough for the forward's quarter walk (four 8x8 blocks on four CUs, three staged batches,
    checkpoints at 192, 384 and 576), which the sparse scenes of tests/test_gpu_fused.py never reach in modes 1, 2 and 3.
    The equalities those tests assert, on this scene: a snapshot iteration (mode 2) against a plain one (mode 0) followed by
    gfl_fit_snapshot (mode 1) -- render, final_T, n_contrib bit for bit, the three uint8 images byte for byte --, and with a
    footprint mask the plain iteration (mode 3: footprint workgroups behind the blend's) against the snapshot iteration
    (a footprint launch of its own): the same keep, the same render."""
    sc, img, dep, sets, _ = _case("pile")
    hyper = dict(lr=2e-4, lr_camera=0.0, total_iters=100, **REGIME_LAMBDAS)
    a = _engine(sc["raw"], sc, img, dep, pose=POSE, **hyper)
    b = _engine(sc["raw"], sc, img, dep, pose=POSE, **hyper)
    got = a.iteration(snapshot=True).clone()
    b.iteration(reserved=False)
    want = b.snapshot()
    a.check_overflow(); b.check_overflow()
    for e in (a, b):
        tr = e.tile_range[sc["pile_tile"]].cpu()
        assert int(tr[1] - tr[0]) > max(448, 3 * 192), f"the pile's list has {int(tr[1] - tr[0])} entries"
    assert torch.equal(a.render, b.render) and torch.equal(a.final_T, b.final_T) and torch.equal(a.n_contrib, b.n_contrib)
    for k, name in enumerate(("rgb", "depth_map_color", "center")):
        assert torch.equal(got[k], want[k]), f"{name}: {(got[k] != want[k]).float().mean().item():.2e} of the bytes differ"
    # mode 3 against mode 2 + footprint_kernel: every sixteenth row behind the pile is flagged as moving (the pile's own splats
    # are 20-60 pixels wide: any eleven of them cover the image); the footprint's workgroup still walks the pile tile's list
    n = sc["raw"]["xyz"].shape[0]
    moving = (torch.arange(n) >= sc["n_pile"]) & ((torch.arange(n) % 16) == 0)
    move_mask = torch.zeros(sc["H"], sc["W"], dtype=torch.bool)
    move_mask[2:6, 30:40] = True
    c = _engine(sc["raw"], sc, img, dep, pose=POSE, **hyper)
    d = _engine(sc["raw"], sc, img, dep, pose=POSE, **hyper)
    for e in (c, d):
        e.set_footprint_mask(move_mask, moving)
    c.iteration()
    d.iteration(snapshot=True)
    c.check_overflow(); d.check_overflow()
    masked = 1.0 - c.keep.float().mean().item()
    assert float(move_mask.float().mean()) < masked < 1.0, f"{masked:.3f} of the pixels masked: the footprint case is degenerate"
    assert torch.equal(c.keep, d.keep) and torch.equal(c.render, d.render)
    assert torch.equal(c.final_T, d.final_T) and torch.equal(c.n_contrib, d.n_contrib)


# ------------------------------------------------------------------------------------------------ fused render operator
def test_render_operator_per_regime():
    """gfl_render_fwd / _bwd on ACTIVATED rows (splat_from_row's other branch): values, and the gradients with respect to the
    activated opacity, rgb, scale, rotation and xyz per regime.  No sigmoid damps the cap here: d / d o at a capped pixel is
    the straight-through term itself."""
    import gflow_amd.render as R
    sc, img, dep, sets, _ = _case("regimes")
    W, H, bg = sc["W"], sc["H"], 0.33
    n = sc["raw"]["xyz"].shape[0]
    act = dict(zip(NAMES, FO.activate(sc["raw"])))
    extr = LO.pose_to_extr(POSE)
    w = _weights(H, W, n, 5)
    leaves_c = {k: act[k].clone().requires_grad_(True) for k in NAMES}
    oc = MO.render_multiple([*[leaves_c[k] for k in NAMES], sc["intr"], extr, bg, W, H], ["rgb", "uv", "depth", "depth_map"])
    _loss(oc, w).backward()
    leaves_g = {k: act[k].clone().to(DEV).requires_grad_(True) for k in NAMES}
    og = R.render(leaves_g, dict(intr=sc["intr"].to(DEV), extr=extr.to(DEV), W=W, H=H), bg)
    for k in ("rgb", "depth_map"):
        close_frac(og[k], oc[k], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=f"[regimes] render(): {k}")
    _loss(og, [t.to(DEV) for t in w]).backward()
    for k in NAMES:
        want = leaves_c[k].grad.reshape(n, -1)
        got = leaves_g[k].grad.cpu().reshape(n, -1)
        rel = ((got - want).norm() / want.norm()).item()
        observe(f"[regimes] render(): d_{k}: relative L2 {rel:.2e} (bound 0.002)")
        assert rel < 2e-3, f"render(): d_{k}: relative L2 error {rel:.2e}"
        _regime_check(got, want, sets, "regimes", f"[regimes] render(): d_{k}", 2e-3, 5e-3, 5e-4, 1e-2)
        inv = sets["invisible"]
        if k in ("scale", "rotate", "opacity", "rgb"):            # (xyz carries the weights on uv and depth)
            assert float(got[inv].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ operator path
@pytest.mark.parametrize("C,bg", [(3, 0.0), (4, 1.0)])
def test_blend_operator_per_regime(C, bg):
    """msplat.alpha_blending (gfl_blend.hip) forward and backward on the regime scene at the bounds of
    test_gpu_parity.test_blend_forward_backward, then per regime with the regime's own scale for atol."""
    ms = _ms()
    sc, img, dep, sets, _ = _case("regimes")
    W, H = sc["W"], sc["H"]
    fe = oracle_front_end(sc, POSE, torch.float32)
    ids, tr = fe["ids"], fe["tile_range"]
    g = torch.Generator().manual_seed(7 + C)
    feat = torch.rand(fe["uv"].shape[0], C, generator=g)
    inputs = (fe["uv"], fe["conic"], fe["opacity"], feat)
    leaves_c = [t.detach().clone().requires_grad_(True) for t in inputs]
    leaves_g = [t.detach().clone().to(DEV).requires_grad_(True) for t in inputs]
    out_c = MO.alpha_blending(*leaves_c, ids, tr, bg, W, H)
    out_g = ms.alpha_blending(*leaves_g, ids.to(DEV), tr.to(DEV), bg, W, H)
    close_frac(out_g, out_c, 1e-4, 1e-5, bad_frac=1e-4, hard=5e-3, what=f"[regimes] blend C={C}")
    w = torch.randn(out_c.shape, generator=g)
    (out_c * w).sum().backward()
    (out_g * w.to(DEV)).sum().backward()
    for name, a, b in zip(("d_uv", "d_conic", "d_opacity", "d_feature"), leaves_g, leaves_c):
        want = b.grad
        close_frac(a.grad, want, 1e-3, 1e-4 * want.abs().max().item(), bad_frac=2e-3, what=f"[regimes] blend {name} C={C}")
        rel = ((a.grad.cpu() - want).norm() / want.norm()).item()
        assert rel < 2e-4, f"blend {name}: relative L2 error {rel:.2e}"
        _regime_check(a.grad, want, sets, "regimes", f"[regimes] blend {name} C={C}", 2e-4, 1e-3, 1e-4, 2e-3)
        assert float(a.grad.cpu()[sets["invisible"]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answers_through_the_blend_operator():
    """tests/scenes.py:opacity_known_answers in float32 arithmetic through msplat.alpha_blending: pixel values to 1e-6, and
    d pixel / d o of a splat at the cap = G (f - bg)."""
    ms = _ms()
    ka = opacity_known_answers("float32")
    W, H, bg = ka["W"], ka["H"], ka["bg"]
    for case in ka["cases"]:
        uv, conic, op, feat, depth, radius, tiles = known_answer_inputs(case, ka)
        ids, tr = MO.sort_gaussian(uv, depth, W, H, radius, tiles)
        op_g = op.to(DEV).requires_grad_(True)
        out = ms.alpha_blending(uv.to(DEV), conic.to(DEV), op_g, feat.to(DEV), ids.to(DEV), tr.to(DEV), bg, W, H)
        for (x, y), want in case["px"].items():
            assert abs(out[0, y, x].item() - want) < 1e-6, (case["name"], x, y, out[0, y, x].item(), want)
        if "d_o" in case:
            cx, cy = ka["centre"]
            (g,) = torch.autograd.grad(out[0, cy, cx], op_g)
            assert abs(g[0, 0].item() - case["d_o"]) < 1e-6, (g, case["d_o"])


def test_known_answers_through_the_fused_iteration():
    """The same pixels out of a one-iteration engine with lr = 0: splats on the optical axis of a 16 x 16 camera with the
    principal point on pixel (8, 8), scaled so that the EWA covariance is (1 / A) I exactly as the known answers assume
    ((f s / z)^2 + 0.3 = 20); raw opacity 2.0 activates to 1.0f, logit(o) / 10 to the threshold cases."""
    ka = opacity_known_answers("float32")
    W, H, bg, f = ka["W"], ka["H"], ka["bg"], 16.0
    g = torch.Generator().manual_seed(0)
    img, dep = torch.rand(H, W, 3, generator=g), 1.0 + torch.rand(H, W, 1, generator=g)
    for case in ka["cases"]:
        n = len(case["o"])
        z = 2.0 + 0.5 * torch.arange(n, dtype=torch.float64)
        s = (torch.tensor(1.0 / ka["A"] - 0.3, dtype=torch.float64).sqrt() * z / f).float()
        o = torch.tensor(case["o"], dtype=torch.float64)
        raw_o = torch.where(o >= 1.0, torch.full_like(o, 2.0), torch.log(o / (1.0 - o).clamp(min=1e-300)) / 10.0)
        feat = torch.tensor(case["f"], dtype=torch.float64)
        raw = dict(xyz=torch.stack([torch.zeros(n), torch.zeros(n), z.float()], dim=1), scale=s.unsqueeze(1).repeat(1, 3),
                   rotate=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1), opacity=raw_o.float().unsqueeze(1),
                   rgb=torch.log(feat / (1.0 - feat)).float().unsqueeze(1).repeat(1, 3))
        cam = dict(W=W, H=H, intr=torch.tensor([f, f, 8.0, 8.0]))
        eng = _engine(raw, cam, img, dep, bg=bg, lr=0.0, lr_camera=0.0, lambda_rgb=1.0)
        eng.iteration()
        eng.check_overflow()
        if min(case["o"]) >= 1.0 / 255.0:
            conic = eng.rec[:n, 2:5].cpu()
            assert (conic - torch.tensor([ka["A"], 0.0, ka["A"]])).abs().max().item() < 1e-7
        out = eng.render.cpu()
        for (x, y), want in case["px"].items():
            for c in range(3):
                assert abs(out[c, y, x].item() - want) < 1e-6, (case["name"], x, y, c, out[c, y, x].item(), want)
        assert torch.equal(eng.params[:n, :14].cpu()[:, 10], raw["opacity"].reshape(-1))        # lr = 0: nothing moved
