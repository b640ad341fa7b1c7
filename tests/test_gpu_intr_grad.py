"""The gradient of the camera intrinsics through gflow_amd.msplat.project_point / ewa_project, gflow_amd.render.render and
render_multiple on both routes (``-m gpu``), against the CPU oracle's autograd in FLOAT64 (the float32 scene upcast).

Bounds are the ones d_extr -- which goes through the same reduction -- is held to: relative L2 1e-3 through the operators
and render_multiple's operator route (tests/test_gpu_parity.py), 2e-3 through the fused render() (tests/test_gpu_render_op.py).
The float32 oracle differs from the float64 one by at most 2.5e-5 (render) and 5e-7 (operators) on d_intr at these shapes.
A single component of d_intr is checked (to the same bound, relative to itself) only in a weight set where the reference
component is at least 10 % of the vector's norm; that is asserted on the CPU before anything runs on the device."""
import math

import pytest
import torch

from oracle import msplat_oracle as MO
from tests.scenes import CAMERAS, CLAMPING, assert_regime, camera_scene, take_rows
from tests.test_gpu_parity import DEV, observe, rel_l2, to_dev
from tests.test_gpu_render_op import NAMES, _loss, _weights
from tests.test_intr_grad_host import check_jacobians, known_answer_jacobians, operator_jacobians

pytestmark = pytest.mark.gpu

INTR_NAMES = ("fx", "fy", "cx", "cy")
MIN_SHARE = 0.10
F64 = torch.float64


def _ms():
    import gflow_amd.msplat as ms
    return ms


def _check_d_intr(got, ref, bound, what, components):
    """``got`` (4,) against the float64 ``ref``: relative L2 of the vector, then each of ``components`` relative to itself."""
    got, ref = got.detach().double().cpu().reshape(4), ref.detach().double().reshape(4)
    rel = rel_l2(got, ref)
    observe(f"{what}: d_intr relative L2 {rel:.2e} (bound {bound:g})")
    assert rel < bound, f"{what}: d_intr relative L2 error {rel:.2e}\n{got}\n{ref}"
    for k in components:
        err = abs(float(got[k] - ref[k])) / abs(float(ref[k]))
        observe(f"{what}: d_{INTR_NAMES[k]} off by {err:.2e} of itself (bound {bound:g})")
        assert err < bound, f"{what}: d_{INTR_NAMES[k]} {float(got[k]):.9g} against {float(ref[k]):.9g}"


def _assert_shares(ref, components, what):
    """(on the CPU, before the device runs) the components a weight set is for carry at least MIN_SHARE of the norm"""
    ref = ref.detach().double().reshape(4)
    share = ref.abs() / ref.norm()
    for k in components:
        assert float(share[k]) >= MIN_SHARE, f"{what}: the reference d_{INTR_NAMES[k]} is {float(share[k]):.3f} of the norm"
    return share


# ------------------------------------------------------------------ 1. operators under the four cameras
def _projection_weights(s):
    """Two weight sets on (uv, depth).  ``abs``: |randn| -- the sums of du, dv do not cancel: cx, cy.  ``signed``:
    |randn| sign(u - cx), |randn| sign(v - cy) -- the sums of du px/pz, dv py/pz do not cancel: fx, fy.  (Random signs leave
    d_fx, d_fy at ~1e-3 of the norm under a centred camera.)"""
    g = torch.Generator().manual_seed(21)
    n = s["xyz"].shape[0]
    a = torch.randn(n, 2, generator=g).abs()
    wd = torch.randn(n, 1, generator=g)
    uv, _ = MO.project_point(s["xyz"], s["intr"], s["extr"], s["W"], s["H"])
    sign = torch.sign(uv - s["intr"][2:4])
    return {"abs": (a, wd, (2, 3)), "signed": (a * sign, wd, (0, 1))}


def _project_reference(s, wu, wd):
    intr = s["intr"].to(F64).requires_grad_(True)
    extr = s["extr"].to(F64).requires_grad_(True)
    uv, dep = MO.project_point(s["xyz"].to(F64), intr, extr, s["W"], s["H"])
    ((uv * wu.to(F64)).sum() + (dep * wd.to(F64)).sum()).backward()
    return intr.grad, extr.grad


def _check_project_intr(s, tag):
    ms = _ms()
    sets = _projection_weights(s)
    refs = {}
    for name, (wu, wd, comps) in sets.items():
        refs[name] = _project_reference(s, wu, wd)
        _assert_shares(refs[name][0], comps, f"{tag}project_point, weights {name}")
    d = to_dev(s)
    for name, (wu, wd, comps) in sets.items():
        intr = d["intr"].clone().requires_grad_(True)
        extr = d["extr"].clone().requires_grad_(True)
        uv, dep = ms.project_point(d["xyz"], intr, extr, s["W"], s["H"])
        ((uv * wu.to(DEV)).sum() + (dep * wd.to(DEV)).sum()).backward()
        assert intr.grad.shape == (4,) and intr.grad.dtype == torch.float32 and intr.grad.device == intr.device
        _check_d_intr(intr.grad, refs[name][0], 1e-3, f"{tag}project_point, weights {name}", comps)
        rel = rel_l2(extr.grad, refs[name][1])
        observe(f"{tag}project_point, weights {name}: d_extr relative L2 {rel:.2e} (bound 0.001)")
        assert rel < 1e-3


def _ewa_inputs(s):
    """uv, visibility and cov3d of the float32 oracle: the same inputs go to the float64 reference and to the device"""
    uv, depth = MO.project_point(s["xyz"], s["intr"], s["extr"], s["W"], s["H"])
    vis = depth != 0
    return uv, vis, MO.compute_cov3d(s["scale"], s["rotate"], vis)


def _ewa_reference(s, uv, vis, cov, w):
    intr = s["intr"].to(F64).requires_grad_(True)
    extr = s["extr"].to(F64).requires_grad_(True)
    conic = MO.ewa_project(s["xyz"].to(F64), cov.to(F64), intr, extr, uv.to(F64), s["W"], s["H"], vis)[0]
    (conic * w.to(F64)).sum().backward()
    return intr.grad, extr.grad


def _check_ewa_intr(s, tag):
    ms = _ms()
    uv, vis, cov = _ewa_inputs(s)
    w = torch.randn(s["xyz"].shape[0], 3, generator=torch.Generator().manual_seed(22)).abs()
    ref_intr, ref_extr = _ewa_reference(s, uv, vis, cov, w)
    _assert_shares(ref_intr, (0, 1), f"{tag}ewa_project, weights abs")
    assert float(ref_intr[2]) == 0 and float(ref_intr[3]) == 0          # the conic does not depend on cx, cy
    d = to_dev(s)
    intr = d["intr"].clone().requires_grad_(True)
    extr = d["extr"].clone().requires_grad_(True)
    conic = ms.ewa_project(d["xyz"], cov.to(DEV), intr, extr, uv.to(DEV), s["W"], s["H"], vis.to(DEV))[0]
    (conic * w.to(DEV)).sum().backward()
    assert intr.grad.shape == (4,) and intr.grad.dtype == torch.float32
    _check_d_intr(intr.grad, ref_intr, 1e-3, f"{tag}ewa_project, weights abs", (0, 1))
    assert float(intr.grad[2]) == 0 and float(intr.grad[3]) == 0
    rel = rel_l2(extr.grad, ref_extr)
    observe(f"{tag}ewa_project, weights abs: d_extr relative L2 {rel:.2e} (bound 0.001)")
    assert rel < 1e-3


_CAM_SCENES = {}


def _cam_scene(cam):
    if cam not in _CAM_SCENES:
        s = camera_scene(3000, 200, 136, cam, seed=11, sigma_px=2.5)
        sets = assert_regime(cam, s)
        only = None
        if cam in CLAMPING:
            only = take_rows(s, sets["any"])
            assert bool(assert_regime(cam, only)["any"].all())
        _CAM_SCENES[cam] = (s, only)
    return _CAM_SCENES[cam]


@pytest.mark.parametrize("cam", CAMERAS)
def test_operator_intrinsics_gradient_under_camera(cam):
    """d_intr of project_point and of ewa_project as a 4-vector and component by component; under the clamping cameras
    once more on the clamped splats alone -- that gradient is the clamp branch's and nothing else's."""
    s, only = _cam_scene(cam)
    _check_project_intr(s, f"[{cam}] ")
    _check_ewa_intr(s, f"[{cam}] ")
    if only is not None:
        _check_project_intr(only, f"[{cam}, clamped splats only] ")
        _check_ewa_intr(only, f"[{cam}, clamped splats only] ")


# ------------------------------------------------------------------ 2. known answers on the device
def test_known_answers_through_msplat():
    """The seven splats of ``clamp_known_answers`` through msplat.project_point / ewa_project on the device, against the
    closed-form central differences of the host test: relative 2e-5, ``check_known_answers``' tolerance for the conics."""
    ms = _ms()
    ka, want = known_answer_jacobians()
    d_uv, d_conic, depth, radius = operator_jacobians(ka, ms.project_point, ms.compute_cov3d, ms.ewa_project,
                                                      torch.float32, DEV)
    assert int((depth != 0).sum()) == 6 and int((radius > 0).sum()) == 6
    check_jacobians(ka, want, d_uv, d_conic, 2e-5, observe)


# ------------------------------------------------------------------ 3. reduction edges
def _edge_scene(n):
    # (one splat: in the middle of the frustum, so that it has a footprint and a gradient)
    return camera_scene(n, 200, 136, "general", seed=7, sigma_px=2.5, **(dict(spread=0.5, behind=0.0) if n == 1 else {}))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_reduction_edges_of_the_cam_entries(n):
    """The 16-wide reduction at the last lane of a block and the first of the next (255 / 256 / 257) and at the first
    size at which a thread of the fold takes a second row (65 537): d_extr of the _cam entry has the bits of the old
    entry's, d_intr is within 1e-3 of the oracle.  Per-splat work only."""
    from gflow_amd import _lib as L
    lib = L.load()
    ms = _ms()
    s = _edge_scene(n)
    W, H = s["W"], s["H"]
    g = torch.Generator().manual_seed(23)
    wu, wd, wc = torch.randn(n, 2, generator=g).abs(), torch.randn(n, 1, generator=g), torch.randn(n, 3, generator=g).abs()
    uv_c, vis_c, cov_c = _ewa_inputs(s)
    ref_p = _project_reference(s, wu, wd)[0]
    ref_e = _ewa_reference(s, uv_c, vis_c, cov_c, wc)[0]
    assert float(ref_p.norm()) > 0 and float(ref_e.norm()) > 0
    d = to_dev(s)
    xyz, intr, extr = d["xyz"].contiguous(), d["intr"].contiguous(), d["extr"].contiguous()
    f32 = dict(dtype=torch.float32, device=DEV)
    with torch.no_grad():
        uv, depth = ms.project_point(xyz, intr, extr, W, H)
        cov = cov_c.to(DEV)
        radius = ms.ewa_project(xyz, cov, intr, extr, uv_c.to(DEV), W, H, vis_c.to(DEV))[1].contiguous()
    ws12 = L.scratch(lib.gfl_reduce_workspace_bytes(n), DEV)
    ws16 = L.scratch(lib.gfl_reduce_cam_workspace_bytes(n), DEV)
    assert lib.gfl_reduce_cam_workspace_bytes(n) == ((n + 255) // 256) * 16 * 4
    du, dd, dc = wu.to(DEV).contiguous(), wd.to(DEV).contiguous(), wc.to(DEV).contiguous()
    # project_point
    dx_a, dx_b = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
    de_a, de_b, di = torch.empty(12, **f32), torch.empty(12, **f32), torch.empty(4, **f32)
    L.check(lib.gfl_project_point_bwd(L.ptr(xyz), L.ptr(intr), L.ptr(extr), L.ptr(depth), L.ptr(du), L.ptr(dd), n, L.ptr(dx_a),
                                      L.ptr(de_a), L.ptr(ws12), ws12.numel(), L.stream()), "project_point backward")
    L.check(lib.gfl_project_point_bwd_cam(L.ptr(xyz), L.ptr(intr), L.ptr(extr), L.ptr(depth), L.ptr(du), L.ptr(dd), n,
                                          L.ptr(dx_b), L.ptr(de_b), L.ptr(di), L.ptr(ws16), ws16.numel(), L.stream()),
            "project_point backward with d_intr")
    assert torch.equal(de_a, de_b) and torch.equal(dx_a, dx_b)
    _check_d_intr(di, ref_p, 1e-3, f"[N = {n}] gfl_project_point_bwd_cam", ())
    # ewa_project
    dx_a, dx_b = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
    dv_a, dv_b = torch.empty(n, 6, **f32), torch.empty(n, 6, **f32)
    de_a, de_b, di = torch.empty(12, **f32), torch.empty(12, **f32), torch.empty(4, **f32)
    L.check(lib.gfl_ewa_bwd(L.ptr(xyz), L.ptr(cov), L.ptr(intr), L.ptr(extr), L.ptr(radius), L.ptr(dc), n, W, H, L.ptr(dx_a),
                            L.ptr(dv_a), L.ptr(de_a), L.ptr(ws12), ws12.numel(), L.stream()), "ewa_project backward")
    L.check(lib.gfl_ewa_bwd_cam(L.ptr(xyz), L.ptr(cov), L.ptr(intr), L.ptr(extr), L.ptr(radius), L.ptr(dc), n, W, H,
                                L.ptr(dx_b), L.ptr(dv_b), L.ptr(de_b), L.ptr(di), L.ptr(ws16), ws16.numel(), L.stream()),
            "ewa_project backward with d_intr")
    assert torch.equal(de_a, de_b) and torch.equal(dx_a, dx_b) and torch.equal(dv_a, dv_b)
    _check_d_intr(di, ref_e, 1e-3, f"[N = {n}] gfl_ewa_bwd_cam", ())


# ------------------------------------------------------------------ 4. N = 0
def test_no_splats_give_a_zero_intrinsics_gradient():
    import gflow_amd.render as R
    ms = _ms()
    s = to_dev(camera_scene(8, 96, 80, "general", seed=1))
    e = {k: s[k][:0] for k in NAMES}
    zero = torch.zeros(4)
    intr = s["intr"].clone().requires_grad_(True)
    uv, depth = ms.project_point(e["xyz"], intr, s["extr"], 96, 80)
    (uv.sum() + depth.sum()).backward()
    assert intr.grad is not None and torch.equal(intr.grad.cpu(), zero)
    intr = s["intr"].clone().requires_grad_(True)
    vis = torch.zeros(0, 1, dtype=torch.bool, device=DEV)
    conic = ms.ewa_project(e["xyz"], torch.zeros(0, 6, device=DEV), intr, s["extr"], torch.zeros(0, 2, device=DEV), 96, 80, vis)[0]
    conic.sum().backward()
    assert intr.grad is not None and torch.equal(intr.grad.cpu(), zero)
    intr = s["intr"].clone().requires_grad_(True)
    out = R.render(e, dict(intr=intr, extr=s["extr"], W=96, H=80), 0.33)
    (out["rgb"].sum() + out["depth_map"].sum() + out["uv"].sum() + out["depth"].sum()).backward()
    assert intr.grad is not None and intr.grad.shape == (4,) and torch.equal(intr.grad.cpu(), zero)


# ------------------------------------------------------------------ 5. / 6. render() and render_multiple
_RENDER_REFS = {}


def _render_reference(key, s, bg):
    """float64 oracle of ``_check_render_operator``'s set-up (weights seed 5 on rgb, depth_map, uv, depth), computed once"""
    if key not in _RENDER_REFS:
        n, W, H = s["xyz"].shape[0], s["W"], s["H"]
        w = _weights(H, W, n, 5)
        intr = s["intr"].to(F64).requires_grad_(True)
        extr = s["extr"].to(F64).requires_grad_(True)
        oc = MO.render_multiple([*[s[k].to(F64) for k in NAMES], intr, extr, bg, W, H], ["rgb", "uv", "depth", "depth_map"])
        _loss(oc, [t.to(F64) for t in w]).backward()
        _RENDER_REFS[key] = (w, intr.grad.clone(), extr.grad.clone())
    return _RENDER_REFS[key]


def _device_render_grads(s, w, bg, fn):
    d = to_dev(s)
    leaves = {k: d[k].clone().requires_grad_(True) for k in NAMES}
    intr = d["intr"].clone().requires_grad_(True)
    extr = d["extr"].clone().requires_grad_(True)
    out = fn(leaves, intr, extr)
    _loss(out, [t.to(DEV) for t in w]).backward()
    return intr.grad, extr.grad


def _check_render_intr(key, s, bg, tag):
    import gflow_amd.render as R
    w, ref_intr, ref_extr = _render_reference(key, s, bg)
    # one weight set here: the components that carry MIN_SHARE of the reference's norm are checked one by one -- all four
    # under ``general`` (0.53, 0.12, 0.80, 0.25 of the norm), all but d_fx (0.09) under ``fov90``, all four on the clamped splats
    components = tuple(k for k in range(4) if float(ref_intr[k].abs() / ref_intr.norm()) >= MIN_SHARE)
    assert len(components) >= (4 if key.startswith("general") else 3), f"{tag}: {ref_intr / ref_intr.norm()}"
    d_intr, d_extr = _device_render_grads(
        s, w, bg, lambda lv, intr, extr: R.render(lv, dict(intr=intr, extr=extr, W=s["W"], H=s["H"]), bg))
    assert d_intr.shape == (4,) and d_intr.dtype == torch.float32 and d_intr.is_cuda
    _check_d_intr(d_intr, ref_intr, 2e-3, tag, components)
    rel = rel_l2(d_extr, ref_extr)
    observe(f"{tag}: d_extr relative L2 {rel:.2e} (bound 0.002)")
    assert rel < 2e-3


@pytest.mark.parametrize("cam", ["general", "fov90"])
def test_render_intrinsics_gradient_under_camera(cam):
    """render() with intr.requires_grad_() on both sides, in ``_check_render_operator``'s set-up (bg 0.33 as its
    under-camera test): the 4-vector to 2e-3, the components that qualify to 2e-3 of themselves; ``general`` once more on
    its clamped splats alone."""
    s, only = _cam_scene(cam)
    _check_render_intr(cam, s, 0.33, f"[{cam}] render()")
    if only is not None:
        _check_render_intr(cam + "/clamped", only, 0.33, f"[{cam}, clamped splats only] render()")


def test_render_multiple_carries_the_intrinsics_gradient_on_both_routes():
    """render_multiple through the fused operator (2e-3) and through the five operators (1e-3) against the oracle, and
    the two routes against each other (2e-3)."""
    import gflow_amd.render as R
    s, _ = _cam_scene("general")
    bg, want = 0.33, ["rgb", "uv", "depth", "depth_map"]
    w, ref_intr, _ = _render_reference("general", s, bg)
    fn = lambda lv, intr, extr: R.render_multiple([*[lv[k] for k in NAMES], intr, extr, bg, s["W"], s["H"]], want)
    assert R.USE_FUSED
    fused = _device_render_grads(s, w, bg, fn)[0]
    R.USE_FUSED = False
    try:
        ops = _device_render_grads(s, w, bg, fn)[0]
    finally:
        R.USE_FUSED = True
    _check_d_intr(fused, ref_intr, 2e-3, "[general] render_multiple, fused route", ())
    _check_d_intr(ops, ref_intr, 1e-3, "[general] render_multiple, operator route", ())
    rel = rel_l2(fused, ops)
    observe(f"[general] render_multiple: d_intr of the fused route against the operator route, relative L2 {rel:.2e} (bound 0.002)")
    assert rel < 2e-3


# ------------------------------------------------------------------ 7. asking changes nothing else
def _render_once(s, ask):
    import gflow_amd.render as R
    leaves = {k: s[k].clone().requires_grad_(True) for k in NAMES}
    intr = s["intr"].clone().requires_grad_(ask)
    extr = s["extr"].clone().requires_grad_(True)
    out = R.render(leaves, dict(intr=intr, extr=extr, W=s["W"], H=s["H"]), 0.0)
    (out["rgb"].sum() + out["depth_map"].sum()).backward()
    grads = {k: leaves[k].grad.clone() for k in NAMES}
    grads["extr"] = extr.grad.clone()
    return grads, (intr.grad.clone() if ask else intr.grad)


def test_asking_for_the_intrinsics_gradient_changes_nothing_else():
    s = to_dev(camera_scene(1200, 96, 80, "general", seed=1, sigma_px=2.5))
    torch.use_deterministic_algorithms(True)
    try:
        without, none = _render_once(s, False)
        with_a, di_a = _render_once(s, True)
        with_b, di_b = _render_once(s, True)
    finally:
        torch.use_deterministic_algorithms(False)
    assert none is None
    for k in (*NAMES, "extr"):
        assert torch.equal(without[k], with_a[k]) and torch.equal(with_a[k], with_b[k]), k
    assert torch.equal(di_a, di_b) and bool((di_a != 0).all())
    # default mode: run-to-run differences of the backward blend's LDS adds, the tolerance of
    # test_two_forwards_before_their_backwards_and_empty_input
    without, _ = _render_once(s, False)
    with_a, _ = _render_once(s, True)
    for k in (*NAMES, "extr"):
        x, y = with_a[k], without[k]
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-6 * float(y.abs().max()) + 1e-7), k


# ------------------------------------------------------------------ 8. the gradient is usable
@pytest.mark.parametrize("k0", [1.06, 0.94])
@pytest.mark.parametrize("cam", ["general", "fov90"])
def test_focal_scale_is_recovered_by_adam(cam, k0):
    """One scalar log k scales fx and fy; the target is render() at the true intr.  Adam(lr 5e-3), 120 iterations on
    mse(rgb) + 0.1 mse(depth_map).  The oracle alone ends at |k - 1| <= 8e-5 on the CPU; the bound is 25 x that and is
    passed only by a gradient of the right sign and scale."""
    import gflow_amd.render as R
    s = to_dev(camera_scene(1200, 96, 80, cam, seed=1, sigma_px=2.5))
    gs = {k: s[k] for k in NAMES}
    cam_of = lambda intr: dict(intr=intr, extr=s["extr"], W=s["W"], H=s["H"])
    with torch.no_grad():
        target = R.render(gs, cam_of(s["intr"]), 0.0)
        target = {k: target[k].clone() for k in ("rgb", "depth_map")}
    log_k = torch.tensor(math.log(k0), dtype=torch.float32, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([log_k], lr=5e-3)
    mse = torch.nn.functional.mse_loss
    for _ in range(120):
        opt.zero_grad()
        k = torch.exp(log_k)
        intr = torch.stack([s["intr"][0] * k, s["intr"][1] * k, s["intr"][2], s["intr"][3]])
        out = R.render(gs, cam_of(intr), 0.0)
        loss = mse(out["rgb"], target["rgb"]) + 0.1 * mse(out["depth_map"], target["depth_map"])
        loss.backward()
        opt.step()
    k = math.exp(float(log_k))
    observe(f"[{cam}] focal scale from k = {k0}: |k - 1| = {abs(k - 1):.2e} after 120 Adam steps (bound 0.002)")
    assert abs(k - 1.0) < 2e-3, f"k = {k}"
