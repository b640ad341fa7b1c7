"""CPU: the gradient of the camera intrinsics -- the library's new entry points reject bad arguments before any launch,
and the reference the GPU tests hold that gradient to (the oracle's float64 autograd) is itself pinned against central
differences of closed forms worked out in python floats."""
import ctypes

import torch

from oracle import msplat_oracle as MO
from tests.scenes import clamp_known_answers

FOV_CLAMP, LOWPASS = 1.3, 0.3


# ------------------------------------------------------------------ closed forms, python floats only
def closed_uv(intr, rx, ry):
    fx, fy, cx, cy = intr
    return (fx * rx + cx, fy * ry + cy)


def closed_conic(intr, rx, ry, s, z, W, H):
    """Conic of an isotropic splat (scale s, depth z, x / z = rx, y / z = ry) under the identity extrinsic, with the
    dependence of the clamp on the focal lengths explicit: limx = FOV_CLAMP W / (2 fx).  On a clamped branch
    a = (s/z)^2 (fx^2 + (FOV_CLAMP W/2)^2) + LOWPASS: the off-diagonal column of the Jacobian no longer carries fx."""
    fx, fy = intr[0], intr[1]
    limx, limy = FOV_CLAMP * W / (2.0 * fx), FOV_CLAMP * H / (2.0 * fy)
    tx, ty = max(min(rx, limx), -limx), max(min(ry, limy), -limy)
    k = s / z
    if abs(rx) > limx:
        a = k * k * (fx * fx + (FOV_CLAMP * W / 2.0) ** 2) + LOWPASS
    else:
        a = (fx * k) ** 2 * (1.0 + rx * rx) + LOWPASS
    if abs(ry) > limy:
        c = k * k * (fy * fy + (FOV_CLAMP * H / 2.0) ** 2) + LOWPASS
    else:
        c = (fy * k) ** 2 * (1.0 + ry * ry) + LOWPASS
    b = (fx * k) * (fy * k) * tx * ty
    det = a * c - b * b
    return (c / det, -b / det, a / det)


def central_difference(f, intr, j, h=1e-3):
    """d f / d intr[j] of a tuple-valued python function, step h (2.5e-5 of the smaller focal: truncation ~1e-9 relative,
    rounding ~1e-11; no step crosses a clamp boundary, the nearest case sits 10 % from it)."""
    lo, hi = list(intr), list(intr)
    lo[j] -= h
    hi[j] += h
    return [(p - m) / (2.0 * h) for p, m in zip(f(hi), f(lo))]


def known_answer_jacobians():
    """Per splat of ``clamp_known_answers``: visible, d uv / d intr (2 x 4) and d conic / d (fx, fy) (3 x 2) by central
    differences of the closed forms.  The splats' inputs are the float32 scene's values read as python floats."""
    ka = clamp_known_answers()
    W, H = ka["W"], ka["H"]
    intr = [float(a) for a in ka["intr"]]
    out = {}
    for name, (k, visible, _, _) in ka["expect"].items():
        x, y, z = (float(a) for a in ka["xyz"][k])
        s = float(ka["scale"][k, 0])
        rx, ry = x / z, y / z
        d_uv = [[central_difference(lambda i: closed_uv(i, rx, ry), intr, j)[r] for j in range(4)] for r in range(2)]
        d_conic = [[central_difference(lambda i: closed_conic(i, rx, ry, s, z, W, H), intr, j)[r] for j in range(2)]
                   for r in range(3)]
        out[name] = (k, visible, torch.tensor(d_uv, dtype=torch.float64), torch.tensor(d_conic, dtype=torch.float64))
    return ka, out


def operator_jacobians(ka, project_point, compute_cov3d, ewa_project, dtype, device="cpu"):
    """The same Jacobians from any implementation of the three operators, by one backward per output entry:
    d_uv (N, 2, 4) and d_conic (N, 3, 4) -- the intrinsics gradient of every entry of uv and of conic."""
    n = ka["xyz"].shape[0]
    xyz, scale, rot, extr = (ka[k].to(dtype).to(device) for k in ("xyz", "scale", "rotate", "extr"))
    intr = ka["intr"].to(dtype).to(device).requires_grad_(True)
    uv, depth = project_point(xyz, intr, extr, ka["W"], ka["H"])
    vis = depth != 0
    conic, radius, _ = ewa_project(xyz, compute_cov3d(scale, rot, vis), intr, extr, uv.detach(), ka["W"], ka["H"], vis)
    d_uv = torch.zeros(n, 2, 4, dtype=torch.float64)
    d_conic = torch.zeros(n, 3, 4, dtype=torch.float64)
    for k in range(n):
        for r in range(2):
            d_uv[k, r] = torch.autograd.grad(uv[k, r], intr, retain_graph=True)[0].double().cpu()
        for r in range(3):
            d_conic[k, r] = torch.autograd.grad(conic[k, r], intr, retain_graph=True)[0].double().cpu()
    return d_uv, d_conic, depth.detach().cpu(), radius.detach().cpu()


def check_jacobians(ka, want, d_uv, d_conic, rel, observe=None):
    """Visible splats: every gradient vector within ``rel`` of the closed form's, relative to that vector's largest entry;
    the conic does not depend on cx, cy at all.  The culled splat: zero rows."""
    worst = 0.0
    for name, (k, visible, uv_ref, conic_ref) in want.items():
        if not visible:
            assert torch.all(d_uv[k] == 0) and torch.all(d_conic[k] == 0), name
            continue
        assert torch.all(d_conic[k][:, 2:] == 0), f"{name}: the conic's gradient has a cx / cy part"
        for what, got, ref in (("d uv / d intr", d_uv[k], uv_ref), ("d conic / d fx", d_conic[k][:, 0], conic_ref[:, 0]),
                               ("d conic / d fy", d_conic[k][:, 1], conic_ref[:, 1])):
            assert float(ref.abs().max()) > 0, (name, what)
            err = float((got - ref).abs().max() / ref.abs().max())
            worst = max(worst, err)
            if observe is not None:
                observe(f"known answers, {name}: {what} off by {err:.2e} of its largest entry (bound {rel:g})")
            assert err < rel, f"{name}: {what} off by {err:.3e} (bound {rel:g})\n{got}\n{ref}"
    return worst


# ------------------------------------------------------------------ tests
def test_cam_entries_reject_bad_arguments_without_a_gpu():
    """A null d_intr is GFL_ERR_INVALID before any launch, for each of the three entries; the 16-wide workspace is
    rows x 16 floats and the 12-wide one is what it was."""
    from gflow_amd import _lib, fused
    lib = _lib.load()
    fused._declare(lib)
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)          # any non-null address: nothing may be read or launched before the refusal
    assert lib.gfl_project_point_bwd_cam(one, one, one, one, one, one, 5, one, one, null, one, 1 << 20, null) == -1
    assert lib.gfl_project_point_bwd_cam(one, one, one, one, one, one, 5, one, null, one, one, 1 << 20, null) == -1
    assert lib.gfl_ewa_bwd_cam(one, one, one, one, one, one, 5, 64, 48, one, one, one, null, one, 1 << 20, null) == -1
    assert lib.gfl_ewa_bwd_cam(one, one, one, one, one, one, 5, 64, 48, one, one, null, one, one, 1 << 20, null) == -1
    st, hp = fused.FitState(), fused.FitHyper()
    assert lib.gfl_render_bwd_cam(ctypes.byref(st), ctypes.byref(hp), one, null, null, one, one, null, null) == -1
    assert lib.gfl_render_bwd_cam(ctypes.byref(st), ctypes.byref(hp), one, null, null, one, null, one, null) == -1
    # too little workspace is its own status, also before any launch
    assert lib.gfl_project_point_bwd_cam(one, one, one, one, one, one, 5, one, one, one, one, 16 * 4 - 1, null) == -2
    assert lib.gfl_ewa_bwd_cam(one, one, one, one, one, one, 5, 64, 48, one, one, one, one, one, 16 * 4 - 1, null) == -2
    assert lib.gfl_reduce_cam_workspace_bytes(60000) == 235 * 16 * 4
    assert lib.gfl_reduce_workspace_bytes(60000) == 235 * 12 * 4
    assert lib.gfl_version() >= 309


def test_oracle_float64_intrinsics_gradient_matches_closed_form_differences():
    """The seven splats of ``clamp_known_answers`` (64 x 48, intr = (40, 27, 16, 34), every clamp branch): the oracle's
    float64 autograd in intr against central differences of the closed forms, relative 1e-6; zero rows for the culled one."""
    ka, want = known_answer_jacobians()
    d_uv, d_conic, depth, radius = operator_jacobians(ka, MO.project_point, MO.compute_cov3d, MO.ewa_project, torch.float64)
    n_vis = sum(1 for v in want.values() if v[1])
    assert n_vis == 6 and int((depth != 0).sum()) == 6 and int((radius > 0).sum()) == 6
    # the clamped branches really have no fx in the Jacobian's third column: d a / d fx = 2 (s/z)^2 fx there
    k, _, _, conic_ref = want["x_clamped"]
    assert float(conic_ref[:, 0].abs().max()) > 0
    check_jacobians(ka, want, d_uv, d_conic, 1e-6)
