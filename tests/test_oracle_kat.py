"""Known-answer and self-consistency tests of the rasteriser oracle (CPU).
The rasteriser oracle is PARITY-UNPINNED against real msplat (oracle/__init__.py);
these tests pin it analytically instead (last row)."""
import math

import numpy as np
import pytest
import torch

from oracle import msplat_oracle as MO
from tests.scenes import camera, random_scene, scene_group


def _one_blob(W, H, u, v, conic, opacity, feat, bg, C):
    uv = torch.tensor([[u, v]], dtype=torch.float32)
    con = torch.tensor([conic], dtype=torch.float32)
    op = torch.tensor([[opacity]], dtype=torch.float32)
    f = torch.tensor([feat], dtype=torch.float32)
    ids, tr = MO.sort_gaussian(uv, torch.tensor([[1.0]]), W, H, torch.tensor([[6]], dtype=torch.int32),
                               torch.tensor([[0]], dtype=torch.int32))
    return MO.alpha_blending(uv, con, op, f, ids, tr, bg, W, H)


def test_center_recipe_single_blob():
    # the reference's own "center" recipe: conic [1,0,1], opacity 1 (render.py:93-97)
    W, H = 48, 32
    out = _one_blob(W, H, 20.0, 12.0, [1.0, 0.0, 1.0], 1.0, [0.2, 0.5, 0.9], 0.33, 3)
    tile_x0, tile_x1 = 0, 32    # radius 6 around u=20 touches tile columns 0 and 1
    for (x, y) in [(20, 12), (21, 12), (22, 14), (17, 9), (26, 12)]:
        r2 = (20 - x) ** 2 + (12 - y) ** 2
        a = min(0.99, math.exp(-0.5 * r2))
        a = a if a >= 1 / 255 else 0.0
        for c, f in enumerate([0.2, 0.5, 0.9]):
            assert abs(out[c, y, x].item() - (a * f + (1 - a) * 0.33)) < 1e-6
    # far away: background only
    assert abs(out[0, 30, 46].item() - 0.33) < 1e-7


def test_depth_order_matters():
    W, H = 32, 32
    uv = torch.tensor([[10.0, 10.0], [11.0, 10.0]])
    con = torch.tensor([[0.3, 0.0, 0.3], [0.3, 0.0, 0.3]])
    op = torch.tensor([[0.8], [0.8]])
    f = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    rad = torch.tensor([[8], [8]], dtype=torch.int32)
    tl = torch.zeros(2, 1, dtype=torch.int32)
    imgs = []
    for d in ([[1.0], [2.0]], [[2.0], [1.0]]):
        ids, tr = MO.sort_gaussian(uv, torch.tensor(d), W, H, rad, tl)
        imgs.append(MO.alpha_blending(uv, con, op, f, ids, tr, 0.0, W, H))
    a0 = 0.8
    a1 = 0.8 * math.exp(-0.5 * 0.3)
    # pixel (10,10): splat 0 centred there
    assert abs(imgs[0][0, 10, 10].item() - a0) < 1e-6
    assert abs(imgs[0][1, 10, 10].item() - a1 * (1 - a0)) < 1e-6
    assert abs(imgs[1][1, 10, 10].item() - a1) < 1e-6
    assert abs(imgs[1][0, 10, 10].item() - a0 * (1 - a1)) < 1e-6


def test_culled_points_signal_zero():
    W, H = 64, 48
    intr, extr = camera(W, H)
    xyz = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, 0.1], [0.0, 0.0, 2.0], [100.0, 0.0, 1.0]])
    uv, depth = MO.project_point(xyz, intr, extr, W, H)
    assert depth[0, 0] == 0 and depth[1, 0] == 0 and depth[3, 0] == 0
    assert torch.all(uv[0] == 0) and torch.all(uv[1] == 0) and torch.all(uv[3] == 0)
    assert depth[2, 0] == 2.0 and abs(uv[2, 0].item() - W / 2) < 1e-5 and abs(uv[2, 1].item() - H / 2) < 1e-5


def test_depth_channel_with_background():
    W, H = 32, 16
    out = _one_blob(W, H, 8.0, 8.0, [0.5, 0.0, 0.5], 0.6, [2.5], 1.0, 1)
    a = 0.6
    assert abs(out[0, 8, 8].item() - (a * 2.5 + (1 - a) * 1.0)) < 1e-6
    assert out.shape == (1, H, W)


def test_empty_input_gives_background():
    W, H = 40, 24
    s = random_scene(0, W, H)
    out = MO.render_multiple(scene_group(s, bg=0.33), ["rgb", "depth_map", "uv"])
    assert out["rgb"].shape == (3, H, W) and torch.all(out["rgb"] == 0.33)
    assert torch.all(out["depth_map"] == 0.33) and out["uv"].shape == (0, 2)


def test_identity_cov_projects_to_isotropic_conic():
    # unit-quaternion, isotropic scale s at depth z on the axis: Sigma2 = (f s / z)^2 I + 0.3 I
    W, H = 64, 64
    intr, extr = camera(W, H, f=50.0)
    xyz = torch.tensor([[0.0, 0.0, 2.0]])
    sc = torch.tensor([[0.1, 0.1, 0.1]])
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    uv, depth = MO.project_point(xyz, intr, extr, W, H)
    cov = MO.compute_cov3d(sc, q, depth != 0)
    np.testing.assert_allclose(cov.numpy(), [[0.01, 0, 0, 0.01, 0, 0.01]], atol=1e-8)
    conic, radius, tiles = MO.ewa_project(xyz, cov, intr, extr, uv, W, H, depth != 0)
    var = (50.0 * 0.1 / 2.0) ** 2 + 0.3
    np.testing.assert_allclose(conic.numpy(), [[1 / var, 0, 1 / var]], rtol=1e-5, atol=1e-7)
    assert radius.item() == math.ceil(3 * math.sqrt(var + math.sqrt(0.1)))
    assert tiles.item() == 4          # centre (32,32) radius 8 -> tiles 1..2 in x and y


@pytest.mark.parametrize("seed", [0, 1])
def test_vectorised_blend_matches_literal_loops(seed):
    W, H = 40, 36                      # ragged: 2.5 x 2.25 tiles
    s = random_scene(300, W, H, seed=seed, sigma_px=3.0)
    uv, depth = MO.project_point(s["xyz"], s["intr"], s["extr"], W, H)
    vis = depth != 0
    cov = MO.compute_cov3d(s["scale"], s["rotate"], vis)
    conic, radius, tiles = MO.ewa_project(s["xyz"], cov, s["intr"], s["extr"], uv, W, H, vis)
    ids, tr = MO.sort_gaussian(uv, depth, W, H, radius, tiles)
    assert ids.numel() == int(tiles.sum())
    feat = torch.cat([s["rgb"], depth], dim=1)
    fast = MO.alpha_blending(uv, conic, s["opacity"], feat, ids, tr, 0.33, W, H)
    slow, final_T, ncon = MO.alpha_blending_loops(uv, conic, s["opacity"], feat, ids, tr, 0.33, W, H)
    np.testing.assert_allclose(fast.numpy(), slow, rtol=2e-5, atol=2e-6)
    assert ncon.max() > 3             # the scene really has overlapping splats


def test_termination_branch_is_exercised():
    # a stack of opaque splats: T falls below 1e-4 and later splats must not contribute
    W, H = 16, 16
    n = 12
    uv = torch.full((n, 2), 8.0)
    con = torch.tensor([[0.05, 0.0, 0.05]]).repeat(n, 1)
    op = torch.full((n, 1), 0.95)
    f = torch.linspace(0.1, 1.0, n).unsqueeze(1)
    d = torch.linspace(1.0, 2.0, n).unsqueeze(1)
    ids, tr = MO.sort_gaussian(uv, d, W, H, torch.full((n, 1), 10, dtype=torch.int32), torch.zeros(n, 1, dtype=torch.int32))
    fast = MO.alpha_blending(uv, con, op, f, ids, tr, 1.0, W, H)
    slow, final_T, ncon = MO.alpha_blending_loops(uv, con, op, f, ids, tr, 1.0, W, H)
    np.testing.assert_allclose(fast.numpy(), slow, rtol=1e-5, atol=1e-7)
    assert ncon[8, 8] == 3             # 0.05^3 = 1.25e-4 >= 1e-4 > 0.05^4
    assert abs(final_T[8, 8] - 0.05 ** 3) < 1e-9


def test_gradcheck_float64_ops():
    W, H = 32, 32
    s = random_scene(6, W, H, seed=3, dtype=torch.float64, sigma_px=3.0, behind=0.0, spread=0.6)
    xyz = s["xyz"].clone().requires_grad_(True)
    extr = s["extr"].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, e: MO.project_point(a, s["intr"], e, W, H), (xyz, extr), atol=1e-7)
    sc = s["scale"].clone().requires_grad_(True)
    q = s["rotate"].clone().requires_grad_(True)
    vis = torch.ones(6, 1, dtype=torch.bool)
    assert torch.autograd.gradcheck(lambda a, b: MO.compute_cov3d(a, b, vis), (sc, q), atol=1e-7)
    uv, depth = MO.project_point(s["xyz"], s["intr"], s["extr"], W, H)
    cov = MO.compute_cov3d(s["scale"], s["rotate"], vis).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, c, e: MO.ewa_project(a, c, s["intr"], e, uv, W, H, vis)[0], (xyz, cov, extr), atol=1e-6)


def test_gradcheck_float64_full_render():
    W, H = 32, 32
    s = random_scene(5, W, H, seed=5, dtype=torch.float64, sigma_px=3.0, behind=0.0, spread=0.5)
    leaves = [s[k].clone().requires_grad_(True) for k in ("xyz", "scale", "rotate", "opacity", "rgb")]
    extr = s["extr"].clone().requires_grad_(True)
    wts = torch.rand(4, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(0))

    def fn(xyz, scale, rot, op, rgb, e):
        o = MO.render_multiple([xyz, scale, rot, op, rgb, s["intr"], e, 0.2, W, H], ["rgb", "depth_map"])
        return (torch.cat([o["rgb"], o["depth_map"]]) * wts).sum()

    assert torch.autograd.gradcheck(fn, (*leaves, extr), atol=1e-6, rtol=1e-4, nondet_tol=0.0)


def test_sh_basis_is_orthonormal_on_the_sphere():
    """The only pin available for A17 (no reference call site): the 16 real harmonics are
    orthonormal, integral over the unit sphere of Y_i Y_j = delta_ij (Gauss-Legendre x uniform
    azimuth quadrature, exact for these polynomial degrees), and degree 0 is the constant
    1 / (2 sqrt(pi))."""
    nz, nphi = 16, 32
    zs, wz = np.polynomial.legendre.leggauss(nz)
    phi = (np.arange(nphi) + 0.5) * 2 * np.pi / nphi
    Z, PHI = np.meshgrid(zs, phi, indexing="ij")
    R = np.sqrt(1 - Z ** 2)
    dirs = torch.tensor(np.stack([R * np.cos(PHI), R * np.sin(PHI), Z], -1).reshape(-1, 3))
    w = torch.tensor(np.repeat(wz, nphi) * 2 * np.pi / nphi)
    B = MO.sh_basis(dirs, 16)                                    # (Q,16) float64
    gram = (B * w.unsqueeze(1)).T @ B
    np.testing.assert_allclose(gram.numpy(), np.eye(16), atol=1e-12)
    assert abs(B[0, 0].item() - 0.5 / np.sqrt(np.pi)) < 1e-15


def test_sh_degree_zero_is_constant_and_visible_masks():
    g = torch.Generator().manual_seed(1)
    shs = torch.randn(5, 4, 3, generator=g, dtype=torch.float64)
    d = torch.nn.functional.normalize(torch.randn(5, 3, generator=g, dtype=torch.float64), dim=1)
    out0 = MO.compute_sh(shs[:, :1], d)
    np.testing.assert_allclose(out0.numpy(), (MO.SH_C0 * shs[:, 0]).numpy(), rtol=1e-15)
    vis = torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool).reshape(5, 1)
    out = MO.compute_sh(shs, d, vis)
    assert torch.all(out[~vis.reshape(-1)] == 0)


# ------------------------------------------------------- general cameras: fx != fy, off-centre pp, the EWA clamp
def test_clamp_known_answers_oracle():
    """Closed-form conics on and off the clamp (tests/scenes.py: clamp_known_answers): the clamped Jacobian uses the
    LIMIT, not x / z; the frustum test is about W / 2, the clamp about cx -- a splat one pixel past 1.15 W is culled, one
    whose |u - cx| is past 0.65 W but whose u is not is visible and clamped."""
    from tests.scenes import check_known_answers, clamp_known_answers, clamp_sets
    ka = clamp_known_answers()
    W, H = ka["W"], ka["H"]
    uv, depth = MO.project_point(ka["xyz"], ka["intr"], ka["extr"], W, H)
    vis = depth != 0
    cov = MO.compute_cov3d(ka["scale"], ka["rotate"], vis)
    conic, radius, tiles = MO.ewa_project(ka["xyz"], cov, ka["intr"], ka["extr"], uv, W, H, vis)
    check_known_answers(ka, uv, depth, conic, radius)
    # the figures the clamp is about, spelled out
    e = ka["expect"]
    np.testing.assert_allclose(conic[e["on_axis"][0]].numpy(), [1 / 4.3, 0.0, 1 / 2.1225], rtol=2e-5)
    a_clamped, a_free = 4.0 * (1 + 1.04 ** 2) + 0.3, 4.0 * (1 + (1.2 * 1.04) ** 2) + 0.3
    np.testing.assert_allclose(conic[e["x_clamped"][0]].numpy(), [1 / a_clamped, 0.0, 1 / 2.1225], rtol=2e-5)
    assert a_free - a_clamped > 1.5                         # (10.53 against 8.63: far above any tolerance in use)
    # and the helper that names the clamped sets agrees with the table
    sets = clamp_sets(ka)
    names = {name: k for name, (k, *_r) in e.items()}
    assert sets["live"].tolist() == [name != "past_the_frustum_by_a_pixel" for name in names]
    assert [n for n, k in names.items() if sets["x"][k]] == ["x_clamped", "both_clamped", "clamped_by_cx_inside_frustum"]
    assert [n for n, k in names.items() if sets["y"][k]] == ["y_clamped", "both_clamped"]
    assert [n for n, k in names.items() if sets["both"][k]] == ["both_clamped"]


def test_camera_scene_keeps_random_scene_and_fills_the_regimes():
    """The general-camera builder gives random_scene's splats under random_scene's camera (to rounding: it divides by
    sqrt(f f)), and the named cameras are in the regimes their tests rely on."""
    from tests.scenes import CAMERAS, assert_regime, camera_scene
    W, H = 200, 136
    a = random_scene(400, W, H, seed=11, sigma_px=2.5)
    b = camera_scene(400, W, H, (0.6 * W, 0.6 * W, W / 2, H / 2), seed=11, sigma_px=2.5)
    for k in ("xyz", "scale", "rotate", "opacity", "rgb", "intr", "extr"):
        np.testing.assert_allclose(b[k].numpy(), a[k].numpy(), rtol=1e-6, atol=0, err_msg=k)
    for name in CAMERAS:
        s = camera_scene(3000, W, H, name, seed=11, sigma_px=2.5)
        sets = assert_regime(name, s)
        assert int(sets["live"].sum()) > 2500
        # a clamped splat is one whose u, v is further than 0.65 W, 0.65 H from the PRINCIPAL POINT
        uv, _ = MO.project_point(s["xyz"], s["intr"], s["extr"], W, H)
        far_x = (uv[:, 0] - s["intr"][2]).abs() > 0.65 * W
        assert (far_x & sets["live"] != sets["x"]).sum() <= 2              # (float32 ties at the limit)


def _general_gradcheck_scene():
    """Eight float64 splats under ``general`` at 48 x 32 with the tilted extrinsic, PLACED on the branches: x-clamped,
    y-clamped, doubly clamped and free ones, all reaching into the image so the render sees them."""
    from tests.scenes import camera_scene, clamp_sets
    W, H = 48, 32
    s = camera_scene(8, W, H, "general", seed=7, dtype=torch.float64, sigma_px=3.0, behind=0.0)
    fx, fy, cx, cy = s["intr"].tolist()
    #                      x-clamped    y-clamped     both          both         free      free      x-clamped   y-clamped
    uv = torch.tensor([[47.0, 10.0], [20.0, -1.5], [46.0, -1.0], [45.5, 0.5], [20, 15], [30, 20], [44.5, 12], [10.0, -2.0]],
                      dtype=torch.float64)
    z = torch.linspace(1.5, 3.0, 8, dtype=torch.float64)
    cam = torch.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], dim=1)
    s["xyz"] = ((cam - s["extr"][:, 3]) @ s["extr"][:, :3]).contiguous()
    sets = clamp_sets(s)
    assert sets["live"].all()
    assert int(sets["x"].sum()) == 4 and int(sets["y"].sum()) == 4 and int(sets["both"].sum()) == 2, sets
    assert int((sets["x"] & ~sets["y"]).sum()) >= 1 and int((sets["y"] & ~sets["x"]).sum()) >= 1 and int((~sets["any"]).sum()) >= 1
    # finite differences are valid: every splat at least 1e-3 from the clamp kinks (in x / z, y / z) and from the cull
    # limits (in pixels and in depth)
    pc = s["xyz"] @ s["extr"][:, :3].T + s["extr"][:, 3]
    rx, ry = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    limx, limy = MO.FOV_CLAMP * W / (2 * fx), MO.FOV_CLAMP * H / (2 * fy)
    assert ((rx.abs() - limx).abs().min() > 1e-3) and ((ry.abs() - limy).abs().min() > 1e-3)
    u, v = fx * rx + cx, fy * ry + cy
    for val, half in ((u, W / 2), (v, H / 2)):
        assert (((val - half).abs() - MO.EXTENT * half).abs().min() > 1e-3)
    assert (pc[:, 2] - MO.NEAREST).min() > 1e-3
    return s, sets


def test_gradcheck_float64_ops_general_camera():
    """project_point and ewa_project under fx != fy, an off-centre principal point and the tilted extrinsic, with splats
    on every branch of the EWA clamp: autograd against finite differences in float64."""
    s, sets = _general_gradcheck_scene()
    W, H = s["W"], s["H"]
    xyz = s["xyz"].clone().requires_grad_(True)
    extr = s["extr"].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, e: MO.project_point(a, s["intr"], e, W, H), (xyz, extr), atol=1e-7)
    vis = torch.ones(8, 1, dtype=torch.bool)
    uv, depth = MO.project_point(s["xyz"], s["intr"], s["extr"], W, H)
    assert (depth != 0).all()
    cov = MO.compute_cov3d(s["scale"], s["rotate"], vis).clone().requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, c, e: MO.ewa_project(a, c, s["intr"], e, uv, W, H, vis)[0], (xyz, cov, extr), atol=1e-6)
    # the clamp cuts the gradient where it should: d conic / d x_cam = 0 for an x-clamped splat, not for a free one
    # (identity extrinsic so that x_cam is xyz[:, 0])
    eye = torch.eye(4, dtype=torch.float64)[:3]
    cam = (s["xyz"] @ s["extr"][:, :3].T + s["extr"][:, 3]).clone().requires_grad_(True)
    con = MO.ewa_project(cam, cov.detach(), s["intr"], eye, uv, W, H, vis)[0]
    g = torch.autograd.grad(con.sum(), cam)[0]
    assert torch.all(g[sets["x"], 0] == 0) and torch.all(g[~sets["x"], 0] != 0)
    assert torch.all(g[sets["y"], 1] == 0) and torch.all(g[~sets["y"], 1] != 0)
    assert torch.all(g[:, 2] != 0)


def test_gradcheck_float64_full_render_general_camera():
    s, sets = _general_gradcheck_scene()
    W, H = s["W"], s["H"]
    leaves = [s[k].clone().requires_grad_(True) for k in ("xyz", "scale", "rotate", "opacity", "rgb")]
    extr = s["extr"].clone().requires_grad_(True)
    wts = torch.rand(4, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(0))

    def fn(xyz, scale, rot, op, rgb, e):
        o = MO.render_multiple([xyz, scale, rot, op, rgb, s["intr"], e, 0.2, W, H], ["rgb", "depth_map"])
        return (torch.cat([o["rgb"], o["depth_map"]]) * wts).sum()

    # every placed splat colours pixels: the gradient the check sees goes through the clamped conics
    g = torch.autograd.grad(fn(*leaves, extr), leaves[1])[0]
    assert torch.all(g.abs().sum(1) > 0)
    assert torch.autograd.gradcheck(fn, (*leaves, extr), atol=1e-6, rtol=1e-4, nondet_tol=0.0)
