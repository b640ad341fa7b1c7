"""Small seeded splat scenes shared by the oracle and GPU parity tests."""
import math

import numpy as np
import torch


def camera(W, H, f=None, dtype=torch.float32, tilt=False):
    f = float(f if f is not None else 0.6 * W)
    intr = torch.tensor([f, f, W / 2.0, H / 2.0], dtype=dtype)
    if tilt:
        a, b = 0.07, -0.05
        Ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=dtype)
        Rx = torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]], dtype=dtype)
        extr = torch.cat([Ry @ Rx, torch.tensor([[0.05], [-0.03], [0.1]], dtype=dtype)], dim=1)
    else:
        extr = torch.eye(4, dtype=dtype)[:3].clone()
    return intr, extr


def random_scene(N, W, H, seed=0, dtype=torch.float32, sigma_px=2.0, spread=1.15, tilt=True, behind=0.05):
    """N splats scattered over (and a little beyond) the frustum, depth 1..4,
    projected sigma about ``sigma_px`` pixels (log-normal), random rotations,
    opacities in (0.05,0.999).  A fraction ``behind`` sits behind the camera."""
    g = torch.Generator().manual_seed(seed)
    intr, extr = camera(W, H, dtype=dtype, tilt=tilt)
    f = intr[0].item()
    z = 1.0 + 3.0 * torch.rand(N, generator=g, dtype=torch.float64)
    u = (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * W * spread + W / 2
    v = (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * H * spread + H / 2
    x = (u - W / 2) / f * z
    y = (v - H / 2) / f * z
    nb = int(N * behind)
    if nb:
        z[:nb] = -z[:nb]
    xyz_cam = torch.stack([x, y, z], dim=1)
    R = extr[:, :3].double()
    t = extr[:, 3].double()
    xyz = (xyz_cam - t) @ R                       # inverse of R x + t  (R orthonormal)
    sig = sigma_px * torch.exp(0.5 * torch.randn(N, generator=g, dtype=torch.float64))
    aniso = torch.exp(0.4 * torch.randn(N, 3, generator=g, dtype=torch.float64))
    scale = (sig / f * z.abs()).unsqueeze(1) * aniso
    rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g, dtype=torch.float64), dim=1)
    opacity = 0.05 + 0.949 * torch.rand(N, 1, generator=g, dtype=torch.float64)
    rgb = torch.rand(N, 3, generator=g, dtype=torch.float64)
    cast = lambda a: a.to(dtype).contiguous()
    return dict(xyz=cast(xyz), scale=cast(scale), rotate=cast(rot), opacity=cast(opacity), rgb=cast(rgb),
                intr=intr, extr=extr, W=W, H=H)


def scene_group(s, bg=0.0):
    return [s["xyz"], s["scale"], s["rotate"], s["opacity"], s["rgb"], s["intr"], s["extr"], bg, s["W"], s["H"]]


# ------------------------------------------------------------------ general cameras
# name -> (fx / W, fy / W, cx / W, cy / H): the ratios of the 200 x 136 set, for any size
_CAMERA_RATIOS = {
    "aniso": (0.62, 0.43, 0.5, 0.5),              # fx != fy, centred
    "offcentre": (0.6, 0.6, 0.25, 0.7),           # fx == fy, principal point off the centre: the EWA clamp is live
    "general": (0.62, 0.43, 0.25, 0.7),           # both
    "fov90": (0.5, None, 0.5, 0.5),               # fy = H / 2: SimpleGaussian's default, 90 degrees per axis
}
CAMERAS = tuple(_CAMERA_RATIOS)
CLAMPING = ("offcentre", "general")               # the cameras under which visible splats take the EWA clamp


def named_intr(name, W, H):
    rx, ry, rcx, rcy = _CAMERA_RATIOS[name]
    return (rx * W, ry * W if ry is not None else H / 2.0, rcx * W, rcy * H)


def camera_scene(N, W, H, intr, extr=None, seed=0, dtype=torch.float32, sigma_px=2.0, spread=1.15, tilt=True, behind=0.05):
    """``random_scene`` under any pinhole camera: ``intr`` is (fx, fy, cx, cy) or a name of ``CAMERAS``.  u, v uniform
    over ``spread`` x the image around its CENTRE (not the principal point), back-projected with the given intrinsics;
    projected sigma about ``sigma_px`` pixels of the focal sqrt(fx fy).  ``extr`` (3,4) overrides the tilted / identity one."""
    g = torch.Generator().manual_seed(seed)
    name = intr if isinstance(intr, str) else None
    fx, fy, cx, cy = (float(a) for a in (named_intr(intr, W, H) if name else intr))
    intr_t = torch.tensor([fx, fy, cx, cy], dtype=dtype)
    extr = camera(W, H, dtype=dtype, tilt=tilt)[1] if extr is None else extr.to(dtype).clone()
    z = 1.0 + 3.0 * torch.rand(N, generator=g, dtype=torch.float64)
    u = (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * W * spread + W / 2
    v = (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * H * spread + H / 2
    x = (u - cx) / fx * z
    y = (v - cy) / fy * z
    nb = int(N * behind)
    if nb:
        z[:nb] = -z[:nb]
    xyz_cam = torch.stack([x, y, z], dim=1)
    R = extr[:, :3].double()
    t = extr[:, 3].double()
    xyz = (xyz_cam - t) @ R
    f = math.sqrt(fx * fy)
    sig = sigma_px * torch.exp(0.5 * torch.randn(N, generator=g, dtype=torch.float64))
    aniso = torch.exp(0.4 * torch.randn(N, 3, generator=g, dtype=torch.float64))
    scale = (sig / f * z.abs()).unsqueeze(1) * aniso
    rot = torch.nn.functional.normalize(torch.randn(N, 4, generator=g, dtype=torch.float64), dim=1)
    opacity = 0.05 + 0.949 * torch.rand(N, 1, generator=g, dtype=torch.float64)
    rgb = torch.rand(N, 3, generator=g, dtype=torch.float64)
    cast = lambda a: a.to(dtype).contiguous()
    return dict(xyz=cast(xyz), scale=cast(scale), rotate=cast(rot), opacity=cast(opacity), rgb=cast(rgb),
                intr=intr_t, extr=extr, W=W, H=H, camera=name)


def take_rows(s, rows):
    """The scene with only the splats ``rows`` (a boolean mask or an index)."""
    return {k: (v[rows].contiguous() if k in ("xyz", "scale", "rotate", "opacity", "rgb") else v) for k, v in s.items()}


def clamp_sets(s, extr=None):
    """From the oracle, which splats are LIVE (inside the frustum, a footprint of at least one tile) and have their
    x / z, y / z clamped in the EWA Jacobian: boolean (N,) masks ``x``, ``y``, ``both`` (the intersection) and ``any``
    (the union), plus ``live``.  The xyz, scale and rotate of ``s`` are taken as activated values."""
    from oracle import msplat_oracle as MO
    extr = s["extr"] if extr is None else extr
    W, H, intr = s["W"], s["H"], s["intr"]
    xyz = s["xyz"].detach()
    uv, depth = MO.project_point(xyz, intr, extr, W, H)
    vis = depth != 0
    cov = MO.compute_cov3d(s["scale"].detach(), s["rotate"].detach(), vis)
    radius = MO.ewa_project(xyz, cov, intr, extr, uv, W, H, vis)[1]
    live = (radius > 0).reshape(-1)
    pc = xyz @ extr[:, :3].T + extr[:, 3]
    z = torch.where(live, pc[:, 2], torch.ones_like(pc[:, 2]))
    cx = live & ((pc[:, 0] / z).abs() > MO.FOV_CLAMP * W / (2.0 * intr[0]))
    cy = live & ((pc[:, 1] / z).abs() > MO.FOV_CLAMP * H / (2.0 * intr[1]))
    return dict(live=live, x=cx, y=cy, both=cx & cy, any=cx | cy)


def assert_regime(name, s, sets=None):
    """A scene under the camera ``name`` is what its tests are about (checked on the CPU): enough live splats on every
    clamp branch under the off-centre cameras and none under the centred ones, fx and fy at least 20 % apart under the
    anisotropic ones.  Returns the clamp sets."""
    sets = clamp_sets(s) if sets is None else sets
    nx, ny, nb = (int(sets[k].sum()) for k in ("x", "y", "both"))
    if name in CLAMPING:
        assert nx >= 100 and ny >= 100 and nb >= 10, f"{name}: {nx} x-clamped, {ny} y-clamped, {nb} doubly clamped live splats"
    else:
        assert nx == 0 and ny == 0, f"{name}: {nx} x-clamped, {ny} y-clamped live splats under a centred camera"
    fx, fy = float(s["intr"][0]), float(s["intr"][1])
    if name in ("aniso", "general", "fov90"):
        assert abs(fx - fy) >= 0.2 * min(fx, fy), f"{name}: fx {fx} and fy {fy} are less than 20 % apart"
    return sets


def clamp_known_answers():
    """Closed-form answers for an isotropic splat (scale s, unit quaternion) under W, H = 64, 48, intr = (40, 27, 16, 34)
    and the identity extrinsic -- worked out here with python floats, independent of autograd and of any operator:
    Sigma = s^2 I, so Sigma2 = s^2 J J^T + 0.3 I with J = [[fx/z, 0, -fx tx/z^2], [0, fy/z, -fy ty/z^2]] and
    tx / z, ty / z the CLAMPED x / z, y / z.  Returns the inputs and, per splat, (visible, uv, conic or None)."""
    W, H = 64, 48
    fx, fy, cx, cy = 40.0, 27.0, 16.0, 34.0
    s, z = 0.1, 2.0
    limx, limy = 1.3 * W / (2 * fx), 1.3 * H / (2 * fy)
    hi_u = 0.5 * W * (1 + 1.3)

    def conic(rx, ry):                                  # rx, ry: x / z, y / z after the clamp
        a = (fx * s / z) ** 2 * (1 + rx * rx) + 0.3
        c = (fy * s / z) ** 2 * (1 + ry * ry) + 0.3
        b = (fx * s / z) * (fy * s / z) * rx * ry
        det = a * c - b * b
        return (c / det, -b / det, a / det)

    cases = {                                           # name: (x / z, y / z, what the Jacobian sees)
        "on_axis": (0.0, 0.0, (0.0, 0.0)),
        "x_clamped": (1.2 * limx, 0.0, (limx, 0.0)),                      # u = 65.92 <= 1.15 W = 73.6: visible
        "y_clamped": (0.0, -1.2 * limy, (0.0, -limy)),                    # v = -3.44 >= -0.15 H = -7.2: visible
        "both_clamped": (1.1 * limx, -1.1 * limy, (limx, -limy)),
        "unclamped_off_axis": (0.9 * limx, -0.9 * limy, (0.9 * limx, -0.9 * limy)),
        "clamped_by_cx_inside_frustum": ((70.0 - cx) / fx, 0.1, (limx, 0.1)),     # u = 70: |u - cx| = 54 > 41.6, u <= 73.6
        "past_the_frustum_by_a_pixel": ((hi_u + 1.0 - cx) / fx, 0.0, None),        # u = 74.6 > 73.6: culled
    }
    xyz, expect = [], {}
    for k, (name, (rx, ry, seen)) in enumerate(cases.items()):
        xyz.append([rx * z, ry * z, z])
        expect[name] = (k, seen is not None, (fx * rx + cx, fy * ry + cy), conic(*seen) if seen is not None else None)
    n = len(xyz)
    return dict(W=W, H=H, intr=torch.tensor([fx, fy, cx, cy]), extr=torch.eye(4)[:3].clone(), xyz=torch.tensor(xyz),
                scale=torch.full((n, 3), s), rotate=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1), expect=expect,
                limx=limx, limy=limy)


def check_known_answers(ka, uv, depth, conic, radius):
    """``uv, depth, conic, radius`` of the splats of ``clamp_known_answers`` from any implementation."""
    uv, depth, conic, radius = (torch.as_tensor(a).detach().double().cpu() for a in (uv, depth, conic, radius))
    for name, (k, visible, uv_ref, conic_ref) in ka["expect"].items():
        if not visible:
            assert depth[k, 0] == 0 and torch.all(uv[k] == 0) and radius[k, 0] == 0 and torch.all(conic[k] == 0), name
            continue
        assert depth[k, 0] == 2.0 and radius[k, 0] > 0, name
        np.testing.assert_allclose(uv[k].numpy(), uv_ref, rtol=1e-6, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(conic[k].numpy(), conic_ref, rtol=2e-5, atol=1e-7, err_msg=name)
