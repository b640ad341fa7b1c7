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


# ------------------------------------------------------------------ opacity regimes
# Raw (pre-activation) rows, the activations being trainer.py:64-69: |scale|, normalised quaternion, sigmoid(10 opacity),
# sigmoid(rgb).  Three regimes of the activated opacity o that the blend treats on branches of their own:
#   capped     o G > ALPHA_MAX at some pixel: alpha = 0.99 there, the gradient passes straight through
#   threshold  1/255 <= o < 1.05/255: no exact-disc culling in the fused path, one to three pixels see the splat at all
#   invisible  o < 1/255: in no list
GROUPS = ("rest", "capped", "threshold", "invisible")
ATTRS = ("xyz", "scale", "rotate", "opacity", "rgb")
FRAGILE_MARGIN = 1e-4         # |255 o G - 1| below this: the pair's alpha test hangs on the last bits of exp()
FRAGILE_SHARE = 0.03          # of a regime's rows may be fragile, no more


def raw_rows(s, seed=0):
    """Raw parameters whose activations reproduce the scene ``s`` (seeded: the signs of the raw scales)."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(s["scale"].shape, generator=g) > 0.3, 1.0, -1.0).to(s["scale"].dtype)
    return dict(xyz=s["xyz"].clone(), scale=s["scale"] * sign, rotate=s["rotate"] * 1.7,
                opacity=torch.logit(s["opacity"].clamp(0.02, 0.98)) / 10.0, rgb=torch.logit(s["rgb"].clamp(0.02, 0.98)))


def opacity_regime_scene(N, W, H, seed, n_capped=600, n_threshold=300, n_invisible=300, sigma_px=2.5):
    """``random_scene(tilt=False)`` as raw rows, with disjoint random subsets of the rows re-drawn into the three opacity
    regimes: raw opacity uniform in [0.55, 2.0] (o >= 0.9959, part of it exactly 1.0f), o uniform in [1/255, 1.05/255)
    with raw = logit(o) / 10 worked out in float64, raw opacity uniform in [-1.5, -0.6] (o < 1/255).  The rest keeps
    logit(o.clamp(0.02, 0.98)) / 10.  Returns the scene's camera and size, ``raw`` and ``group`` (index into GROUPS)."""
    s = random_scene(N, W, H, seed=seed, sigma_px=sigma_px, tilt=False)
    raw = raw_rows(s, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    perm = torch.randperm(N, generator=g)
    group = torch.zeros(N, dtype=torch.int64)
    a, b, c = n_capped, n_capped + n_threshold, n_capped + n_threshold + n_invisible
    assert c <= N
    group[perm[:a]], group[perm[a:b]], group[perm[b:c]] = 1, 2, 3
    op = raw["opacity"].double().clone()
    rnd = torch.rand(N, 1, generator=g, dtype=torch.float64)
    o_thr = (1.0 + 0.05 * rnd) / 255.0
    op = torch.where((group == 1).unsqueeze(1), 0.55 + 1.45 * rnd, op)
    op = torch.where((group == 2).unsqueeze(1), torch.log(o_thr / (1.0 - o_thr)) / 10.0, op)
    op = torch.where((group == 3).unsqueeze(1), -1.5 + 0.9 * rnd, op)
    raw["opacity"] = op.float()
    return dict(raw=raw, group=group, intr=s["intr"], extr=s["extr"], W=W, H=H)


def capped_pile_scene(W=48, H=48, seed=0, n_pile=700, n_rest=300, tile=(1, 1), extr=None, sigma=(20.0, 60.0)):
    """``n_pile`` capped splats (raw opacity in [0.55, 2.0]) with distinct depths and centres inside ONE 16 x 16 tile,
    ``sigma`` pixels wide, on top of ``n_rest`` ordinary rows: every pixel of that tile has alpha between ~0.9 and the cap
    from the nearest layers on and stops after two to four of them, with hundreds of entries of its list behind the stop.
    The two nearest splats of the pile sit in opposite corners of the tile so that no pixel has both of its first two
    layers AT the cap: (1 - 0.99)^2 against T_MIN = 1e-4 is decided by the rounding of 0.99 in the number format (float32
    stops, float64 does not), and that is not what the scene is for.  The pile's rows come first; ``extr`` (3, 4) is the
    camera the pile is placed for (the identity if None)."""
    s = random_scene(n_rest, W, H, seed=seed, sigma_px=2.5, tilt=False, behind=0.0)
    rest = raw_rows(s, seed)
    g = torch.Generator().manual_seed(seed + 2000)
    f = float(s["intr"][0])
    z = 1.0 + 2.0 * (torch.randperm(n_pile, generator=g).double() + 0.5) / n_pile          # distinct, 1 .. 3
    x0, y0 = 16.0 * tile[0], 16.0 * tile[1]
    u = x0 + 0.5 + 14.0 * torch.rand(n_pile, generator=g, dtype=torch.float64)
    v = y0 + 0.5 + 14.0 * torch.rand(n_pile, generator=g, dtype=torch.float64)
    near = torch.argsort(z)[:2]
    u[near[0]], v[near[0]], u[near[1]], v[near[1]] = x0 + 1.0, y0 + 1.0, x0 + 14.0, y0 + 14.0
    sig = sigma[0] * torch.exp(math.log(sigma[1] / sigma[0]) * torch.rand(n_pile, generator=g, dtype=torch.float64))
    scale = (sig / f * z).unsqueeze(1) * torch.exp(0.1 * torch.randn(n_pile, 3, generator=g, dtype=torch.float64))
    sign = torch.where(torch.rand(n_pile, 3, generator=g) > 0.3, 1.0, -1.0).double()
    rot = 1.7 * torch.nn.functional.normalize(torch.randn(n_pile, 4, generator=g, dtype=torch.float64), dim=1)
    xyz = torch.stack([(u - W / 2) / f * z, (v - H / 2) / f * z, z], dim=1)
    if extr is not None:
        xyz = (xyz - extr[:, 3].double()) @ extr[:, :3].double()           # inverse of R x + t
    # the 24 nearest layers -- the only ones a pixel ever reaches -- keep out of raw opacities between 0.75 and 1.75: there 1 - o
    # is a few float32 ulps of o, the chain rule's 10 o (1 - o) of a float32 reference is good to a percent only, and over a
    # dozen contributing rows that does not average out (the regime scene has hundreds of rows in that band)
    op = 0.55 + 1.45 * torch.rand(n_pile, 1, generator=g, dtype=torch.float64)
    r = torch.rand(24, 1, generator=g, dtype=torch.float64)
    op[torch.argsort(z)[:24]] = torch.where(r < 0.5, 0.55 + 0.4 * r, 1.5 + 0.5 * r)
    pile = dict(xyz=xyz, scale=scale * sign, rotate=rot, opacity=op,
                rgb=torch.logit(0.02 + 0.96 * torch.rand(n_pile, 3, generator=g, dtype=torch.float64)))
    raw = {k: torch.cat([pile[k].float(), rest[k]]).contiguous() for k in ATTRS}
    group = torch.cat([torch.ones(n_pile, dtype=torch.int64), torch.zeros(n_rest, dtype=torch.int64)])
    return dict(raw=raw, group=group, intr=s["intr"], extr=s["extr"], W=W, H=H, pile_tile=tile[1] * ((W + 15) // 16) + tile[0],
                n_pile=n_pile)


def oracle_front_end(scene, pose, dtype):
    """Activations, projection, EWA and the sorted lists of the oracle for the raw rows of ``scene`` under ``pose``."""
    from oracle import fit_oracle as FO
    from oracle import loss_oracle as LO
    from oracle import msplat_oracle as MO
    W, H = scene["W"], scene["H"]
    xyz, scale, rot, op, rgb = FO.activate({k: v.detach().to(dtype) for k, v in scene["raw"].items()})
    intr, extr = scene["intr"].to(dtype), LO.pose_to_extr(pose.detach().to(dtype))
    uv, depth = MO.project_point(xyz, intr, extr, W, H)
    vis = depth != 0
    conic, radius, tiles = MO.ewa_project(xyz, MO.compute_cov3d(scale, rot, vis), intr, extr, uv, W, H, vis)
    ids, tr = MO.sort_gaussian(uv, depth, W, H, radius, tiles)
    return dict(uv=uv, depth=depth, conic=conic, radius=radius, tiles=tiles, ids=ids, tile_range=tr, opacity=op, rgb=rgb,
                act=(xyz, scale, rot, op, rgb), extr=extr, intr=intr)


def _pair_walk(fe, W, H, max_elems=3_000_000):
    """The (pixel, splat) pairs of ``MO.alpha_blending`` with the oracle's own decisions, tile batch by tile batch:
    yields g (nt, L) splat ids and, shaped (nt, 256, L): live (a list entry seen from a pixel inside the image),
    power, o G, use (passes the alpha test), contrib (use, before the stop) and incl (transmittance behind the pair)."""
    from oracle import msplat_oracle as MO
    uv, conic, op, ids_all = fe["uv"], fe["conic"], fe["opacity"], fe["ids"].to(torch.int64)
    dt = uv.dtype
    gx, gy = MO.tile_grid(W, H)
    tr = fe["tile_range"].to(torch.int64)
    lens = tr[:, 1] - tr[:, 0]
    order = torch.argsort(lens, descending=True)
    order = order[lens[order] > 0]
    px_off = torch.arange(MO.TILE, dtype=dt) + MO.PIXEL_CENTER
    pos = 0
    while pos < order.numel():
        L = int(lens[order[pos]])
        nt = max(1, min(order.numel() - pos, max_elems // (MO.TILE * MO.TILE * L)))
        tids = order[pos:pos + nt]
        pos += nt
        ar = torch.arange(L)
        valid = ar.unsqueeze(0) < lens[tids].unsqueeze(1)
        idx = torch.where(valid, tr[tids, 0].unsqueeze(1) + ar.unsqueeze(0), torch.zeros(1, dtype=torch.int64))
        g = ids_all[idx]
        pxx = (tids % gx).to(dt).unsqueeze(1) * MO.TILE + px_off.unsqueeze(0)
        pyy = (tids // gx).to(dt).unsqueeze(1) * MO.TILE + px_off.unsqueeze(0)
        PX = pxx.unsqueeze(1).expand(nt, MO.TILE, MO.TILE).reshape(nt, -1, 1)
        PY = pyy.unsqueeze(2).expand(nt, MO.TILE, MO.TILE).reshape(nt, -1, 1)
        inside = (PX < W) & (PY < H)
        gu, gc = uv[g], conic[g]
        dx = gu[:, :, 0].unsqueeze(1) - PX
        dy = gu[:, :, 1].unsqueeze(1) - PY
        power = -0.5 * (gc[:, :, 0].unsqueeze(1) * dx * dx + gc[:, :, 2].unsqueeze(1) * dy * dy) - gc[:, :, 1].unsqueeze(1) * dx * dy
        araw = op[g].reshape(nt, 1, L) * torch.exp(power)
        alpha = torch.clamp(araw, max=MO.ALPHA_MAX)
        live = valid.unsqueeze(1) & inside
        use = live & (power <= 0) & (alpha >= MO.ALPHA_MIN)
        incl = torch.cumprod(torch.where(use, 1.0 - alpha, torch.ones_like(alpha)), dim=2)
        contrib = use & (incl >= MO.T_MIN)
        yield g, live, power, araw, use, contrib, incl


def opacity_sets(scene, pose, margin=FRAGILE_MARGIN):
    """From the FLOAT64 oracle, boolean masks over the rows of ``scene`` under ``pose``:
      capped     at least one contributing (pixel, splat) pair with o G > ALPHA_MAX
      threshold  1/255 <= o and 255 o < 1.05 (the fused path's no-culling branch), contributing at one pixel or more
      invisible  o < 1/255
      saturated  the float32 activation gives o == 1
      fragile    a pair with power <= 0 and |255 o G - 1| < ``margin``: a last-bit difference between two exp()
                 implementations switches the row's contribution at that pixel on or off
    plus ``contributing`` (any pair that reaches the image), ``n_capped_pairs``, ``n_stop_edge`` (pairs whose transmittance
    lands within 1e-5 of T_MIN, relative: the stop rule there is decided by rounding) and ``o`` (float64)."""
    from oracle import msplat_oracle as MO
    fe = oracle_front_end(scene, pose, torch.float64)
    N = scene["raw"]["xyz"].shape[0]
    W, H = scene["W"], scene["H"]
    o = fe["opacity"].reshape(-1)
    count = {k: torch.zeros(N, dtype=torch.int64) for k in ("capped", "contrib", "fragile")}
    n_stop_edge = 0
    for g, live, power, araw, use, contrib, incl in _pair_walk(fe, W, H):
        flat = g.reshape(-1)
        count["capped"].index_add_(0, flat, (contrib & (araw > MO.ALPHA_MAX)).sum(dim=1).reshape(-1))
        count["contrib"].index_add_(0, flat, contrib.sum(dim=1).reshape(-1))
        count["fragile"].index_add_(0, flat, (live & (power <= 0) & ((255.0 * araw - 1.0).abs() < margin)).sum(dim=1).reshape(-1))
        excl = torch.cat([torch.ones_like(incl[:, :, :1]), incl[:, :, :-1]], dim=2)
        n_stop_edge += int((use & (excl >= MO.T_MIN) & ((incl / MO.T_MIN - 1.0).abs() < 1e-5)).sum())
    o32 = torch.sigmoid(10.0 * scene["raw"]["opacity"].float()).reshape(-1)
    return dict(capped=count["capped"] > 0, threshold=(o >= MO.ALPHA_MIN) & (255.0 * o < 1.05) & (count["contrib"] > 0),
                invisible=o < MO.ALPHA_MIN, saturated=o32 == 1.0, fragile=count["fragile"] > 0, contributing=count["contrib"] > 0,
                n_capped_pairs=int(count["capped"].sum()), n_stop_edge=n_stop_edge, o=o)


def regime_rows(sets, name):
    """The rows a per-regime comparison runs over: the regime's, minus the fragile ones."""
    return sets[name] & ~sets["fragile"]


def assert_opacity_regime(sets, ref_grads=None, min_rows=None):
    """The scene is what its tests are about (checked on the CPU).  ``ref_grads``: the reference gradients by attribute --
    with them, the threshold rows counted are those with a non-zero gradient.  ``min_rows`` overrides the counts."""
    need = dict(capped=100, threshold=100, invisible=100, saturated=50, capped_pairs=200)
    need.update(min_rows or {})
    thr = sets["threshold"]
    if ref_grads is not None:
        nz = torch.zeros_like(thr)
        for k in ATTRS:
            nz |= (ref_grads[k].detach().reshape(thr.shape[0], -1) != 0).any(dim=1)
        thr = thr & nz
    n = dict(capped=int(sets["capped"].sum()), threshold=int(thr.sum()), invisible=int(sets["invisible"].sum()),
             saturated=int(sets["saturated"].sum()), capped_pairs=sets["n_capped_pairs"])
    for k, v in need.items():
        assert n[k] >= v, f"{k}: {n[k]} (at least {v} wanted)  {n}"
    for k in ("capped", "threshold"):
        if int(sets[k].sum()):
            share = int((sets[k] & sets["fragile"]).sum()) / int(sets[k].sum())
            assert share <= FRAGILE_SHARE, f"{k}: {share:.3f} of the rows are fragile (at most {FRAGILE_SHARE})"
    assert sets["n_stop_edge"] == 0, f"{sets['n_stop_edge']} pairs sit on the stop rule's boundary"
    # a threshold / invisible row must be on its branch in float32 as well: o not within 1e-5 (relative) of a branch point
    o = sets["o"]
    for edge in (1.0 / 255.0, 1.05 / 255.0):
        assert not bool(((o / edge - 1.0).abs() < 1e-5).any()), f"a row's opacity sits on the branch point {edge:.6f}"
    return n


REGIME_LAMBDAS = dict(lambda_rgb=1.0, lambda_depth=0.1, lambda_var=0.0)     # (with lambda_var = 10 the variance term is most of d_scale)


def reference_fit(scene, pose, img, dep, dtype=torch.float32, lam=REGIME_LAMBDAS, bg=0.0, ab=None):
    """One forward + backward of the oracle's fit iteration on the raw rows of ``scene``: the render (4, H, W), the
    gradients by attribute (N, width), those of the pose and of the depth affine, the loss terms and the pair count.
    ``ab``: the depth affine (2,) the iteration starts from ((1, 0) if None: a fresh engine's)."""
    from oracle import fit_oracle as FO
    rc = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in scene["raw"].items()}
    p = pose.detach().to(dtype).clone().requires_grad_(True)
    ab = torch.tensor([1.0, 0.0], dtype=dtype) if ab is None else ab.detach().to(dtype).clone()
    ab.requires_grad_(True)
    frame = dict(image=img.to(dtype), depth=dep.to(dtype))
    loss, info = FO.fit_loss(rc, p, ab, scene["intr"].to(dtype), frame, bg, lam["lambda_rgb"], lam["lambda_depth"], lam["lambda_var"])
    loss.backward()
    n = rc["xyz"].shape[0]
    grads = {k: (rc[k].grad if rc[k].grad is not None else torch.zeros_like(rc[k])).reshape(n, -1) for k in ATTRS}
    return dict(render=info["render4"].detach(), grads=grads, d_pose=p.grad, d_ab=ab.grad, l_rgb=info["l_rgb"].item(),
                l_depth=info["l_depth"].item(), K=info["K"])


def regime_error(got, ref, rows):
    """(relative L2, share of entries off rtol 5e-3 / atol 5e-4 max|ref|) of ``got`` against ``ref`` over ``rows`` only --
    the norm and the atol are the ROWS' own.  A reference that is zero over the rows gives (0 or inf, share)."""
    a, b = got.detach().double().cpu()[rows], ref.detach().double().cpu()[rows]
    err = (a - b).abs()
    den = b.norm().item()
    rel = (a - b).norm().item() / den if den > 0 else (0.0 if float(err.max()) == 0 else float("inf"))
    bad = (err > 5e-4 * b.abs().max().item() + 5e-3 * b.abs()).double().mean().item()
    return rel, bad


# ------------------------------------------------------------------ a running engine: rows that change their pair-row layout
# The fused backward keeps a pair's gradient row at (splat, index of the tile in the splat's tile rectangle): 32 rows of its
# own for a splat of up to SLOT_MAX = 32 tiles, a run out of a pool for a wider one; rows are never cleared, a stamp says
# which forward wrote them.  LAYOUT: 0 = at most 16 tiles, 1 = 17 .. 32, 2 = more than 32 (the pool).
CLASS_RADII = (3, 7, 12, 20, 24, 28, 31, 33, 36, 40, 44, 48, 56, 70)
CLASS_PER_RADIUS = 12
N_CULLED = 6                  # the last class rows: behind the camera on odd steps of ``apply_transition``


def layout_class(tiles):
    """0 / 1 / 2 for a tile count of at most 16 / 17 .. 32 / more than 32 (-1 for a row in no tile)."""
    t = tiles.reshape(-1).long()
    return torch.where(t <= 0, -1, torch.where(t <= 16, 0, torch.where(t <= 32, 1, 2)))


def transition_scene(W=168, H=120, seed=14, extr=None, n_base=1500):
    """``CLASS_PER_RADIUS`` "class" rows per pixel radius of ``CLASS_RADII`` in front of (as rows: before) ``n_base`` ordinary
    rows (random_scene seed 31, as raw rows).  A class row of wanted radius r has sigma = sqrt(((r - 0.5) / 3)^2 - 0.3) pixels
    on its longest axis (the EWA radius is ceil(3 sqrt(lambda_max + 0.3))) and 0.8, 0.6 of that on the others under a random
    rotation; centres uniform over the WHOLE image, so the tile rectangles are cut by all four borders and by the partial
    right column / bottom row; depth 1 .. 4; opacity 0.05 .. 0.30: nothing saturates and the exact-disc test prunes the
    corners of the rectangles.  ``extr`` (3, 4): the camera the class rows are placed for (the identity if None).
    Returns the camera, ``raw`` and ``rows`` (the class rows' indices)."""
    s = random_scene(n_base, W, H, seed=31, sigma_px=2.5, tilt=False)
    base = raw_rows(s)
    g = torch.Generator().manual_seed(seed)
    f = float(s["intr"][0])
    n = CLASS_PER_RADIUS * len(CLASS_RADII)
    r = torch.tensor(CLASS_RADII, dtype=torch.float64).repeat_interleave(CLASS_PER_RADIUS)
    r = r[torch.randperm(n, generator=g)]                                  # (the culled rows: the last six, of any radius)
    sig = torch.sqrt(((r - 0.5) / 3.0) ** 2 - 0.3)
    z = 1.0 + 3.0 * torch.rand(n, generator=g, dtype=torch.float64)
    u = W * torch.rand(n, generator=g, dtype=torch.float64)
    v = H * torch.rand(n, generator=g, dtype=torch.float64)
    xyz = torch.stack([(u - W / 2) / f * z, (v - H / 2) / f * z, z], dim=1)
    if extr is not None:
        xyz = (xyz - extr[:, 3].double()) @ extr[:, :3].double()           # inverse of R x + t
    scale = (sig / f * z).unsqueeze(1) * torch.tensor([1.0, 0.8, 0.6], dtype=torch.float64)
    sign = torch.where(torch.rand(n, 3, generator=g) > 0.3, 1.0, -1.0).double()
    rot = 1.7 * torch.nn.functional.normalize(torch.randn(n, 4, generator=g, dtype=torch.float64), dim=1)
    o = 0.05 + 0.25 * torch.rand(n, 1, generator=g, dtype=torch.float64)
    cls = dict(xyz=xyz, scale=scale * sign, rotate=rot, opacity=torch.logit(o) / 10.0,
               rgb=torch.logit(0.02 + 0.96 * torch.rand(n, 3, generator=g, dtype=torch.float64)))
    raw = {k: torch.cat([cls[k].float(), base[k]]).contiguous() for k in ATTRS}
    return dict(raw=raw, rows=torch.arange(n), intr=s["intr"], extr=s["extr"], W=W, H=H)


def apply_transition(raw, rows, step, f):
    """Edits the class rows ``rows`` of ``raw`` (a dict of (N, k) tensors or of live views of an engine's rows, on any
    device) IN PLACE.  Odd ``step``: raw scale x 1.25 on the even class rows and / 1.25 on the odd ones, every class row
    9 pixels to the right (x += 9 / f |z|), and the last ``N_CULLED`` class rows behind the camera (z -> -z).  Even ``step``
    (> 0): the inverse.  ``f``: the scene's focal length in pixels (``intr[0]``)."""
    if step <= 0:
        return
    f = float(f)
    rows = rows.to(raw["xyz"].device)
    odd = step % 2 == 1
    even_rows, odd_rows = rows[0::2], rows[1::2]
    k = 1.25 if odd else 1.0 / 1.25
    raw["scale"][even_rows] = raw["scale"][even_rows] * k
    raw["scale"][odd_rows] = raw["scale"][odd_rows] / k
    culled = rows[-N_CULLED:]
    if not odd:
        raw["xyz"][culled, 2] = -raw["xyz"][culled, 2]
    raw["xyz"][rows, 0] = raw["xyz"][rows, 0] + (9.0 if odd else -9.0) / f * raw["xyz"][rows, 2].abs()
    if odd:
        raw["xyz"][culled, 2] = -raw["xyz"][culled, 2]


def rect_facts(fe, W, H):
    """Of the oracle front end ``fe``: per row, the tile count and whether its UNCLIPPED tile rectangle crosses the left,
    right, top, bottom border of the tile grid (boolean (N,) each; rows in no tile: False)."""
    from oracle import msplat_oracle as MO
    gx, gy = MO.tile_grid(W, H)
    r = fe["radius"].reshape(-1).to(fe["uv"].dtype)
    u, v = fe["uv"][:, 0], fe["uv"][:, 1]
    live = fe["tiles"].reshape(-1) > 0
    return dict(tiles=fe["tiles"].reshape(-1).long(), left=live & (u - r < 0), top=live & (v - r < 0),
                right=live & (torch.trunc((u + r + 15) / 16) > gx), bottom=live & (torch.trunc((v + r + 15) / 16) > gy))


def pile_toggle_rows(sc, n=40):
    """The ``n`` nearest rows of the capped pile (smallest raw z among the pile's rows)."""
    return torch.argsort(sc["raw"]["xyz"][:sc["n_pile"], 2])[:n]


def pile_phase(sc, phase, rows=None):
    """The capped pile with its ``pile_toggle_rows`` invisible (phase "A": raw opacity -1.0, o = 4.5e-5 < 1/255) or as
    committed (phase "B").  A copy; ``sc`` is left as it is."""
    rows = pile_toggle_rows(sc) if rows is None else rows
    out = dict(sc)
    out["raw"] = {k: v.clone() for k, v in sc["raw"].items()}
    if phase == "A":
        out["raw"]["opacity"][rows] = -1.0
    return out


# ------------------------------------------------------------------ known answers at the cap and at the threshold
def _f32(x):
    import struct
    return struct.unpack("f", struct.pack("f", x))[0]


def opacity_known_answers(fmt="float64"):
    """Closed-form pixels of isotropic splats (conic [A, 0, A], A = 0.05) centred on pixel (8, 8) of a 16 x 16 image over
    background 0.25, in python floats, without autograd or operators.  ``fmt`` = "float32": the one place where the format
    decides the ANSWER is honoured -- two layers exactly at the cap leave T (1 - alpha) = (1 - 0.99)^2, which is >= T_MIN =
    1e-4 with 0.99 and 1e-4 rounded to float64 and < T_MIN with both rounded to float32 (0.0099999905^2 = 9.99998e-5 against
    9.9999997e-5): the second layer contributes in float64 arithmetic and is stopped in float32 arithmetic.  One pixel
    further out nothing is at the cap and both formats agree.  Returns a list of cases: name, opacities, features (one
    channel), depths, {(x, y): value} and, where it applies, d value / d o of the first splat at the centre pixel."""
    A, bg, c = 0.05, 0.25, (8, 8)
    r = (lambda x: _f32(x)) if fmt == "float32" else (lambda x: x)
    cap, amin, tmin = r(0.99), r(1.0 / 255.0), r(1e-4)

    def pixel(ops, feats, x, y):
        G = math.exp(-0.5 * A * ((c[0] - x) ** 2 + (c[1] - y) ** 2))
        T, acc = 1.0, 0.0
        for o, f in zip(ops, feats):
            a = min(cap, o * G)
            if a < amin:
                continue
            if r(T * r(1.0 - a)) < tmin:
                break
            acc += f * a * T
            T = r(T * r(1.0 - a))
        return acc + T * bg

    cases = []
    f = (0.8, 0.3, 0.6)
    G1 = math.exp(-0.5 * A)
    # one splat, o = 1: the centre pixel is 0.99 f + 0.01 bg, its neighbour G f + (1 - G) bg; d pixel / d o = G (f - bg) with
    # G = 1 at the centre: NOT cut by the cap
    cases.append(dict(name="one_capped", o=[1.0], f=f[:1], px={c: 0.99 * f[0] + 0.01 * bg, (9, 8): G1 * f[0] + (1 - G1) * bg},
                      d_o=1.0 * (f[0] - bg)))
    # two: at the centre the second adds 0.99 * 0.01 f2 (float64) or is stopped (float32); at the neighbour both formats blend two
    two_c = 0.99 * f[0] + 0.99 * 0.01 * f[1] + 0.01 * 0.01 * bg if fmt != "float32" else 0.99 * f[0] + 0.01 * bg
    two_n = G1 * f[0] + G1 * (1 - G1) * f[1] + (1 - G1) ** 2 * bg
    cases.append(dict(name="two_capped", o=[1.0, 1.0], f=f[:2], px={c: two_c, (9, 8): two_n}))
    # three: the third is stopped everywhere near the centre (0.01^3, (1 - G1)^3 = 1.5e-5 < 1e-4)
    cases.append(dict(name="three_capped", o=[1.0, 1.0, 1.0], f=f, px={c: two_c, (9, 8): two_n}))
    # at the threshold: 1.02 / 255 is seen at its centre pixel only (1.02 G1 = 0.995 < 1), 0.99 / 255 nowhere
    o_in, o_out = 1.02 / 255.0, 0.99 / 255.0
    cases.append(dict(name="just_visible", o=[o_in], f=f[:1], px={c: o_in * f[0] + (1 - o_in) * bg, (9, 8): bg, (8, 7): bg, (9, 9): bg}))
    cases.append(dict(name="just_invisible", o=[o_out], f=f[:1], px={c: bg, (9, 8): bg, (0, 0): bg}))
    for case in cases:        # the closed forms above against the literal loop, in the format's arithmetic
        for (x, y), want in case["px"].items():
            assert abs(pixel(case["o"], case["f"], x, y) - want) < 1e-7, (case["name"], x, y)
    return dict(W=16, H=16, A=A, bg=bg, centre=c, cases=cases)


def known_answer_inputs(case, ka, dtype=torch.float32):
    """uv, conic, opacity, feature, depth of a case of ``opacity_known_answers`` (nearest first) and the radius / tile
    count an operator-level caller passes to sort_gaussian."""
    n = len(case["o"])
    uv = torch.tensor([[float(ka["centre"][0]), float(ka["centre"][1])]] * n, dtype=dtype)
    conic = torch.tensor([[ka["A"], 0.0, ka["A"]]] * n, dtype=dtype)
    op = torch.tensor(case["o"], dtype=dtype).reshape(n, 1)
    feat = torch.tensor(case["f"], dtype=dtype).reshape(n, 1)
    depth = torch.arange(1, n + 1, dtype=dtype).reshape(n, 1)
    radius = torch.full((n, 1), 14, dtype=torch.int32)
    return uv, conic, op, feat, depth, radius, torch.ones(n, 1, dtype=torch.int32)
