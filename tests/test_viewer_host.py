"""The viewer's host side (no GPU): the camera-to-world quaternion / position conversion of gflow/viewer.py:66-82, the camera
paths, the checkpoint loader of viewer.py:38-64, the --path parser, and the argument checks of gfl_render_batch, which
answer before anything touches a device."""
import ctypes
import math
import os

import pytest
import torch

from gflow_amd import _lib as L
from gflow_amd import viewer as V

D = torch.float64


def _rot(axis, angle):
    a = torch.tensor(axis, dtype=D)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=D)
    return torch.eye(3, dtype=D) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _extr(R, t):
    return torch.cat([R, torch.tensor(t, dtype=D).reshape(3, 1)], dim=1)


def _rigid_transforms():
    """100 seeded rigid transforms: random ones, rotations by exactly pi about random and coordinate axes, near-identity ones"""
    g = torch.Generator().manual_seed(7)
    out = []
    for k in range(100):
        axis = torch.randn(3, generator=g, dtype=D).tolist()
        if k < 60:
            angle = float(torch.rand(1, generator=g, dtype=D)) * 2 * math.pi - math.pi
        elif k < 80:
            angle = math.pi
            if k < 66:
                axis = [[1, 0, 0], [0, 1, 0], [0, 0, 1]][k % 3]
        else:
            angle = 10.0 ** (-3 - (k - 80) / 3.0)               # 1e-3 .. 5e-10
        out.append(_extr(_rot(axis, angle), (3 * torch.randn(3, generator=g, dtype=D)).tolist()))
    return out


# ------------------------------------------------------------------ pose conversion
def test_identity_and_a_quarter_turn_about_y_by_hand():
    q, pos = V.extr_to_quat_pos(torch.eye(4, dtype=D)[:3])
    assert torch.equal(q, torch.tensor([0, 0, 0, 1], dtype=D)) and torch.equal(pos, torch.zeros(3, dtype=D))
    # world -> camera: a turn by +90 degrees about y, then t = (1, 2, 3).  R = [[0,0,1],[0,1,0],[-1,0,0]]; camera -> world turns
    # by -90 degrees about y: q = (0, -sin 45, 0, cos 45); position -R^T t = -(R^T (1,2,3)) = -(-3, 2, 1) = (3, -2, -1)
    E = _extr(_rot([0, 1, 0], math.pi / 2), [1.0, 2.0, 3.0])
    q, pos = V.extr_to_quat_pos(E)
    h = math.sqrt(0.5)
    assert torch.allclose(q, torch.tensor([0, -h, 0, h], dtype=D), atol=1e-12)
    assert torch.allclose(pos, torch.tensor([3.0, -2.0, -1.0], dtype=D), atol=1e-12)
    assert torch.allclose(V.quat_pos_to_extr(q, pos), E, atol=1e-12)


def test_round_trip_of_100_rigid_transforms_and_the_double_cover():
    n_pi = n_near = 0
    for E in _rigid_transforms():
        q, pos = V.extr_to_quat_pos(E)
        assert abs(float(q.norm()) - 1) < 1e-12
        back = V.quat_pos_to_extr(q, pos)
        assert float((back - E).abs().max()) < 1e-6
        assert float((V.quat_pos_to_extr(-q, pos) - back).abs().max()) < 1e-12
        tr = float(E[0, 0] + E[1, 1] + E[2, 2])
        n_pi += abs(tr + 1) < 1e-9
        n_near += 3 - tr < 1e-5 and not torch.equal(E[:, :3], torch.eye(3, dtype=D))
    assert n_pi >= 20 and n_near >= 10


# ------------------------------------------------------------------ camera paths
def _training_cameras():
    return torch.stack(_rigid_transforms()[:6])


def test_follow_fixed_and_offset():
    E = _training_cameras()
    assert torch.equal(V.follow(E), E)
    F = V.fixed(E, 2)
    assert F.shape == E.shape and all(torch.equal(F[k], E[2]) for k in range(E.shape[0]))
    b = 0.37
    O = V.offset(E, b, 0.0, 0.0)
    for k in range(E.shape[0]):
        assert torch.equal(O[k][:, :3], E[k][:, :3])
        c0, c1 = V.extr_to_quat_pos(E[k])[1], V.extr_to_quat_pos(O[k])[1]
        x_axis = E[k][0, :3]                                   # the camera's own x axis in the world
        assert torch.allclose(c1 - c0, b * x_axis, atol=1e-12)


def test_orbit_keeps_the_look_at_point_on_every_axis_at_one_distance():
    E = _training_cameras()[1]
    fx, fy, cx, cy = 120.0, 95.0, 101.5, 63.25
    depth, radius = 2.5, 0.6
    centre = V.extr_to_quat_pos(E)[1]
    P = centre + depth * E[2, :3]
    cams = V.orbit(E, 7, radius, depth)
    assert cams.shape == (7, 3, 4)
    centres = []
    for k in range(7):
        R = cams[k][:, :3]
        assert torch.allclose(R @ R.T, torch.eye(3, dtype=D), atol=1e-12) and float(torch.linalg.det(R)) > 0
        pc = R @ P + cams[k][:, 3]
        assert float(pc[2]) > 0
        u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
        assert abs(float(u) - cx) < 1e-4 and abs(float(v) - cy) < 1e-4
        assert abs(float(pc.norm()) - math.sqrt(depth ** 2 + radius ** 2)) < 1e-9
        centres.append(V.extr_to_quat_pos(cams[k])[1])
        assert abs(float((centres[-1] - centre).norm()) - radius) < 1e-9
    assert min(float((centres[i] - centres[j]).norm()) for i in range(7) for j in range(i)) > 0.1


def test_lerp_ends_and_midpoint():
    E = _training_cameras()
    path = V.lerp(E[0], E[3], 5)
    assert path.shape == (5, 3, 4)
    assert float((path[0] - E[0]).abs().max()) < 1e-9 and float((path[-1] - E[3]).abs().max()) < 1e-9
    # two cameras that differ by a rotation theta about one axis (camera -> world): the midpoint is theta / 2 about it
    theta, axis = 1.1, [0.3, -0.5, 0.8]
    A = V.quat_pos_to_extr(torch.tensor([0, 0, 0, 1], dtype=D), torch.tensor([0.0, 0.0, 0.0], dtype=D))
    c2w = _rot(axis, theta)
    B = torch.cat([c2w.T, -(c2w.T @ torch.tensor([[2.0], [0.0], [-1.0]], dtype=D))], dim=1)
    mid = V.lerp(A, B, 3)[1]
    assert torch.allclose(mid[:, :3].T, _rot(axis, theta / 2), atol=1e-9)
    assert torch.allclose(V.extr_to_quat_pos(mid)[1], torch.tensor([1.0, 0.0, -0.5], dtype=D), atol=1e-9)


# ------------------------------------------------------------------ loader
def test_log_loader_and_load_ckpt_read_what_save_checkpoint_writes(tmp_path):
    g = torch.Generator().manual_seed(3)
    os.makedirs(tmp_path / "ckpt")
    raws = {}
    for name, n in (("frame_0002", 5), ("frame_0000", 7), ("frame_0001", 3)):
        attrs = {"xyz": torch.randn(n, 3, generator=g), "scale": torch.randn(n, 3, generator=g),
                 "rotate": 2.0 * torch.randn(n, 4, generator=g), "opacity": 0.3 * torch.randn(n, 1, generator=g),
                 "rgb": torch.randn(n, 3, generator=g)}
        extr = torch.cat([torch.eye(3), torch.randn(3, 1, generator=g)], dim=1)
        raws[name] = (attrs, extr)
        torch.save({"attributes": attrs, "intr": torch.tensor([48.0, 32.0, 48.0, 32.0]), "extr": extr, "still_mask": None,
                    "move_seg": None, "last_uv": None, "width": 96 if name == "frame_0000" else 11, "height": 64},
                   tmp_path / "ckpt" / f"{name}.tar")
    (tmp_path / "ckpt" / "notes.txt").write_text("not a checkpoint")
    files, W, H = V.log_loader(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["frame_0000.tar", "frame_0001.tar", "frame_0002.tar"]
    assert (W, H) == (96, 64)                                   # of the FIRST checkpoint
    for f in files:
        attrs, extr_ref = raws[os.path.basename(f)[:-4]]
        xyz, scale, rotate, opacity, rgb, intr, extr = V.load_ckpt(f, "cpu")
        a = {k: v.double() for k, v in attrs.items()}
        assert torch.equal(xyz, attrs["xyz"]) and torch.equal(extr, extr_ref)
        assert torch.equal(intr, torch.tensor([48.0, 32.0, 48.0, 32.0]))
        assert torch.allclose(scale.double(), a["scale"].abs(), rtol=1e-6, atol=0)
        assert torch.allclose(rotate.double(), a["rotate"] / a["rotate"].norm(dim=1, keepdim=True), rtol=1e-6, atol=1e-7)
        assert torch.allclose(opacity.double(), 1 / (1 + torch.exp(-10 * a["opacity"])), rtol=1e-6, atol=1e-7)
        assert torch.allclose(rgb.double(), 1 / (1 + torch.exp(-a["rgb"])), rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------ --path
def test_path_parser():
    assert V.parse_path("follow") == ("follow", ())
    assert V.parse_path("fixed:3") == ("fixed", (3,))
    assert V.parse_path("offset:0.1,-0.2,0") == ("offset", (0.1, -0.2, 0.0))
    assert V.parse_path("orbit:2,32,0.5") == ("orbit", (2, 32, 0.5))
    assert V.parse_path("lerp:0,5,12") == ("lerp", (0, 5, 12))
    for bad in ("", "spin", "follow:1", "fixed", "fixed:a", "fixed:1,2", "offset:1,2", "offset:1,2,x", "orbit:1,0,0.5",
                "orbit:1,4", "lerp:0,1,0", "lerp:0,1", "orbit:1,4,-1"):
        with pytest.raises(ValueError) as e:
            V.parse_path(bad)
        assert repr(bad) in str(e.value)


# ------------------------------------------------------------------ gfl_render_batch: arguments
def test_render_batch_workspace_grows_with_every_argument():
    lib = L.load()
    size = lib.gfl_render_batch_workspace_bytes
    base = dict(J=4, rows=12000, K=100000, W=200, H=136)
    b = size(*base.values())
    assert b > 0
    for k, more in (("J", 8), ("rows", 24000), ("K", 200000), ("W", 400), ("H", 272)):
        assert size(*{**base, k: more}.values()) > b, k
    # at least: records, 12 bytes per pair, and a count, an offset and a range per (job, tile)
    tiles = 4 * 13 * 9
    assert b >= 12000 * 48 + 100000 * 12 + tiles * 16
    for bad in (dict(J=-1), dict(rows=-1), dict(K=0), dict(W=0), dict(H=-3)):
        assert size(*{**base, **bad}.values()) == 0


def test_render_batch_rejects_bad_arguments_before_touching_a_device():
    lib = L.load()
    INVALID = -1
    assert lib.gfl_status_string(INVALID).decode().lower().find("invalid") >= 0
    mem = (ctypes.c_char * 4096)()                           # host bytes: a rejected call reads none of its pointers
    p = ctypes.c_void_p(ctypes.addressof(mem))
    J, rows, W, H, K = 2, 100, 64, 48, 5000
    ws = lib.gfl_render_batch_workspace_bytes(J, rows, K, W, H)
    good = dict(params=p, R=100, job_rows=p, job_cam=p, J=J, rows_total=rows, W=W, H=H, K_cap=K, out_f32=p, out_u8=p, out_rec=None,
                overflow=p, workspace=p, workspace_bytes=ws, stream=None)
    bads = [dict(J=-1), dict(W=0), dict(H=0), dict(W=-5), dict(K_cap=0), dict(K_cap=-1), dict(R=-1), dict(rows_total=-1),
            dict(workspace_bytes=ws - 1), dict(workspace_bytes=0), dict(out_f32=None, out_u8=None), dict(job_rows=None),
            dict(job_cam=None), dict(overflow=None), dict(workspace=None), dict(params=None)]
    for bad in bads:
        assert lib.gfl_render_batch(*{**good, **bad}.values()) == INVALID, bad
    # no jobs: success, nothing written, nothing needed but an output
    none = {**good, "J": 0, "job_rows": None, "job_cam": None, "overflow": None, "workspace": None, "workspace_bytes": 0}
    assert lib.gfl_render_batch(*none.values()) == 0
    assert lib.gfl_render_batch(*{**none, "out_f32": None, "out_u8": None}.values()) == INVALID
    assert bytes(mem) == bytes(4096)
