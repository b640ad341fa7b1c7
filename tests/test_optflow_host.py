"""CPU: optical flow from the images -- the float64 restatement (tests/optflow_ref.py) estimates the synthetic scenes' flows,
Jacobi sweeps do not depend on how the image is tiled, the host side of gflow_amd/optflow.py, the loader option, the
fit_video flag and the ABI entries.  Also holds the cases the GPU tests (tests/test_gpu_optflow.py) share."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import optflow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    """(S, region rows, region columns) of csrc/gfl_optflow.hip: the fused depth = the ring's width, and the region of a
    workgroup (a launch of the tiled path writes the region minus the ring; a level that fits the region is one workgroup)"""
    src = open(os.path.join(ROOT, "gflow_amd", "csrc", "gfl_optflow.hip")).read()
    val = lambda name: int(re.search(rf"^#define {name} (\d+)$", src, flags=re.M).group(1))
    rx = int(re.search(r"constexpr int OF_RX = (\d+)", src).group(1))
    return val("GFL_OF_S"), val("GFL_OF_RY"), rx


# ------------------------------------------------------------------------------------------------------------ the cases
SCENES = [(H, W, seed) for (H, W) in ((96, 128), (120, 214)) for seed in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def scene_pair(H, W, seed):
    """(a, b, truth): frames 2 -> 3 and 3 -> 2 of synthetic._Scene(H, W, seed) as P = 2 problems: a, b (2, H, W, 3) float32,
    truth (2, H, W, 2) float64 = frame(2)["flow"] and backward_flow(3).  Computed once, shared, left unchanged."""
    from gflow_amd import synthetic as S
    sc = S._Scene(H, W, seed)
    f2, f3 = sc.frame(2), sc.frame(3)
    i2, i3 = torch.as_tensor(f2["image"]).float(), torch.as_tensor(f3["image"]).float()
    truth = torch.stack([torch.as_tensor(f2["flow"]).double(), torch.as_tensor(sc.backward_flow(3)).double()])
    return torch.stack([i2, i3]), torch.stack([i3, i2]), truth


@functools.lru_cache(maxsize=None)
def scene_reference(H, W, seed):
    """the float64 restatement's flow of scene_pair, defaults: (2, H, W, 2)"""
    a, b, _ = scene_pair(H, W, seed)
    return R.estimate_flow(a, b)


def epe(flow, truth):
    """mean end-point error per problem"""
    return (flow.double() - truth).norm(dim=-1).mean(dim=(1, 2))


def level_images(P, H, W):
    """grey images (P, H, W) float64 in [0, 255] with different content per problem: b is a displaced by a fraction of a
    pixel that differs per problem"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    tex = lambda x, y, p: (127.0 + 60.0 * torch.sin(x / 3.1 + p) * torch.cos(y / 2.7) + 40.0 * torch.sin((x + y) / 5.3 + 2.0 * p))
    a = torch.stack([tex(x, y, float(p)) for p in range(P)])
    b = torch.stack([tex(x + 0.8 + 0.2 * p, y - 0.6, float(p)) for p in range(P)])
    return a, b


def start_flow(kind, P, H, W):
    """(P, H, W, 2) float64: "zero"; "smooth", a 1.5 px field; "outside", a field that points up to 4 px outside the image
    along every border, so that `inside` and the clamps are hit"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    out = torch.zeros(P, H, W, 2, dtype=torch.float64)
    if kind == "zero":
        return out
    for p in range(P):
        if kind == "smooth":
            out[p, ..., 0] = 1.5 * torch.sin(x / 6.0 + 0.4 * p) * torch.cos(y / 7.0)
            out[p, ..., 1] = 1.5 * torch.cos(x / 5.0) * torch.sin(y / 8.0 + 0.3 * p)
        elif kind == "outside":
            ramp = lambda t: (1.0 - t / 4.0).clamp(min=0.0)
            core = torch.minimum(torch.minimum(x, W - 1 - x), torch.minimum(y, H - 1 - y)).clamp(0.0, 4.0) / 4.0
            out[p, ..., 0] = -4.0 * ramp(x) + 4.0 * ramp(W - 1 - x) + 0.75 * core * torch.sin(y / 3.0 + p)
            out[p, ..., 1] = -4.0 * ramp(y) + 4.0 * ramp(H - 1 - y) + 0.75 * core * torch.cos(x / 3.0 + p)
        else:
            raise ValueError(kind)
    return out


# -------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("H,W,seed", SCENES)
def test_the_reference_estimates_the_scenes_flow(H, W, seed):
    """Measured (float64, defaults): mean EPE 0.046 - 0.106 px forward and backward against true flows of mean magnitude
    2.01 - 2.06 px (96 x 128: 0.054 / 0.053, 0.051 / 0.051, 0.106 / 0.085; 120 x 214: 0.046 / 0.046, 0.048 / 0.062,
    0.089 / 0.085 for the seeds 0, 1, 2).  A restatement that misreads a sign or a border does not get there."""
    _, _, truth = scene_pair(H, W, seed)
    err = epe(scene_reference(H, W, seed), truth)
    mag = truth.norm(dim=-1).mean(dim=(1, 2))
    print(H, W, seed, "EPE", err.tolist(), "mean |flow|", mag.tolist())
    assert (err < 0.25).all() and (err < 0.1 * mag).all()


def test_level_sizes_follow_the_definition():
    assert R.level_sizes(96, 128) == [(96, 128), (48, 64), (24, 32)]
    assert R.level_sizes(33, 47) == [(33, 47), (17, 24)] and R.level_sizes(65, 31) == [(65, 31)]
    assert R.level_sizes(65, 31, min_side=8) == [(65, 31), (33, 16), (17, 8)]
    assert R.level_sizes(480, 854) == [(480, 854), (240, 427), (120, 214), (60, 107), (30, 54)]
    # the binomial of a constant is the constant, of a ramp the ramp away from the border; sizes are ceil(n / 2)
    ramp = torch.arange(11, dtype=torch.float64).expand(7, 11).contiguous()
    down = R.pyr_down(ramp)
    assert down.shape == (4, 6) and torch.equal(down[:, 1:5], torch.tensor([2.0, 4.0, 6.0, 8.0]).double().expand(4, 4))
    assert torch.equal(R.pyr_down(torch.full((9, 8), 3.0, dtype=torch.float64)), torch.full((5, 4), 3.0, dtype=torch.float64))


def test_jacobi_sweeps_do_not_depend_on_the_tiling():
    """S sweeps on a tile with an S-pixel ring equal S sweeps on the whole image, bit for bit in float64: at tiles that
    straddle the image's corners (the ring outside the image does not exist there: the edge weights are zero) and inside"""
    S = kernel_constants()[0]
    H, W = 37, 45
    Ia, Ib = level_images(1, H, W)
    flow = start_flow("smooth", 1, H, W)
    u, v = flow[..., 0], flow[..., 1]
    t = R.warp_terms(Ia, Ib, u, v)
    g = torch.Generator().manual_seed(3)
    du, dv = 0.3 * torch.randn(1, H, W, generator=g, dtype=torch.float64), 0.3 * torch.randn(1, H, W, generator=g, dtype=torch.float64)
    c = R.coefficients(t, u, v, du, dv, 5.0)
    full = (du, dv)
    for _ in range(S):
        full = R.jacobi_sweep(c, u, v, *full)
    for (y0, y1, x0, x1) in ((0, 9, 0, 11), (H - 9, H, W - 11, W), (0, 9, W - 11, W), (12, 21, 15, 26)):
        ys, xs = slice(max(y0 - S, 0), min(y1 + S, H)), slice(max(x0 - S, 0), min(x1 + S, W))
        cut = lambda f: f[:, ys, xs]
        ct = {k: cut(f) for k, f in c.items()}
        tile = (cut(du), cut(dv))
        for _ in range(S):
            tile = R.jacobi_sweep(ct, cut(u), cut(v), *tile)
        iy, ix = slice(y0 - ys.start, y1 - ys.start), slice(x0 - xs.start, x1 - xs.start)
        for got, want in zip(tile, full):
            assert torch.equal(got[:, iy, ix], want[:, y0:y1, x0:x1])
        # and the ring is needed: one pixel less and the tile's edge is wrong
        assert not torch.equal(tile[0], full[0][:, ys, xs])


# ------------------------------------------------------------------------------------------------------------ the ABI
def _host_buffer(nbytes=256):
    """a 64-byte aligned host buffer standing in for a device pointer in calls that are refused before any launch"""
    raw = ctypes.create_string_buffer(nbytes + 64)
    addr = (ctypes.addressof(raw) + 63) // 64 * 64
    return raw, ctypes.c_void_p(addr)


def test_abi_entries_within_312():
    from gflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    assert int(re.search(r"^#define GFL_VERSION (\d+)$", hdr, flags=re.M).group(1)) == 312 == _lib.MIN_VERSION
    for name, n_args in (("gfl_optflow_workspace_bytes", 4), ("gfl_optflow", 15), ("gfl_optflow_level", 13)):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", hdr) and len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.SIGNATURES["gfl_optflow_workspace_bytes"][0] is ctypes.c_size_t
    assert "NOT a learned one" in hdr[hdr.index("---- optical flow"):hdr.index("size_t gfl_optflow_workspace_bytes")]


def test_workspace_query_and_refusals_without_a_gpu():
    from gflow_amd import _lib
    lib = _lib.load()
    q = lib.gfl_optflow_workspace_bytes
    # the level's planes alone: two (du, dv) copies, four terms, nine coefficients = 68 bytes per pixel
    assert q(1, 8, 8, 16) >= 68 * 64 and q(118, 480, 854, 16) > 68 * 118 * 480 * 854
    assert q(2, 96, 128, 16) > q(2, 96, 128, 64) > 0                          # (pyramid levels cost workspace)
    for bad in ((0, 96, 128, 16), (1, 7, 128, 16), (1, 96, 7, 16), (1 << 11, 1 << 10, 1 << 10, 16), (1, 1 << 15, (1 << 15) + 1, 16),
                (1, 96, 128, 1), (1, 96, 128, 0), (-1, 96, 128, 16)):
        assert q(*bad) == 0, bad
    assert q(1 << 10, 1 << 10, 1 << 10, 16) > 0                               # (exactly 2^30 pixels are accepted)
    keep, p = _host_buffer()
    nan, inf = float("nan"), float("inf")
    big = ctypes.c_size_t(1 << 40)
    good = dict(P=1, H=8, W=8, alpha=5.0, warps=1, outer=1, sweeps=1, min_side=16)

    def flow(a=p, b=p, u8=0, out=p, ws=p, nbytes=big, **kw):
        k = dict(good, **kw)
        return lib.gfl_optflow(a, b, u8, k["P"], k["H"], k["W"], k["alpha"], k["warps"], k["outer"], k["sweeps"], k["min_side"],
                               out, ws, nbytes, None)

    def level(a=p, b=p, fl=p, ws=p, nbytes=big, **kw):
        k = dict(good, **kw)
        return lib.gfl_optflow_level(a, b, fl, k["P"], k["H"], k["W"], k["alpha"], k["warps"], k["outer"], k["sweeps"], ws, nbytes,
                                     None)

    for fn in (flow, level):
        for kw in (dict(a=None), dict(b=None), dict(ws=None), dict(H=7), dict(W=7), dict(P=0), dict(sweeps=0), dict(warps=0),
                   dict(outer=0), dict(alpha=nan), dict(alpha=inf), dict(alpha=0.0), dict(alpha=-1.0),
                   dict(P=1 << 11, H=1 << 10, W=1 << 10)):
            assert fn(**kw) == -1, (fn.__name__, kw)
        assert fn(nbytes=ctypes.c_size_t(16)) == -2                           # "workspace too small", before any launch
    assert flow(out=None) == -1 and level(fl=None) == -1 and flow(min_side=1) == -1 and flow(u8=2) == -1
    odd = ctypes.c_void_p(p.value + 4)
    assert flow(out=odd) == -1 and level(fl=odd) == -1 and flow(a=ctypes.c_void_p(p.value + 1)) == -1
    assert lib.gfl_status_string(-2) == b"workspace too small"
    del keep


# ------------------------------------------------------------------------------------------------- the Python layer, host
def test_estimate_flow_argument_checks_and_no_cpu_fallback():
    from gflow_amd import optflow as OF
    z = torch.zeros(8, 8, 3)
    for bad in ((torch.zeros(8, 8), torch.zeros(8, 8)), (torch.zeros(8, 8, 2), torch.zeros(8, 8, 2)), (z, torch.zeros(8, 9, 3)),
                (torch.zeros(7, 8, 3), torch.zeros(7, 8, 3)), (torch.zeros(0, 8, 8, 3), torch.zeros(0, 8, 8, 3)),
                (z, torch.zeros(8, 8, 3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            OF.estimate_flow(*bad)
    for kw in (dict(alpha=float("nan")), dict(alpha=0.0), dict(alpha=float("inf")), dict(sweeps=0), dict(warps=0), dict(outer=0),
               dict(sweeps=2.5), dict(min_side=1)):
        with pytest.raises(ValueError):
            OF.estimate_flow(z, z, **kw)
    with pytest.raises(ValueError):
        OF.clip_flows(torch.zeros(1, 8, 8, 3))
    with pytest.raises(ValueError):
        OF.clip_flows(torch.zeros(3, 8, 8, 3), pairs=[2])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            OF.estimate_flow(z, z)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            OF.estimate_flow(np.zeros((2, 8, 8, 3), np.uint8), np.zeros((2, 8, 8, 3), np.uint8))


def _sequence(tmp_path, n=3, H=24, W=32):
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    sc = S._Scene(H, W, 0)
    return gio.write_sequence([sc.frame(k) for k in range(n)], str(tmp_path / "seq"))


def test_load_sequence_flows_option(tmp_path):
    from gflow_amd import io as gio
    sp = _sequence(tmp_path)
    a, b = gio.load_sequence(sp), gio.load_sequence(sp, flows="files")
    for fa, fb in zip(a, b):
        assert sorted(fa) == sorted(fb)
        assert all(torch.equal(fa[k], fb[k]) if torch.is_tensor(fa[k]) else fa[k] == fb[k] for k in fa)
    with pytest.raises(ValueError, match="flows"):
        gio.load_sequence(sp, flows="bogus")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gio.load_sequence(sp, flows="estimate")


def test_cli_refuses_before_it_needs_a_device(tmp_path):
    from gflow_amd import optflow as OF
    sp = _sequence(tmp_path)
    with pytest.raises(SystemExit, match="overwrite"):              # write_sequence left *_pred.flo there
        OF.main(["--img_dir", sp])
    lone = tmp_path / "lone"
    os.makedirs(lone)
    os.replace(os.path.join(sp, "00000.png"), lone / "00000.png")
    with pytest.raises(SystemExit, match="1 images"):
        OF.main(["--img_dir", str(lone)])
    assert not os.path.exists(str(lone) + "_flow_unimatch")


def test_fit_video_make_flows_needs_a_sequence(capsys):
    from gflow_amd import fit_video
    with pytest.raises(SystemExit) as e:
        fit_video.main(["--make-flows", "--help"])                  # (parsed before a device is asked for)
    assert e.value.code == 0 and "--make-flows" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        fit_video.main(["--make-flows"])
    assert e.value.code == 2 and "--make-flows needs --sequence" in capsys.readouterr().err
