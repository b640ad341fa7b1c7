"""Deterministic mode (``-m gpu``; GFL_FIT_DETERMINISTIC, include/gflow_hip.h): exact properties -- the same inputs give the
same bits, engine against engine, eager launches against graph replay, one clip alone against the same clip beside another,
a process with torch's switch against one with the library's -- plus the mode's own correctness against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xyz", "scale", "rotate", "opacity", "rgb")
H, W, N = 480, 854, 60000
# everything an iteration leaves behind that the contract covers (the sorted lists separately: tile by tile)
OUT = ("render", "final_T", "n_contrib", "rec", "params", "adam_m", "adam_v", "pose", "pose_m", "pose_v", "depth_ab", "ab_m",
       "ab_v", "sums", "d_extr", "extr", "step")
SMALL = dict(num_points=1500, iterations_first=60, iterations_after=40, iterations_camera=20, densify_interval=30,
             densify_times=1, densify_interval_after=20, densify_times_after=1, lambda_depth=1e-2)


def _bench_scene():
    from gflow_amd import synthetic as S
    frame = S.make_frame(H, W, seed=0)
    raw = S.init_splats(frame, N, seed=0, grown=True)
    return frame, raw


def _det_engine(raw, frame, deterministic=True, **hyper):
    from tests.test_gpu_fused import _engine
    eng = _engine({k: raw[k] for k in NAMES}, dict(W=frame["image"].shape[1], H=frame["image"].shape[0], intr=raw["intr"]),
                  frame["image"], frame["depth"], **hyper)
    eng.deterministic = deterministic
    return eng


def _lists(eng):
    from tests.test_gpu_fused import _lists as lists
    return lists(eng)


def _assert_same(a, b, what):
    assert a.N == b.N, what
    for k in OUT:
        x, y = getattr(a, k), getattr(b, k)
        if k in ("rec", "params", "adam_m", "adam_v"):
            x, y = x[:a.N], y[:b.N]
        assert torch.equal(x, y), f"{what}: {k} differs"
    la, lb = _lists(a), _lists(b)
    assert all(torch.equal(x, y) for x, y in zip(la, lb)), f"{what}: a tile's sorted list differs"


# the three kinds of iteration of a clip fit: first frame (10 sums per pair), camera-only stage (6), joint stage (7)
STAGES = (("first", dict(freeze_rgb=0, freeze_all_splats=0, lr_camera=0.0)),
          ("camera", dict(freeze_rgb=1, freeze_all_splats=1, lr_camera=1e-3)),
          ("joint", dict(freeze_rgb=1, freeze_all_splats=0, lr_camera=0.0)))


def test_fullsize_engines_are_bit_identical_eager_and_replayed():
    """480x854, the 60 000-splat bench scene: three deterministic engines from the same rows, two launched eagerly, one from
    captured graphs, through iterations of all three kinds -- every output of the contract bit for bit after every stage."""
    frame, raw = _bench_scene()
    hyper = dict(lambda_rgb=1.0, lambda_depth=0.1, lambda_var=10.0, lr=1e-3, total_iters=500)
    a, b, g = (_det_engine(raw, frame, **hyper) for _ in range(3))
    pose0 = torch.tensor([0.002, -0.001, 0.0015, 1.0, 0.01, -0.02, 0.015], device=DEV)
    for e in (a, b, g):
        e.pose.copy_(pose0)
    g.iteration()                        # (graphs are captured once every kernel has been loaded)
    a.iteration()
    b.iteration()
    for name, hp in STAGES:
        for e in (a, b, g):
            for k, v in hp.items():
                setattr(e.hp, k, v)
        for _ in range(3):
            a.iteration()
            b.iteration()
            g.iteration(use_graph=True)
        torch.cuda.synchronize()
        assert a.overflow.tolist()[0] == 0
        _assert_same(a, b, f"{name}: eager engine against eager engine")
        _assert_same(a, g, f"{name}: eager engine against graph replay")
    assert g.graphs.live, "no graph was replayed"


def test_fullsize_deterministic_iteration_matches_oracle_and_default_mode():
    """The deterministic engine is not only repeatable but right: one iteration from a zero Adam state against
    oracle/fit_oracle.py with the bounds of test_gpu_fullsize.py::test_fullsize_fused_iteration_matches_oracle, and
    against the default engine to within rounding."""
    from gflow_amd.fused import COLS
    from oracle import fit_oracle as FO
    from tests.test_gpu_parity import close_frac
    frame, raw = _bench_scene()
    n = raw["xyz"].shape[0]
    lam = dict(lambda_rgb=1.0, lambda_depth=0.1, lambda_var=10.0)
    pose0 = torch.tensor([0.002, -0.001, 0.0015, 1.0, 0.01, -0.02, 0.015])
    det = _det_engine(raw, frame, pose=pose0, lr=1e-4, lr_camera=1e-4, total_iters=500, **lam)
    ref = _det_engine(raw, frame, deterministic=False, pose=pose0, lr=1e-4, lr_camera=1e-4, total_iters=500, **lam)
    det.iteration()
    ref.iteration()
    rc = {k: raw[k].clone().requires_grad_(True) for k in NAMES}
    pose = pose0.clone().requires_grad_(True)
    ab = torch.tensor([1.0, 0.0], requires_grad=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    loss, info = FO.fit_loss(rc, pose, ab, raw["intr"], dict(image=frame["image"], depth=frame["depth"]), 0.0,
                             lam["lambda_rgb"], lam["lambda_depth"], lam["lambda_var"])
    loss.backward()
    bad_frac, hard = 1e-5, 1e-3
    if det.lib.gfl_ewa_on_mfma():
        bad_frac, hard = 5e-5, float(frame["depth"].max()) / 255.0      # (the MFMA build's bound, test_gpu_fullsize.py)
    close_frac(det.render, info["render4"], 1e-4, 1e-5, bad_frac=bad_frac, hard=hard, what="deterministic render vs oracle")
    g_all = (det.adam_m[:n] / 0.1).cpu()
    g_ref = (ref.adam_m[:n] / 0.1).cpu()
    for k, (a, b) in COLS.items():
        want = rc[k].grad.reshape(n, b - a)
        rel = ((g_all[:, a:b] - want).norm() / want.norm()).item()
        assert rel < 2e-4, f"d_{k} relative L2 error against the oracle {rel:.2e}"
        # the two modes add the same terms in other orders: float rounding, nothing more
        rel_d = ((g_all[:, a:b] - g_ref[:, a:b]).norm() / g_ref[:, a:b].norm()).item()
        print(f"observed d_{k}: oracle {rel:.2e}, default mode {rel_d:.2e}")
        assert rel_d < 1e-5, f"d_{k}: deterministic against default mode {rel_d:.2e}"
    gp = (det.pose_m / 0.1).cpu()
    assert ((gp - pose.grad).norm() / pose.grad.norm()).item() < 2e-4
    np.testing.assert_allclose((det.ab_m / 0.1).cpu().numpy(), ab.grad.numpy(), rtol=5e-4)
    torch.testing.assert_close(det.render, ref.render, rtol=0, atol=1e-5)
    assert torch.equal(det.n_contrib, ref.n_contrib)


def _lattice_scene(Hl=320, Wl=320, spacing=1.0, sigma_px=2.0, opacity=0.05):
    """Identical splats on a regular lattice at one depth: every tile away from the border holds a list of the same length
    and, once the backward has counted them, the same units -- ties of the tile weights everywhere, the first round's cutoff
    included."""
    from gflow_amd import synthetic as S
    from gflow_amd.geometry import pix2world
    frame = S.make_frame(Hl, Wl, seed=3)
    base = S.init_splats(frame, 16, seed=3)
    ys, xs = torch.meshgrid(torch.arange(0, Hl, spacing), torch.arange(0, Wl, spacing), indexing="ij")
    uv = torch.stack([xs.reshape(-1), ys.reshape(-1)], dim=1).float()
    n = uv.shape[0]
    depth = torch.full((n, 1), 2.0)
    raw = dict(xyz=pix2world(uv, depth, base["intr"], base["extr"]),
               # (no extent along the view axis: the projected footprint is then the same everywhere on the image)
               scale=torch.cat([(sigma_px * depth / frame["focal"]).repeat(1, 2), torch.zeros(n, 1)], dim=1),
               rotate=torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1),
               opacity=torch.logit(torch.full((n, 1), opacity)) / 10.0,
               rgb=torch.zeros(n, 3))
    raw = {k: v.contiguous() for k, v in raw.items()}
    raw["intr"], raw["extr"] = base["intr"], base["extr"]
    return frame, raw


def test_tied_tile_weights_give_one_schedule():
    """Many tiles of identical weight at the first round's cutoff -- the tiles that are walked in segments (backward) and on
    four CUs (forward) are chosen among ties there.  Two deterministic engines build the same queues, backward and forward,
    and the same render and gradients, with list lengths as weights (first iteration) and with counted units (second)."""
    frame, raw = _lattice_scene()
    hyper = dict(lambda_rgb=1.0, lambda_depth=0.0, lr=1e-3, total_iters=500)
    a, b = _det_engine(raw, frame, **hyper), _det_engine(raw, frame, **hyper)
    for it in range(2):
        a.iteration()
        b.iteration()
        torch.cuda.synchronize()
        assert a.overflow.tolist()[0] == 0
        lens = (a.tile_range[:, 1] - a.tile_range[:, 0]).cpu()
        nq = len(a.schedule())
        if it == 0:
            # the test has power: the weights are tied across the first round's cutoff, and those tiles are long enough to
            # be split both ways (backward segments from 129 splats, the four-CU forward walk from GFL_FWD_SPLIT_MIN)
            srt = lens.sort(descending=True).values
            assert lens.numel() > nq and int(srt[nq - 1]) == int(srt[nq]), (nq, srt[:nq + 2].tolist())
            assert int((lens == srt[nq]).sum()) > nq // 2
            assert int(srt[nq]) > 448, int(srt[nq])
        for fwd in (False, True):
            qa, qb = a.schedule(forward=fwd), b.schedule(forward=fwd)
            assert len(qa) == len(qb) and all(torch.equal(x, y) for x, y in zip(qa, qb)), f"iteration {it}: schedule(forward={fwd})"
        _assert_same(a, b, f"lattice, iteration {it}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2047, 2048, 2049, 480 * 854])
def test_scan_f64(n):
    from gflow_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(n)
    x = torch.rand(n, generator=g, device=DEV, dtype=torch.float64) * 1e-3 + 1e-9
    y = _lib.scan_f64(x)
    want = np.cumsum(x.cpu().numpy())
    err = np.abs(y.cpu().numpy() - want).max() / np.abs(want).max()
    assert err <= 1e-12, err
    assert torch.equal(y, _lib.scan_f64(x)), "two calls differ"
    with torch.cuda.stream(torch.cuda.Stream()):
        z = _lib.scan_f64(x)
    torch.cuda.synchronize()
    assert torch.equal(y, z), "another stream gives other bits"
    # independent of the launch's grid: a prefix (fewer workgroups) gives the prefix's bits
    for m in sorted({1, n // 2, n - 1} - {0}):
        assert torch.equal(_lib.scan_f64(x[:m]), y[:m]), m
    assert float(y[0]) == float(x[0])


def _fit(frames, keep=None, **kw):
    from gflow_amd.fit_video import fit_clip
    return fit_clip(frames, DEV, SMALL, seed=kw.pop("seed", 0), keep=keep, **kw)


def _final(keep):
    tr = keep["trainer"]
    eng = tr.engine
    out = {k: getattr(eng, k)[:eng.N].clone() for k in ("params", "adam_m", "adam_v")}
    out.update({k: getattr(eng, k).clone() for k in ("pose", "depth_ab", "render")})
    out["psnr"] = torch.stack([p.float() for p in keep["psnr"]])
    return out


def test_whole_fit_is_bit_identical_run_to_run():
    from tests.test_gpu_fitvideo import _clip
    frames = _clip()
    cfg_traj = dict(traj_num=40)
    ka, kb = {}, {}
    from gflow_amd.fit_video import fit_clip
    ma = fit_clip(frames, DEV, {**SMALL, **cfg_traj}, seed=0, keep=ka, deterministic=True)
    mb = fit_clip(frames, DEV, {**SMALL, **cfg_traj}, seed=0, keep=kb, deterministic=True)
    ta, tb = ma.pop("traj"), mb.pop("traj")
    assert ma == mb
    assert ma["splats_final"] > SMALL["num_points"]            # densification ran
    fa, fb = _final(ka), _final(kb)
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k
    assert np.array_equal(ta["images"], tb["images"]) and np.array_equal(ta["uv"], tb["uv"]) and ta["index"] == tb["index"]


def test_concurrent_clips_equal_the_clips_fitted_alone():
    from gflow_amd.fit_video import fit_clip, fit_clips_concurrent
    from tests.test_gpu_fitvideo import _clip
    clips = [_clip(seed=4), _clip(seed=5)]
    alone = [fit_clip(c, DEV, SMALL, seed=i, deterministic=True) for i, c in enumerate(clips)]
    together = fit_clips_concurrent(clips, DEV, SMALL, deterministic=True)
    assert together == alone


def test_fused_render_operator_gradients_repeat_under_torchs_switch():
    import gflow_amd.render as R
    frame, raw = _bench_scene()
    act = {"xyz": raw["xyz"], "scale": raw["scale"].abs(), "rotate": torch.nn.functional.normalize(raw["rotate"]),
           "opacity": torch.sigmoid(10 * raw["opacity"]), "rgb": torch.sigmoid(raw["rgb"])}
    cam = dict(intr=raw["intr"].to(DEV), extr=raw["extr"].to(DEV), W=W, H=H)
    before = torch.are_deterministic_algorithms_enabled()
    warn_only = torch.is_deterministic_algorithms_warn_only_enabled()
    grads = []
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        for _ in range(2):
            leaves = {k: v.to(DEV).clone().requires_grad_(True) for k, v in act.items()}
            out = R.render(leaves, cam)
            (out["rgb"].square().sum() + out["depth_map"].sum() + out["uv"].sum()).backward()
            grads.append([out["rgb"].detach()] + [leaves[k].grad for k in NAMES])
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn_only)
    assert all(torch.equal(x, y) for x, y in zip(*grads))


_CHILD = r"""
import json, sys, warnings
import torch
sys.path.insert(0, sys.argv[1])
from gflow_amd.fit_video import fit_clip
from gflow_amd import msplat
from tests.test_gpu_fitvideo import _clip
from tests.test_gpu_deterministic import SMALL
frames = _clip()
res = {}
torch.use_deterministic_algorithms(True)
keep_a = {}
a = fit_clip(frames, "cuda", SMALL, seed=0, keep=keep_a)                  # follows torch's switch
pa = keep_a["trainer"].engine.params[:keep_a["trainer"].engine.N].clone()
res["det_flag_engine"] = bool(keep_a["trainer"].engine.deterministic)
torch.use_deterministic_algorithms(False)
keep_b = {}
b = fit_clip(frames, "cuda", SMALL, seed=0, keep=keep_b, deterministic=True)
pb = keep_b["trainer"].engine.params[:keep_b["trainer"].engine.N]
res["metrics_equal"] = a == b
res["params_equal"] = bool(pa.shape == pb.shape and torch.equal(pa, pb))
# the operator path's blend backward: torch's contract for an op without a deterministic implementation
n, Wd, Hd = 64, 32, 32
g = torch.Generator(device="cuda").manual_seed(0)
uv = (torch.rand(n, 2, device="cuda", generator=g) * 32).requires_grad_(True)
conic = torch.tensor([[0.2, 0.0, 0.2]], device="cuda").repeat(n, 1).requires_grad_(True)
op = torch.full((n, 1), 0.5, device="cuda", requires_grad=True)
feat = torch.rand(n, 3, device="cuda", generator=g).requires_grad_(True)
depth = torch.rand(n, 1, device="cuda", generator=g) + 1.0
radius = torch.full((n,), 6, dtype=torch.int32, device="cuda")
tiles = torch.full((n,), 4, dtype=torch.int32, device="cuda")
def blend():
    ids, tr = msplat.sort_gaussian(uv.detach(), depth, Wd, Hd, radius, tiles)
    return msplat.alpha_blending(uv, conic, op, feat, ids, tr, 0.0, Wd, Hd)
torch.use_deterministic_algorithms(True)
try:
    blend().sum().backward()
    res["raises"] = False
except RuntimeError as e:
    res["raises"] = "deterministic" in str(e)
torch.use_deterministic_algorithms(True, warn_only=True)
with warnings.catch_warnings(record=True) as w:
    warnings.simplefilter("always")
    blend().sum().backward()
res["warns"] = any("deterministic" in str(x.message) for x in w) and uv.grad is not None
print("RESULT " + json.dumps(res))
"""


def test_torchs_switch_in_a_fresh_process():
    """torch.use_deterministic_algorithms(True): a fit completes (torch.cumsum on the device used to raise at the first draw)
    and equals fit_clip(deterministic=True); the operator path's blend backward raises, or warns with warn_only."""
    env = dict(os.environ, CUBLAS_WORKSPACE_CONFIG=":4096:8")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert p.returncode == 0 and lines, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads(lines[-1][7:])
    assert res == dict(det_flag_engine=True, metrics_equal=True, params_equal=True, raises=True, warns=True), res
