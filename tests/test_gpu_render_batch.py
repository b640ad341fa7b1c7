"""The batched inference rasteriser gfl_render_batch (include/gflow_hip.h), its Python layer render_views / render_jobs /
render_block and the headless viewer on top of it (``-m gpu``).  Per job the reference is the CPU oracle's
render_multiple(input_group, ["rgb", "uv", "depth", "depth_map"]) with the tolerances tests/test_gpu_render_op.py holds
render() to: rgb / depth_map (1e-4, 1e-5, bad_frac 3e-4, hard 2e-2), uv (1e-5, 1e-3), depth (1e-6, 1e-6)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import fit_oracle as FO
from oracle import msplat_oracle as MO
from tests.scenes import camera_scene, capped_pile_scene, random_scene
from tests.test_gpu_parity import close_frac, observe

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "scale", "rotate", "opacity", "rgb")
W, H = 200, 136                      # 12.5 x 8.5 tiles
WANT = ["rgb", "uv", "depth", "depth_map"]


def _block(s):
    n = s["xyz"].shape[0]
    return torch.cat([s[k].float().reshape(n, -1) for k in NAMES] + [torch.zeros(n, 2)], dim=1)


def _cam(intr, extr, bg):
    return torch.cat([intr.float().reshape(4), extr.float().reshape(12), torch.tensor([float(bg)])])


def _ry(a):
    return torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float32)


def _oracle(rows, cam, w=W, h=H):
    rows = rows.double()
    group = [rows[:, 0:3], rows[:, 3:6], rows[:, 6:10], rows[:, 10:11], rows[:, 11:14], cam[0:4].double(),
             cam[4:16].double().reshape(3, 4), float(cam[16]), w, h]
    # float32 like the test of render(): the oracle's arithmetic in the kernels' number format
    group = [g.float() if torch.is_tensor(g) else g for g in group]
    return MO.render_multiple(group, WANT)


def run_batch(block, ranges, cams, w=W, h=H, K_cap=None, f32=True, u8=True, rec=True, guard=0):
    """gfl_render_batch through ctypes on device copies of (block, ranges, cams): dict(rc, f32, u8, rec, overflow, guard_ok)"""
    from gflow_amd import _lib as L
    lib = L.load()
    J = len(ranges)
    total = sum(c for _, c in ranges)
    K_cap = K_cap or 400_000
    blk = block.float().contiguous().to(DEV)
    rows = torch.tensor(ranges, dtype=torch.int32).reshape(J, 2).to(DEV)
    cam = torch.stack(list(cams)).float().contiguous().to(DEV) if J else torch.zeros(0, 17, device=DEV)
    out = torch.full((J, 4, h, w), float("nan"), device=DEV) if f32 else None
    img = torch.full((J, h, w, 3), 77, dtype=torch.uint8, device=DEV) if u8 else None
    recs = torch.full((max(total, 1), 12), float("nan"), device=DEV) if rec else None
    ovf = torch.full((max(J, 1),), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.gfl_render_batch_workspace_bytes(J, total, K_cap, w, h)
    ws = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = lib.gfl_render_batch(L.ptr(blk), blk.shape[0], L.ptr(rows), L.ptr(cam), J, total, w, h, K_cap, L.ptr(out), L.ptr(img),
                              L.ptr(recs), L.ptr(ovf), L.ptr(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    return dict(rc=rc, f32=None if out is None else out.cpu(), u8=None if img is None else img.cpu(),
                rec=None if recs is None else recs.cpu()[:total], overflow=ovf.cpu()[:J],
                guard_ok=bool((ws[nbytes:] == 0xA5).all()) if guard else None)


def _u8_of(f32):
    return (torch.clamp(f32[:, :3], 0.0, 1.0) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ the four jobs of tests 1-3, their oracle and one batched call
@pytest.fixture(scope="module")
def four_jobs():
    a = random_scene(3000, W, H, seed=11, sigma_px=2.5)
    g = camera_scene(1500, W, H, "general", seed=11, sigma_px=2.5)
    block = torch.cat([_block(a), _block(g)])
    # sideways and turned by about 10 degrees: chosen here, on the CPU, so that the job keeps visible AND culled splats
    R1 = _ry(math.radians(10.0)) @ a["extr"][:, :3]
    t1 = _ry(math.radians(10.0)) @ a["extr"][:, 3] + torch.tensor([0.25, 0.0, 0.0])
    moved = torch.cat([R1, t1.unsqueeze(1)], dim=1)
    ranges = [(0, 3000), (0, 3000), (3000, 1500), (100, 1200)]
    cams = [_cam(a["intr"], a["extr"], 0.33), _cam(a["intr"], moved, 1.0), _cam(g["intr"], g["extr"], 0.33),
            _cam(a["intr"], a["extr"], 1.0)]
    ref = [_oracle(block[f:f + c], cam) for (f, c), cam in zip(ranges, cams)]
    for j, r in enumerate(ref):
        vis = int((r["depth"] != 0).sum())
        assert 100 <= vis <= ranges[j][1] - 20, f"job {j}: {vis} of {ranges[j][1]} splats visible"
    assert int(((ref[0]["depth"] != 0) != (ref[1]["depth"] != 0)).sum()) >= 50, "the moved camera culls what the first one culls"
    got = run_batch(block, ranges, cams)
    return dict(block=block, ranges=ranges, cams=cams, ref=ref, got=got)


def _rec_rows(res, ranges, j):
    at = sum(c for _, c in ranges[:j])
    return res["rec"][at:at + ranges[j][1]]


def test_every_job_matches_the_oracle(four_jobs):
    fj = four_jobs
    got = fj["got"]
    assert got["rc"] == 0 and got["overflow"].tolist() == [0, 0, 0, 0]
    for j, ref in enumerate(fj["ref"]):
        tag = f"render_batch job {j}: "
        close_frac(got["f32"][j, :3], ref["rgb"], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=tag + "rgb")
        close_frac(got["f32"][j, 3:4], ref["depth_map"], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=tag + "depth_map")
        rec = _rec_rows(got, fj["ranges"], j)
        close_frac(rec[:, 0:2], ref["uv"], 1e-5, 1e-3, what=tag + "uv")
        close_frac(rec[:, 9:10], ref["depth"], 1e-6, 1e-6, what=tag + "depth")


def test_bytes_are_the_floats_clamped_scaled_and_truncated(four_jobs):
    fj = four_jobs
    got = fj["got"]
    assert torch.equal(got["u8"], _u8_of(got["f32"]))
    only_u8 = run_batch(fj["block"], fj["ranges"], fj["cams"], f32=False, rec=False)
    only_f32 = run_batch(fj["block"], fj["ranges"], fj["cams"], u8=False, rec=False)
    assert only_u8["rc"] == 0 and only_f32["rc"] == 0
    assert torch.equal(only_u8["u8"], got["u8"])
    assert torch.equal(only_f32["f32"].view(torch.int32), got["f32"].view(torch.int32))
    # colours and backgrounds that reach exactly 0 and 1: an empty region under bg = 1 and bg = 0, a saturated opaque splat
    w, h = 72, 40
    intr, extr = torch.tensor([40.0, 40.0, 36.0, 20.0]), torch.eye(4)[:3]
    n = 3
    s = dict(xyz=torch.tensor([[-0.5, 0.0, 2.0], [0.3, 0.1, 2.0], [0.3, 0.1, 2.5]]), scale=torch.full((n, 3), 0.12),
             rotate=torch.tensor([[1.0, 0, 0, 0]] * n), opacity=torch.tensor([[1.0], [1.0], [0.7]]),
             rgb=torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0]]))
    res = run_batch(_block(s), [(0, n), (0, n)], [_cam(intr, extr, 1.0), _cam(intr, extr, 0.0)], w=w, h=h)
    assert res["rc"] == 0
    assert torch.equal(res["u8"], _u8_of(res["f32"]))
    assert bool((res["f32"][0, :3, :, -8:] == 1.0).all()) and bool((res["u8"][0, :, -8:] == 255).all())      # nothing there: bg
    assert bool((res["f32"][1, :3, :, -8:] == 0.0).all()) and bool((res["u8"][1, :, -8:] == 0).all())
    assert int(res["u8"][1].max()) >= 252 and int(res["u8"][1].min()) == 0 and int(res["u8"][0].max()) == 255      # 0.99 x 1.0 = 252.45
    assert len(set(res["u8"].reshape(-1).tolist())) > 20


def test_a_job_is_a_function_of_its_own_rows_and_camera(four_jobs):
    fj = four_jobs
    got = fj["got"]
    bits = lambda t: t.contiguous().view(torch.int32)
    solo = [run_batch(fj["block"], [fj["ranges"][j]], [fj["cams"][j]]) for j in range(4)]
    for j in range(4):
        assert torch.equal(bits(solo[j]["f32"][0]), bits(got["f32"][j])), f"job {j} alone"
        assert torch.equal(solo[j]["u8"][0], got["u8"][j])
        assert torch.equal(bits(solo[j]["rec"]), bits(_rec_rows(got, fj["ranges"], j)))
    for perm in ([2, 0, 3, 1], [3, 2, 1, 0], [1, 3, 0, 2]):
        ranges = [fj["ranges"][j] for j in perm]
        res = run_batch(fj["block"], ranges, [fj["cams"][j] for j in perm])
        for pos, j in enumerate(perm):
            assert torch.equal(bits(res["f32"][pos]), bits(got["f32"][j])), f"job {j} at position {pos} of {perm}"
            assert torch.equal(res["u8"][pos], got["u8"][j])
            assert torch.equal(bits(_rec_rows(res, ranges, pos)), bits(_rec_rows(got, fj["ranges"], j)))
    twice = run_batch(fj["block"], [fj["ranges"][1]] * 2, [fj["cams"][1]] * 2)
    assert torch.equal(bits(twice["f32"][0]), bits(twice["f32"][1])) and torch.equal(twice["u8"][0], twice["u8"][1])
    again = run_batch(fj["block"], fj["ranges"], fj["cams"])
    assert torch.equal(again["u8"], got["u8"]) and torch.equal(bits(again["f32"]), bits(got["f32"]))


def test_job_boundaries_empty_tiles_empty_jobs_and_culled_jobs():
    a = random_scene(1200, W, H, seed=4, sigma_px=2.5)
    front = random_scene(800, W, H, seed=5, sigma_px=2.5, behind=0.0)
    intr, extr = a["intr"], a["extr"]
    # job 0: the scene plus three splats in the middle of the LAST tile (x 192 .. 199, y 128 .. 135)
    f = float(intr[0])
    pc = torch.tensor([[(196.0 - W / 2) / f * 2.0, (132.0 - H / 2) / f * 2.0, 2.0]]).repeat(3, 1) + torch.tensor([[0.0], [0.01], [0.02]])
    corner = dict(xyz=(pc - extr[:, 3]) @ extr[:, :3], scale=torch.full((3, 3), 0.02), rotate=torch.tensor([[1.0, 0, 0, 0]] * 3),
                  opacity=torch.full((3, 1), 0.8), rgb=torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]))
    # job 1: the rows that stay well clear of the first tile (or are culled)
    uv_a, depth_a = MO.project_point(a["xyz"], intr, extr, W, H)
    clear = (uv_a[:, 0] > 90) | (uv_a[:, 1] > 90) | (depth_a[:, 0] == 0)
    b1 = _block(a)[clear]
    block = torch.cat([_block(a), _block(corner), b1, _block(front)])
    n0, n1 = 1203, b1.shape[0]
    back = torch.cat([_ry(math.pi) @ extr[:, :3], (_ry(math.pi) @ extr[:, 3]).unsqueeze(1)], dim=1)     # turned by pi about y
    ranges = [(0, n0), (n0, n1), (0, 0), (n0 + n1, 800)]
    cams = [_cam(intr, extr, 0.33), _cam(intr, extr, 0.5), _cam(intr, extr, 0.75), _cam(intr, back, 0.25)]

    # the oracle's lists, on the CPU: job 0's last tile has entries, job 1's first has none, job 3 sees nothing
    def lists(rows, cam):
        r = rows.float()
        e = cam[4:16].reshape(3, 4)
        uv, depth = MO.project_point(r[:, 0:3], cam[0:4], e, W, H)
        vis = depth != 0
        conic, radius, tiles = MO.ewa_project(r[:, 0:3], MO.compute_cov3d(r[:, 3:6], r[:, 6:10], vis), cam[0:4], e, uv, W, H, vis)
        return MO.sort_gaussian(uv, depth, W, H, radius, tiles)[1], depth
    tr0, _ = lists(block[0:n0], cams[0])
    tr1, _ = lists(block[n0:n0 + n1], cams[1])
    _, d3 = lists(block[n0 + n1:], cams[3])
    assert int(tr0[-1, 1] - tr0[-1, 0]) >= 3 and int(tr1[0, 1] - tr1[0, 0]) == 0 and bool((d3 == 0).all())
    res = run_batch(block, ranges, cams)
    assert res["rc"] == 0 and res["overflow"].tolist() == [0, 0, 0, 0]
    assert bool((res["f32"][0, :3, 128:, 192:] != 0.33).any()), "job 0's last tile shows its splats"
    for j, bg in ((2, 0.75), (3, 0.25)):
        assert bool((res["f32"][j] == bg).all()) and bool((res["u8"][j] == int(bg * 255)).all()), f"job {j}: the background"
    assert bool((res["f32"][1, :, :16, :16] == 0.5).all())
    for j in (0, 1):
        solo = run_batch(block, [ranges[j]], [cams[j]])
        assert torch.equal(solo["f32"][0].view(torch.int32), res["f32"][j].view(torch.int32)) and torch.equal(solo["u8"][0], res["u8"][j])


def test_long_lists_alpha_cap_early_stop_and_equal_depths():
    sc = capped_pile_scene(48, 48, n_pile=700, n_rest=300)
    act = FO.activate({k: v.float() for k, v in sc["raw"].items()})
    s = dict(zip(NAMES, act))
    block = _block(s)
    shifted = sc["extr"].clone()
    shifted[:, 3] += torch.tensor([0.02, 0.01, 0.0])
    cams = [_cam(sc["intr"], sc["extr"], 0.33), _cam(sc["intr"], shifted, 1.0)]
    res = run_batch(block, [(0, 1000), (0, 1000)], cams, w=48, h=48)
    assert res["rc"] == 0 and res["overflow"].tolist() == [0, 0]
    for j in (0, 1):
        ref = _oracle(block, cams[j], 48, 48)
        tag = f"render_batch, capped pile, camera {j}: "
        close_frac(res["f32"][j, :3], ref["rgb"], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=tag + "rgb")
        close_frac(res["f32"][j, 3:4], ref["depth_map"], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=tag + "depth_map")
    # 64 exact duplicates of one splat in one tile: equal depth bits, so the list order is the id order, and the weight of
    # duplicate k is a (1 - a)^k -- a colour changed at id 7 or at id 50 moves the image by what the oracle says
    w, h = 32, 32
    intr, extr = torch.tensor([20.0, 20.0, 16.0, 16.0]), torch.eye(4)[:3]
    one = dict(xyz=torch.tensor([[-0.35, -0.3, 2.0]]), scale=torch.tensor([[0.25, 0.2, 0.2]]), rotate=torch.tensor([[1.0, 0, 0, 0]]),
               opacity=torch.tensor([[0.1]]), rgb=torch.tensor([[0.2, 0.5, 0.3]]))
    base = _block({k: v.repeat(64, 1) for k, v in one.items()})
    v7, v50 = base.clone(), base.clone()
    v7[7, 11:14] = torch.tensor([1.0, 0.0, 0.9])
    v50[50, 11:14] = torch.tensor([1.0, 0.0, 0.9])
    block = torch.cat([base, v7, v50])
    cam = _cam(intr, extr, 0.0)
    res = run_batch(block, [(0, 64), (64, 64), (128, 64)], [cam] * 3, w=w, h=h)
    assert res["rc"] == 0
    refs = [_oracle(block[k * 64:(k + 1) * 64], cam, w, h) for k in range(3)]
    assert float((refs[1]["rgb"] - refs[2]["rgb"]).abs().max()) > 5e-3 and float((refs[1]["rgb"] - refs[0]["rgb"]).abs().max()) > 1e-2
    for k in range(3):
        close_frac(res["f32"][k, :3], refs[k]["rgb"], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=f"render_batch, 64 duplicates, variant {k}: rgb")


def test_a_full_pair_pool_truncates_the_last_job_only():
    """Sizes worked out beforehand from the oracle's tiles_touched (an upper bound of a job's pairs: the kernels also drop the
    tiles of a rectangle that the splat's alpha >= 1/255 disc does not reach).  K_cap holds jobs 0 and 1 whole and a quarter
    of job 2's bound; job 2 is ten times as long as the other two."""
    a = random_scene(3000, W, H, seed=11, sigma_px=2.5)
    block = _block(a)
    cam = _cam(a["intr"], a["extr"], 0.33)
    ranges = [(0, 300), (300, 300), (0, 3000)]

    def touched(rows):
        r = rows.float()
        uv, depth = MO.project_point(r[:, 0:3], a["intr"], a["extr"], W, H)
        vis = depth != 0
        return int(MO.ewa_project(r[:, 0:3], MO.compute_cov3d(r[:, 3:6], r[:, 6:10], vis), a["intr"], a["extr"], uv, W, H, vis)[2].sum())
    p = [touched(block[f:f + c]) for f, c in ranges]
    K_cap = p[0] + p[1] + p[2] // 4
    assert p[0] + p[1] < K_cap < sum(p) and p[2] > 4 * (p[0] + p[1])
    roomy = run_batch(block, ranges, [cam] * 3, K_cap=2 * sum(p))
    assert roomy["rc"] == 0 and roomy["overflow"].tolist() == [0, 0, 0]
    tight = run_batch(block, ranges, [cam] * 3, K_cap=K_cap, guard=1 << 16)
    assert tight["rc"] == 0
    assert tight["overflow"].tolist() == [0, 0, 1]
    assert tight["guard_ok"], "bytes behind the pair pool were written"
    for j in (0, 1):
        assert torch.equal(tight["f32"][j].view(torch.int32), roomy["f32"][j].view(torch.int32))
        assert torch.equal(tight["u8"][j], roomy["u8"][j])
    again = run_batch(block, ranges, [cam] * 3, K_cap=K_cap)
    assert torch.equal(again["u8"], tight["u8"]), "a truncated job is reproducible too"


def wide_walk_jobs():
    """The transition scene (168 x 120, 11 x 8 tiles, 168 class rows in front of 1500 ordinary ones) under the pose of
    tests/test_gpu_fused.py as two jobs of one call, rows (0, 1668) and (5, 163), and the float32 oracle's tile count of every
    RECORD row of the call (job 0's rows, then job 1's)."""
    from oracle import loss_oracle as LO
    from tests.scenes import oracle_front_end, rect_facts, transition_scene
    from tests.test_gpu_fused import POSE
    extr = LO.pose_to_extr(POSE)
    sc = transition_scene(extr=extr)
    w, h = sc["W"], sc["H"]
    block = _block(dict(zip(NAMES, FO.activate({k: v.float() for k, v in sc["raw"].items()}))))
    ranges = [(0, 1668), (5, 163)]
    cams = [_cam(sc["intr"], extr, 0.33), _cam(sc["intr"], extr, 1.0)]
    tiles = rect_facts(oracle_front_end(sc, POSE, torch.float32), w, h)["tiles"]
    return dict(block=block, ranges=ranges, cams=cams, w=w, h=h, tiles=torch.cat([tiles[f:f + c] for f, c in ranges]))


def _pairs_of(rec, w, h):
    """The (splat, tile) pairs of record rows as the kernels count them: the tiles of a row's rectangle (tile_rect) that its
    alpha >= 1/255 disc reaches (tile_hit2) -- float32, one rounding per operation, as both are compiled."""
    gx, gy = MO.tile_grid(w, h)
    rad = rec[:, 11].contiguous().view(torch.int32)
    x0, x1, y0, y1 = (t.unsqueeze(1) for t in MO.tile_rect(rec[:, 0:2], rad, w, h))
    tx, ty = torch.arange(gx).repeat(gy).unsqueeze(0), torch.arange(gy).repeat_interleave(gx).unsqueeze(0)
    in_rect = (rad > 0).unsqueeze(1) & (tx >= x0) & (tx < x1) & (ty >= y0) & (ty < y1)
    tx, ty, cutoff = tx.float(), ty.float(), rec[:, 10:11]
    gu, gv = rec[:, 0:1] - MO.PIXEL_CENTER, rec[:, 1:2] - MO.PIXEL_CENTER
    ddx = torch.maximum(torch.maximum(tx * 16.0 - gu, gu - (tx * 16.0 + 15.0)), torch.zeros(1))
    ddy = torch.maximum(torch.maximum(ty * 16.0 - gv, gv - (ty * 16.0 + 15.0)), torch.zeros(1))
    return int((in_rect & (ddx * ddx + ddy * ddy <= cutoff)).sum())


def test_rectangles_the_whole_wave_walks():
    """Splats of more than 16 tiles are walked by their wave, 64 tiles a trip (walk_tiles_wave, gfl_fit.hpp); every other scene
    of this file stays at 3 x 3 tiles.  A (splat, tile) pair the walk loses moves up to 256 of the 20 160 pixels by up to 0.3."""
    wj = wide_walk_jobs()
    block, ranges, cams, w, h, tiles = (wj[k] for k in ("block", "ranges", "cams", "w", "h", "tiles"))
    # ---- what the scene has to hold for this test to test anything, from the oracle alone
    assert (w, h, block.shape[0], tiles.numel()) == (168, 120, 1668, 1831)
    assert bool((tiles == 16).any()) and bool(((tiles >= 17) & (tiles <= 32)).any()) and bool((tiles > 32).any())
    row = torch.arange(tiles.numel())
    wide = tiles > 16
    assert bool((wide & (row % 64 == 0)).any()), "no wave-walked row on the first lane of a wave"
    assert bool((wide & (row % 64 == 63)).any()), "no wave-walked row on the last lane of a wave"
    assert int(torch.bincount(row[wide] // 64).max()) >= 2, "no wave walks two rectangles"
    # ---- the device
    got = run_batch(block, ranges, cams, w=w, h=h)
    assert got["rc"] == 0 and got["overflow"].tolist() == [0, 0]
    bits = lambda t: t.contiguous().view(torch.int32)
    for j, ((f, c), cam) in enumerate(zip(ranges, cams)):
        ref = _oracle(block[f:f + c], cam, w, h)
        tag = f"render_batch, wave-walked rectangles, job {j}: "
        close_frac(got["f32"][j, :3], ref["rgb"], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=tag + "rgb")
        close_frac(got["f32"][j, 3:4], ref["depth_map"], 1e-4, 1e-5, bad_frac=3e-4, hard=2e-2, what=tag + "depth_map")
        rec = _rec_rows(got, ranges, j)
        close_frac(rec[:, 0:2], ref["uv"], 1e-5, 1e-3, what=tag + "uv")
        close_frac(rec[:, 9:10], ref["depth"], 1e-6, 1e-6, what=tag + "depth")
        solo = run_batch(block, [ranges[j]], [cam], w=w, h=h)
        assert solo["rc"] == 0
        assert torch.equal(bits(solo["f32"][0]), bits(got["f32"][j])), f"job {j} alone"
        assert torch.equal(solo["u8"][0], got["u8"][j])
        assert torch.equal(bits(solo["rec"]), bits(rec))
    # ---- a pair pool one pair short: the cut falls inside job 1
    total = _pairs_of(got["rec"], w, h)
    exact = run_batch(block, ranges, cams, w=w, h=h, K_cap=total)
    assert exact["rc"] == 0 and exact["overflow"].tolist() == [0, 0], f"the call has more than {total} pairs"
    tight = run_batch(block, ranges, cams, w=w, h=h, K_cap=total - 1)
    assert tight["rc"] == 0 and tight["overflow"].tolist() == [0, 1], f"the call has fewer than {total} pairs"
    assert torch.equal(bits(tight["f32"][0]), bits(got["f32"][0])) and torch.equal(tight["u8"][0], got["u8"][0])
    again = run_batch(block, ranges, cams, w=w, h=h, K_cap=total - 1)
    assert torch.equal(bits(again["f32"]), bits(tight["f32"])) and torch.equal(again["u8"], tight["u8"]), "a truncated job is reproducible too"


def test_a_captured_call_renders_what_the_camera_tensor_holds_at_the_replay():
    import gflow_amd.render as R
    a = random_scene(3000, W, H, seed=11, sigma_px=2.5)
    gs = {k: a[k].to(DEV) for k in NAMES}
    intr = a["intr"].to(DEV)

    def three(d):
        out = []
        for k in range(3):
            e = a["extr"].clone()
            e[:, 3] += torch.tensor([d * (k + 1), -0.5 * d * k, 0.0])
            out.append(e)
        return torch.stack(out).to(DEV)
    extr = three(0.05)
    cams = dict(intr=intr, extr=extr, W=W, H=H)
    first = R.render_views(gs, cams, bg=1.0, uint8=True)["img"].clone()       # (eager: the workspace exists from here on)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = R.render_views(gs, cams, bg=1.0, uint8=True)["img"]
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    other = three(-0.08)
    extr.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = R.render_views(gs, dict(intr=intr, extr=other, W=W, H=H), bg=1.0, uint8=True)["img"]
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, first)
    R.check_overflow()


def test_python_layer_views_jobs_split_overflow_and_the_pool(four_jobs):
    import gflow_amd.render as R
    a = random_scene(3000, W, H, seed=11, sigma_px=2.5)
    gs = {k: a[k].to(DEV) for k in NAMES}
    cam = dict(intr=a["intr"].to(DEV), extr=a["extr"].to(DEV), W=W, H=H)
    before = R.render(gs, cam, 0.33)
    before = {k: v.clone() for k, v in before.items()}
    # stacked tensors and a list of dicts
    extrs = torch.stack([a["extr"], four_jobs["cams"][1][4:16].reshape(3, 4)]).to(DEV)
    stacked = R.render_views(gs, dict(intr=cam["intr"], extr=extrs, W=W, H=H), bg=0.33, records=True)
    listed = R.render_views(gs, [dict(intr=cam["intr"], extr=extrs[k], W=W, H=H) for k in range(2)], bg=0.33, records=True)
    for k in ("rgb", "depth_map", "uv", "depth"):
        assert torch.equal(stacked[k], listed[k]), k
    assert stacked["rgb"].shape == (2, 3, H, W) and stacked["depth_map"].shape == (2, 1, H, W)
    assert stacked["uv"].shape == (2, 3000, 2) and stacked["depth"].shape == (2, 3000, 1)
    # the library call's own numbers (job 0 of the fixture has this camera and background)
    assert torch.equal(stacked["rgb"][0].cpu().view(torch.int32), four_jobs["got"]["f32"][0, :3].view(torch.int32))
    img = R.render_views(gs, dict(intr=cam["intr"], extr=extrs, W=W, H=H), bg=0.33, uint8=True)["img"]
    assert img.dtype == torch.uint8 and img.shape == (2, H, W, 3) and torch.equal(img[0], R.render2img_device(stacked["rgb"][0]))
    # render_jobs: ragged sets, per-job backgrounds, split into two calls by a lowered limit
    g2 = camera_scene(1500, W, H, "general", seed=11, sigma_px=2.5)
    sets = [gs, {k: g2[k].to(DEV) for k in NAMES}, {k: gs[k][100:1300] for k in NAMES}]
    cams3 = [cam, dict(intr=g2["intr"].to(DEV), extr=g2["extr"].to(DEV), W=W, H=H), cam]
    whole = R.render_jobs(sets, cams3, bg=[0.33, 0.33, 1.0], records=True)
    assert torch.equal(whole["rgb"][1].cpu().view(torch.int32), four_jobs["got"]["f32"][2, :3].view(torch.int32))
    assert torch.equal(whole["rgb"][2].cpu().view(torch.int32), four_jobs["got"]["f32"][3, :3].view(torch.int32))
    assert [tuple(u.shape) for u in whole["uv"]] == [(3000, 2), (1500, 2), (1200, 2)]
    calls = []
    lib = R.L.load()
    orig = lib.gfl_render_batch
    keep = R.BATCH_MAX_JOBS

    def spy(*args):
        calls.append(args[4])
        return orig(*args)
    try:
        R.BATCH_MAX_JOBS = 2
        lib.gfl_render_batch = spy
        split = R.render_jobs(sets, cams3, bg=[0.33, 0.33, 1.0], records=True)
    finally:
        R.BATCH_MAX_JOBS = keep
        lib.gfl_render_batch = orig
    assert calls == [2, 1]
    for k in ("rgb", "depth_map"):
        assert torch.equal(split[k], whole[k]), k
    for k in ("uv", "depth"):
        assert all(torch.equal(x, y) for x, y in zip(split[k], whole[k])), k
    R.check_overflow()
    # an overflowing call raises at check_overflow(), once
    R.render_views(gs, dict(intr=cam["intr"], extr=extrs, W=W, H=H), K_cap=2000)
    with pytest.raises(RuntimeError, match="lost splat-tile pairs"):
        R.check_overflow()
    R.check_overflow()
    # ... or at the next batched call
    R.render_views(gs, dict(intr=cam["intr"], extr=extrs, W=W, H=H), K_cap=2000)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="lost splat-tile pairs"):
        R.render_views(gs, dict(intr=cam["intr"], extr=extrs, W=W, H=H))
    R.check_overflow()
    # render() is what it was: the pool is not disturbed
    after = R.render(gs, cam, 0.33)
    for k in before:
        assert torch.equal(after[k].view(torch.int32), before[k].view(torch.int32)), k
    R.check_overflow()


def test_viewer_end_to_end(tmp_path):
    import gflow_amd.render as R
    from gflow_amd import synthetic as S
    from gflow_amd import viewer as V
    from gflow_amd.trainer import SimpleGaussian
    from PIL import Image
    clip = S.make_clip(2, H=64, W=96, seed=5)
    for k, frame in enumerate(clip):
        tr = SimpleGaussian(frame["image"], frame["depth"], num_points=800, device=DEV, seed=k, log_dir=str(tmp_path))
        tr.load_camera(focal=frame["focal"], pp=frame["pp"], extr=frame["extr_gt"])
        tr.init_gaussians_from_image(frame["image"], frame["depth"], num_points=800)
        tr.train(iterations=8, lr=4e-3, lr_camera=1e-3, lambda_rgb=1.0, lambda_depth=0.1, lambda_var=10.0,
                 move_mask=frame["move_mask"], densify_interval=6, densify_times=1, snapshot_interval=0)
        tr.save_checkpoint(ckpt_name=f"{k:04d}")
    session = V.ViewerSession(str(tmp_path), DEV)
    assert len(session) == 2 and (session.W, session.H) == (96, 64) and session.bg == 1.0
    frames = []
    for t, f in enumerate(session.files):
        xyz, scale, rotate, opacity, rgb, intr, extr = V.load_ckpt(f, DEV)
        ref = R.render2img_device(R.render_multiple([xyz, scale, rotate, opacity, rgb, intr, extr, 1.0, 96, 64], ["rgb"])["rgb"])
        img = session.frame(t)
        assert img.shape == (64, 96, 3) and img.dtype == torch.uint8 and img.is_cuda
        assert session.n_gaussians == xyz.shape[0] and session.fps > 0
        d = (img.int() - ref.int()).abs()
        share = float((d != 0).float().mean())
        observe(f"viewer frame {t}: {share:.2e} of the bytes differ from render_multiple + render2img (allowed 3.0e-04), max {int(d.max())} level(s)")
        assert int(d.max()) <= 1 and share <= 3e-4
        assert len(set(img.reshape(-1).tolist())) > 30
        frames.append(img)
    assert torch.equal(session.play(V.follow(session.extrs)), torch.stack(frames))
    orbit = V.orbit(session.extrs[1], 5, 0.05, session.look_at_depth(1))
    views = session.views(1, orbit.to(DEV))
    assert views.shape == (5, 64, 96, 3)
    assert all(not torch.equal(views[i], views[j]) for i in range(5) for j in range(i))
    assert torch.equal(session.frame(1, orbit[2]), views[2])
    R.check_overflow()
    out = tmp_path / "orbit"
    assert V.main(["--folder", str(tmp_path), "--path", "orbit:1,5,0.05", "--out", str(out)]) == 0
    assert sorted(os.listdir(out)) == [f"{k:06d}.png" for k in range(5)]
    for k in range(5):
        assert np.array_equal(np.asarray(Image.open(out / f"{k:06d}.png")), views[k].cpu().numpy())
    out2 = tmp_path / "follow"
    assert V.main(["--folder", str(tmp_path), "--path", "follow", "--out", str(out2), "--format", "jpeg"]) == 0
    assert sorted(os.listdir(out2)) == ["000000.jpeg", "000001.jpeg"]
