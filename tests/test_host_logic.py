"""CPU: host-side pieces of the path -- sampler, geometry, pose helpers, synthetic inputs,
clip sharding and the end-of-job reduction over a 2-rank gloo group."""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import loss_oracle as LO


def test_sobel_and_sampler_follow_gradient_magnitude():
    from gflow_amd.sampling import _sobel, complex_texture_sampling
    ramp = np.tile(np.arange(8, dtype=np.float32) * 3.0, (6, 1))
    gx, gy = _sobel(ramp)
    assert np.allclose(gx[:, 1:-1], 24.0) and np.allclose(gy, 0.0)
    assert np.allclose(gx[:, 0], 0.0)                         # REFLECT_101 border: zero x-derivative at the edge
    # a faint ramp (tiny gradient everywhere, so the reference's "min positive" floor is tiny)
    # plus one strong vertical edge
    img = (torch.arange(48).float() * 1e-4).reshape(1, 48, 1).repeat(32, 1, 3)
    img[:, 24:] += 0.9
    depth = torch.full((32, 48, 1), 2.0)
    xys, d, sc, rgb, _ = complex_texture_sampling(img, depth, 4000, rng=np.random.default_rng(0))
    assert xys.shape == (4000, 2) and d.shape == (4000, 1) and rgb.shape == (4000, 3)
    near_edge = np.abs(xys[:, 0] - 23.5) <= 1.0
    assert near_edge.mean() > 0.9                              # samples concentrate on the edge
    assert abs(sc.sum() - 100.0) < 1e-6


def test_device_sampler_draws_from_the_same_distribution():
    """sampling.complex_texture_sampling_device (what the trainer uses: no host round trip) against the host version:
    the same probability map to rounding, samples that follow it, the same derived quantities."""
    from gflow_amd import synthetic as S
    from gflow_amd.sampling import _probability, complex_texture_sampling_device, texture_probability_device
    fr = S.make_frame(40, 56, seed=5)
    image = fr["image"].numpy() * 255
    gray = (0.299 * image[..., 0] + 0.587 * image[..., 1] + 0.114 * image[..., 2]).astype(np.float32)
    want = _probability(gray)
    got = texture_probability_device(fr["image"]).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-15)
    n = 200000
    xys, depths, scales, rgbs = complex_texture_sampling_device(fr["image"], fr["depth"], n,
                                                                generator=torch.Generator().manual_seed(0))
    assert xys.shape == (n, 2) and depths.shape == (n, 1) and rgbs.shape == (n, 3) and scales.shape == (n,)
    flat = (xys[:, 1] * 56 + xys[:, 0]).numpy()
    counts = np.bincount(flat, minlength=40 * 56).astype(np.float64)
    expected = want.flatten() * n
    chi2 = ((counts - expected) ** 2 / expected).sum()
    dof = 40 * 56 - 1
    assert abs(chi2 - dof) < 6 * math.sqrt(2 * dof), (chi2, dof)              # a chi-square statistic: mean dof, sd sqrt(2 dof)
    assert torch.equal(depths, fr["depth"][xys[:, 1], xys[:, 0]])
    np.testing.assert_allclose(rgbs.numpy(), fr["image"][xys[:, 1], xys[:, 0]].numpy(), atol=1e-6)
    assert abs(float(scales.sum()) - 100.0) < 1e-6
    np.testing.assert_allclose(scales.numpy() * (1.0 / want.flatten()[flat]).sum() / 100.0, 1.0 / want.flatten()[flat], rtol=1e-6)


def test_native_concave_hull_is_the_numpy_statement_of_the_algorithm():
    """gfl_concave_hull (csrc/gfl_hull.hip, host C++) against hull.concave_hull_py, the numpy statement it was written from:
    the same ring, vertex for vertex, on uniform clouds, clustered clouds, an L shape, a ring, collinear and tiny inputs."""
    from gflow_amd.hull import concave_hull, concave_hull_py
    rng = np.random.default_rng(4)
    cases = [rng.uniform(0, 100, (n, 2)) for n in (4, 5, 17, 300, 2000)]
    blob = np.concatenate([rng.normal((30, 40), 6, (800, 2)), rng.normal((70, 45), 3, (400, 2)), rng.uniform(0, 100, (50, 2))])
    cases.append(blob)
    ell = rng.uniform(0, 100, (3000, 2))
    cases.append(ell[~((ell[:, 0] > 40) & (ell[:, 1] > 40))])
    ang = rng.uniform(0, 2 * np.pi, 1500)
    cases.append(np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(30, 40, (1500, 1)) + 50)
    cases.append(np.stack([np.arange(10.0), 2 * np.arange(10.0)], 1))                      # collinear
    cases.append(np.round(rng.uniform(0, 20, (500, 2))))                                   # integer pixels: duplicates, ties
    cases += [np.zeros((0, 2)), np.array([[1.0, 2.0]]), np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])]
    for pts in cases:
        a, b = concave_hull(pts), concave_hull_py(pts)
        assert a.shape == b.shape and np.array_equal(a, b), (len(pts), a.shape, b.shape)
    # (what the host function buys -- 125 -> 8 ms per clip -- is a measurement; no wall-clock assert in a
    #  correctness test: ADVICE r05)


def test_concave_hull_properties():
    """gflow_amd/hull.py -- the moving-region mask of trainer.py:604-609.  The ring cannot be pinned to the reference's
    ``concave_hull`` package (absent), so it is held to what a concave hull must satisfy: it keeps (nearly) every point
    inside, never leaves the convex hull, and follows a concavity the convex hull bridges."""
    from gflow_amd.hull import FastConcaveHull2D, _convex_hull, concave_hull, gaussian_smooth, polygon_to_mask
    g = np.random.default_rng(0)

    def area(r):
        x, y = r[:, 0], r[:, 1]
        return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(np.roll(x, -1), y))

    pts = g.uniform(0, 100, (5000, 2))
    pts = pts[~((pts[:, 0] > 40) & (pts[:, 1] > 40))]                    # an L: true area 6 400, convex hull ~8 100
    ring = concave_hull(pts)
    conv = pts[_convex_hull(pts)]
    assert 5600 < area(ring) < 6500 and area(conv) > 7800
    ring_set = {tuple(p) for p in ring}
    assert all(tuple(p) in {tuple(q) for q in pts} for p in ring)        # vertices are input points, each once
    assert len(ring_set) == len(ring)
    raw_mask = polygon_to_mask(ring, 128, 128)
    assert raw_mask[pts[:, 1].astype(int), pts[:, 0].astype(int)].mean() > 0.99
    assert raw_mask[70:95, 70:95].sum() == 0                             # the notch of the L stays outside
    conv_mask = polygon_to_mask(conv, 128, 128)
    assert not bool(((raw_mask == 1) & (conv_mask == 0)).any())         # never outside the convex hull
    h = FastConcaveHull2D(torch.from_numpy(pts))
    m = h.mask(128, 128)
    assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1} and m.shape == (128, 128)
    assert m[pts[:, 1].astype(int), pts[:, 0].astype(int)].mean() > 0.98 and abs(h.area() - area(ring)) < 0.03 * area(ring)
    # the smoothing step by itself (concave_hull.py:19-29): twice the vertices, a wrapped filter keeps the centroid
    sq = np.array([[0, 0], [10, 0], [10, 10], [0, 10], [0, 0]], dtype=float)
    x, y = gaussian_smooth(sq)
    assert len(x) == 10 and abs(x.mean() - np.interp(np.linspace(0, 1, 10), np.linspace(0, 1, 5), sq[:, 0]).mean()) < 1e-9
    # a convex cloud: the concave hull stays close to the convex one
    disc = g.normal(size=(3000, 2))
    disc = disc[(disc ** 2).sum(1) < 4] * 20 + 50
    assert area(concave_hull(disc)) > 0.9 * area(disc[_convex_hull(disc)])


def test_pix2world_matches_golden(golden_dir):
    from gflow_amd.geometry import pix2world
    g = np.load(os.path.join(golden_dir, "pix2world.npz"))
    uv, d, intr = (torch.from_numpy(g[k]) for k in ("uv", "depth", "intr"))
    for e, o in (("extr_id", "xyz_id"), ("extr_rt", "xyz_rt")):
        np.testing.assert_allclose(pix2world(uv, d, intr, torch.from_numpy(g[e])).numpy(), g[o], rtol=1e-5, atol=1e-6)


def test_pose_helpers_agree_with_the_oracle():
    from gflow_amd.trainer import pose_to_extr, rotmat_to_unitquat_xyzw
    pose = torch.tensor([0.1, -0.2, 0.3, 0.9, 0.5, -0.4, 0.2])
    e = pose_to_extr(pose)
    np.testing.assert_allclose(e.numpy(), LO.pose_to_extr(pose).numpy(), atol=1e-7)
    R = e[:, :3]
    np.testing.assert_allclose((R @ R.T).numpy(), np.eye(3), atol=1e-6)
    q = rotmat_to_unitquat_xyzw(R)
    qn = pose[:4] / pose[:4].norm()
    assert min((q - qn).abs().max().item(), (q + qn).abs().max().item()) < 1e-6
    ident = pose_to_extr(torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]))
    np.testing.assert_allclose(ident.numpy(), np.eye(4)[:3], atol=0)


def test_synthetic_inputs_are_seeded_and_well_formed():
    from gflow_amd import synthetic as S
    a, b = S.make_frame(48, 64, seed=3), S.make_frame(48, 64, seed=3)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["depth"], b["depth"])
    assert a["image"].shape == (48, 64, 3) and 0.0 <= a["image"].min() and a["image"].max() <= 1.0
    assert a["depth"].shape == (48, 64, 1) and 1.0 <= a["depth"].min() and a["depth"].max() <= 5.0
    assert a["flow"].shape == (48, 64, 2) and a["move_mask"].dtype == torch.bool
    sp = S.init_splats(a, 500, seed=1)
    assert sp["xyz"].shape == (500, 3) and sp["rotate"].shape == (500, 4)
    assert torch.allclose(torch.sigmoid(10 * sp["opacity"]), torch.full((500, 1), 0.99), atol=1e-5)
    assert (sp["scale"] <= 1e-3 + 1e-9).all()                 # trainer.py:225 clamp
    assert not torch.equal(S.make_frame(48, 64, seed=4)["image"], a["image"])


def test_shard_partitions_clips():
    from gflow_amd.fit_video import shard
    for world in (1, 2, 3, 8):
        parts = [shard(11, r, world) for r in range(world)]
        assert sorted(sum(parts, [])) == list(range(11))
        assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    assert [shard(8, r, 4) for r in range(4)] == [[0, 4], [1, 5], [2, 6], [3, 7]]       # equal lengths: i mod world


def test_shard_balances_clips_of_unequal_length():
    """Longest-processing-time-first on the frame counts: the most loaded rank ends within one (longest) clip of the
    ideal, and much closer than i mod world on an adversarial order."""
    import random
    from gflow_amd.fit_video import shard
    rng = random.Random(0)
    for world in (2, 4, 8):
        for trial in range(20):
            lengths = [rng.choice([8, 20, 40, 60, 80, 100]) for _ in range(rng.randint(world, 5 * world))]
            parts = [shard(len(lengths), r, world, lengths) for r in range(world)]
            assert sorted(sum(parts, [])) == list(range(len(lengths)))
            loads = [sum(lengths[i] for i in p) for p in parts]
            assert max(loads) - min(loads) <= max(lengths)
            assert max(loads) <= sum(lengths) / world + max(lengths)
    # long clips at every world-th position: i mod world puts them all on rank 0
    lengths = [100, 10, 10, 10] * 4
    naive = max(sum(lengths[i] for i in range(16) if i % 4 == r) for r in range(4))
    lpt = max(sum(lengths[i] for i in shard(16, r, 4, lengths)) for r in range(4))
    assert naive == 400 and lpt == 130


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from gflow_amd.fit_video import METRIC_NAMES, reduce_metrics, shard
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    clips = shard(5, rank, world)
    local = dict(psnr_sum=30.0 * len(clips), frames=4 * len(clips), iterations=100 * len(clips),
                 rasterisations=110 * len(clips), clips=len(clips), splats_final=1000 * (rank + 1))
    out = reduce_metrics(local, wall_seconds=1.0 + rank, dist=dist, rank=rank, world=world)
    dist.destroy_process_group()
    q.put((rank, out))


def test_two_rank_gloo_reduction():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        o = outs[r]
        assert o["clips"] == 5 and o["frames"] == 20 and o["iterations"] == 500 and o["psnr_sum"] == 150.0
        assert o["wall_s"] == 2.0                               # MAX over ranks
        assert o["rank_wall_s"] == [1.0, 2.0]                   # every rank's own time, from the same SUM
        assert o["splats_final"] == 3000


def _bench_worker(rank, world, port, q):
    import argparse
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    args = argparse.Namespace(steps=100, warmup=10, clip_frames=8, snapshot_interval=10)
    # per-rank numbers as two different scenes would produce them
    local = {"elapsed": 0.020 + 0.005 * rank, "steps": 100, "psnr_step": 30.0 + rank, "K": 240000 + 20000 * rank,
             "clip": dict(frames=8, iterations=3650, rasterisations=4700, psnr_sum=8 * (33.0 + rank), splats_final=67000 + 2000 * rank),
             "clip_wall": 1.0 + 0.25 * rank, "kernels_ms": {"blend_bwd": 0.070, "blend_fwd": 0.035}, "stage_ms": {}}
    out = bench.reduce_and_report(local, dist, torch.device("cpu"), rank, world, args, "gloo", size=(480, 854, 60000))
    dist.destroy_process_group()
    q.put((rank, out))


def test_bench_reduction_under_two_rank_gloo():
    """bench.py's N > 1 line: K is the MEAN of the ranks' pair counts (round 2 divided rank 0's own K by the world
    size), value = frames of all ranks / slowest rank's clip time, the end-to-end rate counts every rank's bytes."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_bench_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert outs[1] is None
    o = outs[0]
    assert o["n_gpus"] == 2 and o["scaling"] == "weak" and o["config"]["collective_backend"] == "gloo"
    assert o["config"]["splat_tile_pairs_K"] == 250000.0
    assert abs(o["value"] - 16 / 1.25) < 1e-9                                # 2 x 8 frames / slowest clip fit
    assert abs(o["ms_per_step"] - 0.25) < 1e-9                                # slowest rank: 25 ms / 100 steps
    assert abs(o["iterations_per_s"] - 200 / 0.025) < 1e-6
    bytes_it = 724 * 60000 + 124 * 250000.0 + 96 * 480 * 854
    assert abs(o["end_to_end_algorithmic_GBps"] - bytes_it * 8000.0 / 1e9) < 1e-6
    assert abs(o["end_to_end_algorithmic_GBps_per_gpu"] - bytes_it * 4000.0 / 1e9) < 1e-6
    assert abs(o["clip_fit"]["psnr_mean_db"] - 33.5) < 1e-9 and o["clip_fit"]["splats_final_mean"] == 68000.0
    assert o["clip_fit"]["rank_wall_s"] == [1.0, 1.25] and o["clip_fit"]["clips_per_rank"] == 1
    # the roofline block describes rank 0's kernels on rank 0's scene
    assert o["roofline"]["kernel"] == "blend_bwd"
    want = (44 * 240000 + 24 * 480 * 854 + 40 * 60000) / 0.070e-3 / 1e9
    assert abs(o["roofline"]["achieved"] - want) < 1e-6 and abs(o["roofline"]["frac"] - want / 8000.0) < 1e-9


def test_readers_match_the_reference_on_the_same_files(tmp_path, golden_dir):
    """gflow_amd/io.py against what the REFERENCE's read_flow / read_depth / read_camera (gflow/utils/read.py:7-38,
    60-89) returned for the very same files: tests/golden/readers.npz keeps the files' bytes and the reference's
    outputs (tests/golden/make_golden.py: readers_fixture)."""
    import json
    from gflow_amd import io as gio
    g = np.load(os.path.join(golden_dir, "readers.npz"))

    def put(name, key):
        path = str(tmp_path / name)
        g[key].tofile(path)
        return path

    flow = gio.read_flow(put("a_pred.flo", "flo_bytes"))
    assert flow.dtype == torch.float32 and tuple(flow.shape) == (5, 7, 2)
    assert np.array_equal(flow.numpy(), g["flow"]) and np.signbit(flow.numpy()[0, 0, 0])      # bit-exact, -0.0 kept
    assert gio.read_flow(put("bad.flo", "flo_bad_bytes")) is None                             # read.py:15-18
    npy = put("00000.npy", "depth_npy_bytes")
    d = gio.read_depth(npy)
    assert d.dtype == torch.float32 and np.array_equal(d.numpy(), g["depth"])
    assert np.array_equal(gio.read_depth(npy, depth_scale=0.5, depth_offset=0.25).numpy(), g["depth_scaled"])
    paths = []
    for i, txt in enumerate(g["camera_json"]):
        paths.append(str(tmp_path / f"{i:05d}.json"))
        with open(paths[-1], "w") as f:
            f.write(str(txt))
    focal, pp, poses = gio.read_camera(paths)
    assert isinstance(focal, float) and focal == float(g["focal"])
    assert pp == g["pp"].tolist() == [428, 240]                       # the LAST file's, python round (halves to even)
    assert poses.shape == (3, 3, 4) and np.array_equal(poses, g["poses"])
    f2, pp2, _ = gio.read_camera(paths[:2])
    assert f2 == float(g["focal_first_two"]) and pp2 == g["pp_first_two"].tolist() == [428, 240]
    assert json.loads(str(g["camera_json"][1]))["pp"] == [427.5, 240.49]


def test_sequence_readers_round_trip(tmp_path):
    """gflow_amd.io: the reference's on-disk convention (fit_video.py:79-99, read.py, conversion.py)."""
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    frames = S.make_clip(3, 48, 80, seed=2)
    seq = gio.write_sequence(frames, str(tmp_path / "clip"))
    p = gio.sequence_paths(seq)
    assert [len(p[k]) for k in ("img", "depth", "flow", "occ", "move", "camera")] == [2, 2, 2, 1, 2, 2]   # frame_range = n-1
    back = gio.load_sequence(seq, frame_range=3)
    assert len(back) == 3
    for a, b in zip(frames, back):
        assert b["image"].shape == (48, 80, 3) and b["depth"].shape == (48, 80, 1)
        assert (b["image"] - a["image"].float()).abs().max() <= 0.5 / 255 + 1e-6
        assert torch.equal(b["depth"].squeeze(-1), a["depth"].squeeze(-1).float())
        assert torch.equal(b["move_mask"], a["move_mask"].bool())
        assert b["focal"] == a["focal"] and list(b["pp"]) == list(a["pp"])
    assert torch.equal(back[0]["flow"], frames[0]["flow"].float())
    assert torch.equal(back[1]["flow"], frames[1]["flow"].float())
    assert "occ_mask" in back[1] and "occ_mask" not in back[0]
    # .flo with a wrong magic number is rejected the way read.py:15-18 does
    bad = tmp_path / "bad.flo"
    np.array([1.0], np.float32).tofile(str(bad))
    assert gio.read_flow(str(bad)) is None
    # Resize(n): the shorter side becomes n, aspect kept (torchvision semantics)
    half = gio.load_sequence(seq, resize=24, frame_range=3)
    assert half[0]["image"].shape == (24, 40, 3) and half[0]["flow"].shape == (24, 40, 2)
    assert half[0]["move_mask"].shape == (24, 40) and half[0]["depth"].shape == (24, 40, 1)


# ---------------------------------------------------------------- hand-worked fixtures (cv2 / torchvision are absent)
def test_sobel_of_the_init_sampler_on_hand_worked_images():
    """cv2.Sobel(gray, CV_64F, 1, 0, ksize=3) / (0, 1) with OpenCV's default BORDER_REFLECT_101
    (complex_texture_sampling.py:13-14), worked out by hand:
    * a ramp g[y][x] = 10 x: away from the left / right border gx = (1 + 2 + 1) * (g[x+1] - g[x-1]) = 4 * 20 = 80;
      in the first and last column the mirrored neighbour is the inner one itself (REFLECT_101), so gx = 0; gy = 0;
    * a single bright pixel of height 1: gx is the kernel mirrored around it, [[1,0,-1],[2,0,-2],[1,0,-1]], and gy
      [[1,2,1],[0,0,0],[-1,-2,-1]]."""
    import numpy as np
    from gflow_amd.sampling import _sobel
    ramp = np.tile(10.0 * np.arange(6), (5, 1))
    gx, gy = _sobel(ramp)
    want = np.full((5, 6), 80.0)
    want[:, 0] = 0.0
    want[:, -1] = 0.0
    assert np.array_equal(gx, want) and np.array_equal(gy, np.zeros((5, 6)))
    gx, gy = _sobel(ramp.T.copy())
    assert np.array_equal(gy, want.T) and np.array_equal(gx, np.zeros((6, 5)))
    imp = np.zeros((5, 5))
    imp[2, 2] = 1.0
    gx, gy = _sobel(imp)
    assert np.array_equal(gx[1:4, 1:4], np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=float))
    assert np.array_equal(gy[1:4, 1:4], np.array([[1, 2, 1], [0, 0, 0], [-1, -2, -1]], dtype=float))
    assert gx[0].sum() == 0 and gx[:, 0].sum() == 0


def test_init_sampler_weights_and_outputs_on_a_hand_worked_image():
    """complex_texture_sampling.py:6-47 on a 4x6 image whose grey level is the ramp above (R = G = B = x / 25.5, so
    gray * 255 = 10 x up to rounding): probability = (|grad| + min positive) / sum = 160 in the interior columns,
    80 in the border columns (the floor alone); scales_norm = 100 / p / sum(1 / p) over the samples; xys are (x, y)."""
    import numpy as np
    import torch
    from gflow_amd.sampling import complex_texture_sampling
    x = torch.arange(6).float() / 25.5
    img = x.reshape(1, 6, 1).repeat(4, 1, 3)
    depth = (1.0 + torch.arange(24).float().reshape(4, 6, 1) / 10.0)
    xys, depths, scales_norm, rgbs, _ = complex_texture_sampling(img, depth, num_points=4000, rng=np.random.default_rng(0))
    assert xys.shape == (4000, 2) and xys[:, 0].max() <= 5 and xys[:, 1].max() <= 3
    # interior columns are drawn twice as often as border columns: 4 x 160 : 2 x 80 per row
    border = np.isin(xys[:, 0], (0, 5)).mean()
    assert abs(border - 160.0 / 800.0) < 0.03
    inv_p = np.where(np.isin(xys[:, 0], (0, 5)), 1.0 / 80.0, 1.0 / 160.0)
    np.testing.assert_allclose(scales_norm, 100.0 * inv_p / inv_p.sum(), rtol=1e-4)
    np.testing.assert_allclose(depths.squeeze(-1).numpy(), 1.0 + (xys[:, 1] * 6 + xys[:, 0]) / 10.0, rtol=1e-6)
    np.testing.assert_allclose(rgbs[:, 0], xys[:, 0] / 25.5, rtol=1e-5)


def test_resize_antialias_on_a_hand_worked_row():
    """transforms.Resize(n, antialias=True) on a tensor is bilinear interpolation with a triangle filter widened by
    the scale factor (conversion.py:11-12).  Halving a row of 8 pixels: output i is centred at 2 i + 1, its filter
    max(0, 1 - |j + 0.5 - c| / 2) covers the inputs j = 2i-1 .. 2i+2 with weights 0.25, 0.75, 0.75, 0.25, renormalised
    where the window leaves the image (first / last output: 0.75, 0.75, 0.25 over 1.75)."""
    import torch
    from gflow_amd.io import _resize_chw
    row = torch.tensor([0.0, 1.0, 4.0, 9.0, 16.0, 25.0, 36.0, 49.0])
    img = row.reshape(1, 1, 8).repeat(1, 8, 1)                         # (C=1, H=8, W=8), constant along y
    out = _resize_chw(img, 4)
    assert out.shape == (1, 4, 4)
    w_edge, w_mid = torch.tensor([0.75, 0.75, 0.25]) / 1.75, torch.tensor([0.25, 0.75, 0.75, 0.25]) / 2.0
    want = torch.stack([(w_edge * row[0:3]).sum(), (w_mid * row[1:5]).sum(), (w_mid * row[3:7]).sum(),
                        (w_edge.flip(0) * row[5:8]).sum()])
    for y in range(4):
        assert torch.allclose(out[0, y], want, atol=1e-5), (out[0, y], want)
    # the shorter side goes to n, the longer keeps the aspect ratio with int() truncation (torchvision's rule)
    assert _resize_chw(torch.zeros(3, 10, 25), 4).shape == (3, 4, 10)
    assert _resize_chw(torch.zeros(3, 25, 10), 4).shape == (3, 10, 4)
    assert _resize_chw(torch.zeros(3, 480, 854), 480).shape == (3, 480, 854)      # DAVIS 480p: a no-op


def test_gen_line_set_equals_the_reference_function(golden_dir):
    """tests/golden/line_set.npz was captured from gflow/utils/trainer_functions.py:5-40 (make_golden.py)."""
    import os
    import numpy as np
    import torch
    from gflow_amd.trajectory import gen_line_set
    d = np.load(os.path.join(golden_dir, "line_set.npz"))
    lx, lc = gen_line_set(torch.from_numpy(d["xyz1"]), torch.from_numpy(d["xyz2"]), torch.from_numpy(d["rgb"]))
    assert np.array_equal(lx.numpy(), d["line_xyz"]) and np.array_equal(lc.numpy(), d["line_rgb"])


def test_cu_partition_masks_are_disjoint_shares_of_every_xcd():
    """_lib.cu_partition: mask bit i = CU i // 8 of XCD i % 8 (tools/cumask_probe.hip); every share must keep CUs in ALL eight
    XCDs (a mask that empties an XCD is not honoured by the driver) and the shares must not overlap."""
    from gflow_amd import _lib
    for parts in (2, 3, 4):
        shares = _lib.cu_partition(parts, cus=256)
        seen = 0
        for words, n in shares:
            bits = sum(w << (32 * k) for k, w in enumerate(words))
            assert bin(bits).count("1") == n == 8 * (32 // parts)
            assert n % 8 == 0                                            # one tile queue per CU, eight XCD bands
            for x in range(8):
                assert sum((bits >> (cu * 8 + x)) & 1 for cu in range(32)) == 32 // parts
            assert bits & seen == 0
            seen |= bits


def test_bench_window_report_and_clip_iteration_model():
    """bench.py's round-6 bookkeeping, on made-up numbers: a window's roofline entries are algorithmic bytes / the library's stage
    time against 8 TB/s, and the clip model weighs the three windows by the stages' shares of a 60-frame clip's 27 050 iterations."""
    import bench
    assert abs(sum(bench.STAGE_SHARE.values()) - 1.0) < 1e-12
    assert abs(bench.STAGE_SHARE["joint"] - 59 * 300 / 27050) < 1e-12
    N, K, P = 72000, 222000.0, 480 * 854
    m = {"ms_per_step": 0.19, "timed_region_s": 0.0038, "K_mean": K, "K_list": [220000, 224000], "void_iterations": 0, "splats": N,
         "stage_ms": {"blend_fwd": 0.040, "loss": 0.030, "blend_bwd": 0.060, "tile_sort": 0.01}, "repeats": {"n": 10, "median": 0.188}}
    w = bench.window_report(m, "joint", {"blend_bwd": "fused_blend_bwd_kernel<7>"}, N, P)
    b = 44 * K + 24 * P + 40 * N
    assert w["kernels"]["blend_bwd"]["algorithmic_bytes"] == b and w["kernels"]["blend_bwd"]["kernel"] == "fused_blend_bwd_kernel<7>"
    assert abs(w["kernels"]["blend_bwd"]["frac_of_hbm_peak"] - b / 0.060e-3 / 1e9 / 8000.0) < 1e-12
    assert w["share_of_the_clips_iterations"] == bench.STAGE_SHARE["joint"] and w["ms_per_step_repeats"]["median"] == 0.188
    assert w["algorithmic_bytes_per_iteration"] == 724 * N + 124 * K + 96 * P
    local = {"elapsed": 0.0039, "steps": 20}
    cw = {"camera": {"ms_per_step": 0.200}, "joint": {"ms_per_step": 0.187}}
    cm = bench.clip_iteration_model(local, cw, {"wall_s": 5.9, "iterations": 27050.0}, world=1)
    want = bench.STAGE_SHARE["first_frame"] * 0.195 + bench.STAGE_SHARE["camera"] * 0.200 + bench.STAGE_SHARE["joint"] * 0.187
    assert abs(cm["windows_weighted_ms_per_iteration"] - want) < 1e-9
    assert abs(cm["clip_fit_ms_per_iteration"] - 5.9 / 27050 * 1e3) < 1e-9 and 0 < cm["unexplained_frac"] < 0.2
    assert bench.clip_iteration_model(local, None, None) is None


def test_bench_write_outputs_keeps_the_types_the_budget_and_the_same_sample(tmp_path):
    """bench.py --dump-outputs: float64 stays float64, everything else is written as float32; under the budget every array is
    written whole, over it every array keeps the same seeded share of its elements -- the same indices in every run."""
    import bench
    arrays = {"img": torch.arange(1200, dtype=torch.float32).reshape(3, 20, 20), "loss": torch.tensor([0.25, 0.5], dtype=torch.float64),
              "count": torch.arange(300, dtype=torch.int32)}
    assert bench.write_outputs(str(tmp_path / "whole"), arrays) == ["count", "img", "loss"]
    got = {k: np.load(tmp_path / "whole" / (k + ".npy")) for k in arrays}
    assert got["img"].dtype == np.float32 and np.array_equal(got["img"], arrays["img"].numpy())
    assert got["loss"].dtype == np.float64 and np.array_equal(got["loss"], [0.25, 0.5])
    assert got["count"].dtype == np.float32 and np.array_equal(got["count"], np.arange(300))
    budget = 2000
    for run in ("a", "b"):
        bench.write_outputs(str(tmp_path / run), arrays, budget=budget)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    b = {k: np.load(tmp_path / "b" / (k + ".npy")) for k in arrays}
    assert sum(v.nbytes for v in a.values()) <= budget
    for k in arrays:
        assert np.array_equal(a[k], b[k]), k
        # a sample of the flattened array, in index order
        flat = arrays[k].reshape(-1).double().numpy()
        assert 0 < a[k].size < flat.size and np.all(np.diff(a[k]) > 0) and np.isin(a[k], flat).all(), k
