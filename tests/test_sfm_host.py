"""CPU: depth and camera from the flows -- the float64 restatement (tests/sfm_ref.py) against analytic ground truth and numpy,
and the host side of gflow_amd.sfm (files, arguments, workspace queries).  The device is compared with the restatement in
tests/test_gpu_sfm.py.

The scene is analytic and static: 36 x 48, f = 40, depth 2 + 0.5 sin(0.2 x) cos(0.15 y) + 0.4 x / W, rotation vector
(0.01, -0.02, 0.005), translation (0.08, 0.02, 0.03), exact flows rounded to float32.  Every bound below is 100 x what the
restatement itself gives on that input (the figure is written beside it): the margin covers other LAPACK builds and
summation orders.

The motions, cameras and sizes that tests/test_gpu_sfm.py compares on the device (sfm_ref.CASES) are held here, on the
restatement alone, to reach the branch each is there for: that makes the choice of inputs checkable without a device."""
import json
import os

import numpy as np
import pytest
import torch

from gflow_amd import sfm
from tests import sfm_ref as R

# measured with the restatement (numpy 2, OpenBLAS): rotation 1.5e-9 deg, translation direction 2.7e-7 deg, relative depth after
# the median scale 6.9e-9 median and 3.1e-8 max; with the moving block 1.6e-9 deg and 2.5e-7 deg
ROT_BOUND_DEG = 1.5e-7
DIR_BOUND_DEG = 2.7e-5
DEPTH_MEDIAN_BOUND, DEPTH_MAX_BOUND = 6.9e-7, 3.1e-6
# the three-frame scene: ratio 1.5 to 4.1e-9; chained poses to 1.1e-8 deg and 1.2e-9 (translation, after the global scale)
RATIO_BOUND = 4.1e-7
CHAIN_ROT_BOUND_DEG, CHAIN_T_BOUND = 1.1e-6, 1.2e-7


@pytest.fixture(scope="module")
def scene():
    sc = R.make_scene()
    sc["two_view"] = R.two_view(sc["flow"], sc["intr"], R.initial_F(sc["flow"]))
    return sc


@pytest.fixture(scope="module")
def block_scene():
    sc = R.make_scene()
    sc["flow"], sc["block"] = R.add_block(sc["flow"])
    sc["two_view"] = R.two_view(sc["flow"], sc["intr"], R.initial_F(sc["flow"]))
    return sc


def pose_errors(tv, sc):
    return R.rotation_angle_deg(tv["R"], sc["R"]), R.angle_deg(tv["t"], sc["t"])


def test_restatement_recovers_the_analytic_scene(scene):
    tv = scene["two_view"]
    rot, direction = pose_errors(tv, scene)
    good = tv["weight"] > 0
    z = 1.0 / tv["rho"][good]
    rel = np.abs(z * np.median(scene["depth"][good] / z) - scene["depth"][good]) / scene["depth"][good]
    print(f"rotation {rot:.3e} deg, direction {direction:.3e} deg, depth median {np.median(rel):.3e} max {rel.max():.3e}")
    assert not tv["degenerate"] and tv["counts"] == (36 * 48, 36 * 48)
    assert good.all() and tv["votes"][0] == 36 * 48 and not tv["votes"][1:].any()      # all pixels pass cheirality
    assert rot < ROT_BOUND_DEG and direction < DIR_BOUND_DEG
    assert np.median(rel) < DEPTH_MEDIAN_BOUND and rel.max() < DEPTH_MAX_BOUND
    assert abs(np.linalg.norm(tv["t"]) - 1.0) < 1e-12 and abs(np.linalg.det(tv["R"]) - 1.0) < 1e-12
    assert abs(np.linalg.norm(tv["F"]) - 1.0) < 1e-12 and tv["F"].reshape(-1)[np.argmax(np.abs(tv["F"]))] > 0


def test_moving_block_is_left_out_and_filled_from_its_ring(block_scene):
    sc, tv = block_scene, block_scene["two_view"]
    block = sc["block"]
    assert block.sum() == 144 and not tv["inlier"][block].any() and tv["inlier"][~block].all()
    assert not tv["weight"][block].any()
    rot, direction = pose_errors(tv, sc)
    print(f"rotation {rot:.3e} deg, direction {direction:.3e} deg")
    assert rot < ROT_BOUND_DEG and direction < DIR_BOUND_DEG
    w = tv["weight"]
    lam = 0.05 * R.lower_median(np.where(w > 0, w, np.nan))[0]
    depth, _ = R.fill(tv["rho"], w, lam)
    ring = np.zeros_like(block)
    ring[9:23, 13:27] = True
    ring &= ~block
    assert (w[ring] > 0).all()
    assert depth[ring].min() <= depth[block].min() and depth[block].max() <= depth[ring].max()


def test_ratio_and_chain_of_three_frames():
    s3 = R.make_scene3()
    res = R.clip_depth_camera(s3["fwd"], s3["bwd"], s3["intr"], median_depth=2.0)
    print("ratio error", abs(res["ratio"][1] - 1.5))
    assert list(res["count"]) == [0, 36 * 48, 0] and np.isnan(res["ratio"][[0, 2]]).all()
    assert abs(res["ratio"][1] - 1.5) < RATIO_BOUND
    assert not res["degenerate"].any() and not res["unreliable"].any()
    assert R.lower_median(res["depth"][0])[0] == pytest.approx(2.0, rel=1e-12)
    s = res["baseline"][0] / s3["baselines"][0]                    # the global scale
    assert abs(res["baseline"][1] / s - s3["baselines"][1]) < RATIO_BOUND
    assert np.array_equal(res["extr"][0], np.eye(4)[:3])
    for i in (1, 2):
        rot = R.rotation_angle_deg(res["extr"][i][:, :3], s3["extr"][i][:, :3])
        dt = np.abs(res["extr"][i][:, 3] / s - s3["extr"][i][:, 3]).max()
        print(f"frame {i}: rotation {rot:.3e} deg, translation {dt:.3e}")
        assert rot < CHAIN_ROT_BOUND_DEG and dt < CHAIN_T_BOUND
    # the depth is the scene's up to the smoothing of the sweeps (under one per cent here)
    for i in range(3):
        assert np.abs(res["depth"][i] / s - s3["depth"][i]).max() < 0.03


def test_forward_flows_alone_chain_through_the_medians():
    s3 = R.make_scene3()
    res = R.clip_depth_camera(s3["fwd"], None, s3["intr"])
    assert not res["count"].any() and not res["unreliable"][:2].any() and res["unreliable"][2]
    # the smoothed median depths of neighbouring frames agree to a few per cent: so does the baseline ratio
    assert abs(res["baseline"][1] / res["baseline"][0] - 1.5) < 0.05
    assert np.all(res["depth"][2] == 1.0)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_case_reaches_what_it_is_there_for(case):
    """the motions, cameras and sizes of tests/test_gpu_sfm.py on the restatement alone: the winner of the vote, the branch
    of the threshold, the flag, both margins and the cap on pixels near the epipole (sfm_ref.check_case); and the
    restatement recovers the true pose of every exact, non-degenerate case: R to 1e-6, t / |t| to 1e-5"""
    motion, H, W, cam = case
    sc = R.case_scene(case)
    with np.errstate(all="ignore"):
        tv = R.two_view(sc["flow"], sc["intr"], R.initial_F(sc["flow"]), **R.case_kw(case))
    info = R.check_case(case, sc["flow"], sc["intr"], tv)
    assert len(tv["margins"]) == 3 and R.threshold_margin(tv) == min(tv["margins"])
    if cam == "centred" and motion == "fwd":                       # the epipole is a pixel's centre
        assert info["left_out"][round(H / 2), round(W / 2)] and info["undecided"].sum() == 1
    if motion == "noisy":
        assert np.abs(sc["flow"] - R.case_scene((("base",) + case[1:]))["flow"]).max() > 0.3
        return
    dR, dt = np.abs(tv["R"] - sc["R"]).max(), np.abs(tv["t"] - sc["t"] / np.linalg.norm(sc["t"])).max()
    print(f"{R.case_id(case)}: R {dR:.2e} t {dt:.2e} votes {tv['votes']} parallax {tv['parallax']:.3f}")
    assert dR < 1e-6                                               # (a degenerate pair keeps its R)
    assert tv["degenerate"] or dt < 1e-5


def test_the_cases_cover_what_the_kernels_branch_on():
    motions = {c[0] for c in R.CASES}
    assert motions == set(R.MOTIONS) and {R.MOTIONS[m][2] for m in motions} == {0, 1, 2, 3}
    for m in motions:                                              # the general camera under every motion
        assert any(c[0] == m and c[3] == "general" for c in R.CASES), m
    for size in R.SIZES:                                           # every size under base, noisy and a rolled view
        for group in (("base",), ("noisy",), ("roll", "roll-neg"), ("fwd",)):
            assert any(c[0] in group and c[1:3] == size for c in R.CASES), (size, group)
    assert sorted({-(-H * W // R.PER_WORKGROUP) for (H, W) in R.SIZES}) == [1, 2, 3] and 64 * 65 - R.PER_WORKGROUP == 64
    assert len(set(R.CASES)) == len(R.CASES) <= 32


def test_the_scene_builders_keep_their_defaults():
    """make_scene and make_scene3 through the general builder: the bits they always gave"""
    sc = R.make_scene()
    depth = R.scene_depth(36, 48)
    flow, _ = R.exact_flow(depth, (40.0, 40.0, 24.0, 18.0), R.rodrigues((0.01, -0.02, 0.005)), (0.08, 0.02, 0.03))
    assert sc["intr"] == (40.0, 40.0, 24.0, 18.0) and sc["flow"].dtype == np.float32 and np.array_equal(sc["flow"], flow)
    assert np.array_equal(R.make_scene_general(36, 48, sc["intr"], (0.01, -0.02, 0.005), (0.08, 0.02, 0.03), noise=(0.0, 1))["flow"], flow)
    noisy = R.make_scene_general(36, 48, sc["intr"], (0.01, -0.02, 0.005), (0.08, 0.02, 0.03), noise=(0.3, 1))["flow"]
    assert noisy.dtype == np.float32 and 0.25 < (noisy - flow).std() < 0.35
    assert R.make_scene3()["intr"] == (40.0, 40.0, 24.0, 18.0) and R.make_scene3(pp=(20.75, 20.5))["intr"] == (40.0, 40.0, 20.75, 20.5)


def test_the_sensitivity_probe():
    """8 repeats under relative 2^-50 perturbations of A^T A: small against the recovery of the pose, not zero, repeatable"""
    sc = R.make_scene()
    F0 = R.initial_F(sc["flow"])
    a, b = R.sensitivity(sc["flow"], sc["intr"], F0), R.sensitivity(sc["flow"], sc["intr"], F0)
    assert a == b and sorted(a) == ["F", "R", "parallax", "t"]
    assert all(0 < v < 1e-9 for v in a.values()), a
    assert R.sensitivity(sc["flow"], sc["intr"], F0, repeats=0) == dict(F=0.0, R=0.0, t=0.0, parallax=0.0)


def test_numpy_ties(scene):
    tv = scene["two_view"]
    Ra, Rb, t0 = R.essential_candidates(tv["F"], scene["intr"])
    fx, fy, cx, cy = scene["intr"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    U, S, Vt = np.linalg.svd(K.T @ tv["F"] @ K)
    assert S[2] < 1e-12 * S[0] and abs(S[0] - S[1]) < 1e-6 * S[0]
    E = U @ np.diag([1.0, 1.0, 0.0]) @ Vt                          # the projection onto the essential matrices
    for Rc in (Ra, Rb):
        assert abs(np.linalg.det(Rc) - 1.0) < 1e-12 and np.abs(Rc @ Rc.T - np.eye(3)).max() < 1e-12
        tx = np.array([[0, -t0[2], t0[1]], [t0[2], 0, -t0[0]], [-t0[1], t0[0], 0]])
        Ec = tx @ Rc                                               # [t]x R is E up to sign
        assert min(np.abs(Ec - E).max(), np.abs(Ec + E).max()) < 1e-12
    assert np.trace(Ra) >= np.trace(Rb) and abs(np.linalg.norm(t0) - 1.0) < 1e-12 and t0[np.argmax(np.abs(t0))] > 0
    assert np.abs(U[:, 2] @ t0) == pytest.approx(1.0, abs=1e-12)
    rng = np.random.default_rng(0)
    for (H, W) in ((8, 8), (9, 13), (33, 47)):
        v, w = rng.uniform(0.1, 2.0, (H, W)), rng.uniform(0.5, 1.5, (H, W))
        assert np.array_equal(R.pull_push(v, w), v)                # fully weighted: the identity
        assert np.array_equal(R.jacobi(v, w, 0.0, v, 5), v)        # lambda = 0: the identity
        hole = w.copy()
        hole[2:5, 3:7] = 0
        filled = R.pull_push(v, hole)
        assert np.array_equal(filled[hole > 0], v[hole > 0]) and v.min() <= filled.min() and filled.max() <= v.max()
        assert np.array_equal(R.jacobi(v, hole, 0.0, filled, 5), filled)
    # the exact lower median
    assert R.lower_median([3.0, 1.0, np.nan, 2.0, 4.0]) == (2.0, 4) and np.isnan(R.lower_median([np.nan])[0])


def test_zero_flow_is_degenerate_and_finite():
    flow = np.zeros((16, 24, 2), dtype=np.float32)
    intr = (24.0, 24.0, 12.0, 8.0)
    with np.errstate(all="ignore"):
        tv = R.two_view(flow, intr, R.initial_F(flow))
    assert tv["degenerate"] and not tv["t"].any() and tv["parallax"] < 0.1
    for k in ("F", "R", "t", "rho", "weight"):
        assert np.isfinite(tv[k]).all(), k
    assert not tv["weight"].any() and not tv["rho"].any()
    res = R.clip_depth_camera([flow, flow], [flow, flow], intr, median_depth=3.0)
    assert res["unreliable"].all() and res["degenerate"].all() and np.all(res["depth"] == 3.0)
    assert np.isfinite(res["extr"]).all() and np.array_equal(res["extr"][0], np.eye(4)[:3])


def test_written_files_round_trip(tmp_path):
    from gflow_amd import io as gio
    rng = np.random.default_rng(1)
    depth = rng.uniform(0.5, 3.0, (3, 9, 11)).astype(np.float32)
    extr = np.stack([np.concatenate([R.rodrigues(rng.normal(size=3) * 0.1), rng.normal(size=(3, 1))], axis=1) for _ in range(3)])
    res = dict(depth=torch.from_numpy(depth), extr=torch.from_numpy(extr), focal=11.0, pp=[6, 4])
    names = ["00000", "00001", "00002"]
    dd, cd = str(tmp_path / "s_depth_mast3r_s2"), str(tmp_path / "s_camera_mast3r_s2")
    paths = sfm.write_depth_camera(res, dd, cd, names)
    assert [os.path.basename(p) for p in paths] == [n + ".npy" for n in names] + [n + ".json" for n in names]
    with pytest.raises(FileExistsError, match="overwrite"):
        sfm.write_depth_camera(res, dd, cd, names)
    sfm.write_depth_camera(res, dd, cd, names, overwrite=True)
    focal, pp, poses = gio.read_camera(paths[3:])
    assert focal == 11.0 and pp == [6, 4] and np.array_equal(poses, extr)
    for i in range(3):
        assert torch.equal(gio.read_depth(paths[i]), torch.from_numpy(depth[i]))
    with open(paths[3]) as f:
        d = json.load(f)
    assert sorted(d) == ["focal", "pose", "pp"] and np.array_equal(np.array(d["pose"])[3], [0, 0, 0, 1])
    assert sfm.default_camera(480, 854) == (854.0, [427, 240]) and sfm.default_camera(480, 854, 500, (1, 2)) == (500.0, [1, 2])


def test_arguments():
    from gflow_amd import fit_video
    from gflow_amd import io as gio
    with pytest.raises(ValueError, match="depth_camera"):
        gio.load_sequence("/nonexistent", depth_camera="x")
    with pytest.raises(ValueError, match="focal"):
        gio.load_sequence("/nonexistent", focal=100.0)
    with pytest.raises(ValueError, match="flow must be"):
        sfm.two_view(np.zeros((8, 8, 3), dtype=np.float32), (8, 8, 4, 4))
    with pytest.raises(ValueError, match="fwd and bwd"):
        sfm.clip_depth_camera(np.zeros((2, 8, 8, 2), dtype=np.float32), np.zeros((1, 8, 8, 2), dtype=np.float32))
    with pytest.raises(ValueError, match="median_depth"):
        sfm.clip_depth_camera(np.zeros((1, 8, 8, 2), dtype=np.float32), None, median_depth=0.0)
    for bad in ((8.0, 8.0, 4.0), (float("nan"), 8.0, 4.0, 4.0), (0.0, 8.0, 4.0, 4.0)):
        with pytest.raises(ValueError, match="intr"):
            sfm._intr(bad)
    with pytest.raises(SystemExit) as e:
        fit_video.main(["--make-depth-camera"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        fit_video.main(["--sequence", "s", "--focal", "100"])
    assert e.value.code == 2


def test_workspace_queries_need_no_device():
    from gflow_amd import _lib as L
    lib = L.load()
    q = lib.gfl_sfm_workspace_bytes
    assert q(1, 8, 8) > 0 and q(4, 36, 48) > q(1, 36, 48) > q(1, 16, 24)
    assert q(118, 480, 854) > 118 * 480 * 854 * 8
    for bad in ((0, 8, 8), (1, 7, 8), (1, 8, 7), (65536, 8, 8), (1, 16385, 8), (1, 8, 16385), (2, 32768 // 2, 32768 + 1),
                (1 << 11, 1 << 10, 1 << 10)):
        assert q(*bad) == 0, bad
