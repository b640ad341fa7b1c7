"""CPU: camera.evaluate (ATE, RPE by Umeyama's closed form) against a direct minimisation over the seven Sim(3) parameters
(tests/camera_ref.py) on a general and on a collinear reference path, and on inputs whose answer is known."""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from gflow_amd import camera as CM
from tests import camera_ref as R

KEYS = ("ATE", "RPE_t", "RPE_r")


def _extr(rot, pos):
    """(T, 3, 4) world-to-camera matrices of cameras with camera-to-world rotations ``rot`` at positions ``pos``"""
    out = np.zeros((len(pos), 3, 4))
    for i, (r, p) in enumerate(zip(rot, pos)):
        out[i, :, :3] = r.T
        out[i, :, 3] = -r.T @ p
    return out


def _general_path(rng, n=8):
    pos = np.cumsum(rng.normal(size=(n, 3)), axis=0)
    rot = Rotation.from_rotvec(0.3 * rng.normal(size=(n, 3))).as_matrix()
    return rot, pos


def _collinear_path(rng, n=8):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    pos = 0.7 + np.outer(np.sort(rng.uniform(0, 3, size=n)), a)
    rot = Rotation.from_rotvec(0.2 * rng.normal(size=(n, 3))).as_matrix()
    return rot, pos


def _noisy(rng, rot, pos, scale=1.7):
    """an estimate: the path under a similarity, then noise on positions and orientations"""
    g = Rotation.from_rotvec([0.4, -0.9, 0.3]).as_matrix()
    p = (pos @ g.T) / scale + np.array([0.5, -2.0, 1.0]) + 0.05 * rng.normal(size=pos.shape)
    r = np.stack([g @ m @ Rotation.from_rotvec(0.03 * rng.normal(size=3)).as_matrix() for m in rot])
    return r, p


@pytest.mark.parametrize("path", [_general_path, _collinear_path], ids=["general", "collinear"])
def test_closed_form_equals_direct_minimisation(path):
    rng = np.random.default_rng(11)
    rot, pos = path(rng)
    e_rot, e_pos = _noisy(rng, rot, pos)
    gt, est = _extr(rot, pos), _extr(e_rot, e_pos)
    got, want = CM.evaluate(est, gt), R.evaluate(est, gt)
    print(path.__name__, got, want)
    for k in KEYS:
        assert want[k] > 1e-3                                 # (the noise shows in all three)
        assert got[k] == pytest.approx(want[k], rel=1e-6), k


def test_collinear_path_has_covariance_rank_one():
    rng = np.random.default_rng(11)
    rot, pos = _collinear_path(rng)
    e_rot, e_pos = _noisy(rng, rot, pos)
    *_, rank = CM.umeyama(e_pos, pos)
    assert rank == 1
    rot, pos = _general_path(rng)
    *_, rank = CM.umeyama(_noisy(rng, rot, pos)[1], pos)
    assert rank == 3


@pytest.mark.parametrize("path", [_general_path, _collinear_path], ids=["general", "collinear"])
def test_a_similarity_of_the_ground_truth_scores_zero(path):
    rng = np.random.default_rng(2)
    rot, pos = path(rng)
    g = Rotation.from_rotvec([1.1, 0.2, -0.7]).as_matrix()
    est = _extr(np.stack([g @ m for m in rot]), 2.5 * pos @ g.T + np.array([3.0, -1.0, 0.5]))
    got = CM.evaluate(est, _extr(rot, pos))
    for k in KEYS:
        assert abs(got[k]) <= 1e-12, (k, got[k])


@pytest.mark.parametrize("theta_deg", [0.5, 7.0, 40.0])
def test_a_growing_rotation_about_the_camera_gives_its_step_as_rpe_r(theta_deg):
    # est_i = gt_i o Rot(i theta) about a fixed axis, the ground-truth cameras all looking the same way: the positions are
    # the ground truth's (ATE 0) and the relative rotation of every consecutive pair differs by Rot(theta).  (RPE_t is not 0:
    # the step p_i+1 - p_i is expressed in frame i's own, rotated, axes.)
    rng = np.random.default_rng(4)
    n = 7
    pos = np.cumsum(rng.normal(size=(n, 3)), axis=0)
    r0 = Rotation.from_rotvec([0.2, 0.5, -0.1]).as_matrix()
    axis = np.array([0.6, 0.0, 0.8])
    rot = np.stack([r0] * n)
    e_rot = np.stack([r0 @ Rotation.from_rotvec(np.radians(i * theta_deg) * axis).as_matrix() for i in range(n)])
    got = CM.evaluate(_extr(e_rot, pos), _extr(rot, pos))
    assert got["RPE_r"] == pytest.approx(theta_deg, rel=1e-12)
    assert abs(got["ATE"]) <= 1e-12


def test_no_alignment_gives_none():
    rng = np.random.default_rng(6)
    rot, pos = _general_path(rng, 5)
    none = {k: None for k in KEYS}
    moving = _extr(rot, pos)
    static = _extr(rot, np.tile(pos[:1], (5, 1)))
    assert CM.evaluate(moving, static) == none               # a static reference camera
    assert CM.evaluate(static, moving) == none               # all estimated positions equal
    assert CM.evaluate(moving[:1], moving[:1]) == none       # T = 1
    assert CM.evaluate(moving[:0], moving[:0]) == none
    with pytest.raises(ValueError):
        CM.evaluate(moving, moving[:3])


def test_synthetic_clip_camera_is_scorable():
    # make_clip's camera moves on a straight line: rank 1, the case evo refuses
    from gflow_amd import synthetic as S
    frames = S.make_clip(4, 24, 32, seed=0)
    gt = np.stack([fr["extr_gt"].numpy() for fr in frames])
    est = gt.copy()
    est[:, 0, 3] *= 1.01
    est[2, 1, 3] += 0.003
    got = CM.evaluate(est, gt)
    assert all(got[k] is not None and np.isfinite(got[k]) for k in KEYS) and got["ATE"] > 0
    want = R.evaluate(est, gt)
    for k in ("ATE", "RPE_t"):
        assert got[k] == pytest.approx(want[k], rel=1e-6), k
    assert got["RPE_r"] == pytest.approx(0.0, abs=1e-9)


def test_recorder_stacks_clones():
    rec = CM.CameraRecorder(3)
    e = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for i in range(3):
        rec.frame(i, e)
        e += 1.0                                             # (the recorder kept a clone: later writes do not show)
    out = rec.result()
    assert out.shape == (3, 3, 4) and out.dtype == np.float32
    np.testing.assert_array_equal(out[:, 0, 0], [0.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        rec.frame(3, e)
    with pytest.raises(ValueError):
        CM.CameraRecorder(2).result()


def test_camera_needs_a_ground_truth_in_every_frame():
    from gflow_amd import synthetic as S
    from gflow_amd.fit_video import fit_clip
    frames = [dict(fr) for fr in S.make_clip(3, 24, 32, seed=0)]
    del frames[1]["extr_gt"]
    with pytest.raises(ValueError, match="neither extr_gt nor extr"):
        fit_clip(frames, "cpu", dict(num_points=50), camera=True)
