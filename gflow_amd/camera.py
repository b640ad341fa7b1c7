"""The camera path of a clip fit and its score: ATE and RPE ("Camera score").

The contract is the reference's trajectory evaluation (gflow/benchmark.py:289-394): every frame's ``extr`` as
``save_checkpoint`` stores it, against the sequence's prepared camera, with evo's ``ape`` (translation part, ``align=True,
correct_scale=True``) and ``rpe`` (delta = 1 frame, translation part and rotation angle in degrees), each as an RMSE.

- ``CameraRecorder.frame`` keeps a clone of the frame's ``get_extr()``: no read-back, no synchronisation while the clip is
  fitted; ``CameraRecorder.result`` is one stacked copy to the host.
- ``evaluate`` is float64 numpy on a few dozen 4 x 4 matrices.

evo is not available where this was written: the score follows evo's public definitions (below) and is held against a
direct minimisation over the seven Sim(3) parameters (tests/camera_ref.py), not against evo itself.

One divergence from evo, on purpose: evo's Umeyama alignment raises "degenerate covariance rank" when the covariance of
the two position sets has rank < 2 -- a collinear reference path, such as synthetic.make_clip's -- and the reference then
writes None.  The three numbers are still well defined at rank 1: with the reference positions on a line of direction a,
the squared error depends on R only through R^T a, which the first singular pair fixes; the scale depends only on the
first singular value; RPE does not depend on the rigid part of the alignment at all.  ``evaluate`` therefore accepts
rank >= 1.  Rank 0 -- a static reference camera, all estimated positions equal, or fewer than two frames -- gives None for
all three, as the reference's ``except`` branch does."""
import numpy as np
import torch

SCORE_KEYS = ("ATE", "RPE_t", "RPE_r")


class CameraRecorder:
    """The per-frame world-to-camera matrices of one clip, kept on the device until ``result``."""

    def __init__(self, n_frames):
        self.T = int(n_frames)
        self.extr = [None] * self.T

    def frame(self, i, extr):
        """Frame ``i``'s (3, 4) ``extr`` (trainer.get_extr()), cloned"""
        if not 0 <= int(i) < self.T:
            raise ValueError(f"CameraRecorder.frame: frame {i} outside [0, {self.T})")
        self.extr[int(i)] = extr.detach().float().clone()

    def result(self):
        """(T, 3, 4) float32: one copy to the host"""
        missing = [t for t, e in enumerate(self.extr) if e is None]
        if missing:
            raise ValueError(f"CameraRecorder.result: frames {missing} were not recorded")
        if not self.T:
            return np.zeros((0, 3, 4), dtype=np.float32)
        return torch.stack(self.extr).cpu().numpy()


def poses_from_extr(extr):
    """(T, 4, 4) float64 camera-to-world poses inv([extr; 0 0 0 1]) of (T, 3, 4) world-to-camera matrices
    (benchmark.py:331-343)"""
    e = np.asarray(extr, dtype=np.float64).reshape(-1, 3, 4)
    m = np.tile(np.eye(4), (e.shape[0], 1, 1))
    m[:, :3, :] = e
    return np.linalg.inv(m) if len(m) else m


def umeyama(x, y):
    """(R, t, c, rank) of the similarity y ~ c R x + t that minimises the squared error over the rows of ``x`` and ``y``
    ((n, 3) each): Umeyama 1991 as evo.core.geometry.umeyama_alignment writes it -- cov = 1/n sum (y - my)(x - mx)^T,
    U D V^T = svd(cov), S = diag(1, 1, sign(det U det V^T)), R = U S V^T, c = tr(D S) / var(x), t = my - c R mx.
    ``rank``: the singular values above machine epsilon (evo's test).  R, t and c are None at rank 0."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    if n < 1:
        return None, None, None, 0
    mx, my = x.mean(axis=0), y.mean(axis=0)
    var_x = ((x - mx) ** 2).sum() / n
    cov = (y - my).T @ (x - mx) / n
    u, d, vt = np.linalg.svd(cov)
    rank = int(np.count_nonzero(d > np.finfo(d.dtype).eps))
    if rank == 0 or not var_x > 0.0:
        return None, None, None, 0
    s = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(vt) < 0.0:
        s[2, 2] = -1.0
    r = u @ s @ vt
    c = float(np.trace(np.diag(d) @ s) / var_x)
    t = my - c * (r @ mx)
    return r, t, c, rank


def rotation_angle(r):
    """The rotation angle of a 3 x 3 rotation in radians: atan2 of the antisymmetric part's norm and the trace (exact to
    rounding near 0, where arccos of the trace alone loses half the digits)"""
    v = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    return float(np.arctan2(0.5 * np.linalg.norm(v), 0.5 * (np.trace(r) - 1.0)))


def align(poses_est, poses_ref):
    """``poses_est`` aligned onto ``poses_ref`` by Sim(3) on the positions, as evo's ``align(correct_scale=True)`` does:
    positions scaled by c, then every pose left-multiplied by (R, t).  None at rank 0."""
    r, t, c, rank = umeyama(poses_est[:, :3, 3], poses_ref[:, :3, 3])
    if rank == 0:
        return None
    out = poses_est.copy()
    out[:, :3, 3] *= c
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = r, t
    return m @ out


def evaluate(extr_est, extr_gt):
    """{ATE, RPE_t, RPE_r} of the (T, 3, 4) world-to-camera matrices ``extr_est`` against ``extr_gt``, float64:
    ATE: the RMSE over the frames of |p_est - p_ref| after the alignment;
    RPE_t, RPE_r: over the T - 1 consecutive pairs, E = (Q_i^-1 Q_i+1)^-1 (P_i^-1 P_i+1) with Q the reference and P the
    aligned estimate -- the RMSE of |E[:3, 3]|, and of the rotation angle of E[:3, :3] in degrees.
    All three None when the alignment is undefined (rank 0: see the module's text)."""
    est, ref = poses_from_extr(extr_est), poses_from_extr(extr_gt)
    if est.shape != ref.shape:
        raise ValueError(f"camera.evaluate: {est.shape[0]} estimated poses against {ref.shape[0]}")
    none = {k: None for k in SCORE_KEYS}
    if est.shape[0] < 2:
        return none
    al = align(est, ref)
    if al is None:
        return none
    ate = float(np.sqrt(np.mean(((al[:, :3, 3] - ref[:, :3, 3]) ** 2).sum(axis=1))))
    inv = np.linalg.inv
    e_t, e_r = [], []
    for i in range(est.shape[0] - 1):
        e = inv(inv(ref[i]) @ ref[i + 1]) @ (inv(al[i]) @ al[i + 1])
        e_t.append(float((e[:3, 3] ** 2).sum()))
        e_r.append(np.degrees(rotation_angle(e[:3, :3])) ** 2)
    return {"ATE": ate, "RPE_t": float(np.sqrt(np.mean(e_t))), "RPE_r": float(np.sqrt(np.mean(e_r)))}
