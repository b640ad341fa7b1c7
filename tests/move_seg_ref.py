"""float64 numpy / scipy restatement of the move mask from the flow (gfl_epi_fundamental, gfl_epi_mask; include/gflow_hip.h,
gflow_amd/move_seg.py): the reference's utility/move_seg.py with the project's own deterministic LMedS in place of
cv2.findFundamentalMat (unpinned against cv2) and scipy.ndimage in place of skimage.morphology (unpinned against skimage).

Correspondences are formed in float32 exactly as move_seg.py:185-203 forms them; everything after that is float64.  The
Sampson error is evaluated element by element in the order the header states (sums from the left, every product and sum
rounded on its own), so a device that follows the header computes the same numbers."""
import numpy as np
from scipy import ndimage

from tests.epipolar_ref import canonical, lower_median  # noqa: F401  (the tests call R.lower_median)
from tests import epipolar_ref as E

OPEN_R, ERODE_R, DILATE_R = 2, 5, 3


def correspondences(flow):
    """(x1 (n, 2), x2 (n, 2)) float64 holding float32 values, known (n,) bool; pixel i = y * W + x"""
    flow = np.asarray(flow, dtype=np.float32)
    H, W, _ = flow.shape
    f32 = np.float32
    xx = (f32(2) * (np.arange(W, dtype=f32) + f32(0.5))) / f32(W) - f32(1)
    yy = (f32(2) * (np.arange(H, dtype=f32) + f32(0.5))) / f32(H) - f32(1)
    x1 = np.stack(np.broadcast_arrays(xx[None, :], yy[:, None]), axis=-1).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.stack([(f32(2) * flow[..., 0]) / f32(W - 1), (f32(2) * flow[..., 1]) / f32(H - 1)], axis=-1).astype(f32)
        x2 = (x1 + d).astype(f32)
    known = np.isfinite(x2).all(axis=-1)
    return x1.reshape(-1, 2).astype(np.float64), x2.reshape(-1, 2).astype(np.float64), known.reshape(-1)


def sampson(F, x1, x2):
    """move_seg.py:57-71 on (n, 2) float64 points, F (3, 3); a zero denominator gives 0"""
    return E.sampson(F, x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1])


def _hartley(p):
    c = p.mean(axis=0)
    q = p - c
    s = np.sqrt(2.0) / np.sqrt((q * q).sum(axis=1)).mean()
    return q * s, np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def eight_point(p1, p2):
    """Hartley-normalised 8-point on (8, 2) points: (F (3, 3) canonical, lambda_1 / lambda_max of A^T A of the normalised
    design matrix -- the second-smallest over the largest eigenvalue: the smallest is 0 for eight rows)"""
    n1, T1 = _hartley(p1)
    n2, T2 = _hartley(p2)
    A = np.stack([n2[:, 0] * n1[:, 0], n2[:, 0] * n1[:, 1], n2[:, 0], n2[:, 1] * n1[:, 0], n2[:, 1] * n1[:, 1], n2[:, 1],
                  n1[:, 0], n1[:, 1], np.ones(8)], axis=1)
    _, s, vt = np.linalg.svd(A)                       # s: 8 values, descending; vt: (9, 9)
    Fn = vt[-1].reshape(3, 3)
    u, sv, wt = np.linalg.svd(Fn)
    Fn = u @ np.diag([sv[0], sv[1], 0.0]) @ wt
    return canonical(T2.T @ Fn @ T1), float((s[-1] / s[0]) ** 2)


def is_degenerate(sample, known):
    s = np.asarray(sample)
    n = known.size
    return bool(((s < 0) | (s >= n)).any() or len(set(s.tolist())) < 8 or not known[s].all())


def fundamental(flow, samples):
    """dict(F_all (K, 3, 3), medians (K,), ratio (K,), best, F) -- a degenerate hypothesis has F = 0, median = +inf and
    ratio = nan; best = -1 and F = 0 if all are"""
    x1, x2, known = correspondences(flow)
    samples = np.asarray(samples).reshape(-1, 8)
    K = samples.shape[0]
    F_all, med, ratio = np.zeros((K, 3, 3)), np.full(K, np.inf), np.full(K, np.nan)
    for k in range(K):
        if is_degenerate(samples[k], known):
            continue
        with np.errstate(all="ignore"):
            F, r = eight_point(x1[samples[k]], x2[samples[k]])
        if not np.isfinite(F).all():
            continue
        F_all[k], ratio[k] = F, r
        med[k] = lower_median(sampson(F, x1[known], x2[known]))
    best = int(np.argmin(med)) if np.isfinite(med).any() else -1
    return dict(F_all=F_all, medians=med, ratio=ratio, best=best, F=F_all[best] if best >= 0 else np.zeros((3, 3)))


def median_of(flow, F):
    """the exact lower median of the Sampson errors of F over the known pixels"""
    x1, x2, known = correspondences(flow)
    return lower_median(sampson(F, x1[known], x2[known]))


def disk(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return xx * xx + yy * yy <= r * r


def erode(mask, r):
    return ndimage.binary_erosion(np.asarray(mask) != 0, structure=disk(r), border_value=1)


def dilate(mask, r):
    return ndimage.binary_dilation(np.asarray(mask) != 0, structure=disk(r), border_value=0)


def opening(mask, r=OPEN_R):
    return dilate(erode(mask, r), r)


def morphology(mask):
    """(open, erode, dilate) uint8 0 / 255 of a mask (nonzero = set)"""
    u8 = lambda m: m.astype(np.uint8) * np.uint8(255)
    return u8(opening(mask)), u8(erode(mask, ERODE_R)), u8(dilate(mask, DILATE_R))


def mask_from(flow, F, threshold=0.01):
    """dict(err_norm (H, W) float64 (before the rounding to float32), mask, open, erode, dilate uint8 0 / 255)"""
    flow = np.asarray(flow, dtype=np.float32)
    H, W, _ = flow.shape
    x1, x2, known = correspondences(flow)
    fac = (H + W) / 2.0
    err = np.where(known, sampson(F, x1, x2) * (fac * fac), 0.0)
    err = np.where(np.isfinite(err), err, 0.0)
    top = err.max()
    norm = err / top if top > 0 else np.zeros_like(err)
    mask = ((norm > threshold) & known).reshape(H, W)
    o, e, d = morphology(mask)
    return dict(err_norm=norm.reshape(H, W), mask=mask.astype(np.uint8) * np.uint8(255), open=o, erode=e, dilate=d)


def move_mask(flow, samples, threshold=0.01):
    f = fundamental(flow, samples)
    return dict(f, **mask_from(flow, f["F"], threshold))
