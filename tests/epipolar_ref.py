"""What the float64 restatements of the move masks (tests/move_seg_ref.py) and of depth and camera (tests/sfm_ref.py) share, as
csrc/gfl_epipolar.hpp shares it on the device: the Sampson error, the lower median's selection rule and the common scale and
sign of a fundamental matrix."""
import numpy as np


def sampson(F, x1, y1, x2, y2):
    """d1 = F h1, d2 = F^T h2, z = h2 . d1, z^2 / (d1x^2 + d1y^2 + d2x^2 + d2y^2), element by element in the order
    include/gflow_hip.h states (sums from the left, every product and sum rounded on its own); a zero denominator gives 0"""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d1x = (F[0] * x1 + F[1] * y1) + F[2]
        d1y = (F[3] * x1 + F[4] * y1) + F[5]
        d1z = (F[6] * x1 + F[7] * y1) + F[8]
        d2x = (F[0] * x2 + F[3] * y2) + F[6]
        d2y = (F[1] * x2 + F[4] * y2) + F[7]
        z = (x2 * d1x + y2 * d1y) + d1z
        den = ((d1x * d1x + d1y * d1y) + d2x * d2x) + d2y * d2y
        return np.where(den == 0.0, 0.0, (z * z) / np.where(den == 0.0, 1.0, den))


def lower_median(values):
    """the value of rank (n - 1) // 2 among the n values given"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    k = (v.size - 1) // 2
    return float(np.partition(v, k)[k])


def canonical(F):
    """(3, 3): ||F||_F = 1 with the entry of largest magnitude positive (the first among equal magnitudes), scaled as the
    device scales it: by (+-1 / sqrt(sum of squares))"""
    F = np.asarray(F, dtype=np.float64).reshape(9)
    big = F[np.argmax(np.abs(F))]
    return (F * ((-1.0 if big < 0 else 1.0) / np.sqrt((F * F).sum()))).reshape(3, 3)
