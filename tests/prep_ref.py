"""Float64 restatement of the frame preparation (include/gflow_hip.h, "frame preparation"; gflow_amd/prep.py) from its weight
matrices: what tests/test_prep_host.py ties to torch's CPU kernels and tests/test_gpu_prep.py compares gfl_prep_frames with.

The weights are the definition's: formed in float64 one operation at a time, normalised, rounded to float32.  Everything
after that (the sums of the passes, mul and add) is carried in float64 here, so this is the exact value the device's float32
sums approximate."""
import numpy as np

U = 2.0 ** -24                     # float32's unit roundoff


def out_shape(h, w, resize):
    if resize is None:
        return h, w
    return (resize, int(resize * w / h)) if h <= w else (int(resize * h / w), resize)


def axis_taps(n_in, n_out):
    """[(lo, float32 weights of the taps lo ..)] per output of one axis"""
    s = np.float64(n_in) / np.float64(n_out)
    support = s if s > 1.0 else np.float64(1.0)
    inv = np.float64(1.0) / support
    rows = []
    for i in range(n_out):
        c = s * (np.float64(i) + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(int(c + support + 0.5), n_in)
        w = [max(np.float64(0.0), 1.0 - abs((np.float64(j) - c + 0.5) * inv)) for j in range(lo, hi)]
        total = np.float64(0.0)
        for v in w:                                   # ascending, one rounding per add
            total = total + v
        rows.append((lo, np.array([v / total if total != 0.0 else v for v in w], dtype=np.float64).astype(np.float32)))
    return rows


def axis_matrix(n_in, n_out):
    """(n_out, n_in) float64 holding the float32 weights, and the largest tap count"""
    m = np.zeros((n_out, n_in), np.float64)
    rows = axis_taps(n_in, n_out)
    for i, (lo, w) in enumerate(rows):
        m[i, lo:lo + len(w)] = w
    return m, max(len(w) for _, w in rows)


def blur_taps(k, sigma):
    x = (np.arange(k, dtype=np.float64) - np.float64(k - 1) * 0.5) / np.float64(np.float32(sigma))
    pdf = np.exp(-0.5 * (x * x))
    total = np.float64(0.0)
    for v in pdf:
        total = total + v
    return (pdf / total).astype(np.float32)


def blur_matrix(n, k, sigma):
    """(n, n) float64: the taps with reflect padding (index -i reads i; the edge is not repeated)"""
    taps, r = blur_taps(k, sigma), k // 2
    assert r < n
    m = np.zeros((n, n), np.float64)
    for i in range(n):
        for j in range(k):
            q = i + j - r
            q = -q if q < 0 else 2 * (n - 1) - q if q >= n else q
            m[i, q] += np.float64(taps[j])
    return m


def convert(src, div):
    """step (a) as float32: the correctly rounded quotient"""
    return src.astype(np.float32) / np.float32(div)


def prep_frames(src, resize=None, *, div=1.0, mul=1.0, add=0.0, blur_k=0, blur_sigma=5.0, as_mask=False):
    """src (T, H, W, C) uint8 or float32 -> float64 (T, H', W', C), or with as_mask bool (T, H', W')"""
    v = convert(src, div).astype(np.float64)
    T, Hs, Ws, C = v.shape
    Hd, Wd = out_shape(Hs, Ws, resize)
    if (Hd, Wd) != (Hs, Ws):
        v = np.einsum("ij,tyjc->tyic", axis_matrix(Ws, Wd)[0], v)
        v = np.einsum("ij,tjxc->tixc", axis_matrix(Hs, Hd)[0], v)
    if blur_k:
        v = np.einsum("ij,tyjc->tyic", blur_matrix(Wd, blur_k, blur_sigma), v)
        v = np.einsum("ij,tjxc->tixc", blur_matrix(Hd, blur_k, blur_sigma), v)
    if as_mask:
        return v.sum(axis=-1) > 0
    if mul != 1.0 or add != 0.0:
        v = v * np.float64(np.float32(mul)) + np.float64(np.float32(add))
    return v


def tolerance(Hs, Ws, resize, vmax, blur_k=0):
    """What float32 arithmetic allows between the device and this restatement: 2 (n_h + n_v + 4) 2^-24 max|v| for the two
    resize passes (n: the largest tap count of a pass; a sum of n products carries at most about (n + 1) roundings of
    values bounded by max|v|, the weights being positive with sum 1), and 2 (2 k + 2) 2^-24 max|v| more for a blur."""
    Hd, Wd = out_shape(Hs, Ws, resize)
    n_h = n_v = 0
    if (Hd, Wd) != (Hs, Ws):
        n_h, n_v = axis_matrix(Ws, Wd)[1], axis_matrix(Hs, Hd)[1]
    tol = 2.0 * (n_h + n_v + 4) * U * vmax
    if blur_k:
        tol += 2.0 * (2 * blur_k + 2) * U * vmax
    return tol
