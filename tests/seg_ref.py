"""This project's own numpy statement of the six counts behind DAVIS J and F and of the two scores, written from the
definition in include/gflow_hip.h (gfl_seg_score) -- what the GPU tests hold the kernel against and the host tests hold
against the golden values captured from the reference (tests/golden/davis_seg.npz)."""
import numpy as np


def boundary(mask):
    """(H, W) bool: a pixel that differs from its right, lower or lower-right neighbour; in the last row only the right
    neighbour counts, in the last column only the lower one, the bottom-right pixel never."""
    m = np.asarray(mask) != 0
    b = np.zeros(m.shape, dtype=bool)
    b[:-1, :-1] = (m[:-1, :-1] != m[:-1, 1:]) | (m[:-1, :-1] != m[1:, :-1]) | (m[:-1, :-1] != m[1:, 1:])
    b[-1, :-1] = m[-1, :-1] != m[-1, 1:]
    b[:-1, -1] = m[:-1, -1] != m[1:, -1]
    return b


def near(b, radius):
    """(H, W) bool: the pixels with a set pixel of ``b`` at (dx, dy), dx^2 + dy^2 <= radius^2; nothing outside the image."""
    H, W = b.shape
    r = int(radius)
    out = np.zeros((H, W), dtype=bool)
    x = np.arange(W)
    for dy in range(-r, r + 1):
        lo, hi = max(0, -dy), min(H, H - dy)                     # rows y with 0 <= y + dy < H
        if lo >= hi:
            continue
        h = int(np.floor(np.sqrt(r * r - dy * dy)))
        while h * h > r * r - dy * dy:
            h -= 1
        while (h + 1) * (h + 1) <= r * r - dy * dy:
            h += 1
        c = np.concatenate([np.zeros((hi - lo, 1), np.int64), np.cumsum(b[lo + dy:hi + dy], axis=1, dtype=np.int64)], axis=1)
        out[lo:hi] |= c[:, np.minimum(x + h + 1, W)] - c[:, np.maximum(x - h, 0)] > 0
    return out


def counts(pred, gt, radius):
    """int64 [inter, uni, n_fg, n_gt, fg_match, gt_match] of one (H, W) mask pair"""
    p, g = np.asarray(pred) != 0, np.asarray(gt) != 0
    bp, bg = boundary(p), boundary(g)
    return np.array([(p & g).sum(), (p | g).sum(), bp.sum(), bg.sum(), (bp & near(bg, radius)).sum(),
                     (bg & near(bp, radius)).sum()], dtype=np.int64)


def counts_stack(pred, gt, radius, valid=None):
    """(T, 6) int64; rows of frames with valid == 0 are zero"""
    out = np.zeros((len(pred), 6), dtype=np.int64)
    for t in range(len(pred)):
        if valid is None or valid[t]:
            out[t] = counts(pred[t], gt[t], radius)
    return out


def scores(c):
    """(J, F) of one row of counts, float64"""
    inter, uni, n_fg, n_gt, fg_match, gt_match = (int(v) for v in c)
    j = 1.0 if uni == 0 else float(np.int64(inter) / np.float32(uni))
    if n_fg == 0 and n_gt > 0:
        p, r = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        p, r = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        p, r = 1.0, 1.0
    else:
        p, r = fg_match / float(n_fg), gt_match / float(n_gt)
    f = 0.0 if p + r == 0 else 2 * p * r / (p + r)
    return j, f
