"""The track overlays' drawing rule (include/gflow_hip.h, "track overlays") restated in numpy, the way a painter works:
primitive by primitive in the reference's order, each as a per-pixel mask that overwrites what lies under it.  Nothing here
knows about paint indices, tiles or lists.  Also the same picture painted with PIL's ImageDraw (``pil_paint``), which is
what the rule is measured against: within one pixel, not equal."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 2 ** 20
LINE_W, CROSS_W, RADIUS = 2, 4, 4


def lut():
    return np.load(os.path.join(ROOT, "gflow_amd", "data", "colormaps.npz"))["gist_rainbow"].astype(np.float32)


def int_coords(tracks):
    """truncation toward zero after clamping to +-2^20; a NaN becomes -2^20"""
    v = np.asarray(tracks, dtype=np.float32).astype(np.float64)
    v = np.where(np.isnan(v), -float(LIMIT), np.clip(v, -LIMIT, LIMIT))
    return np.trunc(v).astype(np.int64)


def inside(p, W, H):
    return 0 <= p[0] < W and 0 <= p[1] < H


def usable(p, W, H):
    return inside(p, W, H) and p[0] != 0 and p[1] != 0


def segment_mask(H, W, a, b, w):
    """(H, W) bool: the pixels on the segment a -> b of width w"""
    py, px = np.mgrid[0:H, 0:W].astype(np.int64)
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    if (ax, ay) == (bx, by):
        return (px == ax) & (py == ay)
    dx, dy = bx - ax, by - ay
    qx, qy = px - ax, py - ay
    dot, dd = qx * dx + qy * dy, dx * dx + dy * dy
    cross = qx * dy - qy * dx
    return (dot >= 0) & (dot <= dd) & (4 * cross * cross <= w * w * dd)


def disc_mask(H, W, c, r=RADIUS):
    py, px = np.mgrid[0:H, 0:W].astype(np.int64)
    return (px - int(c[0])) ** 2 + (py - int(c[1])) ** 2 <= r * r + 2


def cross_mask(H, W, c, size=RADIUS, w=CROSS_W):
    x, y = int(c[0]), int(c[1])
    return segment_mask(H, W, (x - size, y), (x + size, y), w) | segment_mask(H, W, (x, y - size), (x, y + size), w)


def colours(y0, still_length=0, table=None):
    """(N, 3) uint8 from the integer y of frame 0, in floating point as matplotlib's Normalize and colormap call form it"""
    table = lut() if table is None else table
    y0 = np.asarray(y0, dtype=np.int64)
    n = len(y0)
    out = np.zeros((n, 3), dtype=np.uint8)

    def fill(sel, lo, hi):
        for i in sel:
            v = 0.0 if hi == lo else (float(y0[i]) - float(lo)) / (float(hi) - float(lo))
            idx = min(int(v * 256), 255)
            out[i] = np.trunc(table[idx].astype(np.float64) * 255.0).astype(np.uint8)

    if n:
        fill(range(n), y0.min(), y0.max())
        if 0 < still_length < n:
            fill(range(still_length, n), y0[still_length:].min(), y0[still_length:].max())
    return out


def paint(video, tracks, occluded, still_length=0, traces=True):
    """(T, H, W, 3) uint8.  ``traces=False``: the markers only (what a call whose lists did not fit leaves).
    The traces of frame t are those of frame t - 1 with the segments s = t - 1 painted over them, so they are kept as a layer
    of their own (colour and a painted flag) that grows frame by frame and is laid over the frame's video image."""
    video = np.asarray(video, dtype=np.uint8)
    T, H, W = video.shape[:3]
    pts = int_coords(tracks).reshape(T, -1, 2)
    N = pts.shape[1]
    occ = np.asarray(occluded).reshape(T, N) != 0
    col = colours(pts[0, :, 1], still_length) if T else None
    out = np.empty_like(video)
    layer = np.zeros((H, W, 3), dtype=np.uint8)
    painted = np.zeros((H, W), dtype=bool)
    for t in range(T):
        if t > 0 and traces:
            s = t - 1
            for i in range(N):
                a, b = pts[s, i], pts[s + 1, i]
                if inside(a, W, H) and inside(b, W, H) and a[0] != 0 and a[1] != 0:
                    # (the mask is formed on the window the segment can reach: every pixel outside it fails the rule)
                    x0, x1 = max(min(a[0], b[0]) - LINE_W, 0), min(max(a[0], b[0]) + LINE_W, W - 1) + 1
                    y0, y1 = max(min(a[1], b[1]) - LINE_W, 0), min(max(a[1], b[1]) + LINE_W, H - 1) + 1
                    m = segment_mask(y1 - y0, x1 - x0, (a[0] - x0, a[1] - y0), (b[0] - x0, b[1] - y0), LINE_W)
                    layer[y0:y1, x0:x1][m] = col[i]
                    painted[y0:y1, x0:x1][m] = True
        img = np.where(painted[..., None], layer, video[t])
        for i in range(N):
            p = pts[t, i]
            if usable(p, W, H):
                m = cross_mask(H, W, p) if occ[t, i] else disc_mask(H, W, p)
                img[m] = col[i]
        out[t] = img
    return out


def pairs_per_tile(tracks, W, H, tile=16):
    """how many (segment, tile) pairs each tile's list holds under the binning rule: the bounding box grown by the width"""
    pts = int_coords(tracks)
    T, N = pts.shape[:2]
    gx, gy = (W + tile - 1) // tile, (H + tile - 1) // tile
    counts = np.zeros((gy, gx), dtype=np.int64)
    for s in range(T - 1):
        for i in range(N):
            a, b = pts[s, i], pts[s + 1, i]
            if inside(a, W, H) and inside(b, W, H) and a[0] != 0 and a[1] != 0:
                x0, x1 = max(min(a[0], b[0]) - LINE_W, 0) // tile, min(max(a[0], b[0]) + LINE_W, W - 1) // tile
                y0, y1 = max(min(a[1], b[1]) - LINE_W, 0) // tile, min(max(a[1], b[1]) + LINE_W, H - 1) // tile
                counts[y0:y1 + 1, x0:x1 + 1] += 1
    return counts


def pil_paint(video, tracks, occluded, still_length=0):
    """the same picture with PIL's ImageDraw, one call per primitive and frame: what the reference's visualiser does on the
    host (line width 2; a cross of two lines of width 4; an ellipse of radius 4)"""
    from PIL import Image, ImageDraw
    video = np.asarray(video, dtype=np.uint8)
    T, H, W = video.shape[:3]
    pts = int_coords(tracks).reshape(T, -1, 2)
    N = pts.shape[1]
    occ = np.asarray(occluded).reshape(T, N) != 0
    col = [tuple(int(v) for v in c) for c in colours(pts[0, :, 1], still_length)] if T else []
    out = np.empty_like(video)
    for t in range(T):
        img = Image.fromarray(video[t].copy())
        draw = ImageDraw.Draw(img)
        for s in range(t):
            for i in range(N):
                a, b = pts[s, i], pts[s + 1, i]
                if inside(a, W, H) and inside(b, W, H) and a[0] != 0 and a[1] != 0:
                    draw.line((int(a[0]), int(a[1]), int(b[0]), int(b[1])), fill=col[i], width=LINE_W)
        for i in range(N):
            x, y = int(pts[t, i, 0]), int(pts[t, i, 1])
            if usable((x, y), W, H):
                if occ[t, i]:
                    draw.line([(x - RADIUS, y), (x + RADIUS, y)], fill=col[i], width=CROSS_W)
                    draw.line([(x, y - RADIUS), (x, y + RADIUS)], fill=col[i], width=CROSS_W)
                else:
                    draw.ellipse([(x - RADIUS, y - RADIUS), (x + RADIUS, y + RADIUS)], fill=col[i], outline=col[i])
        out[t] = np.array(img)
    return out
