"""A numpy restatement of the reference's tracking frame loop (gflow/benchmark.py:98-139), written for the tests: what
gflow_amd.tracking's kernels must reproduce bit for bit, plus this project's documented divergences (frames before a
query's frame: (0, 0) and occluded; a rounded pixel outside the image: occluded)."""
import numpy as np


def nearest(uv, xy):
    """np.argmin over the rows of uv (float32, N x 2) of the float64 squared distance to each query (x, y)"""
    uv = np.asarray(uv, dtype=np.float32)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    d = np.sum((uv[:, None].astype(np.float64) - xy[None]) ** 2, axis=-1)
    return np.argmin(d, axis=0)


def track_loop(queries, frames, thr=0.05):
    """queries: (Q, 3) rows [t, y, x] (pixels); frames: per fitted frame (uv (N, 2) float32, depth (N,) float32,
    depth_map (H, W) float32).  Returns dict(tracks, occluded, anchor, shift)."""
    q = np.asarray(queries, dtype=np.float64)
    Q, T = q.shape[0], len(frames)
    tracks = np.zeros((Q, T, 2), np.float32)
    occ = np.ones((Q, T), bool)
    anchor = np.zeros(Q, np.int64)
    shift = np.zeros((Q, 2), np.float64)
    done = np.zeros(Q, bool)
    thr32 = np.float32(thr)
    for i, (uv, depth, dm) in enumerate(frames):
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        depth = np.asarray(depth, np.float32).reshape(-1)
        dm = np.asarray(dm, np.float32).reshape(dm.shape[-2], dm.shape[-1])
        H, W = dm.shape
        new = np.where(q[:, 0] == i)[0]
        if len(new):
            xy = q[new][:, [2, 1]]
            a = nearest(uv, xy)
            anchor[new] = a
            shift[new] = xy - uv[a].astype(np.float64)
            done[new] = True
        idx = np.where(done)[0]
        if len(idx) == 0:
            continue
        a = anchor[idx]
        tracks[idx, i] = (uv[a].astype(np.float64) + shift[idx]).astype(np.float32)
        ru, rv = np.round(uv[a, 0]), np.round(uv[a, 1])              # (float32, half to even)
        inside = (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
        o = np.ones(len(idx), bool)
        px = np.where(inside, ru, 0).astype(np.int64)
        py = np.where(inside, rv, 0).astype(np.int64)
        diff = np.abs(dm[py, px] - depth[a])
        o[inside] = (diff > thr32)[inside]
        occ[idx, i] = o
    return dict(tracks=tracks, occluded=occ, anchor=anchor, shift=shift)
