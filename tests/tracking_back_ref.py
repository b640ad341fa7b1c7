"""A numpy restatement of backward point tracking ("Point tracking"; include/gflow_hip.h,
gfl_track_history / gfl_track_backward), written for the tests: what the kernels must reproduce bit for bit.

For a query [t, y, x] with t > 0 and every frame i < t, with N_i the rows frame i has (N_0 <= N_1 <= ...):
  b = argmin over n < N_i of the float64 squared distance from (x, y) to uv_t[n]   (np.argmin: a NaN first, the lowest index
      among equal minima; the positions of the query's own frame, the candidates cut to frame i's rows)
  track = float32(float64(uv_i[b]) + ((x, y) - float64(uv_t[b])))
  occluded = |depth_map_i[rint(v)][rint(u)] - depth_i[b]| > thr in float32 at (u, v) = uv_i[b], rint half to even, a rounded
      pixel outside the image occluded.
Everything else -- the columns i >= t, anchor, shift, queries with t == 0 -- is tests/tracking_ref.py's track_loop."""
import numpy as np

from tests import tracking_ref as R


def row_occlusion(uv, depth, dm, thr=0.05):
    """the occlusion flag of EVERY row of one frame (what gfl_track_history keeps): (N,) bool"""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    depth = np.asarray(depth, np.float32).reshape(-1)
    dm = np.asarray(dm, np.float32)
    dm = dm.reshape(dm.shape[-2], dm.shape[-1])
    H, W = dm.shape
    ru, rv = np.round(uv[:, 0]), np.round(uv[:, 1])                  # (float32, half to even)
    inside = (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
    px = np.where(inside, ru, 0).astype(np.int64)
    py = np.where(inside, rv, 0).astype(np.int64)
    occ = np.ones(len(uv), bool)
    occ[inside] = (np.abs(dm[py, px] - depth) > np.float32(thr))[inside]
    return occ


def backward(queries, frames, thr=0.05):
    """queries: (Q, 3) rows [t, y, x]; frames: per fitted frame (uv (N_i, 2), depth (N_i,), depth_map (H, W)), float32.
    Returns dict(tracks (Q, T, 2) float32, occluded (Q, T) bool, back_anchor (Q, T) int32, written (Q, T) bool): only the
    columns i < t are written (``written``); the others are 0 / False / -1."""
    q = np.asarray(queries, dtype=np.float64)
    Q, T = q.shape[0], len(frames)
    uvs = [np.asarray(f[0], np.float32).reshape(-1, 2) for f in frames]
    occs = [row_occlusion(f[0], f[1], f[2], thr) for f in frames]
    tracks = np.zeros((Q, T, 2), np.float32)
    occluded = np.zeros((Q, T), bool)
    back = np.full((Q, T), -1, np.int32)
    written = np.zeros((Q, T), bool)
    for k in range(Q):
        t = int(q[k, 0])
        xy = q[k, [2, 1]]
        then = uvs[t].astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = np.sum((then - xy[None]) ** 2, axis=-1)
        for i in range(t):
            n_i = uvs[i].shape[0]
            b = int(np.argmin(d[:n_i]))
            back[k, i] = b
            with np.errstate(invalid="ignore"):
                tracks[k, i] = (uvs[i][b].astype(np.float64) + (xy - then[b])).astype(np.float32)
            occluded[k, i] = occs[i][b]
            written[k, i] = True
    return dict(tracks=tracks, occluded=occluded, back_anchor=back, written=written)


def track_loop(queries, frames, thr=0.05):
    """The whole contract of Tracker(backward=True): tests/tracking_ref.py's track_loop with the columns i < t replaced by
    ``backward``'s.  Returns dict(tracks, occluded, anchor, shift, back_anchor)."""
    out = R.track_loop(queries, frames, thr)
    back = backward(queries, frames, thr)
    w = back["written"]
    out["tracks"][w] = back["tracks"][w]
    out["occluded"][w] = back["occluded"][w]
    out["back_anchor"] = back["back_anchor"]
    return out
