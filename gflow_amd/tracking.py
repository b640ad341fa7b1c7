"""Point tracking through a clip fit, and its TAP-Vid score ("Point tracking").

The contract is the reference's ``eval_tracking`` (gflow/benchmark.py:54-178), computed on the device while the clip is
fitted instead of from per-frame checkpoints afterwards:

- a query ``[t, y, x]`` (pixels, float64) is anchored at the end of frame ``t`` to the splat whose projection lies closest
  (np.argmin over ALL rows, culled ones at (0, 0) included), with ``shift = (x, y) - uv[anchor]`` in float64
  (gfl_track_anchor);
- at the end of every frame ``i >= t``: ``track = float32(uv_i[anchor] + shift)`` and
  ``occluded = |depth_map_i[rint(v)][rint(u)] - depth_i[anchor]| > 0.05`` in float32 at the anchor's own (u, v)
  (gfl_track_frame).

Splat rows are only ever appended (densification writes the new rows behind the old ones, trainer.densification_postfix),
so an anchor's row index stays valid in every later frame.  Divergences where the reference is undefined or fails: frames
before a query's frame give (0, 0) and occluded; a rounded pixel outside the image is occluded.

Backward tracking (``Tracker(backward=True)``, opt-in) fills the frames before a query's frame instead.  Frame ``i < t`` has
only the first ``N_i`` of frame ``t``'s rows, so the query is carried back by ``b = back_anchor[q][i]``: the argmin over the
rows ``n < N_i`` of the same float64 distance to ``uv_t[n]`` (the query's own frame's positions; gfl_track_anchor's key
order), ``track = float32(uv_i[b] + (xy - uv_t[b]))`` and the occlusion rule above on row ``b`` of frame ``i``
(gfl_track_history per frame, gfl_track_backward once at the end of the clip).  Where the forward anchor already existed in
frame ``i`` (``anchor < N_i``) it is the minimum of the prefix too: ``b == anchor``, and the column is what the forward rule
would give run backwards; another splat is chosen only where the anchor was born later.

``tapvid_metrics`` is the TAP-Vid metric (Doersch et al., 2022) -- occlusion accuracy, position accuracy below 1, 2, 4, 8,
16 pixels and Jaccard at those thresholds -- with the inputs, keys and query modes of the reference's
``compute_tapvid_metrics``.  ``evaluate`` scores a clip's tracks the way ``eval_tracking`` does (coordinates rescaled to
256 x 256, 'strided' queries)."""
import pickle

import numpy as np
import torch

from . import _lib as L

THRESHOLDS = (1, 2, 4, 8, 16)
OCC_THRESHOLD = 0.05              # benchmark.py's depth test, scene depth units


def check_queries(queries, n_frames):
    """``queries`` as a (Q, 3) float64 array of rows [t, y, x]; ValueError unless every t is an integer in [0, n_frames)
    and every x, y is finite."""
    q = np.asarray(queries, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 3:
        raise ValueError(f"track queries: expected rows [t, y, x], got shape {q.shape}")
    t = q[:, 0]
    bad_t = ~np.isfinite(t) | (t != np.round(t)) | (t < 0) | (t >= n_frames)
    if bad_t.any():
        raise ValueError(f"track queries: {int(bad_t.sum())} query frame(s) are not a fitted frame in [0, {n_frames}) "
                         f"(first: {t[np.argmax(bad_t)]})")
    if not np.isfinite(q[:, 1:]).all():
        raise ValueError("track queries: x and y must be finite")
    return q


class Tracker:
    """The device side of point tracking for one clip: the queries sorted by frame once (frame i's new queries are then a
    contiguous range the host knows -- nothing is read back per frame), the output buffers filled with (0, 0) and
    occluded up front, and per frame one gfl_track_anchor for the frame's new queries and one gfl_track_frame for every
    query anchored so far.

    ``backward=True``: the frames before a query's frame are tracked too (the module's docstring).  ``frame()`` must then be
    called for the frames 0, 1, ... in order, every frame with at least one row and no fewer than the frame before; each call
    also keeps the frame's (u, v) and per-row occlusion bit (one more launch, 9 bytes per row: about 54 MB for 60 frames of
    100 k splats, and as much again while ``result()`` joins the slices); ``result()`` runs the backward pass once and has
    ``back_anchor`` as well."""

    def __init__(self, queries, n_frames, device, occ_threshold=OCC_THRESHOLD, backward=False):
        q = check_queries(queries, n_frames)
        self.Q, self.T = q.shape[0], int(n_frames)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        L.need_device(torch.empty(0, device=self.device))
        self.occ_threshold = float(occ_threshold)
        t = q[:, 0].astype(np.int64)
        self.order = np.argsort(t, kind="stable")
        self.starts = np.searchsorted(t[self.order], np.arange(self.T + 1), side="left").tolist()   # frame i: [starts[i], starts[i+1])
        Q, T = self.Q, self.T
        self.backward = bool(backward)
        self._kept = []
        # one device buffer behind all outputs: result() is one copy to the host
        off = self._offsets()
        self._buf = torch.zeros(max(off[-1], 16), dtype=torch.uint8, device=self.device)
        self.shift = self._buf[off[0]:off[1]].view(torch.float64).view(Q, 2)
        self.tracks = self._buf[off[1]:off[2]].view(torch.float32).view(Q, T, 2)
        self.anchor = self._buf[off[2]:off[3]].view(torch.int32).view(Q)
        self.occluded = self._buf[off[4]:off[5]].view(Q, T)
        self.occluded.fill_(1)
        if self.backward:
            self.back_anchor = self._buf[off[3]:off[4]].view(torch.int32).view(Q, T)
            self.back_anchor.fill_(-1)
            self._hist, self._rows = [], []                                      # per frame: (uv, occ) slices; N_i
            self._query_frame = self._upload(np.ascontiguousarray(t[self.order].astype(np.int32)))
        xy = np.ascontiguousarray(q[self.order][:, [2, 1]])                  # (x, y), the order of uv
        self.query_xy = torch.empty(Q, 2, dtype=torch.float64, device=self.device)
        self.query_xy.copy_(torch.from_numpy(xy).pin_memory() if self.device.type == "cuda" else torch.from_numpy(xy),
                            non_blocking=True)
        self._xy_host = xy                                                       # (kept alive until the copy has run)
        self._ws = None
        self.frames_done = []

    def _offsets(self):
        """byte offsets of shift, tracks, anchor, back_anchor (empty without ``backward``) and occluded in the output buffer"""
        Q, T = self.Q, self.T
        nb = [16 * Q, 8 * Q * T, 4 * Q, 4 * Q * T if self.backward else 0, Q * T]
        return np.concatenate([[0], np.cumsum(nb)]).astype(np.int64).tolist()

    def _upload(self, a):
        """a host array as a device tensor, copied without a synchronisation (the pinned source is kept alive)"""
        src = torch.from_numpy(a)
        if self.device.type == "cuda":
            src = src.pin_memory()
        out = torch.empty(a.shape, dtype=src.dtype, device=self.device)
        out.copy_(src, non_blocking=True)
        self._kept.append(src)
        return out

    def frame(self, i, uv, uv_stride, depth, depth_stride, depth_map):
        """Frame ``i``'s state: ``uv`` (N rows, (u, v) in the first two of every ``uv_stride`` floats), ``depth`` (N rows of
        ``depth_stride`` floats), ``depth_map`` (H, W) -- float32 device tensors (views of the fit records are fine).
        Enqueued on the current stream; nothing is read back."""
        i = int(i)
        if not 0 <= i < self.T:
            raise ValueError(f"Tracker.frame: frame {i} outside [0, {self.T})")
        for x in (uv, depth, depth_map):
            if x.dtype != torch.float32 or x.device != self.device:
                raise ValueError("Tracker.frame: uv, depth and depth_map must be float32 tensors on the tracker's device")
        N = int(uv.shape[0])
        H, W = int(depth_map.shape[-2]), int(depth_map.shape[-1])
        if not depth_map.is_contiguous() or depth_map.numel() != H * W:
            raise ValueError("Tracker.frame: depth_map must be a contiguous (H, W) plane")
        if uv.storage_offset() + (N - 1) * uv_stride + 2 > uv.untyped_storage().nbytes() // 4 and N > 0:
            raise ValueError("Tracker.frame: uv rows reach past the end of their storage")
        if depth.storage_offset() + (N - 1) * depth_stride + 1 > depth.untyped_storage().nbytes() // 4 and N > 0:
            raise ValueError("Tracker.frame: depth rows reach past the end of their storage")
        if self.backward:
            if i != len(self._rows):
                raise ValueError(f"Tracker.frame(backward=True): frame {i} given, frame {len(self._rows)} is next")
            if N < 1 or (self._rows and N < self._rows[-1]):
                raise ValueError(f"Tracker.frame(backward=True): frame {i} has {N} rows"
                                 + (f", the frame before {self._rows[-1]}" if self._rows else "")
                                 + ": every frame needs one, and rows are only ever appended")
        lib = L.load()
        s = L.stream()
        a, b = self.starts[i], self.starts[i + 1]
        if self.backward and self.Q:
            h_uv = torch.empty(N, 2, dtype=torch.float32, device=self.device)
            h_occ = torch.empty(N, dtype=torch.uint8, device=self.device)
            L.check(lib.gfl_track_history(L.ptr(uv), int(uv_stride), L.ptr(depth), int(depth_stride), N, L.ptr(depth_map), W, H,
                                          self.occ_threshold, L.ptr(h_uv), L.ptr(h_occ), s), "track history")
            self._hist.append((h_uv, h_occ))
        if self.backward:
            self._rows.append(N)
        if b > a:
            if N < 1:
                raise ValueError(f"Tracker.frame: frame {i} has queries and no splats")
            need = lib.gfl_track_anchor_workspace_bytes(b - a, N)
            if self._ws is None or self._ws.numel() < need:
                self._ws = L.scratch(need, self.device)
            L.check(lib.gfl_track_anchor(L.ptr(uv), int(uv_stride), N, L.ptr(self.query_xy[a:b]), b - a,
                                         L.ptr(self.anchor[a:b]), L.ptr(self.shift[a:b]), L.ptr(self._ws), self._ws.numel(), s),
                    "track anchor")
        if b > 0:
            L.check(lib.gfl_track_frame(L.ptr(uv), int(uv_stride), L.ptr(depth), int(depth_stride), N, L.ptr(depth_map), W, H,
                                        L.ptr(self.anchor), L.ptr(self.shift), b, i, self.T, self.occ_threshold,
                                        L.ptr(self.tracks), L.ptr(self.occluded), s), "track frame")
        self.frames_done.append(i)

    def _run_backward(self):
        """gfl_track_backward over the frames recorded so far, for the queries whose frame is among them; the history
        slices are joined once and dropped"""
        n_rec = len(self._hist)
        n_q = self.starts[n_rec] if n_rec else 0                                 # (sorted by frame: a prefix)
        if n_rec < 2 or n_q == 0:
            self._hist = []
            return
        lib = L.load()
        hist_uv = torch.cat([h[0] for h in self._hist])
        hist_occ = torch.cat([h[1] for h in self._hist])
        self._hist = []
        # (the outputs' rows have T columns: a frame that was never recorded is an empty one, behind every query's frame)
        rows = self._rows[:n_rec] + [0] * (self.T - n_rec)
        row_start = self._upload(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64))
        ws = L.scratch(lib.gfl_track_backward_workspace_bytes(n_q, self.T), self.device)
        L.check(lib.gfl_track_backward(L.ptr(hist_uv), L.ptr(hist_occ), L.ptr(row_start), self.T, L.ptr(self.query_xy),
                                       L.ptr(self._query_frame), n_q, L.ptr(self.tracks), L.ptr(self.occluded),
                                       L.ptr(self.back_anchor), L.ptr(ws), ws.numel(), L.stream()), "track backward")

    def result(self):
        """dict(tracks (Q, T, 2) float32, occluded (Q, T) bool, anchor (Q,) int64, shift (Q, 2) float64), host arrays in
        the caller's query order.  One device-to-host copy.  With ``backward=True`` the backward pass runs first (once) and
        the dict also has back_anchor (Q, T) int32: the row that carries query q in frame i < t, -1 where nothing was
        written (i >= t)."""
        if self.backward and self._hist:
            self._run_backward()
        buf = self._buf.cpu().numpy()
        Q, T = self.Q, self.T
        off = self._offsets()
        shift = buf[off[0]:off[1]].view(np.float64).reshape(Q, 2)
        tracks = buf[off[1]:off[2]].view(np.float32).reshape(Q, T, 2)
        anchor = buf[off[2]:off[3]].view(np.int32).reshape(Q)
        occ = buf[off[4]:off[5]].reshape(Q, T)
        out = dict(tracks=np.empty((Q, T, 2), np.float32), occluded=np.empty((Q, T), bool), anchor=np.empty(Q, np.int64),
                   shift=np.empty((Q, 2), np.float64))
        out["tracks"][self.order] = tracks
        out["occluded"][self.order] = occ != 0
        out["anchor"][self.order] = anchor
        out["shift"][self.order] = shift
        if self.backward:
            out["back_anchor"] = np.empty((Q, T), np.int32)
            out["back_anchor"][self.order] = buf[off[3]:off[4]].view(np.int32).reshape(Q, T)
        return out


# ---------------------------------------------------------------------------------------------------------- TAP-Vid data
def first_visible_queries(points, occluded, H, W):
    """Rows [t, y, x] (float64, pixels) of the first frame where each ground-truth track is visible (frame 0 for a track
    that is never visible), as the reference's extract_first_visible_points + the scaling of benchmark.py:86-88.
    ``points``: (Q, T, 2) normalised (x, y); ``occluded``: (Q, T) bool."""
    points, occluded = np.asarray(points), np.asarray(occluded, dtype=bool)
    t = np.argmax(~occluded, axis=1)
    at = points[np.arange(points.shape[0]), t]                              # (Q, 2) x, y at that frame
    q = np.empty((points.shape[0], 3), dtype=np.float64)
    q[:, 0] = t
    q[:, 1] = at[:, 1]
    q[:, 2] = at[:, 0]
    q[:, 1] = q[:, 1] * H
    q[:, 2] = q[:, 2] * W
    return q


def strided_queries(points, occluded, H, W, stride=5):
    """TAP-Vid's 'strided' protocol (Doersch et al., 2022, sample_queries_strided): one query per ground-truth track and per
    ``stride``-th frame (0, stride, 2 stride, ...) where the track is visible.  Returns (queries (M, 3) float64 rows
    [t, y, x] in pixels, scaled as first_visible_queries scales them; source (M,) int64, the track each query was taken
    from), ordered by frame, then by track.  Most of these queries have frames before them: ``Tracker(backward=True)``."""
    points, occluded = np.asarray(points), np.asarray(occluded, dtype=bool)
    if int(stride) < 1:
        raise ValueError(f"strided_queries: stride {stride}")
    rows, src = [], []
    for t in range(0, occluded.shape[1], int(stride)):
        j = np.where(~occluded[:, t])[0]
        q = np.empty((len(j), 3), dtype=np.float64)
        q[:, 0] = t
        q[:, 1] = points[j, t, 1]
        q[:, 2] = points[j, t, 0]
        q[:, 1] = q[:, 1] * H
        q[:, 2] = q[:, 2] * W
        rows.append(q)
        src.append(j)
    return np.concatenate(rows) if rows else np.empty((0, 3)), (np.concatenate(src) if src else np.empty(0)).astype(np.int64)


def read_tapvid_pickle(path):
    """(points (Q, T, 2) normalised x, y; occluded (Q, T) bool) of a TAP-Vid ``tracking.pkl``"""
    with open(path, "rb") as f:
        d = pickle.load(f)
    return np.asarray(d["points"]), np.asarray(d["occluded"], dtype=bool)


def write_tapvid_pickle(path, points, occluded):
    with open(path, "wb") as f:
        pickle.dump({"points": np.asarray(points, dtype=np.float32), "occluded": np.asarray(occluded, dtype=bool)}, f)


def tapvid_metrics(query_points, gt_occluded, gt_tracks, pred_occluded, pred_tracks, query_mode, trackwise=False):
    """TAP-Vid metrics per video (``trackwise``: per track).  Shapes: query_points (b, n, 3) rows [t, y, x];
    gt_occluded / pred_occluded (b, n, T) bool; gt_tracks / pred_tracks (b, n, T, 2) rows [x, y] in the raster the
    thresholds are meant for (256 x 256 in the paper).  ``query_mode`` 'first': only the frames after a track's query
    frame count; 'strided': every frame but the query frame.  Returns occlusion_accuracy, pts_within_{1,2,4,8,16},
    jaccard_{1,2,4,8,16}, average_jaccard, average_pts_within_thresh as float64 arrays of shape (b,) or (b, n).  A ratio
    with nothing to count is NaN (0 / 0)."""
    gt_occluded = np.asarray(gt_occluded, dtype=bool)
    pred_occluded = np.asarray(pred_occluded, dtype=bool)
    n_t = gt_tracks.shape[2]
    qt = np.round(np.asarray(query_points)[..., 0]).astype(np.int32)[..., None]          # (b, n, 1)
    frames = np.arange(n_t, dtype=np.int32)
    if query_mode == "first":
        counted = frames > qt
    elif query_mode == "strided":
        counted = frames != qt
    else:
        raise ValueError(f"unknown query mode {query_mode!r}")
    axes = (2,) if trackwise else (1, 2)
    total = lambda m: np.sum(m & counted, axis=axes)
    vis_gt, vis_pred = ~gt_occluded, ~pred_occluded
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["occlusion_accuracy"] = total(gt_occluded == pred_occluded) / np.sum(counted, axis=axes)
        d2 = np.sum(np.square(pred_tracks - gt_tracks), axis=-1)
        n_vis = total(vis_gt)
        pts, jac = [], []
        for th in THRESHOLDS:
            close = d2 < np.square(th)
            hit = close & vis_gt
            pts.append(total(hit) / n_vis)
            wrong_visible = vis_pred & (gt_occluded | ~close)
            jac.append(total(hit & vis_pred) / (n_vis + total(wrong_visible)))
            out[f"pts_within_{th}"] = pts[-1]
            out[f"jaccard_{th}"] = jac[-1]
        out["average_jaccard"] = np.mean(np.stack(jac, axis=1), axis=1)
        out["average_pts_within_thresh"] = np.mean(np.stack(pts, axis=1), axis=1)
    return out


def evaluate(pred, points, occluded, H, W, n_frames, queries=None, source=None):
    """The clip's score as benchmark.py:144-172 forms it: ``pred`` is Tracker.result() (or fit_clip's ``out["tracks"]``)
    for the first-visible queries of (``points``, ``occluded``) -- the tracking.pkl arrays, normalised -- over the
    ``n_frames`` fitted frames (the reference fits len - 1 frames and slices its ground truth with [:, :-1]; here the
    ground truth is cut to the fitted frames).  Coordinates go to x / W * 255, y / H * 255; 'strided' queries.  Returns a
    dict of floats.
    ``queries`` (M, 3) with ``source`` (M,): ``pred`` is for these queries instead (strided_queries' pair, or a subset of
    it), query m scored against the ground-truth track ``source[m]``."""
    points, occluded = np.asarray(points), np.asarray(occluded, dtype=bool)
    if (queries is None) != (source is None):
        raise ValueError("evaluate: queries and source come together")
    if queries is None:
        q = first_visible_queries(points, occluded, H, W)
    else:
        q, source = np.asarray(queries, dtype=np.float64), np.asarray(source, dtype=np.int64)
        if q.ndim != 2 or q.shape[1] != 3 or source.shape != (q.shape[0],):
            raise ValueError(f"evaluate: queries {q.shape} and source {source.shape} do not match")
        points, occluded = points[source], occluded[source]
    gt = points[None, :, :n_frames].copy()
    gt[..., 0] = gt[..., 0] * W
    gt[..., 1] = gt[..., 1] * H
    gt[..., 0] = gt[..., 0] / W * 255
    gt[..., 1] = gt[..., 1] / H * 255
    pt = np.asarray(pred["tracks"])[None].copy()
    pt[..., 0] = pt[..., 0] / W * 255
    pt[..., 1] = pt[..., 1] / H * 255
    m = tapvid_metrics(q[None], occluded[None, :, :n_frames], gt, np.asarray(pred["occluded"])[None], pt, "strided")
    return {k: float(v[0]) for k, v in m.items()}
