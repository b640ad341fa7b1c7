"""Object masks through a clip fit, and their DAVIS J & F per object ("Object propagation").

The semi-supervised half of DAVIS: the first frame's annotation -- an id per pixel, 0 = background -- is given, and every
later frame's ids are asked for.  The fit already knows which splats every pixel is made of and with what weight, so the
ids ride on the splats and are composited like a colour:

- ``ObjectRecorder.frame`` is called at the end of every frame with the frame's fit records and sorted tile lists (what
  one forward leaves on the device, as for ``flow.FlowRecorder``).  On frame 0 every splat takes the id of the prompt pixel
  its centre lies on (gfl_label_assign: the reference's ``init_mask_prompt_pts``, with ids).  On every frame
  gfl_label_frame (csrc/gfl_label.hip) composites the splats' ids into the frame's id map under the operator blend's own
  rule; then the rows that carry no id yet -- appended by a densification event, or outside the image until now -- take
  the id of the pixel of THIS map they lie on (gfl_label_assign again).  Nothing is read back;
- ``ObjectRecorder.result`` makes one copy of the maps to the host and, given ground truth, scores every object of every
  later frame with ONE gfl_seg_score launch (``segmentation.seg_counts``); ``evaluate`` forms the clip's means.

A pixel is UNKNOWN (255) where the labelled splats give less than ``min_weight`` of its blend weight: mostly background
colour, or splats that have no id yet.  An unknown pixel belongs to no object.

The frame with the prompt is never scored.  The DAVIS-2017 kit also drops the LAST frame of a sequence; this one keeps
it."""
import math

import numpy as np
import torch

from . import _lib as L
from . import segmentation as SG
from .fused import check_list_state, tile_count

UNKNOWN = 255                     # a map pixel without a label; a splat without one
MAX_ID = 15                       # gfl_label_frame composites at most 16 classes


def _id_map(a, H, W, what):
    """(H, W) uint8 host array of ids from an array or tensor of any integer (or bool) type"""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.shape != (H, W):
        raise ValueError(f"{what} must be ({H}, {W}), got {tuple(a.shape)}")
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must hold integer ids, got {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) > 255):
        raise ValueError(f"{what}: ids must lie in [0, 255]")
    return np.ascontiguousarray(a.astype(np.uint8))


class ObjectRecorder:
    """The per-frame object id maps of one clip.  ``prompt``: (H, W) integer ids of frame 0, 0 = background, at most
    ``MAX_ID``; K = the largest id + 1 classes are composited.  ``min_weight``: the blend weight (``sum of alpha T`` over
    the labelled splats) a pixel needs to get a label."""

    def __init__(self, n_frames, H, W, device, prompt, min_weight=0.5):
        self.T, self.H, self.W = int(n_frames), int(H), int(W)
        if self.T < 1 or self.H < 1 or self.W < 1:
            raise ValueError(f"ObjectRecorder: {self.T} frames of {self.H} x {self.W}")
        if not 0.0 < float(min_weight) <= 1.0:
            raise ValueError(f"ObjectRecorder: min_weight must lie in (0, 1], got {min_weight}")
        prompt = _id_map(prompt, self.H, self.W, "ObjectRecorder: prompt")
        top = int(prompt.max())
        if top > MAX_ID:
            raise ValueError(f"ObjectRecorder: object ids up to {MAX_ID}, the prompt has {top}")
        if top < 1:
            raise ValueError("ObjectRecorder: the prompt has no object (no non-zero id)")
        self.K = top + 1
        self.min_weight = float(min_weight)
        self.tiles = tile_count(self.W, self.H)
        if self.tiles > 16384:
            raise ValueError(f"ObjectRecorder: {self.W} x {self.H} has more than 16384 tiles")
        self.radius = SG.bound_pix(self.H, self.W)
        if not 1 <= self.radius <= SG.MAX_RADIUS:
            raise ValueError(f"ObjectRecorder: boundary tolerance {self.radius} px outside [1, {SG.MAX_RADIUS}]")
        self.device = torch.device(device)
        self.prompt = torch.from_numpy(prompt).to(self.device)
        L.need_device(self.prompt)
        self.maps = torch.full((self.T, self.H, self.W), UNKNOWN, dtype=torch.uint8, device=self.device)
        self._labels = torch.full((1024,), UNKNOWN, dtype=torch.uint8, device=self.device)   # rows >= _n are always 255
        self._n = 0
        self._last = -1
        self.rows = []                                     # the row count of every frame so far

    def _grow(self, n):
        """the label vector covers ``n`` rows, the new ones unlabelled (no allocation while the capacity lasts)"""
        if self._labels.shape[0] < n:
            buf = torch.full((max(n, 2 * self._labels.shape[0]),), UNKNOWN, dtype=torch.uint8, device=self.device)
            buf[:self._n].copy_(self._labels[:self._n])
            self._labels = buf
        self._n = n

    def frame(self, i, rec, n, ids, tile_range):
        """Frame ``i``'s final state: ``rec`` (>= n rows of 12 float32: the fit records), ``ids`` / ``tile_range`` (its sorted
        tile lists, int32, ``tile_range`` (tiles, 2)).  Frames come in order, rows are only ever appended.  Enqueued on the
        current stream; nothing is read back."""
        i, n = int(i), int(n)
        if i != self._last + 1 or i >= self.T:
            raise ValueError(f"ObjectRecorder.frame: frame {i} after frame {self._last} of {self.T}")
        if n < self._n:
            raise ValueError(f"ObjectRecorder.frame: {n} rows after {self._n} (rows are only ever appended)")
        check_list_state("ObjectRecorder.frame", rec, n, ids, tile_range, self.tiles)
        if not ids.is_contiguous() or not tile_range.is_contiguous():
            raise ValueError("ObjectRecorder.frame: ids and tile_range must be contiguous")
        lib = L.load()
        self._grow(n)
        assign = lambda m: L.check(lib.gfl_label_assign(L.ptr(rec), n, L.ptr(m), self.W, self.H, L.ptr(self._labels),
                                                        L.stream()), "label assign")
        if i == 0:
            assign(self.prompt)
        L.check(lib.gfl_label_frame(L.ptr(rec), n, L.ptr(ids), L.ptr(tile_range), L.ptr(self._labels), n, self.K, self.W,
                                    self.H, self.min_weight, UNKNOWN, L.ptr(self.maps[i]), None, L.stream()), "label frame")
        if i >= 1:
            assign(self.maps[i])
        self.rows.append(n)
        self._last = i

    @property
    def labels(self):
        """the splats' ids so far, (N,) uint8 on the device (255: none yet)"""
        return self._labels[:self._n]

    def result(self, gt=None):
        """dict(maps (T, H, W) uint8 -- ids, 255 = unknown --, labels (N,) uint8, rows (frames so far,) int64 -- every frame's
        row count --, n_objects = K - 1).  With ``gt``, a list of
        T per-frame (H, W) id maps (arrays or tensors) or None for a frame without one, also the score of the frames
        1 .. T - 1 that have one, per object k = 1 .. K - 1 the mask ``maps == k`` against ``gt == k``: counts (T, K - 1, 6)
        int64 (segmentation.COUNT_NAMES), J, F, JF (T, K - 1) float64 (0 in frames that are not scored), scored (T,) bool,
        and ``flat``: dict(J, F, JF, valid) over the (frame, object) pairs in a row -- what segmentation.evaluate and
        clip_reduce.reduce_davis take.  One copy of the maps to the host, one gfl_seg_score launch, one copy of its counts."""
        T, K = self.T, self.K
        out = dict(maps=self.maps.cpu().numpy(), labels=self.labels.cpu().numpy(), rows=np.asarray(self.rows, dtype=np.int64),
                   n_objects=K - 1)
        if gt is None:
            return out
        if len(gt) != T:
            raise ValueError(f"ObjectRecorder.result: {len(gt)} ground-truth maps for {T} frames")
        scored = np.zeros(T, dtype=bool)
        frames = [t for t in range(1, min(T, self._last + 1)) if gt[t] is not None]
        scored[frames] = True
        counts = np.zeros((T, K - 1, 6), dtype=np.int64)
        if frames:
            truth = torch.from_numpy(np.stack([_id_map(gt[t], self.H, self.W, f"ObjectRecorder.result: gt[{t}]")
                                               for t in frames])).to(self.device)
            ks = torch.arange(1, K, dtype=torch.uint8, device=self.device).view(1, K - 1, 1, 1)
            stack = lambda m: (m.unsqueeze(1) == ks).to(torch.uint8).reshape(-1, self.H, self.W)
            counts[frames] = SG.seg_counts(stack(self.maps[frames]), stack(truth), self.radius).reshape(len(frames), K - 1, 6)
        J, F, JF = (a.reshape(T, K - 1) for a in SG.scores_from_counts(counts.reshape(-1, 6)))
        J[~scored], F[~scored], JF[~scored] = 0.0, 0.0, 0.0
        out.update(counts=counts, J=J, F=F, JF=JF, scored=scored,
                   flat=dict(J=J.reshape(-1), F=F.reshape(-1), JF=JF.reshape(-1), valid=np.repeat(scored, K - 1)))
        return out


def write_id_maps(directory, maps, names, palette=None):
    """Write ``maps`` (T, H, W) uint8 as ``directory/<name>.png``, unknown pixels as 0: palette PNGs with ``palette``
    (PIL's flat [r, g, b, ...] list, the prompt file's), grey ids without one; returns the paths."""
    import os
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    paths = []
    for m, name in zip(np.asarray(maps, dtype=np.uint8), names):
        img = Image.fromarray(np.where(m == UNKNOWN, 0, m).astype(np.uint8), mode="P" if palette is not None else "L")
        if palette is not None:
            img.putpalette(palette)
        paths.append(os.path.join(directory, f"{name}.png"))
        img.save(paths[-1])
    return paths


def evaluate(result):
    """The clip's score: the means of J, F and J&F over the scored (frame, object) pairs of ``result``
    (ObjectRecorder.result(gt), or fit_clip's ``out["propagation"]``), ``per_object``: the same means per object id
    1 .. K - 1 over its scored frames, ``frames_scored`` and ``pairs_scored``.  NaN where nothing was scored.  The frame
    with the prompt is never scored; the last frame is (the DAVIS-2017 kit drops it)."""
    s = np.asarray(result["scored"], dtype=bool)
    n = int(s.sum())
    J, F, JF = (np.asarray(result[k], dtype=np.float64) for k in ("J", "F", "JF"))
    mean = lambda a: float(np.mean(a[s])) if n and a[s].size else math.nan
    per = [{"J": mean(J[:, k]), "F": mean(F[:, k]), "J&F": mean(JF[:, k])} for k in range(J.shape[1])]
    return {"J": mean(J), "F": mean(F), "J&F": mean(JF), "per_object": per, "frames_scored": n,
            "pairs_scored": n * J.shape[1]}
