"""The moving region through a clip fit, and its DAVIS J & F score ("Moving-region segmentation").

The contract is the reference's segmentation evaluation (gflow/benchmark.py:244-285): every frame's ``move_mask_*.png``
-- the smoothed concave hull of the moving splats' projections that the trainer forms after the frame's joint stage
(trainer.py:604-609) -- against the frame's ground-truth mask, with the DAVIS measures J (utils/measures/jaccard.py:
region intersection over union) and F (utils/measures/f_boundary.py: the F-measure of boundary precision and recall
within ``bound_pix`` pixels), and J&F their mean.

Recorded frame by frame on the device, finished once the clip is fitted:

- ``MoveSegRecorder.record`` keeps what ``SimpleGaussian._relabel_after_stage`` already has -- the projections ``uv`` and
  the selection ``within & ~still_mask`` -- as references: no copy, no read-back, no synchronisation while the clip is
  fitted;
- ``MoveSegRecorder.result`` makes ONE copy to the host, builds the hull masks there (gflow_amd/hull.py, host work on a
  few thousand points per frame), uploads them once and scores the whole clip with ONE gfl_seg_score launch
  (csrc/gfl_seg.hip), which leaves six integer counts per frame; J and F follow from the counts on the host
  (``scores_from_counts``), in the reference's own arithmetic.

A frame with at most five selected points carries the previous frame's mask (the reference's ``self.move_seg``
persists); a frame before any mask exists is invalid and not scored (the reference writes no file for it)."""
import math

import numpy as np
import torch

from . import _lib as L

COUNT_NAMES = ("inter", "uni", "n_fg", "n_gt", "fg_match", "gt_match")
MIN_POINTS = 6                    # trainer.py:606: a hull needs more than five points
MAX_RADIUS = 64                   # gfl_seg_score's largest disc


def bound_pix(H, W, bound_th=0.008):
    """The boundary tolerance in pixels as db_eval_boundary forms it (f_boundary.py:32-33): ``bound_th`` itself if it is
    >= 1 (an integer: the disc's radius), else ceil(bound_th * the length of the image's diagonal)."""
    if bound_th >= 1:
        if bound_th != int(bound_th):
            raise ValueError(f"bound_pix: bound_th >= 1 is a radius in pixels and must be an integer, got {bound_th}")
        return int(bound_th)
    return int(np.ceil(bound_th * np.linalg.norm((H, W))))


def seg_counts(pred, gt, radius, valid=None):
    """(T, 6) int64 counts (COUNT_NAMES) of the (T, H, W) uint8 device tensors ``pred`` and ``gt`` (nonzero = foreground):
    one gfl_seg_score launch on the current stream and one copy of the counts to the host.  ``valid``: (T,) uint8 device
    tensor or None; frames with 0 are not read and give a row of zeros."""
    L.need_device(pred, gt, valid)
    if pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or pred.dim() != 3 or pred.shape != gt.shape:
        raise ValueError("seg_counts: pred and gt must be uint8 tensors of one shape (T, H, W)")
    if valid is not None and (valid.dtype != torch.uint8 or tuple(valid.shape) != (pred.shape[0],)):
        raise ValueError("seg_counts: valid must be a (T,) uint8 tensor")
    pred, gt = pred.contiguous(), gt.contiguous()
    valid = None if valid is None else valid.contiguous()
    T, H, W = (int(v) for v in pred.shape)
    counts = torch.empty((T, 6), dtype=torch.int32, device=pred.device)
    L.check(L.load().gfl_seg_score(L.ptr(pred), L.ptr(gt), L.ptr(valid), T, H, W, int(radius), L.ptr(counts), L.stream()),
            "seg score")
    return (counts.cpu().numpy().view(np.uint32)).astype(np.int64)


def scores_from_counts(counts):
    """(J, F, J&F), float64 arrays of shape (T,), from (T, 6) counts -- in the reference's arithmetic:
    J = np.int64(inter) / np.float32(uni) (jaccard.py:33-34 divides by a float32 sum; the quotient is float64), 1 when
    both masks are empty; F = 2pr / (p + r) with the four precision / recall branches of f_boundary.py:53-64, 0 when
    p + r = 0."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 6)
    J, F = np.empty(len(c), np.float64), np.empty(len(c), np.float64)
    for t, (inter, uni, n_fg, n_gt, fg_match, gt_match) in enumerate(c):
        J[t] = 1.0 if uni == 0 else np.int64(inter) / np.float32(uni)
        if n_fg == 0 and n_gt > 0:
            p, r = 1.0, 0.0
        elif n_fg > 0 and n_gt == 0:
            p, r = 0.0, 1.0
        elif n_fg == 0 and n_gt == 0:
            p, r = 1.0, 1.0
        else:
            p, r = int(fg_match) / float(n_fg), int(gt_match) / float(n_gt)
        F[t] = 0.0 if p + r == 0 else 2 * p * r / (p + r)
    return J, F, (J + F) / 2


def evaluate(seg):
    """The clip's score as benchmark.py:277-285 forms it: the means of J, F and J&F over the scored frames of ``seg``
    (MoveSegRecorder.result(), or fit_clip's ``out["segmentation"]``).  NaN when no frame was scored."""
    v = np.asarray(seg["valid"], dtype=bool)
    n = int(v.sum())
    mean = lambda a: float(np.mean(np.asarray(a, dtype=np.float64)[v])) if n else math.nan
    return {"J": mean(seg["J"]), "F": mean(seg["F"]), "J&F": mean(seg["JF"]), "frames_scored": n}


class MoveSegRecorder:
    """The per-frame moving-region masks of one clip and their score.  ``frame`` is the frame the next ``record`` belongs
    to (fit_clip_steps sets it); a frame that is never recorded -- one without a joint stage -- carries the previous mask
    like a frame with too few points."""

    def __init__(self, T, H, W, device, bound_th=0.008):
        self.T, self.H, self.W = int(T), int(H), int(W)
        self.device = torch.device(device)
        self.radius = bound_pix(self.H, self.W, bound_th)
        if not 1 <= self.radius <= MAX_RADIUS:
            raise ValueError(f"MoveSegRecorder: boundary tolerance {self.radius} px outside [1, {MAX_RADIUS}]")
        self.frame = 0
        self.inputs = [None] * self.T                     # per frame (uv (N, 2) float32, sel (N,) bool), device tensors

    def record(self, uv, sel):
        """Frame ``self.frame``'s projections and selection, kept as they are (the caller no longer writes to them)."""
        if not 0 <= self.frame < self.T:
            raise ValueError(f"MoveSegRecorder.record: frame {self.frame} outside [0, {self.T})")
        self.inputs[self.frame] = (uv, sel)

    def fetch(self):
        """The recorded inputs on the host, per frame (uv float32 (N, 2), sel bool (N,)) or None: one device-to-host copy."""
        rec = [(t, x) for t, x in enumerate(self.inputs) if x is not None]
        out = [None] * self.T
        if not rec:
            return out
        parts = [x[0].detach().float().contiguous().view(torch.uint8).reshape(-1) for _, x in rec] \
            + [x[1].detach().to(torch.uint8).reshape(-1) for _, x in rec]
        buf = torch.cat(parts).cpu().numpy()
        n = [int(x[0].shape[0]) for _, x in rec]
        o_uv = np.concatenate([[0], np.cumsum([8 * k for k in n])])
        o_sel = o_uv[-1] + np.concatenate([[0], np.cumsum(n)])
        for j, (t, _) in enumerate(rec):
            uv = buf[o_uv[j]:o_uv[j + 1]].view(np.float32).reshape(n[j], 2)
            out[t] = (uv, buf[o_sel[j]:o_sel[j + 1]] != 0)
        return out

    def masks(self, host_inputs):
        """(masks (T, H, W) uint8 of 0 / 255, valid (T,) bool) from fetch()'s list, frames in order"""
        from .hull import FastConcaveHull2D
        masks = np.zeros((self.T, self.H, self.W), dtype=np.uint8)
        valid = np.zeros(self.T, dtype=bool)
        last = None
        for t, x in enumerate(host_inputs):
            if x is not None:
                pts = x[0][x[1]]
                if pts.shape[0] >= MIN_POINTS:
                    last = (FastConcaveHull2D(pts).mask(self.W, self.H) * 255).astype(np.uint8)
            if last is not None:
                masks[t], valid[t] = last, True
        return masks, valid

    def score(self, masks, valid, gt_masks):
        """(T, 6) int64 counts: the masks uploaded once, one gfl_seg_score launch against ``gt_masks`` (T frames of (H, W),
        nonzero / True = moving; device tensors or arrays), one copy back"""
        dev = self.device
        pred = torch.from_numpy(masks).to(dev)
        gt = torch.stack([torch.as_tensor(g).to(dev).reshape(self.H, self.W) != 0 for g in gt_masks]).to(torch.uint8)
        return seg_counts(pred, gt, self.radius, torch.from_numpy(valid.astype(np.uint8)).to(dev))

    def result(self, gt_masks):
        """dict(masks (T, H, W) uint8, valid (T,) bool, counts (T, 6) int64, J, F, JF (T,) float64; 0 in the rows of
        frames that are not valid) against the clip's ``gt_masks``."""
        if len(gt_masks) != self.T:
            raise ValueError(f"MoveSegRecorder.result: {len(gt_masks)} ground-truth masks for {self.T} frames")
        masks, valid = self.masks(self.fetch())
        counts = self.score(masks, valid, gt_masks)
        J, F, JF = scores_from_counts(counts)
        J[~valid], F[~valid], JF[~valid] = 0.0, 0.0, 0.0
        return dict(masks=masks, valid=valid, counts=counts, J=J, F=F, JF=JF)
