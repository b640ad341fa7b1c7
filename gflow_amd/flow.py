"""The dense optical flow a clip fit implies, and its end-point error ("Flow score").

The flow is the input the method is named after; the fit only sees it as a loss on splat centres.  What the fitted splats
say about motion is recorded here pair by pair on the device, read once the clip is fitted:

- ``FlowRecorder.frame`` is called at the end of every frame with the frame's fit records and sorted tile lists (what one
  forward leaves on the device).  From the second frame on it launches gfl_flow_pair (csrc/gfl_flow.hip) for the pair
  (previous frame, this frame): every pixel of the PREVIOUS frame blends the motion ``uv_now - uv_before`` of the splats
  it sees, under the operator blend's own rule, and the result is held against the flow the fit was given.  Then it keeps
  copies of this frame's records and lists for the next call (the engine that made them is reused in between);
- ``FlowRecorder.result`` makes ONE copy to the host; ``evaluate`` pools the pairs into the clip's numbers.

The maps are forward flow ``i -> i + 1`` on frame ``i``'s pixel grid, in pixels, (x, y) order -- the convention of the
``.flo`` files a clip comes with (``frames[i]["flow"]``)."""
import numpy as np
import torch

from . import _lib as L
from .fused import REC, check_list_state, tile_count

CLASSES = ("all", "still", "moving")
SUM_NAMES = ("n_pixels", "n_valid", "epe_sum", "n_1px", "n_3px", "n_5px")
UNKNOWN_FLOW = 1e10               # Middlebury's mark of a pixel without a flow (both components), as written to .flo


def pack_records(uv, conic, opacity, depth):
    """Fit records (N, 12) float32 from the operators' outputs -- uv (N, 2), conic (N, 3), opacity (N, 1), depth (N, 1) --
    in the fused forward's layout (u v A B | C opacity . . | . depth . .): the operator path's input to FlowRecorder."""
    n = uv.shape[0]
    rec = torch.zeros(n, REC, dtype=torch.float32, device=uv.device)
    rec[:, 0:2] = uv.detach().float()
    rec[:, 2:5] = conic.detach().float()
    rec[:, 5] = opacity.detach().float().reshape(-1)
    rec[:, 9] = depth.detach().float().reshape(-1)
    return rec


def operator_state(input_group):
    """(rec, n, ids, tile_range) of the splats of ``input_group`` ([xyz, scale, rotate, opacity, rgb, intr, extr, bg, W, H],
    render.render_multiple's) through the five operators: projection, covariance, EWA, the tile sort -- FlowRecorder.frame's
    arguments where no fused engine holds them."""
    from . import msplat
    xyz, scale, rotate, opacity, rgb, intr, extr, bg, W, H = input_group
    uv, depth = msplat.project_point(xyz, intr, extr, W, H)
    visible = depth != 0
    cov3d = msplat.compute_cov3d(scale, rotate, visible)
    conic, radius, tiles_touched = msplat.ewa_project(xyz, cov3d, intr, extr, uv, W, H, visible)
    ids, tile_range = msplat.sort_gaussian(uv, depth, W, H, radius, tiles_touched)
    return pack_records(uv, conic, opacity, depth), int(uv.shape[0]), ids.to(torch.int32), tile_range.to(torch.int32)


def scores_from_sums(sums):
    """Per-pair ratios from gfl_flow_pair's sums (..., 3, 6): dict of EPE, acc_1px, acc_3px, acc_5px, coverage, each
    (..., 3) float64 over the classes (all, still, moving).  A ratio with nothing to count is NaN."""
    s = np.asarray(sums, dtype=np.float64)
    n_px, n_v = s[..., 0], s[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(EPE=s[..., 2] / n_v, acc_1px=s[..., 3] / n_v, acc_3px=s[..., 4] / n_v, acc_5px=s[..., 5] / n_v,
                    coverage=n_v / n_px)


class FlowRecorder:
    """The per-pair flow sums (and, with ``keep_maps``, the flow maps) of one clip.  ``min_weight``: the blend weight
    (``sum of alpha T`` over the splats that still exist in the next frame) a pixel needs for its flow to count -- below
    it the pixel is mostly background or splats that were culled, and it is left out of the score (``coverage`` says
    how many are in)."""

    def __init__(self, n_frames, H, W, device, min_weight=0.5, keep_maps=False):
        self.T, self.H, self.W = int(n_frames), int(H), int(W)
        if self.T < 1 or self.H < 1 or self.W < 1:
            raise ValueError(f"FlowRecorder: {self.T} frames of {self.H} x {self.W}")
        if not 0.0 < float(min_weight) <= 1.0:
            raise ValueError(f"FlowRecorder: min_weight must lie in (0, 1], got {min_weight}")
        self.min_weight = float(min_weight)
        self.device = torch.device(device)
        self.P = self.T - 1
        self.tiles = tile_count(self.W, self.H)
        self.sums = torch.zeros((max(self.P, 1), 3, 6), dtype=torch.float64, device=self.device)
        L.need_device(self.sums)
        need = L.load().gfl_flow_workspace_bytes(self.W, self.H)
        if need == 0:
            raise ValueError(f"FlowRecorder: {self.W} x {self.H} has more than 16384 tiles")
        self.ws = L.scratch(need, self.device)
        self.keep_maps = bool(keep_maps)
        self.maps = self.valid = None
        if self.keep_maps and self.P > 0:
            self.maps = torch.zeros((self.P, self.H, self.W, 2), dtype=torch.float32, device=self.device)
            self.valid = torch.zeros((self.P, self.H, self.W), dtype=torch.uint8, device=self.device)
        self._rec = self._ids = self._range = None         # frame A: this recorder's own copies
        self._n = 0
        self._last = -1
        self.inputs = None                                 # a list: clones of every pair's kernel inputs are appended

    def _keep(self, name, src):
        """copy ``src`` into this recorder's buffer ``name`` (grown when needed; no allocation in the steady state)"""
        buf = getattr(self, name)
        n = src.shape[0]
        if buf is None or buf.shape[0] < n:
            buf = torch.empty((max(n, 1),) + tuple(src.shape[1:]), dtype=src.dtype, device=self.device)
            setattr(self, name, buf)
        buf[:n].copy_(src)

    def frame(self, i, rec, n, ids, tile_range, gt_flow=None, move_mask=None):
        """Frame ``i``'s final state: ``rec`` (>= n rows of 12 float32: the fit records), ``ids`` / ``tile_range`` (its sorted
        tile lists, int32, ``tile_range`` (tiles, 2)).  For ``i >= 1`` also ``gt_flow`` (H, W, 2) float32 and ``move_mask``
        (H, W) bool / uint8 or None -- those of FRAME ``i - 1``: the flow from it to frame ``i`` on its grid.  Frames come
        in order.  Enqueued on the current stream; nothing is read back."""
        i, n = int(i), int(n)
        if i != self._last + 1 or i >= self.T:
            raise ValueError(f"FlowRecorder.frame: frame {i} after frame {self._last} of {self.T}")
        check_list_state("FlowRecorder.frame", rec, n, ids, tile_range, self.tiles)      # (ids, tile_range: copied below, any strides)
        if i >= 1:
            if gt_flow is None or tuple(gt_flow.shape) != (self.H, self.W, 2):
                raise ValueError(f"FlowRecorder.frame: gt_flow must be ({self.H}, {self.W}, 2)")
            L.need_device(gt_flow, move_mask)
            gt = gt_flow.detach().float().contiguous()
            mm = None
            if move_mask is not None:
                mm = move_mask.detach().reshape(self.H, self.W)
                if mm.dtype == torch.bool:
                    mm = mm.contiguous().view(torch.uint8)          # (a bool is a byte 0 / 1: no copy)
                elif mm.dtype != torch.uint8:
                    mm = (mm != 0).to(torch.uint8)
                mm = mm.contiguous()
            p = i - 1
            uv_b, depth_b = rec[:n, 0:2], rec[:n, 9]
            if self.inputs is not None:
                self.inputs.append(dict(rec_a=self._rec[:self._n].clone(), ids=self._ids.clone(),
                                        tile_range=self._range[:self.tiles].clone(), uv_b=uv_b.clone(),
                                        depth_b=depth_b.clone(), gt_flow=gt.clone(),
                                        move_mask=None if mm is None else mm.clone()))
            L.check(L.load().gfl_flow_pair(
                L.ptr(self._rec), self._n, L.ptr(self._ids), L.ptr(self._range), L.ptr(uv_b), REC, L.ptr(depth_b), REC, n,
                L.ptr(gt), L.ptr(mm), self.W, self.H, self.min_weight, p, self.P, L.ptr(self.sums),
                L.ptr(self.maps[p]) if self.maps is not None else None,
                L.ptr(self.valid[p]) if self.valid is not None else None, L.ptr(self.ws), self.ws.numel(), L.stream()),
                "flow pair")
        if i + 1 < self.T:                                 # (the last frame is nobody's frame A)
            self._keep("_rec", rec[:n])
            self._keep("_ids", ids.reshape(-1))
            self._keep("_range", tile_range)
            self._n = n
        self._last = i

    def result(self):
        """dict(sums (T-1, 3, 6) float64 -- per pair and class (all, still, moving) the numbers SUM_NAMES --, EPE, acc_1px,
        acc_3px, acc_5px, coverage (T-1, 3) float64; with ``keep_maps`` also maps (T-1, H, W, 2) float32 and valid
        (T-1, H, W) bool).  One copy to the host (the maps are a second allocation, so a second one with them)."""
        P = self.P
        sums = self.sums[:P].cpu().numpy().reshape(P, 3, 6)
        out = dict(sums=sums, **scores_from_sums(sums))
        if self.keep_maps:
            if P > 0:
                out["maps"] = self.maps.cpu().numpy()
                out["valid"] = self.valid.cpu().numpy() != 0
            else:
                out["maps"] = np.zeros((0, self.H, self.W, 2), np.float32)
                out["valid"] = np.zeros((0, self.H, self.W), bool)
        return out


EVAL_KEYS = ("EPE", "EPE_still", "EPE_moving", "acc_1px", "acc_3px", "acc_5px", "coverage")


def evaluate(result):
    """The clip's numbers, pooled over its pairs as sums over sums (every valid pixel of the clip counts once): EPE,
    EPE_still, EPE_moving (mean end-point error over all / still / moving valid pixels), acc_1px, acc_3px, acc_5px (the
    share of valid pixels with an error below 1, 3, 5 pixels), coverage (valid / all pixels), pairs.  NaN where nothing
    was counted."""
    s = np.asarray(result["sums"], dtype=np.float64).reshape(-1, 3, 6)
    t = s.sum(axis=0)
    ratio = lambda a, b: float(a / b) if b > 0 else float("nan")
    return {"EPE": ratio(t[0, 2], t[0, 1]), "EPE_still": ratio(t[1, 2], t[1, 1]), "EPE_moving": ratio(t[2, 2], t[2, 1]),
            "acc_1px": ratio(t[0, 3], t[0, 1]), "acc_3px": ratio(t[0, 4], t[0, 1]), "acc_5px": ratio(t[0, 5], t[0, 1]),
            "coverage": ratio(t[0, 1], t[0, 0]), "pairs": int(s.shape[0])}


def flo_map(flow, valid):
    """(H, W, 2) float32 as it is written to a .flo file: ``flow`` with UNKNOWN_FLOW in both components where not ``valid``"""
    out = np.array(flow, dtype=np.float32, copy=True)
    out[~np.asarray(valid, dtype=bool)] = np.float32(UNKNOWN_FLOW)
    return out


def write_flo_maps(directory, result):
    """Write ``result``'s maps (FlowRecorder.result() with keep_maps, or fit_clip's ``out["flow"]`` with flow="maps") as
    ``directory/flow_<frame>.flo``, frame = the pair's first frame; returns the paths."""
    import os
    from . import io as gio
    if "maps" not in result:
        raise ValueError("write_flo_maps: the result has no maps (fit with flow=\"maps\")")
    os.makedirs(directory, exist_ok=True)
    paths = []
    for t in range(len(result["maps"])):
        paths.append(os.path.join(directory, f"flow_{t:05d}.flo"))
        gio.write_flow(paths[-1], flo_map(result["maps"][t], result["valid"][t]))
    return paths
