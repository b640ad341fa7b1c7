"""Track overlays: the reference's trajectory visualiser (gflow/utils/traj_visualizer.py) drawn on the device
("Track overlays"; the drawing rule is written out in include/gflow_hip.h, "track overlays").

The reference calls ``TrajVisualizer.visualize`` at the end of every clip fit (fit_video.py:385-392: all seeds, the still
ones, the moving ones) and after every tracking evaluation (benchmark.py:163-165: predicted and ground-truth tracks): the
tracks as rainbow polylines over the rendered video, a disc where a point is visible, a cross where it is occluded.  It
paints with PIL on the host, one ``ImageDraw`` call per track and trace segment and frame.  Here ONE ``gfl_track_vis`` call
(csrc/gfl_track_vis.hip) paints all frames of a clip from tensors that are already on the device.

``fit_clip(track_vis=True)`` collects the clip's overlays (``out["track_vis"]``); ``python -m gflow_amd.fit_video --track-vis
DIR`` writes them as PNG frames (``write_frames``)."""
import os

import numpy as np
import torch

from . import _lib as L
from . import color
from .fused import tile_count
from .pinned import DeferredRead

STAGE = 256                        # candidates the paint kernel stages at a time (gfl_track_vis.hip: TV_STAGE)
MAX_SIDE = 16384                   # the library's largest image side


def default_k_cap(T, N, W, H):
    """The pool of (segment, tile) pairs ``draw_tracks`` asks for by default: eight tiles per trace segment (a segment of a
    few pixels touches one to four 16 x 16 tiles; one that jumps across the image touches its whole bounding box), at least
    65536 pairs, never more than every segment in every tile."""
    segs = max(int(T) - 1, 0) * int(N)
    return max(1, min(segs * tile_count(W, H), max(65536, 8 * segs)))


def _as_video(video, dev):
    video = torch.as_tensor(video)
    if video.dtype == torch.uint8:
        if video.dim() != 4 or video.shape[-1] != 3:
            raise ValueError("draw_tracks: a uint8 video must be (T, H, W, 3)")
        return video.to(dev).contiguous()
    if not video.is_floating_point() or video.dim() != 4 or video.shape[1] != 3:
        raise ValueError("draw_tracks: video must be (T, H, W, 3) uint8 or (T, 3, H, W) float in [0, 1]")
    from .render import render2img_device
    video = video.to(dev)
    if video.shape[0] == 0:
        return torch.empty((0, video.shape[2], video.shape[3], 3), dtype=torch.uint8, device=dev)
    return torch.stack([render2img_device(f) for f in video])


def draw_tracks(video, tracks, occluded, still_length=0, K_cap=None):
    """The clip's frames with the tracks painted over them: (T, H, W, 3) uint8 on the device.

    ``video``: (T, H, W, 3) uint8, or (T, 3, H, W) float in [0, 1] (it then goes through ``render2img_device``);
    ``tracks``: (T, N, 2) float, (x, y) in pixels; ``occluded``: (T, N) bool.  Device or host tensors (or arrays); the work
    runs on the device of the first of them that lies on one, else on the current HIP device.
    ``still_length``: with 0 < still_length < N the tracks from ``still_length`` on are coloured over their own y range (the
    seeds of a clip fit: still ones first, then the moving ones).  The reference compares ``still_length`` with the number
    of FRAMES there (traj_visualizer.py:222), which makes the colouring depend on the clip's length; this compares with N.
    ``K_cap``: the pool of (trace segment, tile) pairs; ``default_k_cap`` of T, N and the image size by default.  A clip
    that needs more raises RuntimeError (the library then leaves the markers only, never a part of the traces).

    One library call, nothing allocated or read back inside it; the overflow flag is looked at through a DeferredRead
    behind the call (not while a graph is being captured)."""
    tensors = [torch.as_tensor(x) for x in (video, tracks, occluded)]
    dev = next((t.device for t in tensors if t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    video = _as_video(tensors[0], dev)
    tracks = tensors[1].to(dev).float().contiguous()
    occ = (tensors[2].to(dev) != 0).to(torch.uint8).contiguous()
    L.need_device(video, tracks, occ)
    T, H, W = (int(v) for v in video.shape[:3])
    if tracks.dim() != 3 or tracks.shape[0] != T or tracks.shape[2] != 2:
        raise ValueError(f"draw_tracks: tracks must be ({T}, N, 2), got {tuple(tracks.shape)}")
    N = int(tracks.shape[1])
    if tuple(occ.shape) != (T, N):
        raise ValueError(f"draw_tracks: occluded must be ({T}, {N}), got {tuple(occ.shape)}")
    if K_cap is None:
        K_cap = default_k_cap(T, N, W, H)
    K_cap = int(K_cap)
    lib = L.load()
    out = torch.empty_like(video)
    if T == 0:
        return out
    need = lib.gfl_track_vis_workspace_bytes(T, N, W, H, K_cap)
    if need == 0:
        raise ValueError(f"draw_tracks: unsupported sizes T={T} N={N} W={W} H={H} K_cap={K_cap} (sides up to {MAX_SIDE}, "
                         "T N below 2^31, K_cap > 0)")
    ws = L.scratch(need, dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.gfl_track_vis(L.ptr(video), L.ptr(tracks), L.ptr(occ), T, N, W, H, int(still_length),
                                  L.ptr(color.lut("gist_rainbow", dev)), K_cap, L.ptr(out), L.ptr(ovf), L.ptr(ws), ws.numel(),
                                  L.stream()), "track vis")
        if not torch.cuda.is_current_stream_capturing():
            read = DeferredRead(1)
            read.watch(ovf)
            if read.read()[0]:
                raise RuntimeError(f"gflow_amd.track_vis: the clip's trace segments need more than K_cap={K_cap} (segment, "
                                   "tile) pairs; raise K_cap")
    return out


def seed_occlusions(move_segs, tracks):
    """The reference's ``process_occu`` (utils/tracking.py:10-22): (T, N) bool.  ``move_segs``: the T per-frame moving-region
    masks, (H, W) each, nonzero = moving; ``tracks``: (T, N, 2), (x, y).  A seed that started OUTSIDE the first frame's
    moving mask is "occluded" in every frame where it lies on that frame's moving mask (a still seed the moving region has
    moved over); a seed that started on it never is.  Coordinates are clipped to the image and rounded half to even, like
    Python's ``round``."""
    masks = np.stack([np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m) != 0 for m in move_segs])
    tr = np.asarray(tracks.cpu() if isinstance(tracks, torch.Tensor) else tracks, dtype=np.float64)
    T, H, W = masks.shape
    if tr.shape[0] != T or tr.ndim != 3 or tr.shape[2] != 2:
        raise ValueError(f"seed_occlusions: {T} masks, tracks {tr.shape}")
    x = np.rint(np.clip(np.nan_to_num(tr[..., 0]), 0, W - 1)).astype(np.int64)
    y = np.rint(np.clip(np.nan_to_num(tr[..., 1]), 0, H - 1)).astype(np.int64)
    on = masks[np.arange(T)[:, None], y, x]                         # (T, N): the seed lies on its frame's moving mask
    return ~on[0][None, :] & on


def write_frames(images, dir):
    """``images`` (T, H, W, 3) uint8 (device tensor or array) as ``dir/00000.png``, ``dir/00001.png``, ...: one image per
    frame.  (No mp4 writer; and neither the visualiser's ``show_first_frame`` duplication of the first frame nor the last
    frame its ``save_video`` drops, traj_visualizer.py:171 and :328, are reproduced.)  Returns the paths."""
    from PIL import Image
    a = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[-1] != 3:
        raise ValueError("write_frames: images must be (T, H, W, 3) uint8")
    os.makedirs(dir, exist_ok=True)
    paths = []
    for t in range(a.shape[0]):
        paths.append(os.path.join(dir, f"{t:05d}.png"))
        Image.fromarray(a[t]).save(paths[-1])
    return paths


def write_video(images, path, fps=5):
    """``images`` (T, H, W, 3) uint8 (device tensor or array) as ONE file: a Motion-JPEG AVI at ``fps`` (5: the reference's
    save_video, traj_visualizer.py:171), the frames coded on the device (gflow_amd.video.write_avi; INTEGRATION.md, "Video
    files").  Returns dict(frames, bytes)."""
    from . import video
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    return video.write_avi(path, images, fps=fps)


def clip_overlays(video, pred=None, seeds=None, extra=None):
    """What ``fit_clip(track_vis=...)`` adds: a dict of (T, H, W, 3) uint8 host arrays, drawn on the device over ``video``
    ((T, H, W, 3) uint8 on the device) and copied to the host together.
    ``pred`` = (tracks (Q, T, 2), occluded (Q, T)) as ``Tracker.result()`` has them -> ``"pred"`` (benchmark.py:164).
    ``seeds`` = (uv (T, S, 2), occluded (T, S), split) -> ``"seeds"`` with still_length = split (fit_video.py:386),
    ``"seeds_still"`` = the columns before ``split`` and, when there are any behind it, ``"seeds_move"`` (:389, :392; each with
    its own columns of the flags -- the reference hands both the first columns).
    ``extra``: name -> (tracks (T, N, 2), occluded (T, N)), further tracks over the same frames (the ground truth of
    benchmark.py:165)."""
    jobs = []                                           # (name, tracks, occluded, still_length)
    if pred is not None:
        tracks, occ = pred
        jobs.append(("pred", np.ascontiguousarray(np.transpose(tracks, (1, 0, 2))), np.ascontiguousarray(np.transpose(occ)), 0))
    if seeds is not None:
        uv, occ, split = seeds
        uv, occ = np.asarray(uv), np.asarray(occ)
        n = int(uv.shape[1])
        split = n if split is None else int(split)
        jobs.append(("seeds", uv, occ, split))
        jobs.append(("seeds_still", np.ascontiguousarray(uv[:, :split]), np.ascontiguousarray(occ[:, :split]), 0))
        if split < n:
            jobs.append(("seeds_move", np.ascontiguousarray(uv[:, split:]), np.ascontiguousarray(occ[:, split:]), 0))
    for name, (tracks, occ) in (extra or {}).items():
        if any(name == j[0] for j in jobs):
            raise ValueError(f"clip_overlays: {name!r} is taken")
        jobs.append((name, tracks, occ, 0))
    if not jobs:
        return {}
    host = torch.stack([draw_tracks(video, tracks, occ, still_length=sl) for _, tracks, occ, sl in jobs]).cpu().numpy()
    return {j[0]: host[k] for k, j in enumerate(jobs)}
