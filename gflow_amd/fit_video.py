"""Video driver -- the counterpart of gflow/fit_video.py's frame loop, plus clip sharding.

``fit_clip`` keeps the reference's structure (fit_video.py:105-349): first-frame fit with
``iterations_first``; then for every later frame an optional camera-only fit
(``iterations_camera``, ``lr_camera_after``) followed by the full fit (``iterations_after``,
``lr_after``, occlusion-mask densification at iteration 0).  Inputs are in-memory frames (dicts
as produced by ``gflow_amd.synthetic.make_clip``: image, depth, flow, move_mask, occ_mask, focal,
pp); the reference's file readers and video writers are out of scope.

Multi-GPU: clips are independent, frames of one clip are not.  One process per GPU,
the clips dealt to the ranks by length (``shard``: longest first, each to the least loaded rank -- the
reference walks its sequences one after another, benchmark_multi.py:23-37), no data-path collective; at
the end ONE all-reduce(SUM) of a small metrics vector (which also carries every rank's own wall time in
a slot of its own) and ONE all-reduce(MAX) of the wall time (RCCL over xGMI on a node, tens of bytes:
pure latency).  ``--clips-per-gpu c``: a rank fits c of its clips AT THE SAME TIME on its GPU
(``fit_clips_concurrent``: one fit leaves the chip partly idle) -- the throughput mode of a node with more
clips than GPUs.

    python -m torch.distributed.run --nproc-per-node 8 -m gflow_amd.fit_video --clips 24 --frames 60 --clips-per-gpu 3
"""
import argparse
import json
import math
import os
import sys
import time

import torch

from . import camera as CM
from . import flow as FL
from . import quality as QL
from . import segmentation as SG
from . import tracking as TK

# Canonical hyper-parameters: the README's example (README.md:85-110), which is what BASELINE.json's configs quote
# (60 000 splats, 500 / 300 iterations, 150 camera-only).  scripts/fit_video.sh:16-39 runs a different set
# (50 000 splats, lambda_depth 0.1, lambda_var 50, lambda_still 0, lr_after 4e-3, lr_camera_after 1e-3,
# densify_times_after 2, densify_occ_percent 0.5): pass those as ``cfg`` (SCRIPT_OVERRIDES) to reproduce that script.
# bench.py's STEP uses lambda_depth 0.1 so that the depth term is exercised at a weight where it matters; its clip fit
# uses these defaults.
SCRIPT_OVERRIDES = dict(num_points=50000, lr_after=4e-3, lr_camera_after=1e-3, densify_times_after=2,
                        densify_occ_percent=0.5, lambda_depth=0.1, lambda_var=50.0, lambda_still=0.0)
DEFAULTS = dict(num_points=60000, lr=4e-3, lr_camera=0.0, iterations_first=500, lr_after=1e-3, iterations_after=300,
                camera_first=True, lr_camera_after=5e-4, iterations_camera=150, densify_interval=150, densify_times=2,
                densify_interval_after=100, densify_times_after=1, densify_occ_percent=1.0, densify_err_thre=1e-2,
                densify_err_percent=1.0, lambda_rgb=1.0, lambda_depth=1e-4, lambda_var=10.0, lambda_still=10.0,
                lambda_flow=0.01, lambda_scale=0.0, background="black",
                # trajectories (fit_video.py:34-35 defaults 0 / 0; the README's and scripts/fit_video.sh's flags: 100 / 2):
                # with traj_num > 0 every frame ends with trainer.eval(traj_index, line_scale=0.5, point_scale=2., alpha=0.8)
                # and project_points of the seeds (fit_video.py:226-238, 335-349)
                traj_num=0, traj_offset=0)

METRIC_NAMES = ("psnr_sum", "frames", "iterations", "rasterisations", "clips", "splats_final")


def shard(n_items, rank, world, lengths=None):
    """Indices of the clips rank ``rank`` fits.  Clips cost what their frames cost (500 iterations for the first, 450 for
    every other one), and a job lasts as long as its slowest rank: longest-processing-time-first -- the clips in
    descending length (ties: lower index first), each to the rank with the least work so far (ties: lower rank) -- ends
    within one clip of the ideal.  Every rank computes the same assignment from the same lengths: nothing is exchanged.
    ``lengths=None``: all clips equally long (then this is i mod world)."""
    lengths = [1] * n_items if lengths is None else [int(v) for v in lengths]
    if len(lengths) != n_items:
        raise ValueError("shard: one length per clip")
    load = [0] * world
    mine = []
    for i in sorted(range(n_items), key=lambda j: (-lengths[j], j)):
        r = min(range(world), key=lambda q: (load[q], q))
        load[r] += lengths[i]
        if r == rank:
            mine.append(i)
    return sorted(mine)


def reduce_metrics(local, wall_seconds, dist=None, device="cpu", rank=0, world=1):
    """SUM of the metrics vector and MAX of the wall time over all ranks (identity without dist).  The vector's tail
    has one slot per rank: every rank writes its own wall time into its slot, so the one SUM also hands every rank all
    the ranks' times (``rank_wall_s``: the imbalance of the shard)."""
    own = [0.0] * world
    own[rank] = float(wall_seconds)
    vec = torch.tensor([float(local.get(k, 0.0)) for k in METRIC_NAMES] + own, dtype=torch.float64, device=device)
    wall = torch.tensor([float(wall_seconds)], dtype=torch.float64, device=device)
    if dist is not None and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM)
        dist.all_reduce(wall, op=dist.ReduceOp.MAX)
    vals = vec.tolist()
    out = {k: float(v) for k, v in zip(METRIC_NAMES, vals)}
    out["wall_s"] = float(wall.item())
    out["rank_wall_s"] = [float(v) for v in vals[len(METRIC_NAMES):]]
    return out


TAPVID_KEYS = ("occlusion_accuracy", "average_jaccard", "average_pts_within_thresh")
DAVIS_KEYS = ("J", "F", "J&F")
RECON_KEYS = ("PSNR", "SSIM")
CAMERA_KEYS = CM.SCORE_KEYS
FLOW_KEYS = FL.EVAL_KEYS


def _mean_over_clips(keys, scores, totals, dist=None, device="cpu", none=float("nan")):
    """What the ``reduce_*`` blocks of the JSON line share.  ``scores``: per clip of this rank a dict with a value for every
    key of ``keys`` -- None or NaN where the clip has no such number; ``totals``: this rank's integers that ride along.
    Returns every key's mean over the clips of ALL ranks where it is a number (``none`` where no clip has it), then every
    total summed, as ints: ONE small all-reduce(SUM) of (the sums, a clip count per key, the totals)."""
    n = len(keys)
    sums, counts = [0.0] * n, [0.0] * n
    for m in scores:
        for j, k in enumerate(keys):
            if m[k] is not None and not math.isnan(m[k]):
                sums[j] += float(m[k])
                counts[j] += 1.0
    vec = torch.tensor(sums + counts + [float(t) for t in totals.values()], dtype=torch.float64, device=device)
    if dist is not None and dist.is_initialized():
        dist.all_reduce(vec, op=dist.ReduceOp.SUM)
    v = vec.tolist()
    out = {k: v[j] / v[n + j] if v[n + j] else none for j, k in enumerate(keys)}
    out.update(zip(totals, (int(t) for t in v[2 * n:])))
    return out


def reduce_tapvid(preds, gts, n_frames, dropped, dist=None, device="cpu"):
    """The "tapvid" block: every clip's TAP-Vid score (tracking.evaluate), averaged over the clips as benchmark.py averages
    its videos; ``clips`` is their number, ``queries_dropped`` what the caller left out.  ``gts[ci]``: (points, occluded, H,
    W), or with (queries, source) behind them for a query set other than the first-visible one (tracking.evaluate)."""
    ms = [TK.evaluate(p, *gts[ci][:4], n_frames[ci], *gts[ci][4:]) for ci, p in preds.items()]
    return _mean_over_clips(TAPVID_KEYS, ms, dict(clips=len(ms), queries_dropped=dropped), dist, device)


def reduce_davis(segs, dist=None, device="cpu"):
    """The "davis" block: every clip's J, F and J&F (segmentation.evaluate: means over its scored frames), averaged over
    the clips that have a scored frame (``clips``); ``frames_scored`` is their total."""
    ms = [SG.evaluate(seg) for seg in segs.values()]
    totals = dict(frames_scored=sum(m["frames_scored"] for m in ms), clips=sum(1 for m in ms if m["frames_scored"]))
    return _mean_over_clips(DAVIS_KEYS, ms, totals, dist, device)


def reduce_recon(recons, dist=None, device="cpu"):
    """The "recon" block: every clip's PSNR and SSIM (quality.evaluate: means over its frames), averaged over the clips
    that have a frame (``clips``); ``frames`` is their total."""
    ms = [QL.evaluate(rec) for rec in recons.values()]
    totals = dict(frames=sum(m["frames"] for m in ms), clips=sum(1 for m in ms if m["frames"]))
    return _mean_over_clips(RECON_KEYS, ms, totals, dist, device)


def reduce_camera(cams, dist=None, device="cpu"):
    """The "camera" block: every clip's ATE, RPE_t and RPE_r (fit_clip's ``out["camera"]``), averaged over the clips that
    have a score (``clips``); a clip whose score is None (camera.evaluate: no alignment exists) counts in
    ``clips_unscored``, not in the mean.  The three are None when no clip was scored."""
    scored = [cam for cam in cams.values() if not any(cam[k] is None for k in CAMERA_KEYS)]
    totals = dict(clips=len(scored), clips_unscored=len(cams) - len(scored))
    return _mean_over_clips(CAMERA_KEYS, scored, totals, dist, device, none=None)


def reduce_flow(flows, dist=None, device="cpu"):
    """The "flow" block: every clip's numbers (flow.evaluate: pooled over its pairs), each averaged over the clips where
    it is a number (a clip without a moving pixel has no EPE_moving; a one-frame clip has nothing); ``pairs`` is the
    clips' total, ``clips`` those with a pair.  None where no clip has the number."""
    ms = [FL.evaluate(fl) for fl in flows.values()]
    totals = dict(pairs=sum(m["pairs"] for m in ms), clips=sum(1 for m in ms if m["pairs"]))
    return _mean_over_clips(FLOW_KEYS, ms, totals, dist, device, none=None)


def csv_metrics(out):
    """The JSON line's blocks under the reference's metrics.csv keys (quality.CSV_KEYS); only the blocks that are there"""
    m = {}
    if "recon" in out:
        m.update({"PSNR": out["recon"]["PSNR"], "SSIM": out["recon"]["SSIM"]})
    if "tapvid" in out:
        m.update({"Occlusion_Accuracy": out["tapvid"]["occlusion_accuracy"], "Average_Jaccard": out["tapvid"]["average_jaccard"],
                  "Average_PTS_within_threshold": out["tapvid"]["average_pts_within_thresh"]})
    if "davis" in out:
        m.update({"J_zero": out["davis"]["J"], "F_zero": out["davis"]["F"], "J&F_zero": out["davis"]["J&F"]})
    if "camera" in out:
        m.update({k: out["camera"][k] for k in CAMERA_KEYS})
    return m


_FIT_STREAMS = {}


def upload_clip(frames, device):
    """The clip's frames with every tensor resident on ``device`` (and ``occ_count``, the number of set pixels of the
    occlusion mask, counted here on the host).  torch copies pageable host memory to the device synchronously: handing
    the frames over one ``set_gt_*`` at a time, as the reference does after reading each frame from disk, stopped the
    host -- and drained the device's queue -- five times per frame.  A frame is ~10 MB (image, depth, flow, masks): a
    60-frame clip is 0.6 GB of 288."""
    out = []
    for fr in frames:
        d = dict(fr)
        occ = fr.get("occ_mask")
        if occ is not None and "occ_count" not in d:
            m = torch.as_tensor(occ).squeeze()
            if m.dim() == 3:
                m = m[..., 0] if m.shape[-1] in (1, 3) else m[0]
            d["occ_count"] = int((m > 0).sum())
        for k, v in fr.items():
            if isinstance(v, torch.Tensor) and k != "extr":
                d[k] = v.to(device, non_blocking=True)
        out.append(d)
    return out


def select_traj_seeds(tr, traj_num, traj_offset):
    """The splats whose trajectories are drawn (fit_video.py:163-211, ``grid_traj = True`` as the reference hard-codes it):
    pixels of a grid -- stride 50 inside the eroded still region, stride 15 inside the eroded moving region (``move_seg``, the
    hull mask of the first frame's fit; a 10 x 10 erosion, cv2.erode's default border: nothing eroded from the image's edge) --
    and for every grid pixel the splat whose projection (``last_uv``) lies closest, kept if its still / moving label is the
    region's.  Returns (indices: still seeds first, split_interval = their number or None without moving seeds).
    Without a hull mask (fewer than six moving splats: the reference would fail in cv2.erode) the plain rule of
    fit_video.py:165-167, every (N / traj_num)-th splat from ``traj_offset``.  Once per clip; the nearest-splat search runs on
    the device (the reference forms an N x Q x 2 array in numpy), one read-back of the few hundred indices."""
    import numpy as np
    from scipy.ndimage import minimum_filter
    n = tr.current_pts_num()
    interval = max(int(n / traj_num), 1)
    plain = list(range(n))[traj_offset::interval]
    move_seg = getattr(tr, "move_seg", None)
    if move_seg is None:
        return plain, None
    H, W = tr.H, tr.W
    erode = lambda m: minimum_filter(m, size=10, mode="constant", cval=255)       # kernel 10 x 10, anchor (5, 5): x-5 .. x+4
    move_er = erode(np.asarray(move_seg, dtype=np.uint8))
    still_er = erode((255 - np.asarray(move_seg, dtype=np.int32)).astype(np.uint8))
    s_still, s_move = 50, 15
    grid = lambda lo_i, hi_i, lo_j, hi_j, s: [(j, i) for i in range(lo_i, hi_i, s) for j in range(lo_j, hi_j, s)]
    sparse = [(j, i) for (j, i) in grid(s_still, H, s_still, W, s_still) if still_er[i, j]]
    if len(sparse) == 0:
        sparse = grid(s_still, H, s_still, W, s_still)
    dense = [(j, i) for (j, i) in grid(s_move, H - s_move, s_move, W - s_move, s_move) if move_er[i, j]]
    if len(sparse) == 0:                                 # (sic: the reference tests the SPARSE list again, :197)
        dense = grid(s_move, H - s_move, s_move, W - s_move, s_move)
    uv = tr.last_uv.detach().double()
    still = tr.still_mask.detach()

    def closest(points):                                 # utils.find_closest_point (tracking.py:24-26): argmin over the splats
        q = torch.tensor(points, dtype=torch.float64, device=uv.device)
        out = []
        for a in range(0, q.shape[0], 256):              # (chunks: N x 256 distances at a time)
            d = ((uv[:, None, :] - q[None, a:a + 256, :]) ** 2).sum(-1)
            out.append(d.argmin(dim=0))
        return torch.cat(out)

    if len(sparse) == 0:
        # (H or W <= 50: the stride-50 grid has no pixel at all -- the reference would index an empty array, :200-203; the
        #  plain rule is what it falls back to without a mask)
        return plain, None
    sp = closest(sparse)
    sp_still = sp[still[sp]]
    if len(dense):
        de = closest(dense)
        de_move = de[~still[de]]
        return torch.cat([sp_still, de_move]).tolist(), int(sp_still.shape[0])
    return sp_still.tolist(), None


def begin_frame(tr, frames, i, load_extr=True):
    """What the frame loop does before frame i >= 1 is fitted (fit_video.py:242-253): the new targets, the flow from frame
    i - 1 to i, the frame's camera pose if the sequence carries one."""
    fr = frames[i]
    tr.set_gt_image(fr["image"])
    tr.set_gt_depth(fr["depth"])
    tr.set_gt_flow(frames[i - 1]["flow"])                # flow from frame i-1 to i (fit_video.py:250)
    if load_extr and fr.get("extr") is not None:
        tr.load_camera(extr=fr["extr"])                  # fit_video.py:252-253


def stage_kwargs(c, frames, i, stage):
    """The keyword arguments of frame i's (>= 1) two ``train`` calls -- ``stage`` "camera": the camera-only stage
    (fit_video.py:256-278), "joint": splats and nothing else (:288-315) -- without the per-call ones (snapshot interval,
    loss weights every call shares).  One place, because bench.py pins its mid-clip step windows on exactly these stages."""
    fr = frames[i]
    if stage == "camera":
        return dict(iterations=c["iterations_camera"], lr_camera=c["lr_camera_after"], lambda_var=0.0, lambda_still=0.0,
                    lambda_flow=c["lambda_flow"], densify_interval=c["densify_interval"], densify_times=c["densify_times"],
                    camera_only=True, move_mask=fr["move_mask"])
    if stage == "joint":
        return dict(iterations=c["iterations_after"], lr=c["lr_after"], lr_camera=0.0, lambda_var=c["lambda_var"],
                    lambda_still=c["lambda_still"], lambda_flow=c["lambda_flow"], densify_interval=c["densify_interval_after"],
                    densify_times=c["densify_times_after"], mask=fr.get("occ_mask"), mask_count=fr.get("occ_count"),
                    move_mask=fr["move_mask"])
    raise ValueError(stage)


def fit_clip(frames, device, cfg=None, fused=True, deterministic=None, **options):
    """Fit one clip; returns the metrics dict of this clip.  ``options``: fit_clip_steps' (whose docstring names them all),
    without ``chunk`` and ``cu_count``.  On a device the fit runs on a stream of its own, which the current stream waits
    for."""
    if deterministic and not fused:
        raise ValueError("fit_clip(deterministic=True) needs fused=True: the operator path's alpha_blending backward has no "
                         "deterministic implementation")
    from .trainer import run_to_end
    dev_ = torch.device(device)
    g = fit_clip_steps(frames, device, cfg, fused=fused, deterministic=deterministic, chunk=None, cu_count=0, **options)

    drive = lambda: run_to_end(g)
    if dev_.type == "cuda" and torch.cuda.current_stream(dev_) == torch.cuda.default_stream(dev_):
        # Never fit on the default stream: it is HIP's legacy NULL stream, which every other (blocking) stream
        # synchronises with -- the snapshot copies on the copy stream then run BETWEEN the fit's launches instead of
        # beside them (measured: the same 8-frame clip fit 0.95 s on a stream of its own, 1.09 s on the default stream).
        key = dev_.index
        if key not in _FIT_STREAMS:
            _FIT_STREAMS[key] = torch.cuda.Stream(device=dev_)
        fs = _FIT_STREAMS[key]
        fs.wait_stream(torch.cuda.current_stream(dev_))
        with torch.cuda.stream(fs):
            out = drive()
        torch.cuda.current_stream(dev_).wait_stream(fs)
        return out
    return drive()


def fit_clip_steps(frames, device, cfg=None, seed=0, snapshot_interval=0, fused=True, log=None, load_extr=True, chunk=None,
                   async_snapshots=True, keep=None, cu_count=0, deterministic=None, track_queries=None, segment=False,
                   recon=False, camera=False, flow=False, track_backward=False, track_vis=False):
    """fit_clip as a generator: yields after every ``chunk`` iterations of a stage (None: never) and returns the metrics
    dict of the clip (PSNR summed over its frames; with ``cfg["traj_num"]`` > 0 also ``"traj"``: the per-frame trajectory
    images and seed projections, host arrays -- what the reference's frame loop collects in
    ``frames_sequence_traj / frames_sequence_traj_upon / sequence_traj``).  The caller owns the stream the work is enqueued
    on (fit_clips_concurrent gives every clip its own; ``cu_count``: that stream is CU-masked to so many CUs).  The
    options, which fit_clip and fit_clips_concurrent hand through:
    ``load_extr`` (default True, like the reference's flag): frames that carry a camera pose
    (``extr``, read from the sequence's camera files) load it before they are fitted
    (fit_video.py:115-116, :252-253).  ``keep``: a dict that receives the trainer (``keep["trainer"]``) and the
    per-frame PSNR as device scalars (``keep["psnr"]``) -- for tests and tools; with ``cfg["traj_num"]`` also the per-frame
    trajectory images and seed projections as they left for the host (``keep["traj"]``).
    ``async_snapshots``: the snapshots of ``snapshot_interval`` are composed beside the next iterations (trainer.py), not
    behind theirs.
    ``deterministic``: the same frames, cfg and seed give the same metrics, parameters and trajectory outputs bit for bit
    (SimpleGaussian(deterministic=)); None follows torch.are_deterministic_algorithms_enabled().  Needs
    ``fused=True``.
    ``track_queries``: rows [t, y, x] (pixels) of points to track (gflow_amd.tracking.Tracker; ValueError unless every t is
    a frame of the clip): every query is anchored at the end of its frame and tracked, with an occlusion flag, at the end of
    every later one; the dict then has ``"tracks"`` (Tracker.result()).  ``keep["record_track_inputs"] = True``: the
    per-frame (uv, depth, depth_map) the tracker read, cloned, in ``keep["track_inputs"]``.
    ``track_backward`` (needs ``track_queries``, else ValueError): the frames before a query's frame are tracked too
    (Tracker(backward=True); INTEGRATION.md, "Point tracking"): one more launch per frame on the forward the tracker already
    reads (``rasterisations`` does not change), one pass at the end of the clip; ``"tracks"`` then has ``back_anchor``.
    ``segment``: also the moving region of every frame and its DAVIS score against the frame's ``move_mask``
    (gflow_amd.segmentation.MoveSegRecorder; INTEGRATION.md, "Moving-region segmentation"): the dict then has
    ``"segmentation"`` = dict(masks (T, H, W) uint8, valid (T,) bool, counts (T, 6) int64, J, F, JF (T,) float64).  Nothing
    is read back while the clip is fitted.  ``keep["record_seg_inputs"] = True``: the per-frame (uv, sel) the masks are
    built from, cloned, in ``keep["seg_inputs"]`` (None for a frame without a joint stage).
    ``recon``: also every frame's reconstruction score (gflow_amd.quality.ReconRecorder; INTEGRATION.md, "Reconstruction
    score"): where the frame's PSNR is taken, one gfl_recon_frame call on ``last_render`` and ``gt_image``; the dict then has
    ``"recon"`` = dict(sse, ssim_sum, PSNR, SSIM (T,) float64).  ``keep["record_recon_inputs"] = True``: a clone of each
    frame's ``last_render[:3]`` in ``keep["recon_inputs"]``.
    ``camera``: also the camera path and its score (gflow_amd.camera; INTEGRATION.md, "Camera score"): the dict then has
    ``"camera"`` = dict(extr (T, 3, 4) float32 -- every frame's ``get_extr()`` at its end --, ATE, RPE_t, RPE_r: floats or
    None) against each frame's ``extr_gt`` if it has one, else its ``extr``; a frame with neither is a ValueError before
    anything is fitted.
    ``flow``: also the dense optical flow the fitted splats imply between consecutive frames and its end-point error
    against the flow the fit was given (gflow_amd.flow.FlowRecorder; INTEGRATION.md, "Flow score"): the dict then has
    ``"flow"`` = dict(sums (T-1, 3, 6), EPE, acc_1px, acc_3px, acc_5px, coverage (T-1, 3) float64 -- per pair and class (all,
    still, moving)); ``flow="maps"`` also keeps the maps: ``maps`` (T-1, H, W, 2) float32, frame i -> i + 1 on frame i's
    grid, and ``valid`` (T-1, H, W) bool.  A one-frame clip gives empty arrays.  ``keep["record_flow_inputs"] = True``: clones
    of each pair's kernel inputs (dicts) in ``keep["flow_inputs"]``.
    ``track_vis`` (needs ``track_queries`` or ``cfg["traj_num"]`` > 0, else ValueError): also the reference's track overlays
    (gflow_amd.track_vis; INTEGRATION.md, "Track overlays"): every frame's final render is kept as uint8 on the device, taken
    where the frame's PSNR is taken, and once the clip is fitted the tracks are painted over them on the device (one
    gfl_track_vis call per overlay, no rasterisation) and copied to the host together; the dict then has ``"track_vis"``, a
    dict of (T, H, W, 3) uint8 arrays: with ``track_queries`` ``pred`` (the tracker's tracks and occlusion flags;
    benchmark.py:164), with ``traj_num`` ``seeds`` (every seed, still_length = the split; the flags are
    track_vis.seed_occlusions of the frames' hull masks, which a MoveSegRecorder collects as for ``segment``),
    ``seeds_still`` and, when there are moving seeds, ``seeds_move`` (fit_video.py:386-392).  ``keep`` then also receives
    ``keep["track_vis_inputs"]`` = dict(video (T, H, W, 3) uint8, masks (T, H, W) uint8 with ``traj_num``), host arrays.
    ``track_vis`` may also be a dict name -> (tracks (T, N, 2), occluded (T, N)) of further tracks to paint over the same
    renders, one more array each (the command line's ``gt``: benchmark.py:165)."""
    if track_backward and track_queries is None:
        raise ValueError("fit_clip(track_backward=True) needs track_queries")
    if track_vis and track_queries is None and not int((cfg or {}).get("traj_num", DEFAULTS["traj_num"])) > 0:
        raise ValueError("fit_clip(track_vis=True) needs track_queries or cfg['traj_num'] > 0")
    from .trainer import SimpleGaussian
    c = dict(DEFAULTS)
    c.update(cfg or {})
    if any(isinstance(v, torch.Tensor) and not v.is_cuda for k, v in frames[0].items() if k != "extr"):
        frames = upload_clip(frames, device)         # (bench.py uploads before its clock starts: "inputs resident in HBM")
    f0 = frames[0]
    tracker = None
    if track_queries is not None:
        # (ValueError before anything is fitted)
        tracker = TK.Tracker(track_queries, len(frames), device, backward=bool(track_backward))
    cam_rec = None
    if camera:
        cam_gt = [fr["extr_gt"] if fr.get("extr_gt") is not None else fr.get("extr") for fr in frames]
        missing = [t for t, e in enumerate(cam_gt) if e is None]
        if missing:
            raise ValueError(f"fit_clip(camera=True): frames {missing} carry neither extr_gt nor extr")
        cam_rec = CM.CameraRecorder(len(frames))
    tr = SimpleGaussian(f0["image"], f0["depth"], num_points=c["num_points"], background=c["background"],
                        device=device, seed=seed, fused=fused, deterministic=deterministic)
    tr.async_snapshots = bool(async_snapshots)       # (trainer.py: snapshots composed beside the next iterations, or behind theirs)
    tr.cu_count = int(cu_count)                      # (the caller's stream is CU-masked: fit_clips_concurrent(partition=True))
    if segment or (track_vis and int(c["traj_num"]) > 0):
        tr.seg_recorder = SG.MoveSegRecorder(len(frames), tr.H, tr.W, tr.device)
    vis_frames = []                                  # track_vis: every frame's final render, (H, W, 3) uint8 on the device
    recon_rec = None
    if recon:
        recon_rec = QL.ReconRecorder(len(frames), tr.H, tr.W, tr.device)
    flow_rec = None
    if flow:
        flow_rec = FL.FlowRecorder(len(frames), tr.H, tr.W, tr.device, keep_maps=flow == "maps")
        if keep is not None and keep.get("record_flow_inputs"):
            flow_rec.inputs = keep.setdefault("flow_inputs", [])
    tr.load_camera(focal=f0["focal"], pp=f0["pp"])
    if load_extr and f0.get("extr") is not None:
        tr.load_camera(extr=f0["extr"])
    tr.init_gaussians_from_image(f0["image"], f0["depth"], num_points=c["num_points"])
    common = dict(lambda_rgb=c["lambda_rgb"], lambda_depth=c["lambda_depth"], lambda_scale=c["lambda_scale"],
                  densify_occ_percent=c["densify_occ_percent"], densify_err_thre=c["densify_err_thre"],
                  densify_err_percent=c["densify_err_percent"], snapshot_interval=snapshot_interval,
                  lazy_images=True,        # (the image lists train() returns are not read here: do not wait for them)
                  chunk=chunk)
    # first frame (fit_video.py:119-142)
    traj = int(c["traj_num"]) > 0
    yield from tr.train_steps(iterations=c["iterations_first"], lr=c["lr"], lr_camera=c["lr_camera"],
                              lambda_var=c["lambda_var"], densify_interval=c["densify_interval"],
                              densify_times=c["densify_times"], move_mask=f0["move_mask"],
                              move_seg=traj,   # (the seeds' grid needs the first frame's hull mask: host work, once per clip)
                              **common)
    traj_rec = []                                        # per frame: where the seeds are, the camera, the scene's rgb image
    final = []                                           # this frame's final_forward, once it has run (end_of_frame empties it)

    def final_forward():
        # The forward of THIS frame's final state on the second engine (fused path): run when the first of the frame's
        # recorders asks for it, shared by those after it -- the frame is rasterised once more, not once per recorder.  (The
        # trajectory recorder asks first and has the scene's images taken from it: see there.)
        if not final:
            final.append(tr._aux_forward())
            final[0].watch_overflow()
            tr.rasterisations_done += 1
        return final[0]

    def record_trajectories():
        # fit_video.py:226-238 / 335-349 call trainer.eval + project_points here, after every frame.  What they need of THIS
        # frame is recorded on the device -- the seeds' positions, the camera, the rendered scene (the fused kernels, now) --
        # and the trajectory overlays of all frames are drawn once the clip is fitted (draw_trajectories): a poly-line's point
        # count is data and the operator path sizes its lists on the host, i.e. two or three full stops of the host per frame
        # here, each with the next frame's set-up behind it (60-frame clip fit: 9.76 -> 9.24 frames/s when drawn per frame).
        with torch.no_grad():
            xyz_now = tr.get_attribute("xyz")[traj_index_t].detach().float().clone()
            extr_now = tr.get_extr().detach().clone()
            if tr.engine_current:
                # (the frame's forward, the snapshot of its images, then the overflow watch: final_forward's forward with
                #  the snapshot in between, so it is handed to final_forward's readers)
                rgb_u8 = tr._render_scene_fused()[0].clone()
                final.append(tr._aux)
            else:
                from . import render as render_mod
                rgb_u8 = render_mod.render2img_device(render_mod.render_multiple(tr._input_group(detach=True), ["rgb"])["rgb"])
            tr.rasterisations_done += 1
        traj_rec.append((xyz_now, extr_now, rgb_u8))

    def record_tracks(i):
        # benchmark.py:98-139 for frame i, on the frame's final state: the uv / depth / depth_map of one forward go to the
        # tracker's two launches; nothing is read back
        with torch.no_grad():
            if tr.engine_current:
                from .fused import REC
                aux = final_forward()
                n = aux.N
                uv, uv_stride, depth, depth_stride, dm = aux.rec[:n, 0:2], REC, aux.rec[:n, 9], REC, aux.render[3]
            else:
                from . import render as render_mod
                o = render_mod.render_multiple(tr._input_group(detach=True), ["uv", "depth", "depth_map"])
                uv, depth = o["uv"].float().contiguous(), o["depth"].float().reshape(-1).contiguous()
                dm = o["depth_map"].float().reshape(tr.H, tr.W).contiguous()
                uv_stride, depth_stride = 2, 1
                tr.rasterisations_done += 1
            tracker.frame(i, uv, uv_stride, depth, depth_stride, dm)
            if keep is not None and keep.get("record_track_inputs"):
                keep.setdefault("track_inputs", []).append((uv.clone(), depth.clone(), dm.clone()))

    def record_flow(i):
        # frame i's final records and sorted tile lists go to the flow recorder (on the operator path the five operators'
        # outputs, packed).  From frame 1 on one gfl_flow_pair for the pair (i - 1, i); nothing is read back
        with torch.no_grad():
            if tr.engine_current:
                aux = final_forward()
                rec, n, ids, tile_range = aux.rec, aux.N, aux.ids, aux.tile_range
            else:
                rec, n, ids, tile_range = FL.operator_state(tr._input_group(detach=True))
                tr.rasterisations_done += 1
            prev = frames[i - 1] if i else None
            flow_rec.frame(i, rec, n, ids, tile_range, prev["flow"] if prev else None, prev["move_mask"] if prev else None)

    def record_scores(i):
        # benchmark.py:191-230 and :323-329 for frame i, on what the frame's PSNR is taken from and what save_checkpoint
        # stores: two small launches that write one row of the clip's sums, and a clone of the pose; nothing is read back
        with torch.no_grad():
            if recon_rec is not None:
                recon_rec.frame(i, tr.last_render, tr.gt_image)
                if keep is not None and keep.get("record_recon_inputs"):
                    keep.setdefault("recon_inputs", []).append(tr.last_render[:3].clone())
            if cam_rec is not None:
                cam_rec.frame(i, tr.get_extr())

    def draw_trajectories():
        from . import msplat
        from . import render as render_mod
        imgs, uvs = [], []
        with torch.no_grad():
            for xyz_now, extr_now, rgb_u8 in traj_rec:
                overlay = tr.eval_trajectories(xyz_now, extr_now, line_scale=0.5, point_scale=2.0, alpha=0.8,
                                               split_interval=split_interval)
                img_traj = render_mod.render2img_device(overlay)
                # screen blending as trainer.eval forms it (numpy: float64, truncation)
                upon = 1.0 - (1.0 - rgb_u8.double() / 255.0) * (1.0 - img_traj.double() / 255.0)
                imgs.append(torch.stack([img_traj, (upon * 255.0).to(torch.uint8)]))
                uvs.append(msplat.project_point(xyz_now, tr.intr, extr_now, tr.W, tr.H)[0])       # trainer.project_points
                if keep is not None:
                    keep.setdefault("traj_groups", []).append([x.clone() if isinstance(x, torch.Tensor) else x
                                                               for x in tr.last_traj_group])
        return torch.stack(imgs), torch.stack(uvs)

    psnr_sum = None

    def end_of_frame(i):
        # what every frame ends with, once its stages are fitted: the recorders that read the frame's final state (which share
        # final_forward's forward), its PSNR, the scores taken where the PSNR is
        nonlocal psnr_sum
        final.clear()
        if traj:
            record_trajectories()
        if tracker is not None:
            record_tracks(i)
        if flow_rec is not None:
            record_flow(i)
        # (PSNR stays on the device and is read ONCE at the end of the clip: a float() per frame drained the queue between
        #  two frames; with a log callback the caller asked for the numbers as they come)
        p = tr.psnr()
        psnr_sum = p.double() if psnr_sum is None else psnr_sum + p.double()
        if recon_rec is not None or cam_rec is not None:
            record_scores(i)
        if track_vis:
            from .render import render2img_device
            vis_frames.append(render2img_device(tr.last_render[:3]))
        if keep is not None:
            keep["psnr"].append(p)
        if log:
            log(f"frame {i}: psnr {float(p):.2f} dB, splats {tr.current_pts_num()}")

    if traj:
        traj_index, split_interval = select_traj_seeds(tr, int(c["traj_num"]), int(c["traj_offset"]))
        traj_index_t = torch.as_tensor(traj_index, device=tr.device).long()
    if keep is not None:
        keep["trainer"], keep["psnr"] = tr, []
    end_of_frame(0)
    for i in range(1, len(frames)):
        begin_frame(tr, frames, i, load_extr)
        if tr.seg_recorder is not None:
            tr.seg_recorder.frame = i
        if c["camera_first"]:                            # fit_video.py:256-278
            yield from tr.train_steps(**stage_kwargs(c, frames, i, "camera"), **common)
        if c["iterations_after"] > 0:                    # fit_video.py:288-315
            yield from tr.train_steps(**stage_kwargs(c, frames, i, "joint"), **common)
        end_of_frame(i)
    if tr.engine is not None:
        tr.engine.check_overflow()
    if traj:
        # one copy of every frame's two images and seed projections to the host, at the end of the clip (the reference copies
        # five images and the projections per frame, blocking: render2img, .cpu().numpy())
        imgs_d, uvs_d = draw_trajectories()
        if imgs_d.is_cuda:
            from .pinned import PINNED
            block = PINNED.take(imgs_d.numel())
            imgs_h = block[0][:imgs_d.numel()].view(imgs_d.shape)
            imgs_h.copy_(imgs_d, non_blocking=True)
            uvs_h = uvs_d.cpu()                          # (small; waits for the stream, and with it for the images above)
            traj_out = dict(images=PINNED.hand_out(block, [imgs_h])[0], uv=uvs_h.numpy(), index=list(traj_index),
                            split_interval=split_interval)
            PINNED.release(block)
        else:
            traj_out = dict(images=imgs_d.numpy(), uv=uvs_d.numpy(), index=list(traj_index), split_interval=split_interval)
        if keep is not None:
            keep["traj"] = traj_out
    out = dict(psnr_sum=float(psnr_sum), frames=len(frames), iterations=tr.iterations_done,
               rasterisations=tr.rasterisations_done, clips=1, splats_final=tr.current_pts_num(),
               # iterations that stepped nothing because a tile outgrew its reserved region, and were made up for
               void_iterations=tr.engine.regions_outgrown if tr.engine is not None else 0)
    if traj:
        # what the reference appends per frame -- frames_sequence_traj, frames_sequence_traj_upon, sequence_traj
        # (fit_video.py:226-238, 335-349): images (frames, 2, H, W, 3) uint8 [trajectories alone, upon the render],
        # uv (frames, seeds, 2), index, split_interval.  Not a number: callers that sum the dicts skip it (NUMERIC_KEYS)
        out["traj"] = traj_out
    if tracker is not None:
        out["tracks"] = tracker.result()              # (one copy to the host; not a number either)
    if segment:
        # one copy of every frame's (uv, sel) to the host, the hull masks, one launch that scores them all
        rec = tr.seg_recorder
        if keep is not None and keep.get("record_seg_inputs"):
            keep["seg_inputs"] = [None if x is None else (x[0].clone(), x[1].clone()) for x in rec.inputs]
        out["segmentation"] = rec.result([fr["move_mask"] for fr in frames])
    if recon_rec is not None:
        out["recon"] = recon_rec.result()             # (one copy of the (T, 2) sums)
    if cam_rec is not None:
        import numpy as np
        extr = cam_rec.result()                       # (one stacked copy)
        gt = np.stack([torch.as_tensor(e).detach().cpu().double().numpy().reshape(3, 4) for e in cam_gt])
        out["camera"] = dict(extr=extr, **CM.evaluate(extr, gt))
    if flow_rec is not None:
        out["flow"] = flow_rec.result()               # (one copy of the (T-1, 3, 6) sums; with "maps" the maps behind it)
    if track_vis:
        from . import track_vis as TV
        video = torch.stack(vis_frames)
        pred = seeds = masks = None
        if tracker is not None:
            pred = (out["tracks"]["tracks"], out["tracks"]["occluded"])
        if traj:
            # (the hull masks are host work on a few thousand points per frame, as for ``segment``; a frame before any mask
            #  exists has an empty one: nothing is occluded there)
            rec = tr.seg_recorder
            masks = out["segmentation"]["masks"] if segment else rec.masks(rec.fetch())[0]
            seeds = (traj_out["uv"], TV.seed_occlusions(masks, traj_out["uv"]), split_interval)
        out["track_vis"] = TV.clip_overlays(video, pred, seeds, track_vis if isinstance(track_vis, dict) else None)
        if keep is not None:
            keep["track_vis_inputs"] = dict(video=video.cpu().numpy(), masks=masks)
    return out


# the keys of fit_clip's dict that are per-clip numbers (sums over clips make sense); "traj" is the trajectory output,
# "tracks" the tracker's, "segmentation" the moving-region masks and their score, "recon" and "camera" the per-frame
# reconstruction sums and the camera path with its score, "flow" the per-pair flow sums (and maps)
NUMERIC_KEYS = ("psnr_sum", "frames", "iterations", "rasterisations", "clips", "splats_final", "void_iterations")


def fit_clips_concurrent(clips, device, cfg=None, seeds=None, chunk=32, partition=False, deterministic=None,
                         track_queries=None, track_backward=False, track_vis=False, **options):
    """Fit several clips AT THE SAME TIME on ONE device, in one host thread: every clip has its own trainer, engine and
    STREAM, and the clips take turns enqueueing ``chunk`` iterations each (fit_clip_steps), so their graph launches
    interleave on the device.  One fit leaves the chip partly idle -- its kernels are a chain of dependent launches,
    several of them latency bound with about one wave per SIMD, and the blend launches end with a tail of a few busy CUs
    -- so the launches of a second and third fit fill the gaps.  Clips are independent: this is the same
    sharding as one clip per GPU, applied inside a GPU.  A value read back by one fit (a densification event) stops
    the host only until THAT fit's stream has caught up; the others have their chunks queued meanwhile.
    (One host thread on purpose: with a thread per clip, graph captures of one thread and launches / allocations of
    another crashed inside the HIP runtime of ROCm 7.2 about once in four runs -- aborts in hipGraphDestroy, segmentation
    faults beside hipStreamEndCapture, silent exits.)  Returns the clips' metrics dicts in order; the caller times the call.
    ``partition``: every clip's stream is CU-MASKED to its own share of every XCD (_lib.cu_partition: 256 CUs / n, each share
    spanning all eight XCDs and their L2s) and its engines size their persistent blend grids and tile queues for that share
    (gfl_fit_state.cu_count) -- the clips then run SIDE BY SIDE instead of taking turns on every CU.  Results do not depend
    on it (the schedule never enters a result).  Measured in bench.py's ``clips_per_gpu`` table.
    ``deterministic`` (None: torch's switch): every clip's result is bit for bit that of fit_clip(..., deterministic=True)
    with the same seed -- without ``partition``, which changes the number of tile queues (include/gflow_hip.h).
    ``track_queries``: None, or one entry (fit_clip_steps' ``track_queries``, or None) per clip; ``track_backward``:
    fit_clip_steps' for every clip that has queries (ValueError without ``track_queries``).  ``track_vis``: fit_clip_steps',
    for all clips, or a list with one entry per clip.  ``options``: fit_clip_steps'
    other ones, for all clips (``async_snapshots`` and ``cu_count`` are set here)."""
    n = len(clips)
    if track_queries is not None and len(track_queries) != n:
        raise ValueError("fit_clips_concurrent: track_queries needs one entry per clip")
    if track_backward and track_queries is None:
        raise ValueError("fit_clips_concurrent(track_backward=True) needs track_queries")
    if isinstance(track_vis, (list, tuple)) and len(track_vis) != n:
        raise ValueError("fit_clips_concurrent: a list of track_vis needs one entry per clip")
    seeds = list(range(n)) if seeds is None else seeds
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    cur = torch.cuda.current_stream(dev)
    shares = None
    if partition and n > 1:
        from . import _lib
        shares = _lib.cu_partition(n, dev)
        streams = [_lib.masked_stream(words, dev) for words, _ in shares]
    else:
        streams = [torch.cuda.Stream(device=dev) for _ in range(n)]
    for s in streams:
        s.wait_stream(cur)
    # (a lone fit takes its snapshots on a side stream; several fits already fill each other's gaps, and a side stream + shadow
    #  engine per clip cost them more than they give)
    gens = [fit_clip_steps(clips[i], dev, cfg, seed=seeds[i], chunk=chunk, async_snapshots=n == 1,
                           cu_count=shares[i][1] if shares else 0, deterministic=deterministic,
                           track_queries=None if track_queries is None else track_queries[i],
                           track_backward=bool(track_backward) and track_queries[i] is not None,
                           track_vis=track_vis[i] if isinstance(track_vis, (list, tuple)) else track_vis, **options)
            for i in range(n)]
    results = [None] * n
    live = list(range(n))
    while live:
        for i in list(live):
            with torch.cuda.stream(streams[i]):
                try:
                    next(gens[i])
                except StopIteration as e:
                    results[i] = e.value
                    live.remove(i)
    for s in streams:
        cur.wait_stream(s)
    return results


def main(argv=None):
    ap = argparse.ArgumentParser(description="fit synthetic clips, one process per GPU")
    ap.add_argument("--clips", type=int, default=1)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--num_points", type=int, default=60000)
    ap.add_argument("--iterations_first", type=int, default=500)
    ap.add_argument("--iterations_after", type=int, default=300)
    ap.add_argument("--iterations_camera", type=int, default=150)
    ap.add_argument("--frames-list", default=None, help="comma-separated frame counts, one per synthetic clip (clips of "
                                                        "unequal length: the shard balances them)")
    ap.add_argument("--clips-per-gpu", type=int, default=1,
                    help="clips a rank fits at the same time on its GPU (fit_clips_concurrent)")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--sequence", action="append", default=None,
                    help="path of a prepared sequence folder (images + the reference's sibling folders, "
                         "gflow_amd/io.py); may be given several times, one clip each; default: synthetic clips")
    ap.add_argument("--resize", type=int, default=None, help="shorter image side after loading a --sequence")
    ap.add_argument("--deterministic", action="store_true",
                    help="bit-identical results for identical inputs (the library's deterministic mode, INTEGRATION.md)")
    ap.add_argument("--track", action="store_true",
                    help="track the first-visible query points of each clip's tracking.pkl (synthetic clips: their "
                         "make_clip_tracks) through the fit and score them with TAP-Vid (a \"tapvid\" block in the line)")
    ap.add_argument("--track-backward", action="store_true",
                    help="with --track: also track every query through the frames before its own (the \"tapvid\" block "
                         "then carries \"backward\": true)")
    ap.add_argument("--track-queries", choices=("first", "strided"), default="first",
                    help="with --track: the query protocol -- each track's first visible frame, or TAP-Vid's strided one "
                         "(every fifth frame where the track is visible; wants --track-backward)")
    ap.add_argument("--track-out", default=None, help="with --track: write each clip's predicted tracks to DIR/clip_<i>.npz")
    ap.add_argument("--track-vis", default=None,
                    help="paint the tracks over every frame's render on the device (the reference's trajectory visualiser) and "
                         "write DIR/clip_<i>/<name>/<frame>.png: with --track `pred` and `gt` (the ground-truth tracks and "
                         "occlusion flags), with --traj-num `seeds`, `seeds_still`, `seeds_move`")
    ap.add_argument("--traj-num", type=int, default=0,
                    help="trajectory seeds per clip (cfg traj_num; the reference's scripts use 100)")
    ap.add_argument("--seg", action="store_true",
                    help="keep every frame's moving-region mask and score it against the frame's move_mask with DAVIS J, F "
                         "and J&F (a \"davis\" block in the line)")
    ap.add_argument("--seg-out", default=None,
                    help="with --seg: write each clip's masks to DIR/clip_<i>/move_mask_<frame>.png")
    ap.add_argument("--recon", action="store_true",
                    help="score every frame's render with PSNR and SSIM on the device (a \"recon\" block in the line)")
    ap.add_argument("--camera", action="store_true",
                    help="keep every frame's camera and score the path against the clip's own (extr_gt, else extr) with "
                         "ATE and RPE (a \"camera\" block in the line)")
    ap.add_argument("--flow", action="store_true",
                    help="the dense optical flow the fitted splats imply between consecutive frames, scored against the flow "
                         "the clip came with: end-point error, still / moving, accuracies, coverage (a \"flow\" block in the "
                         "line)")
    ap.add_argument("--flow-out", default=None,
                    help="with --flow: write each clip's flow maps to DIR/clip_<i>/flow_<frame>.flo (frame -> frame + 1 on "
                         "the frame's grid; pixels without a flow are 1e10, Middlebury's mark)")
    ap.add_argument("--no-load-extr", action="store_true",
                    help="do not load the frames' camera poses (extr): the camera-only stages estimate them, as the "
                         "reference's scripts/fit_video.sh runs")
    ap.add_argument("--make-move-masks", action="store_true",
                    help="with --sequence: compute every frame's move_mask from its forward flow on the device "
                         "(gflow_amd.move_seg, before the clock starts) instead of reading <seq>_epipolar")
    ap.add_argument("--make-occ-masks", action="store_true",
                    help="with --sequence: compute every frame's occ_mask from its forward and backward flows "
                         "(<seq>_flow_unimatch/*pred.flo, *pred_bwd.flo) on the device (gflow_amd.occlusion, before the clock "
                         "starts) instead of reading *occ_bwd.png")
    ap.add_argument("--metrics-csv", default=None,
                    help="rank 0 writes the blocks that were asked for as key,value lines under the reference's "
                         "metrics.csv keys")
    args = ap.parse_args(argv)
    if args.track_backward and not args.track:
        ap.error("--track-backward needs --track")
    if args.track_vis and not (args.track or args.traj_num > 0):
        ap.error("--track-vis needs --track or --traj-num")
    if args.track and args.track_queries == "strided" and not args.track_backward:
        print("warning: --track-queries strided without --track-backward: every frame before a query is a miss",
              file=sys.stderr)
    det = True if args.deterministic else None
    from . import synthetic as S
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    n_dev = torch.cuda.device_count()
    if n_dev < 1:
        raise RuntimeError("gflow_amd.fit_video needs a HIP device (there is no CPU rasteriser)")
    # (ranks share devices only on a box with fewer GPUs than ranks -- a functional run; RCCL refuses two ranks on
    # one device, so the two small metric all-reduces then go over gloo, as in bench.py)
    shared = world > n_dev
    torch.cuda.set_device(local_rank % n_dev)
    dev = torch.device("cuda", local_rank % n_dev)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if shared:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=dev)
    cfg = dict(num_points=args.num_points, iterations_first=args.iterations_first,
               iterations_after=args.iterations_after, iterations_camera=args.iterations_camera)
    if args.traj_num > 0:
        cfg["traj_num"] = args.traj_num
    local = {k: 0.0 for k in METRIC_NAMES}
    n_clips = len(args.sequence) if args.sequence else args.clips
    # how long is every clip?  (every rank must see the same numbers: they decide who fits what)
    if args.sequence:
        from . import io as gio
        lengths = [len(gio.sequence_paths(p)["img"]) for p in args.sequence]
    elif args.frames_list:
        lengths = [int(v) for v in args.frames_list.split(",")]
        if len(lengths) != n_clips:
            raise SystemExit("--frames-list needs one length per clip")
    else:
        lengths = [args.frames] * n_clips
    mine = shard(n_clips, rank, world, lengths)
    # reading / synthesising the clips is not part of the fit: do it before the clock starts
    t_load = time.perf_counter()
    clips = {}
    for ci in mine:
        if args.sequence:
            clips[ci] = gio.load_sequence(args.sequence[ci], resize=args.resize,
                                          move_masks="epipolar" if args.make_move_masks else "files",
                                          occ_masks="flow" if args.make_occ_masks else "files")
        else:
            clips[ci] = upload_clip(S.make_clip(lengths[ci], args.height, args.width, seed=ci, device=dev), dev)
    # point tracking: the ground truth of every clip, its first-visible queries (those whose frame is not fitted: dropped)
    gts, queries, dropped = {}, {}, 0
    if args.track:
        for ci in mine:
            h, w = clips[ci][0]["image"].shape[:2]
            if args.sequence:
                pts, occ = TK.read_tapvid_pickle(os.path.join(args.sequence[ci], "tracking.pkl"))
            else:
                g = S.make_clip_tracks(lengths[ci], args.height, args.width, seed=ci)
                pts, occ = g["points"].astype("float32"), g["occluded"]
            if args.track_queries == "strided":
                q, src = TK.strided_queries(pts, occ, h, w)
                keep = q[:, 0] < len(clips[ci])
                gts[ci] = (pts, occ, h, w, q[keep], src[keep])
            else:
                q = TK.first_visible_queries(pts, occ, h, w)
                keep = q[:, 0] < len(clips[ci])
                gts[ci] = (pts[keep], occ[keep], h, w)
            dropped += int((~keep).sum())
            queries[ci] = q[keep]
    t_load = time.perf_counter() - t_load
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = max(1, args.clips_per_gpu)
    order = sorted(clips, key=lambda j: (-lengths[j], j))          # (clips of similar length share the GPU)
    options = dict(track_backward=args.track_backward, deterministic=det, segment=args.seg, recon=args.recon, camera=args.camera,
                   flow=("maps" if args.flow_out else True) if args.flow else False, load_extr=not args.no_load_extr)

    def vis_option(ci):
        # --track-vis: with --track the ground truth as one more overlay, scaled to pixels like benchmark.py:151-154
        if not args.track_vis:
            return False
        if ci not in gts:
            return True
        import numpy as np
        pts, occ, h, w = gts[ci][:4]
        n = len(clips[ci])
        xy = pts[:, :n].astype(np.float32) * np.array([w, h], dtype=np.float32)
        return dict(gt=(np.ascontiguousarray(xy.transpose(1, 0, 2)), np.ascontiguousarray(occ[:, :n].T)))

    results = {}
    for g0 in range(0, len(order), c):
        group = order[g0:g0 + c]
        if len(group) == 1:
            ci = group[0]
            res = [fit_clip(clips[ci], dev, cfg, seed=ci, track_queries=queries.get(ci), track_vis=vis_option(ci), **options,
                            log=(lambda s, ci=ci: print(f"[rank {rank} clip {ci}] {s}")) if args.verbose else None)]
        else:
            res = fit_clips_concurrent([clips[ci] for ci in group], dev, cfg, seeds=group,
                                       track_queries=[queries.get(ci) for ci in group] if args.track else None,
                                       track_vis=[vis_option(ci) for ci in group], **options)
        for ci, m in zip(group, res):
            for k in METRIC_NAMES:
                local[k] += m[k]
            results[ci] = m
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    of = lambda key: {ci: m[key] for ci, m in results.items()}         # (a block that was asked for is in every clip's dict)
    over_ranks = (dist, torch.device("cpu") if (world > 1 and shared) else dev)
    out = reduce_metrics(local, wall, *over_ranks, rank=rank, world=world)
    if args.track:
        preds = of("tracks")
        out["tapvid"] = reduce_tapvid(preds, gts, {ci: len(clips[ci]) for ci in clips}, dropped, *over_ranks)
        if args.track_backward:
            out["tapvid"]["backward"] = True
        if args.track_out:
            import numpy as np
            os.makedirs(args.track_out, exist_ok=True)
            for ci, p in preds.items():
                np.savez(os.path.join(args.track_out, f"clip_{ci}.npz"), queries=queries[ci], **p)
    if args.track_vis:
        from . import track_vis as TV
        for ci, vis in of("track_vis").items():
            for name, imgs in vis.items():
                TV.write_frames(imgs, os.path.join(args.track_vis, f"clip_{ci}", name))
    if args.seg:
        out["davis"] = reduce_davis(of("segmentation"), *over_ranks)
        if args.seg_out:
            from PIL import Image
            for ci, seg in of("segmentation").items():
                d = os.path.join(args.seg_out, f"clip_{ci}")
                os.makedirs(d, exist_ok=True)
                for t in range(len(seg["masks"])):
                    if seg["valid"][t]:                      # (no file for a frame without a mask, like the reference)
                        Image.fromarray(seg["masks"][t]).save(os.path.join(d, f"move_mask_{t:05d}.png"))
    if args.recon:
        out["recon"] = reduce_recon(of("recon"), *over_ranks)
    if args.camera:
        out["camera"] = reduce_camera(of("camera"), *over_ranks)
    if args.flow:
        out["flow"] = reduce_flow(of("flow"), *over_ranks)
        if args.flow_out:
            for ci, fl in of("flow").items():
                FL.write_flo_maps(os.path.join(args.flow_out, f"clip_{ci}"), fl)
    if rank == 0 and args.metrics_csv:
        QL.write_metrics_csv(args.metrics_csv, csv_metrics(out))
    if rank == 0:
        out["frames_per_s"] = out["frames"] / out["wall_s"]
        out["iterations_per_s"] = out["iterations"] / out["wall_s"]
        out["psnr_mean_db"] = out["psnr_sum"] / max(out["frames"], 1.0)
        out["n_gpus"] = world
        out["clips_per_gpu"] = c
        out["load_s_rank0"] = t_load
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()
    return out if rank == 0 else None


if __name__ == "__main__":
    main()
