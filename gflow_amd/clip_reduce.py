"""What a job sums over its clips and ranks (host-only code; importable from ``gflow_amd.fit_video`` as before).

Multi-GPU: clips are independent, frames of one clip are not.  One process per GPU, the clips dealt to the
ranks by length (``shard``), no data-path collective; at the end ONE all-reduce(SUM) of a small metrics vector (which also
carries every rank's own wall time in a slot of its own) and ONE all-reduce(MAX) of the wall time (``reduce_metrics``), then
one small all-reduce(SUM) per block of the JSON line that was asked for (``_mean_over_clips`` behind the five ``reduce_*``)."""
import math

import torch

from . import camera as CM
from . import flow as FL
from . import quality as QL
from . import segmentation as SG
from . import tracking as TK

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
