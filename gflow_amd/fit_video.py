"""Video driver -- the public module of the clip fit and its command line, plus clip sharding.

The fit of one clip lives in ``gflow_amd.clip_fit`` (``ClipFit``, ``fit_clip``, ``fit_clip_steps``, ``fit_clips_concurrent``
and what they share), what a job sums over its clips and ranks in ``gflow_amd.clip_reduce`` (``shard``, ``reduce_*``); every
name of both is importable from here, as it always was.  ``main`` is the command line: a sequence of named steps.

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
import os
import sys
import time

import numpy as np
import torch

from . import flow as FL
from . import io as gio
from . import propagation as PG
from . import quality as QL
from . import synthetic as S
from . import track_vis as TV
from . import tracking as TK
from .clip_fit import (DEFAULTS, NUMERIC_KEYS, SCRIPT_OVERRIDES, ClipFit, begin_frame, fit_clip,      # noqa: F401  (public here)
                       fit_clip_steps, fit_clips_concurrent, select_traj_seeds, stage_kwargs, upload_clip)
from .clip_reduce import (CAMERA_KEYS, DAVIS_KEYS, FLOW_KEYS, METRIC_NAMES, RECON_KEYS, TAPVID_KEYS,  # noqa: F401  (public here)
                          _mean_over_clips, csv_metrics, reduce_camera, reduce_davis, reduce_flow, reduce_metrics,
                          reduce_recon, reduce_tapvid, shard)


def _parser():
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
                         "gflow_amd/io.py), or of a Motion-JPEG .avi file that stands for the folder of its frames; may be "
                         "given several times, one clip each; default: synthetic clips")
    ap.add_argument("--resize", type=int, default=None, help="shorter image side after loading a --sequence")
    ap.add_argument("--blur", action="store_true",
                    help="with --sequence: GaussianBlur(7, 5.0) on the image, the occlusion mask and the flow after the resize "
                         "(the reference's blur option)")
    ap.add_argument("--prep", choices=("host", "device"), default="host",
                    help="with --sequence: where the decoded files are converted, resized and blurred -- on the host with "
                         "torch, one file at a time, or as whole stacks on this rank's device (gflow_amd.prep)")
    ap.add_argument("--decode", choices=("host", "device", "device-all"), default="host",
                    help="with --sequence: where the image files are decoded -- PIL on the host, or the JPEG files as one stack "
                         "on this rank's device (gflow_amd.video.decode_jpeg: the same bits; implies --prep device); "
                         "device-all decodes the PNG images and masks there too (gflow_amd.png.decode_png).  A "
                         "--sequence that is a .avi file is always decoded and prepared on the device")
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
    ap.add_argument("--video", action="store_true",
                    help="with --track-vis: also write every overlay as DIR/clip_<i>/<name>.avi beside its folder of PNGs, a "
                         "Motion-JPEG AVI at 5 fps coded on the device (gflow_amd.video)")
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
    ap.add_argument("--propagate", action="store_true",
                    help="propagate the object ids of the first frame's annotation (<seq>_mask/*.png; a synthetic clip's first "
                         "move mask) through the clip and score every later frame that has one with DAVIS J, F and J&F per "
                         "object (a \"davis_semi\" block in the line)")
    ap.add_argument("--propagate-out", default=None,
                    help="with --propagate: write each clip's id maps to DIR/clip_<i>/<frame name>.png (with the prompt "
                         "file's palette if it has one, else grey ids; unknown pixels are 0)")
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
    ap.add_argument("--make-flows", action="store_true",
                    help="with --sequence: estimate every pair's forward and backward flow from the images on the device "
                         "(gflow_amd.optflow, a classical variational estimate, before the clock starts) instead of reading "
                         "<seq>_flow_unimatch/*pred.flo, *pred_bwd.flo; --make-move-masks and --make-occ-masks then run on "
                         "the estimated flows")
    ap.add_argument("--make-depth-camera", action="store_true",
                    help="with --sequence: estimate every frame's depth and pose from the flows on the device (gflow_amd.sfm, "
                         "classical two-view geometry, NOT MASt3R: depth only where the camera translates, moving and "
                         "occluded regions filled from their surroundings; before the clock starts) instead of reading "
                         "<seq>_depth_mast3r_s2/*.npy and <seq>_camera_mast3r_s2/*.json; with --make-flows "
                         "--make-move-masks --make-occ-masks a sequence needs only its images")
    ap.add_argument("--focal", type=float, default=None,
                    help="with --make-depth-camera: the focal length in pixels of the native images (default: max(W, H), an "
                         "assumption)")
    ap.add_argument("--out", default=None,
                    help="save every clip's fit as the reference's log folder DIR/clip_<i>/ (ckpt/, images/, images_seg/, the "
                         "sequence*.avi files; gflow_amd.log_folder): `python -m gflow_amd.viewer --folder DIR/clip_0` opens it")
    ap.add_argument("--metrics-csv", default=None,
                    help="rank 0 writes the blocks that were asked for as key,value lines under the reference's "
                         "metrics.csv keys")
    return ap


def _check_args(ap, args):
    if args.make_flows and not args.sequence:
        ap.error("--make-flows needs --sequence")
    if args.make_depth_camera and not args.sequence:
        ap.error("--make-depth-camera needs --sequence")
    if args.focal is not None and not args.make_depth_camera:
        ap.error("--focal needs --make-depth-camera")
    if args.track_backward and not args.track:
        ap.error("--track-backward needs --track")
    if args.track_vis and not (args.track or args.traj_num > 0):
        ap.error("--track-vis needs --track or --traj-num")
    if args.propagate_out and not args.propagate:
        ap.error("--propagate-out needs --propagate")
    if args.video and not args.track_vis:
        ap.error("--video needs --track-vis")
    if args.track and args.track_queries == "strided" and not args.track_backward:
        print("warning: --track-queries strided without --track-backward: every frame before a query is a miss",
              file=sys.stderr)


def _ranks():
    """(rank, world, this rank's device, torch.distributed or None, (dist, device) of the small metric all-reduces)"""
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
    return rank, world, dev, dist, (dist, torch.device("cpu") if (world > 1 and shared) else dev)


def _clip_lengths(args):
    """how long is every clip?  (every rank must see the same numbers: they decide who fits what)"""
    n_clips = len(args.sequence) if args.sequence else args.clips
    if args.sequence:
        return [len(gio.sequence_paths(p)["img"]) for p in args.sequence]
    if args.frames_list:
        lengths = [int(v) for v in args.frames_list.split(",")]
        if len(lengths) != n_clips:
            raise SystemExit("--frames-list needs one length per clip")
        return lengths
    return [args.frames] * n_clips


def _load_clips(args, mine, lengths, dev):
    clips = {}
    for ci in mine:
        if args.sequence:
            clips[ci] = gio.load_sequence(args.sequence[ci], resize=args.resize,
                                          move_masks="epipolar" if args.make_move_masks else "files",
                                          occ_masks="flow" if args.make_occ_masks else "files", blur=args.blur,
                                          device=dev if (args.prep == "device" or args.decode != "host"
                                                         or gio.is_video(args.sequence[ci])) else None,
                                          decode=args.decode,
                                          flows="estimate" if args.make_flows else "files",
                                          depth_camera="estimate" if args.make_depth_camera else "files", focal=args.focal,
                                          object_masks="files" if args.propagate else "none")
        else:
            clips[ci] = upload_clip(S.make_clip(lengths[ci], args.height, args.width, seed=ci, device=dev), dev)
            if args.propagate:                   # (a synthetic clip's one object is its moving disc)
                for fr in clips[ci]:
                    fr["object_mask"] = fr["move_mask"].to(torch.uint8)
        if args.propagate and (not clips[ci] or clips[ci][0].get("object_mask") is None):
            raise SystemExit(f"--propagate: clip {ci} has no annotation of its first frame (<seq>_mask/*.png)")
    return clips


def _tracking_ground_truth(args, clips, lengths):
    """point tracking: the ground truth of every clip, its queries (those whose frame is not fitted: dropped).  Returns
    (gts, queries, dropped); ``gts[ci]`` is what reduce_tapvid and _vis_option read"""
    gts, queries, dropped = {}, {}, 0
    if not args.track:
        return gts, queries, dropped
    for ci in clips:
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
    return gts, queries, dropped


def _vis_option(args, gts, clips, ci):
    # --track-vis: with --track the ground truth as one more overlay, scaled to pixels like benchmark.py:151-154
    if not args.track_vis:
        return False
    if ci not in gts:
        return True
    pts, occ, h, w = gts[ci][:4]
    n = len(clips[ci])
    xy = pts[:, :n].astype(np.float32) * np.array([w, h], dtype=np.float32)
    return dict(gt=(np.ascontiguousarray(xy.transpose(1, 0, 2)), np.ascontiguousarray(occ[:, :n].T)))


def _fit_groups(args, clips, lengths, dev, cfg, gts, queries, rank):
    """Every clip of this rank fitted, ``--clips-per-gpu`` at a time: {clip: its dict}, in the order they were fitted"""
    c = max(1, args.clips_per_gpu)
    order = sorted(clips, key=lambda j: (-lengths[j], j))          # (clips of similar length share the GPU)
    options = dict(track_backward=args.track_backward, deterministic=True if args.deterministic else None, segment=args.seg,
                   recon=args.recon, camera=args.camera, flow=("maps" if args.flow_out else True) if args.flow else False,
                   load_extr=not args.no_load_extr)
    prompt = lambda ci: clips[ci][0]["object_mask"] if args.propagate else None
    folder = lambda ci: os.path.join(args.out, f"clip_{ci}") if args.out else None
    results = {}
    for g0 in range(0, len(order), c):
        group = order[g0:g0 + c]
        if len(group) == 1:
            ci = group[0]
            res = [fit_clip(clips[ci], dev, cfg, seed=ci, track_queries=queries.get(ci),
                            track_vis=_vis_option(args, gts, clips, ci), propagate=prompt(ci), save=folder(ci), **options,
                            log=(lambda s, ci=ci: print(f"[rank {rank} clip {ci}] {s}")) if args.verbose else None)]
        else:
            res = fit_clips_concurrent([clips[ci] for ci in group], dev, cfg, seeds=group,
                                       track_queries=[queries.get(ci) for ci in group] if args.track else None,
                                       track_vis=[_vis_option(args, gts, clips, ci) for ci in group],
                                       propagate=[prompt(ci) for ci in group] if args.propagate else None,
                                       save=[folder(ci) for ci in group] if args.out else None, **options)
        results.update(zip(group, res))
    return results


def _report(args, results, wall, clips, gts, queries, dropped, rank, world, over_ranks):
    """The reductions over clips and ranks, the files that were asked for, the CSV: the JSON line's dict without rank 0's tail"""
    local = {k: sum((m[k] for m in results.values()), 0.0) for k in METRIC_NAMES}
    of = lambda key: {ci: m[key] for ci, m in results.items()}         # (a block that was asked for is in every clip's dict)
    out = reduce_metrics(local, wall, *over_ranks, rank=rank, world=world)
    if args.track:
        preds = of("tracks")
        out["tapvid"] = reduce_tapvid(preds, gts, {ci: len(clips[ci]) for ci in clips}, dropped, *over_ranks)
        if args.track_backward:
            out["tapvid"]["backward"] = True
        if args.track_out:
            os.makedirs(args.track_out, exist_ok=True)
            for ci, p in preds.items():
                np.savez(os.path.join(args.track_out, f"clip_{ci}.npz"), queries=queries[ci], **p)
    if args.track_vis:
        for ci, vis in of("track_vis").items():
            for name, imgs in vis.items():
                TV.write_frames(imgs, os.path.join(args.track_vis, f"clip_{ci}", name))
                if args.video:
                    TV.write_video(imgs, os.path.join(args.track_vis, f"clip_{ci}", name + ".avi"))
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
    if args.propagate:
        out["davis_semi"] = reduce_davis({ci: p["flat"] for ci, p in of("propagation").items()}, *over_ranks)
        if args.propagate_out:
            for ci, p in of("propagation").items():
                palette = None
                if args.sequence:
                    from PIL import Image
                    first = Image.open(gio.sequence_paths(args.sequence[ci])["objects"][0])
                    palette = first.getpalette() if first.mode == "P" else None
                PG.write_id_maps(os.path.join(args.propagate_out, f"clip_{ci}"), p["maps"],
                                 [fr.get("name", f"{t:05d}") for t, fr in enumerate(clips[ci])], palette)
    if rank == 0 and args.metrics_csv:
        QL.write_metrics_csv(args.metrics_csv, csv_metrics(out))
    return out


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    _check_args(ap, args)
    rank, world, dev, dist, over_ranks = _ranks()
    cfg = dict(num_points=args.num_points, iterations_first=args.iterations_first,
               iterations_after=args.iterations_after, iterations_camera=args.iterations_camera)
    if args.traj_num > 0:
        cfg["traj_num"] = args.traj_num
    lengths = _clip_lengths(args)
    mine = shard(len(lengths), rank, world, lengths)
    # reading / synthesising the clips is not part of the fit: do it before the clock starts
    t_load = time.perf_counter()
    clips = _load_clips(args, mine, lengths, dev)
    gts, queries, dropped = _tracking_ground_truth(args, clips, lengths)
    t_load = time.perf_counter() - t_load
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    results = _fit_groups(args, clips, lengths, dev, cfg, gts, queries, rank)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out = _report(args, results, wall, clips, gts, queries, dropped, rank, world, over_ranks)
    if rank == 0:
        out["frames_per_s"] = out["frames"] / out["wall_s"]
        out["iterations_per_s"] = out["iterations"] / out["wall_s"]
        out["psnr_mean_db"] = out["psnr_sum"] / max(out["frames"], 1.0)
        out["n_gpus"] = world
        out["clips_per_gpu"] = max(1, args.clips_per_gpu)
        out["load_s_rank0"] = t_load
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()
    return out if rank == 0 else None


if __name__ == "__main__":
    main()
