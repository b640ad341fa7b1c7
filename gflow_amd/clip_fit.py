"""The fit of one clip -- the counterpart of gflow/fit_video.py's frame loop (importable from ``gflow_amd.fit_video`` as before).

``fit_clip`` keeps the reference's structure (fit_video.py:105-349): first-frame fit with
``iterations_first``; then for every later frame an optional camera-only fit
(``iterations_camera``, ``lr_camera_after``) followed by the full fit (``iterations_after``,
``lr_after``, occlusion-mask densification at iteration 0).  Inputs are in-memory frames (dicts
as produced by ``gflow_amd.synthetic.make_clip``: image, depth, flow, move_mask, occ_mask, focal,
pp); the reference's file readers are ``gflow_amd.io``, its log folder -- checkpoints, images, videos -- is what ``save`` writes
(``gflow_amd.log_folder``).

``ClipFit`` is one clip's fit as an object: ``__init__`` refuses what can be refused and builds the trainer and the
recorders that were asked for, ``steps()`` is the frame loop as a generator, ``result()`` the clip's dict.
``fit_clip_steps`` (whose docstring names the options) is the three in a row; ``fit_clip`` drives it to its end on a
stream of its own, ``fit_clips_concurrent`` drives several in turns."""
import numpy as np
import torch

from . import camera as CM
from . import flow as FL
from . import log_folder as LF
from . import msplat
from . import propagation as PG
from . import quality as QL
from . import render as render_mod
from . import segmentation as SG
from . import track_vis as TV
from . import tracking as TK
from .fused import REC
from .pinned import PINNED
from .trainer import SimpleGaussian, run_to_end      # (no cycle: nothing below trainer -> stage -> render imports this module)

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

# the keys of fit_clip's dict that are per-clip numbers (sums over clips make sense); "traj" is the trajectory output,
# "tracks" the tracker's, "segmentation" the moving-region masks and their score, "recon" and "camera" the per-frame
# reconstruction sums and the camera path with its score, "flow" the per-pair flow sums (and maps), "propagation" the object
# id maps and their score
NUMERIC_KEYS = ("psnr_sum", "frames", "iterations", "rasterisations", "clips", "splats_final", "void_iterations")

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


def _closest_splats(uv, points):
    """utils.find_closest_point (tracking.py:24-26): for every pixel of ``points`` the argmin over the splats' ``uv``"""
    q = torch.tensor(points, dtype=torch.float64, device=uv.device)
    out = []
    for a in range(0, q.shape[0], 256):              # (chunks: N x 256 distances at a time)
        d = ((uv[:, None, :] - q[None, a:a + 256, :]) ** 2).sum(-1)
        out.append(d.argmin(dim=0))
    return torch.cat(out)


def select_traj_seeds(tr, traj_num, traj_offset):
    """The splats whose trajectories are drawn (fit_video.py:163-211, ``grid_traj = True`` as the reference hard-codes it):
    pixels of a grid -- stride 50 inside the eroded still region, stride 15 inside the eroded moving region (``move_seg``, the
    hull mask of the first frame's fit; a 10 x 10 erosion, cv2.erode's default border: nothing eroded from the image's edge) --
    and for every grid pixel the splat whose projection (``last_uv``) lies closest, kept if its still / moving label is the
    region's.  Returns (indices: still seeds first, split_interval = their number or None without moving seeds).
    Without a hull mask (fewer than six moving splats: the reference would fail in cv2.erode) the plain rule of
    fit_video.py:165-167, every (N / traj_num)-th splat from ``traj_offset``.  Once per clip; the nearest-splat search runs on
    the device (the reference forms an N x Q x 2 array in numpy), one read-back of the few hundred indices."""
    from scipy.ndimage import minimum_filter
    n = tr.current_pts_num()
    interval = max(int(n / traj_num), 1)
    plain = list(range(n))[traj_offset::interval]
    move_seg = tr.move_seg
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
    if len(sparse) == 0:
        # (H or W <= 50: the stride-50 grid has no pixel at all -- the reference would index an empty array, :200-203; the
        #  plain rule is what it falls back to without a mask)
        return plain, None
    sp = _closest_splats(uv, sparse)
    sp_still = sp[still[sp]]
    if len(dense):
        de = _closest_splats(uv, dense)
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


def _pose_gt(fr):
    """the pose a frame's camera is scored against: its ``extr_gt`` if it has one, else its ``extr`` (None: neither)"""
    return fr["extr_gt"] if fr.get("extr_gt") is not None else fr.get("extr")


class ClipFit:
    """One clip's fit: the options (fit_clip_steps' docstring), the trainer, the recorders that were asked for and what the
    frames leave behind.  Every attribute exists from ``__init__`` on and is None while its option is off or its moment has
    not come.  The next output of a clip goes here: refused and built in ``__init__``, read in ``end_of_frame``, copied out in
    ``result``."""

    def __init__(self, frames, device, cfg=None, seed=0, snapshot_interval=0, fused=True, log=None, load_extr=True, chunk=None,
                 async_snapshots=True, keep=None, cu_count=0, deterministic=None, track_queries=None, segment=False,
                 recon=False, camera=False, flow=False, track_backward=False, track_vis=False, propagate=None, save=None):
        if track_backward and track_queries is None:
            raise ValueError("fit_clip(track_backward=True) needs track_queries")
        # (ValueError before anything is fitted: the operator path, names that are no file names)
        self.clip_log = None if save is None else LF.ClipLog(save, frames, fused=fused)
        if track_vis and track_queries is None and not int((cfg or {}).get("traj_num", DEFAULTS["traj_num"])) > 0:
            raise ValueError("fit_clip(track_vis=True) needs track_queries or cfg['traj_num'] > 0")
        self.tracker = None
        if track_queries is not None:
            # (ValueError before anything is fitted)
            self.tracker = TK.Tracker(track_queries, len(frames), device, backward=bool(track_backward))
        self.cam_rec = None
        if camera:
            missing = [t for t, fr in enumerate(frames) if _pose_gt(fr) is None]
            if missing:
                raise ValueError(f"fit_clip(camera=True): frames {missing} carry neither extr_gt nor extr")
            self.cam_rec = CM.CameraRecorder(len(frames))
        c = dict(DEFAULTS)
        c.update(cfg or {})
        if any(isinstance(v, torch.Tensor) and not v.is_cuda for k, v in frames[0].items() if k != "extr"):
            frames = upload_clip(frames, device)         # (bench.py uploads before its clock starts: "inputs resident in HBM")
        self.cfg, self.frames = c, frames
        self.log, self.load_extr, self.keep, self.segment, self.track_vis = log, load_extr, keep, segment, track_vis
        self.traj = int(c["traj_num"]) > 0
        f0 = frames[0]
        tr = SimpleGaussian(f0["image"], f0["depth"], num_points=c["num_points"], background=c["background"],
                            device=device, seed=seed, fused=fused, deterministic=deterministic)
        tr.async_snapshots = bool(async_snapshots)       # (trainer.py: snapshots composed beside the next iterations, or behind theirs)
        tr.cu_count = int(cu_count)                      # (the caller's stream is CU-masked: fit_clips_concurrent(partition=True))
        if segment or (track_vis and self.traj) or self.clip_log is not None:
            tr.seg_recorder = SG.MoveSegRecorder(len(frames), tr.H, tr.W, tr.device)
        self.tr = tr
        self.vis_frames = [] if track_vis else None      # track_vis: every frame's final render, (H, W, 3) uint8 on the device
        self.recon_rec = QL.ReconRecorder(len(frames), tr.H, tr.W, tr.device) if recon else None
        self.flow_rec = None
        if flow:
            self.flow_rec = FL.FlowRecorder(len(frames), tr.H, tr.W, tr.device, keep_maps=flow == "maps")
            if keep is not None and keep.get("record_flow_inputs"):
                self.flow_rec.inputs = keep.setdefault("flow_inputs", [])
        # (ValueError for a prompt the recorder refuses: nothing has been fitted yet)
        self.object_rec = None if propagate is None else PG.ObjectRecorder(len(frames), tr.H, tr.W, tr.device, propagate)
        tr.load_camera(focal=f0["focal"], pp=f0["pp"])
        if load_extr and f0.get("extr") is not None:
            tr.load_camera(extr=f0["extr"])
        tr.init_gaussians_from_image(f0["image"], f0["depth"], num_points=c["num_points"])
        self.common = dict(lambda_rgb=c["lambda_rgb"], lambda_depth=c["lambda_depth"], lambda_scale=c["lambda_scale"],
                           densify_occ_percent=c["densify_occ_percent"], densify_err_thre=c["densify_err_thre"],
                           densify_err_percent=c["densify_err_percent"], snapshot_interval=snapshot_interval,
                           lazy_images=True,        # (the image lists train() returns are not read here: do not wait for them)
                           chunk=chunk)
        self.traj_rec = [] if self.traj else None        # per frame: where the seeds are, the camera, the scene's rgb image
        # the trajectory seeds (select_traj_seeds, after the first frame's fit): their rows, those on the device, the split
        self.traj_index = self.traj_index_t = self.split_interval = None
        self.final = None                                # the engine of this frame's final_forward, once it has run (end_of_frame forgets it)
        self.final_images = None                         # and the scene's images, if the reader that ran it asked for them
        self.psnr_sum = None

    def final_forward(self, scene=False):
        # The forward of THIS frame's final state on the second engine (fused path): run when the first of the frame's
        # recorders asks for it, shared by those after it -- the frame is rasterised once more, not once per recorder.
        # Returns (that engine, None); the reader that runs it may ask for the scene's images too (``scene=True``, the
        # log recorder and the trajectory recorder, which ask first): (the engine, (3, H, W, 3) uint8) -- the forward, the
        # snapshot of its images, then the overflow watch; the images are kept for a later reader that asks for them too.
        tr = self.tr
        if self.final is None:
            if scene:
                self.final_images = tr.second.scene_u8(tr.engine, tr.bg)
            else:
                tr.second.forward(tr.engine, tr.bg).watch_overflow()
            self.final = tr.second.engine
            tr.rasterisations_done += 1
        return self.final, (self.final_images if scene else None)

    def record_trajectories(self):
        # fit_video.py:226-238 / 335-349 call trainer.eval + project_points here, after every frame.  What they need of THIS
        # frame is recorded on the device -- the seeds' positions, the camera, the rendered scene (the fused kernels, now) --
        # and the trajectory overlays of all frames are drawn once the clip is fitted (draw_trajectories): a poly-line's point
        # count is data and the operator path sizes its lists on the host, i.e. two or three full stops of the host per frame
        # here, each with the next frame's set-up behind it (60-frame clip fit: 9.76 -> 9.24 frames/s when drawn per frame).
        tr = self.tr
        with torch.no_grad():
            xyz_now = tr.get_attribute("xyz")[self.traj_index_t].detach().float().clone()
            extr_now = tr.get_extr().detach().clone()
            if tr.engine_current:
                _, scene = self.final_forward(scene=True)            # (its readers behind this one share the forward)
                rgb_u8 = scene[0].clone()
            else:
                rgb_u8 = render_mod.render2img_device(render_mod.render_multiple(tr._input_group(detach=True), ["rgb"])["rgb"])
                tr.rasterisations_done += 1
        self.traj_rec.append((xyz_now, extr_now, rgb_u8))

    def record_tracks(self, i):
        # benchmark.py:98-139 for frame i, on the frame's final state: the uv / depth / depth_map of one forward go to the
        # tracker's two launches; nothing is read back
        tr, keep = self.tr, self.keep
        with torch.no_grad():
            if tr.engine_current:
                aux, _ = self.final_forward()
                n = aux.N
                uv, uv_stride, depth, depth_stride, dm = aux.rec[:n, 0:2], REC, aux.rec[:n, 9], REC, aux.render[3]
            else:
                o = render_mod.render_multiple(tr._input_group(detach=True), ["uv", "depth", "depth_map"])
                uv, depth = o["uv"].float().contiguous(), o["depth"].float().reshape(-1).contiguous()
                dm = o["depth_map"].float().reshape(tr.H, tr.W).contiguous()
                uv_stride, depth_stride = 2, 1
                tr.rasterisations_done += 1
            self.tracker.frame(i, uv, uv_stride, depth, depth_stride, dm)
            if keep is not None and keep.get("record_track_inputs"):
                keep.setdefault("track_inputs", []).append((uv.clone(), depth.clone(), dm.clone()))

    def final_state(self):
        # (rec, n, ids, tile_range) of THIS frame's final state, the fit records and sorted tile lists: the second engine's
        # after final_forward (shared), on the operator path the five operators' outputs, packed -- one more rasterisation
        # for every reader that asks (nothing is kept between them)
        tr = self.tr
        if tr.engine_current:
            aux, _ = self.final_forward()
            return aux.rec, aux.N, aux.ids, aux.tile_range
        state = FL.operator_state(tr._input_group(detach=True))
        tr.rasterisations_done += 1
        return state

    def record_flow(self, i):
        # frame i's final state goes to the flow recorder.  From frame 1 on one gfl_flow_pair for the pair (i - 1, i);
        # nothing is read back
        with torch.no_grad():
            prev = self.frames[i - 1] if i else None
            self.flow_rec.frame(i, *self.final_state(), prev["flow"] if prev else None, prev["move_mask"] if prev else None)

    def record_objects(self, i):
        # frame i's final state goes to the object recorder, as it goes to the flow recorder: the id map of the frame from
        # one gfl_label_frame, ids for the rows that have none; nothing is read back
        with torch.no_grad():
            self.object_rec.frame(i, *self.final_state())

    def record_scores(self, i):
        # benchmark.py:191-230 and :323-329 for frame i, on what the frame's PSNR is taken from and what save_checkpoint
        # stores: two small launches that write one row of the clip's sums, and a clone of the pose; nothing is read back
        tr, keep = self.tr, self.keep
        with torch.no_grad():
            if self.recon_rec is not None:
                self.recon_rec.frame(i, tr.last_render, tr.gt_image)
                if keep is not None and keep.get("record_recon_inputs"):
                    keep.setdefault("recon_inputs", []).append(tr.last_render[:3].clone())
            if self.cam_rec is not None:
                self.cam_rec.frame(i, tr.get_extr())

    def end_of_frame(self, i):
        # what every frame ends with, once its stages are fitted: the recorders that read the frame's final state (which share
        # final_forward's forward), its PSNR, the scores taken where the PSNR is
        tr = self.tr
        self.final = self.final_images = None
        if self.clip_log is not None:
            self.clip_log.frame(self, i)                 # (first: its layer forwards use the second engine before the shared one)
        if self.traj:
            self.record_trajectories()
        if self.tracker is not None:
            self.record_tracks(i)
        if self.flow_rec is not None:
            self.record_flow(i)
        if self.object_rec is not None:
            self.record_objects(i)
        # (PSNR stays on the device and is read ONCE at the end of the clip: a float() per frame drained the queue between
        #  two frames; with a log callback the caller asked for the numbers as they come)
        p = tr.psnr()
        self.psnr_sum = p.double() if self.psnr_sum is None else self.psnr_sum + p.double()
        if self.recon_rec is not None or self.cam_rec is not None:
            self.record_scores(i)
        if self.track_vis:
            self.vis_frames.append(render_mod.render2img_device(tr.last_render[:3]))
        if self.keep is not None:
            self.keep["psnr"].append(p)
        if self.log:
            self.log(f"frame {i}: psnr {float(p):.2f} dB, splats {tr.current_pts_num()}")

    def steps(self):
        """The frame loop: yields after every ``chunk`` iterations of a stage (None: never)"""
        tr, c, frames, common = self.tr, self.cfg, self.frames, self.common
        # first frame (fit_video.py:119-142)
        yield from tr.train_steps(iterations=c["iterations_first"], lr=c["lr"], lr_camera=c["lr_camera"],
                                  lambda_var=c["lambda_var"], densify_interval=c["densify_interval"],
                                  densify_times=c["densify_times"], move_mask=frames[0]["move_mask"],
                                  move_seg=self.traj,   # (the seeds' grid needs the first frame's hull mask: host work, once per clip)
                                  **common)
        if self.traj:
            self.traj_index, self.split_interval = select_traj_seeds(tr, int(c["traj_num"]), int(c["traj_offset"]))
            self.traj_index_t = torch.as_tensor(self.traj_index, device=tr.device).long()
        if self.keep is not None:
            self.keep["trainer"], self.keep["psnr"] = tr, []
        self.end_of_frame(0)
        for i in range(1, len(frames)):
            begin_frame(tr, frames, i, self.load_extr)
            if tr.seg_recorder is not None:
                tr.seg_recorder.frame = i
            if c["camera_first"]:                            # fit_video.py:256-278
                yield from tr.train_steps(**stage_kwargs(c, frames, i, "camera"), **common)
            if c["iterations_after"] > 0:                    # fit_video.py:288-315
                yield from tr.train_steps(**stage_kwargs(c, frames, i, "joint"), **common)
            self.end_of_frame(i)
        if tr.engine is not None:
            tr.engine.check_overflow()

    def draw_trajectories(self):
        tr, keep = self.tr, self.keep
        imgs, uvs = [], []
        with torch.no_grad():
            for xyz_now, extr_now, rgb_u8 in self.traj_rec:
                overlay = tr.eval_trajectories(xyz_now, extr_now, line_scale=0.5, point_scale=2.0, alpha=0.8,
                                               split_interval=self.split_interval)
                img_traj = render_mod.render2img_device(overlay)
                # screen blending as trainer.eval forms it (numpy: float64, truncation)
                upon = 1.0 - (1.0 - rgb_u8.double() / 255.0) * (1.0 - img_traj.double() / 255.0)
                imgs.append(torch.stack([img_traj, (upon * 255.0).to(torch.uint8)]))
                uvs.append(msplat.project_point(xyz_now, tr.intr, extr_now, tr.W, tr.H)[0])       # trainer.project_points
                if keep is not None:
                    keep.setdefault("traj_groups", []).append([x.clone() if isinstance(x, torch.Tensor) else x
                                                               for x in tr.last_traj_group])
        return torch.stack(imgs), torch.stack(uvs)

    def trajectories(self):
        """What the reference appends per frame -- frames_sequence_traj, frames_sequence_traj_upon, sequence_traj
        (fit_video.py:226-238, 335-349): images (frames, 2, H, W, 3) uint8 [trajectories alone, upon the render],
        uv (frames, seeds, 2), index, split_interval.  One copy of every frame's two images and seed projections to the host,
        at the end of the clip (the reference copies five images and the projections per frame, blocking: render2img,
        .cpu().numpy())"""
        imgs_d, uvs_d = self.draw_trajectories()
        if not imgs_d.is_cuda:
            return dict(images=imgs_d.numpy(), uv=uvs_d.numpy(), index=list(self.traj_index), split_interval=self.split_interval)
        block = PINNED.take(imgs_d.numel())
        imgs_h = block[0][:imgs_d.numel()].view(imgs_d.shape)
        imgs_h.copy_(imgs_d, non_blocking=True)
        uvs_h = uvs_d.cpu()                              # (small; waits for the stream, and with it for the images above)
        traj_out = dict(images=PINNED.hand_out(block, [imgs_h])[0], uv=uvs_h.numpy(), index=list(self.traj_index),
                        split_interval=self.split_interval)
        PINNED.release(block)
        return traj_out

    def overlays(self, out):
        """``out["track_vis"]`` from the frames' renders and what ``out`` already holds ("tracks", "traj", "segmentation")"""
        video = torch.stack(self.vis_frames)
        pred = seeds = masks = None
        if self.tracker is not None:
            pred = (out["tracks"]["tracks"], out["tracks"]["occluded"])
        if self.traj:
            # (the hull masks are host work on a few thousand points per frame, as for ``segment``; a frame before any mask
            #  exists has an empty one: nothing is occluded there)
            rec = self.tr.seg_recorder
            masks = out["segmentation"]["masks"] if self.segment else rec.masks(rec.fetch())[0]
            seeds = (out["traj"]["uv"], TV.seed_occlusions(masks, out["traj"]["uv"]), self.split_interval)
        vis = TV.clip_overlays(video, pred, seeds, self.track_vis if isinstance(self.track_vis, dict) else None)
        if self.keep is not None:
            self.keep["track_vis_inputs"] = dict(video=video.cpu().numpy(), masks=masks)
        return vis

    def result(self):
        """The clip's dict, once ``steps()`` has run to its end"""
        tr, keep, frames = self.tr, self.keep, self.frames
        traj_out = self.trajectories() if self.traj else None
        if self.traj and keep is not None:
            keep["traj"] = traj_out
        out = dict(psnr_sum=float(self.psnr_sum), frames=len(frames), iterations=tr.iterations_done,
                   rasterisations=tr.rasterisations_done, clips=1, splats_final=tr.current_pts_num(),
                   # iterations that stepped nothing because a tile outgrew its reserved region, and were made up for
                   void_iterations=tr.engine.regions_outgrown if tr.engine is not None else 0)
        if self.traj:
            out["traj"] = traj_out                        # (not a number: callers that sum the dicts skip it, NUMERIC_KEYS)
        if self.tracker is not None:
            out["tracks"] = self.tracker.result()         # (one copy to the host; not a number either)
        if self.segment:
            # one copy of every frame's (uv, sel) to the host, the hull masks, one launch that scores them all
            rec = tr.seg_recorder
            if keep is not None and keep.get("record_seg_inputs"):
                keep["seg_inputs"] = [None if x is None else (x[0].clone(), x[1].clone()) for x in rec.inputs]
            out["segmentation"] = rec.result([fr["move_mask"] for fr in frames])
        if self.recon_rec is not None:
            out["recon"] = self.recon_rec.result()        # (one copy of the (T, 2) sums)
        if self.cam_rec is not None:
            extr = self.cam_rec.result()                  # (one stacked copy)
            gt = np.stack([torch.as_tensor(_pose_gt(fr)).detach().cpu().double().numpy().reshape(3, 4) for fr in frames])
            out["camera"] = dict(extr=extr, **CM.evaluate(extr, gt))
        if self.flow_rec is not None:
            out["flow"] = self.flow_rec.result()          # (one copy of the (T-1, 3, 6) sums; with "maps" the maps behind it)
        if self.object_rec is not None:
            # one copy of the id maps; the frames that carry an "object_mask" are scored with one launch
            out["propagation"] = self.object_rec.result([fr.get("object_mask") for fr in frames])
        if self.track_vis:
            out["track_vis"] = self.overlays(out)
        if self.clip_log is not None:
            # the hull masks as for ``segment`` (host work, once), then the folder: checkpoints, PNG and AVI files
            rec = tr.seg_recorder
            masks, valid = (out["segmentation"]["masks"], out["segmentation"]["valid"]) if self.segment else rec.masks(rec.fetch())
            out["saved"] = self.clip_log.write(masks, valid, traj_out)
        return out


def fit_clip_steps(frames, device, cfg=None, seed=0, snapshot_interval=0, fused=True, log=None, load_extr=True, chunk=None,
                   async_snapshots=True, keep=None, cu_count=0, deterministic=None, track_queries=None, segment=False,
                   recon=False, camera=False, flow=False, track_backward=False, track_vis=False, propagate=None, save=None):
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
    renders, one more array each (the command line's ``gt``: benchmark.py:165).
    ``propagate``: None, or the object ids of frame 0 -- (H, W) integers, 0 = background, at most 15 -- to propagate through
    the clip (gflow_amd.propagation.ObjectRecorder; INTEGRATION.md, "Object propagation"; a prompt it refuses is a ValueError
    before anything is fitted): every frame ends with one gfl_label_frame on the forward the other recorders read, and the
    dict then has ``"propagation"`` = dict(maps (T, H, W) uint8 -- 255 = unknown --, labels (N,) uint8, rows (T,), n_objects; counts
    (T, K - 1, 6), J, F, JF (T, K - 1), scored (T,), flat), scored against the frames' ``"object_mask"`` (frames 1 .. T - 1
    that carry one).  Off by default; nothing about a fit changes with it off.
    ``save``: None, or a folder that becomes the reference's log folder of this clip (gflow_amd.log_folder.ClipLog;
    INTEGRATION.md, "Saving a fit"; needs ``fused=True``, else ValueError): every frame ends with clones of what
    save_checkpoint stores, the scene's three images from the frame's shared final forward and the four layer images (two
    more forwards), all kept on the device; once the clip is fitted ``ckpt/<name>.tar``, the seven ``images/img*_<name>.png``
    and ``images_seg/move_mask_<name>.png`` per frame (PNG coded on the device, gflow_amd.png) and the ``sequence*.avi``
    files at 5 fps are written, with ``traj_num`` also ``sequence_traj.avi``, ``sequence_traj_upon.avi`` and
    ``sequence_traj.pkl``; ``<name>`` is the frame's ``"name"``, else its five-digit index.  The dict then has ``"saved"``, the
    folder.  Saving reads the fit, it never steps it: the splats, the camera and the PSNR are what they are without it
    (``rasterisations`` counts its forwards)."""
    cf = ClipFit(frames, device, cfg, seed=seed, snapshot_interval=snapshot_interval, fused=fused, log=log, load_extr=load_extr,
                 chunk=chunk, async_snapshots=async_snapshots, keep=keep, cu_count=cu_count, deterministic=deterministic,
                 track_queries=track_queries, segment=segment, recon=recon, camera=camera, flow=flow,
                 track_backward=track_backward, track_vis=track_vis, propagate=propagate, save=save)
    yield from cf.steps()
    return cf.result()


def fit_clip(frames, device, cfg=None, fused=True, deterministic=None, **options):
    """Fit one clip; returns the metrics dict of this clip.  ``options``: fit_clip_steps' (whose docstring names them all),
    without ``chunk`` and ``cu_count``.  On a device the fit runs on a stream of its own, which the current stream waits
    for."""
    if deterministic and not fused:
        raise ValueError("fit_clip(deterministic=True) needs fused=True: the operator path's alpha_blending backward has no "
                         "deterministic implementation")
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


def fit_clips_concurrent(clips, device, cfg=None, seeds=None, chunk=32, partition=False, deterministic=None,
                         track_queries=None, track_backward=False, track_vis=False, propagate=None, save=None, **options):
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
    for all clips, or a list with one entry per clip.  ``propagate``: None, or one prompt (fit_clip_steps' ``propagate``, or
    None) per clip.  ``save``: None, or one folder (fit_clip_steps' ``save``, or None) per clip.  ``options``: fit_clip_steps'
    other ones, for all clips (``async_snapshots`` and ``cu_count`` are set here)."""
    n = len(clips)
    if track_queries is not None and len(track_queries) != n:
        raise ValueError("fit_clips_concurrent: track_queries needs one entry per clip")
    if track_backward and track_queries is None:
        raise ValueError("fit_clips_concurrent(track_backward=True) needs track_queries")
    if propagate is not None and len(propagate) != n:
        raise ValueError("fit_clips_concurrent: propagate needs one entry per clip")
    if save is not None and (isinstance(save, (str, bytes)) or len(save) != n):
        raise ValueError("fit_clips_concurrent: save needs one folder per clip")
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
                           track_vis=track_vis[i] if isinstance(track_vis, (list, tuple)) else track_vis,
                           propagate=None if propagate is None else propagate[i],
                           save=None if save is None else save[i], **options)
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
