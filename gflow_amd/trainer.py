"""Per-frame optimiser -- the counterpart of gflow/trainer.py :: SimpleGaussian.

Same public surface for the hot path (``__init__``, ``load_camera``,
``init_gaussians_from_image``, ``get_attribute``, ``get_extr``, ``add_optimizer``,
``train``, ``project_points``, ``save_checkpoint`` / ``load_checkpoint``,
``densify_by_pixels``) and the same optimisation semantics, including the quirks
SURVEY.md A13 lists (Adam + LinearLR rebuilt on every ``train`` call; densification
replaces the optimiser with a constant-lr Adam over the attributes only).

What is different on purpose (results unchanged):
  * rgb and depth are composited in ONE 4-channel blend instead of two;
  * ``depth_map_color`` / ``center`` are rendered only on the iterations whose
    snapshots are kept (every 10th, trainer.py:573-582), not on all of them;
  * no host synchronisation inside an iteration: loss scalars stay on the device
    (the reference calls .item() on every term for its progress bar), the colour map
    runs on the device, masked losses are evaluated as mask-weighted sums rather than
    boolean gathers;
  * densification samples on the device (torch.multinomial) instead of moving the
    error map to the host for np.random.choice.
Visualisation-only pieces (concave-hull segmentation, PNG/MP4 writers) are out of
scope.
"""
import math
import os
import weakref

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import geometry, msplat
from . import render as render_mod
from .geometry import device_constant, pose_to_extr, rotmat_to_unitquat_xyzw      # (importable from here, as they were)
from .optim import Adam
from .pinned import PINNED
from .companion import SecondEngine, SnapshotShadow
from .sampling import complex_texture_sampling
from .stage import FusedStage, OperatorStage, SnapshotRing, StagePlan


def run_to_end(g):
    """drive the generator ``g`` to its end; what it returns"""
    try:
        while True:
            next(g)
    except StopIteration as e:
        return e.value


class SimpleGaussian:
    def __init__(self, gt_image, gt_depth=None, gt_flow=None, num_points=100000, background="black",
                 device=None, log_dir=None, seed=None, fused=True, deterministic=None):
        """``fused=True`` (default) runs each iteration as one call into the native library
        (gflow_amd/fused.py); ``fused=False`` composes the msplat-compatible autograd operators
        the way the reference does (slower, same results).
        ``deterministic``: bit-identical fits for identical inputs and seed (the library's deterministic mode,
        include/gflow_hip.h: GFL_FIT_DETERMINISTIC, and deterministic CDFs for the initial and the densification draws);
        None follows torch.are_deterministic_algorithms_enabled().  Fused path only."""
        self.fused = bool(fused)
        self.deterministic = L.resolve_deterministic(deterministic)
        if self.deterministic and not self.fused and deterministic is not None:
            raise ValueError("SimpleGaussian(deterministic=True) needs fused=True: the operator path's alpha_blending "
                             "backward has no deterministic implementation")
        self.async_snapshots = True      # snapshots composed on a side stream from a copy of the forward's state (FusedStage._launch)
        self.exact_snapshots = True      # iterations whose forward is looked at are never void or behind (FusedStage.one_iteration)
        self.cu_count = 0                # compute units the stream this trainer is driven on may use (0: the device): FitEngine(cu_count=)
        self.use_graph = True          # replay the fused iteration as a hipGraph when nothing else happens in it
        self.engine = None
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("gflow_amd.trainer needs a HIP device (there is no CPU rasteriser)")
        self.gt_image = gt_image.to(self.device)
        self.gt_depth = gt_depth.to(self.device) if gt_depth is not None else None
        self.gt_flow = gt_flow.to(self.device) if gt_flow is not None else None
        self.num_points = num_points
        H, W, _ = gt_image.shape
        self.H, self.W = H, W
        self.bg = {"black": 0.0, "white": 1.0, "cyan": 0.33}.get(background, 0.0)     # trainer.py:29-36
        fov = math.pi / 2.0
        fx = 0.5 * float(W) / math.tan(0.5 * fov)
        fy = 0.5 * float(H) / math.tan(0.5 * fov)
        self.intr = device_constant([fx, fy, W / 2.0, H / 2.0], self.device)
        self.pose = device_constant([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], self.device)
        self.rng = np.random.default_rng(seed)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(0 if seed is None else int(seed))
        N = int(num_points)
        self._activations = {
            "scale": torch.abs,
            "rotate": F.normalize,
            "opacity": lambda x: torch.sigmoid(x * 10.0),
            "rgb": torch.sigmoid,
        }
        self._activations_inv = {
            "scale": torch.abs,
            "rotate": F.normalize,
            "opacity": lambda x: torch.logit(x) / 10.0,
            "rgb": torch.logit,
        }
        rand = lambda *s: torch.rand(*s, device=self.device, generator=self.gen)
        self._attributes = {
            "xyz": rand(N, 3) * 2 - 1,
            "scale": rand(N, 3),
            "rotate": F.normalize(rand(N, 4)),
            "opacity": self._activations_inv["opacity"](0.99 * torch.ones(N, 1, device=self.device)),
            "rgb": rand(N, 3),
        }
        self.dir = log_dir
        if log_dir is not None:
            os.makedirs(log_dir, exist_ok=True)
        self.move_seg = None
        self.seg_recorder = None          # segmentation.MoveSegRecorder of the clip being fitted (fit_clip(segment=True))
        self.iterations_done = 0          # bookkeeping for throughput reports
        self.rasterisations_done = 0
        # ---- what exists only once something has happened: None until then
        self.lr = self.lr_camera = None                  # of the last add_optimizer / fused stage
        self.train_log = self.last_render = None         # the log entries and the final render of the last train() call
        # frame state, None until the first stage that fits the splats has ended (train_steps: _relabel_after_stage)
        self.still_mask = self.still_mask_tentative = self.last_still_mask = self.last_uv = self.last_depth = None
        self.last_xyz = self.last_num = self.move_seg_erode = self.mask_prompt_pts = self.propagate_seg = None
        # trajectory state, None until the first frame's overlay (eval_trajectories)
        self.traj_xyz = self.traj_scale = self.traj_rotate = self.traj_opacity = self.traj_rgb = self.last_traj_group = None
        self._engine_live = False                        # ``_attributes`` were last set to views of the engine's rows
        # beside ``engine``, for this trainer's lifetime (companion.py, stage.py): the second engine, which renders the current
        # splats; the shadow engine of the asynchronous snapshots; the ring the snapshots of a train() call wait in
        # (the factory reaches this trainer weakly: in a reference cycle a dropped trainer's engines -- their HBM, their graphs --
        #  would wait for the cycle collector, which may run in the middle of the next fit)
        factory = weakref.WeakMethod(self._new_engine)
        new_engine = lambda capacity, K_cap=None: factory()(capacity, K_cap)
        self.second = SecondEngine(new_engine)
        self.shadow = SnapshotShadow(new_engine, self.device)
        self.ring = SnapshotRing(H, W, self.device)

    # ------------------------------------------------------------- predicates
    @property
    def later_frame(self):
        """a stage that fits the splats has ended on this trainer (their colours stay frozen, trainer.py:535-538).  NOT
        ``has_still``: ``load_checkpoint`` restores ``still_mask`` and ``last_uv`` but not ``last_xyz``"""
        return self.last_xyz is not None

    @property
    def has_still(self):
        """the splats have still / moving labels (``still_mask``: from the last joint stage, or from a checkpoint)"""
        return self.still_mask is not None

    @property
    def engine_current(self):
        """the fused engine holds the current splats (row for row what ``_attributes`` hold)"""
        return self.fused and self.engine is not None and self.engine.N == self.current_pts_num()

    @property
    def engine_live(self):
        """``_attributes`` ARE the engine's rows: live views of them, nothing to copy in either direction"""
        return (self.engine_current and self._engine_live
                and self._attributes["xyz"].data_ptr() == self.engine.params.data_ptr())

    def set_gt_image(self, gt_image):
        self.gt_image = gt_image.to(self.device)

    def set_gt_depth(self, gt_depth):
        self.gt_depth = gt_depth.to(self.device)

    def set_gt_flow(self, gt_flow):
        self.gt_flow = gt_flow.to(self.device)

    # ------------------------------------------------------------------ camera
    def get_extr(self):
        return pose_to_extr(self.pose)

    def load_camera(self, focal=None, pp=None, extr=None, scale=None, show=False):
        if focal is not None:
            self.intr[:2].fill_(float(focal))
        if pp is not None:
            self.intr[2:3].fill_(float(pp[0]))
            self.intr[3:4].fill_(float(pp[1]))
        if extr is not None:
            extr = torch.as_tensor(extr, dtype=torch.float32, device=self.device)
            T = extr[:3, 3] * (scale if scale is not None else 1.0)
            pose = self.pose.detach().clone()
            pose[0:4] = rotmat_to_unitquat_xyzw(extr[:3, :3])
            pose[4:7] = T
            self.pose = pose
        if show:
            print("[camera] intr:", self.intr, "\n[camera] extr:\n", self.get_extr())

    # -------------------------------------------------------------- parameters
    def current_pts_num(self):
        return self._attributes["xyz"].shape[0]

    def get_attribute(self, name):
        if name not in self._attributes:
            raise ValueError(f"Attribute or activation for {name} is not VALID!")
        act = self._activations.get(name)
        return act(self._attributes[name]) if act is not None else self._attributes[name]

    def init_gaussians_from_image(self, gt_image, gt_depth=None, num_points=None, mask=None, drop_to=None):
        """trainer.py:206-238."""
        num_points = self.num_points if num_points is None else num_points
        self._engine_live = False                    # the attributes are replaced: no longer views of the engine's rows
        if mask is None and drop_to is None:
            # everything on the device (sampling.complex_texture_sampling_device): no image / depth / sample round trip
            from .sampling import complex_texture_sampling_device
            img = gt_image.to(self.device)
            self.gt_depth = gt_depth.float().to(self.device)
            xys, depths, scales, rgbs = complex_texture_sampling_device(img, self.gt_depth, num_points, generator=self.gen,
                                                                        deterministic=self.deterministic)
            n = xys.shape[0]
            xys, depths = xys.float(), depths.float()
            scales = (scales * (depths / depths.min()).squeeze(1).double()).float()
            rgbs = rgbs.float()
        else:
            xys, depths, scales, rgbs, gt_depth = complex_texture_sampling(
                gt_image, gt_depth.cpu(), num_points=num_points, mask=mask, drop_to=drop_to, rng=self.rng)
            n = xys.shape[0]
            xys = torch.from_numpy(xys).float().to(self.device)
            depths = depths.float().to(self.device)
            self.gt_depth = gt_depth.float().to(self.device)
            scales = torch.from_numpy(scales * (depths / depths.min()).squeeze().cpu().numpy()).float().to(self.device)
            rgbs = torch.from_numpy(rgbs).float().contiguous().to(self.device)
        self._attributes["xyz"] = geometry.pix2world(xys, depths, self.intr, self.get_extr().detach())
        scales = scales.unsqueeze(1).repeat(1, 3)
        self._attributes["scale"] = self._activations_inv["scale"](torch.clamp(scales, max=1e-3))
        rgbs = torch.clamp(rgbs.contiguous(), 1e-15, 1 - 1e-15)
        self._attributes["rgb"] = self._activations_inv["rgb"](rgbs)
        self._attributes["opacity"] = self._activations_inv["opacity"](0.99 * torch.ones(n, 1, device=self.device))
        self._attributes["rotate"] = F.normalize(torch.rand(n, 4, device=self.device, generator=self.gen))

    def add_optimizer(self, lr=1e-2, lr_camera=0.0, depth_invariant=True):
        """trainer.py:123-153: group "attributes" (lr), "extr" = pose (lr_camera), depth_a / depth_b
        (lr).  depth_a and depth_b live in one (2,) tensor here."""
        self.lr, self.lr_camera = lr, lr_camera
        self._engine_live = False
        for k in self._attributes:
            self._attributes[k] = nn.Parameter(self._attributes[k].detach().contiguous()).requires_grad_(True)
        self.pose = nn.Parameter(self.pose.detach().clone()).requires_grad_(True)
        self.depth_ab = nn.Parameter(device_constant([1.0, 0.0], self.device)).requires_grad_(depth_invariant)
        groups = [{"params": list(self._attributes.values()), "lr": lr, "name": "attributes"},
                  {"params": [self.pose], "lr": lr_camera, "name": "extr"}]
        if depth_invariant:
            groups.append({"params": [self.depth_ab], "lr": lr, "name": "depth_ab"})
        self.optimizer = Adam(groups)

    # ------------------------------------------------------------------ render
    def _input_group(self, sel=None, detach=False):
        g = []
        for k in ("xyz", "scale", "rotate", "opacity", "rgb"):
            a = self.get_attribute(k)
            if detach:
                a = a.detach()
            if sel is not None:
                a = a[:sel.shape[0]][sel]
            g.append(a)
        return g + [self.intr, self.get_extr(), self.bg, self.W, self.H]

    def _render_rgbd(self, want_extras):
        """One pass of the rasteriser: uv, depth and the 4-plane render (rgb + depth_map);
        optionally the two snapshot-only images."""
        xyz, scale, rotate, opacity, rgb, intr, extr, bg, W, H = self._input_group()
        uv, depth = msplat.project_point(xyz, intr, extr, W, H)
        visible = depth != 0
        cov3d = msplat.compute_cov3d(scale, rotate, visible)
        conic, radius, tiles = msplat.ewa_project(xyz, cov3d, intr, extr, uv, W, H, visible)
        ids, tile_range = msplat.sort_gaussian(uv, depth, W, H, radius, tiles)
        self.last_K = ids.numel()
        render4 = msplat.alpha_blending(uv, conic, opacity, torch.cat([rgb, depth], dim=1), ids, tile_range, bg, W, H)
        extras = None
        if want_extras:
            with torch.no_grad():
                dc = render_mod.apply_float_colormap(depth.detach(), "turbo", non_zero=True)
                depth_color = msplat.alpha_blending(uv.detach(), conic.detach(), opacity.detach(), dc, ids,
                                                    tile_range, bg, W, H)
                unit = device_constant([1.0, 0.0, 1.0], self.device)
                center = msplat.alpha_blending(uv.detach(), torch.ones_like(conic) * unit,
                                               torch.ones_like(opacity.detach()), rgb.detach(), ids, tile_range, bg,
                                               W, H)
            extras = (depth_color, center)
        self.rasterisations_done += 1
        return uv, depth, render4, extras

    def init_mask_prompt_pts(self, mask_prompt, ckpt_name=None):
        """trainer.py:290-330 (fit_video.py:155-157 calls it once, after the first frame's fit, with the first frame's
        segmentation mask): ``self.mask_prompt_pts`` (N,) bool -- the splats that project inside the image AND onto a set
        pixel of ``mask_prompt`` (H, W).  From then on every joint ``train()`` leaves ``self.propagate_seg``, the hull of
        those splats' current projections (trainer.py:611-619).  With a log directory the prompt is written out as
        images_seg/propagate_mask_<ckpt_name>.png like the reference does."""
        with torch.no_grad():
            uv = render_mod.render_multiple(self._input_group(detach=True), ["uv", "center"])["uv"].detach()
        self.rasterisations_done += 1
        mask_prompt = torch.as_tensor(mask_prompt).to(self.device)
        within = geometry.within(uv, self.W, self.H)
        yx = uv.long()
        under = mask_prompt[yx[:, 1].clamp(0, self.H - 1), yx[:, 0].clamp(0, self.W - 1)].bool()
        self.mask_prompt_pts = within & under
        if self.dir is not None and ckpt_name is not None:
            from PIL import Image
            os.makedirs(os.path.join(self.dir, "images_seg"), exist_ok=True)
            Image.fromarray((mask_prompt.detach().cpu().numpy() * 255).astype(np.uint8)).save(
                os.path.join(self.dir, "images_seg", f"propagate_mask_{ckpt_name}.png"))
        return self.mask_prompt_pts

    # ------------------------------------------------------------------- train
    def make_stepper(self, iterations=500, lr=1e-2, lr_camera=0.0, lambda_rgb=1.0, lambda_depth=0.0,
                     lambda_flow=0.0, lambda_var=0.0, lambda_still=0.0, lambda_scale=0.0, move_mask=None,
                     densify_interval=500, densify_times=1, mask=None, camera_only=False, densify_occ_percent=0.1,
                     densify_err_thre=1e-2, densify_err_percent=0.2, snapshot_interval=10, log_interval=0,
                     mask_count=None):
        """Set up one ``train`` call (pre-update, fresh Adam + LinearLR, trainer.py:347-384) and
        return a callable that runs ONE iteration of trainer.py:387-582 per call (gflow_amd/stage.py)."""
        if move_mask is not None:
            move_mask = move_mask.to(self.device).bool()
        if not camera_only and self.has_still:
            self._warp_moving()
        plan = StagePlan(iterations=iterations, lr=lr, lr_camera=lr_camera, lambda_rgb=lambda_rgb, lambda_depth=lambda_depth,
                         lambda_flow=lambda_flow, lambda_var=lambda_var, lambda_still=lambda_still, lambda_scale=lambda_scale,
                         move_mask=move_mask, densify_interval=densify_interval, densify_times=densify_times, mask=mask,
                         camera_only=camera_only, densify_occ_percent=densify_occ_percent, densify_err_thre=densify_err_thre,
                         densify_err_percent=densify_err_percent, snapshot_interval=snapshot_interval,
                         log_interval=log_interval, mask_count=mask_count,
                         occlusion=not camera_only and self.later_frame and mask is not None)
        return (FusedStage if self.fused else OperatorStage)(self, plan)

    def _warp_moving(self):
        """pre-update: carry moving splats along the GT flow (trainer.py:348-376)"""
        W, H = self.W, self.H
        n_last = self.last_still_mask.shape[0]
        moving = ~self.last_still_mask
        uv_last = self.last_uv[:n_last]
        inside = geometry.within(uv_last, W, H) & moving
        yx = uv_last.long()
        flow_at = self.gt_flow[yx[:, 1].clamp(0, H - 1), yx[:, 0].clamp(0, W - 1)]
        uv_new = uv_last + flow_at
        yn = uv_new[:, 1].long().clamp(0, H - 1)
        xn = uv_new[:, 0].long().clamp(0, W - 1)
        depth_new = self.gt_depth[yn, xn]
        xyz_new = geometry.pix2world(uv_new, depth_new.reshape(-1, 1), self.intr, self.get_extr().detach())
        xyz = self._attributes["xyz"].detach().clone()
        xyz[:n_last] = torch.where(inside.unsqueeze(1), xyz_new, xyz[:n_last])
        self._attributes["xyz"] = xyz

    # ---- which rows the regularisers of a stage act on: ONE selection for both paths (the arithmetic stays theirs: the
    # ---- operator path divides a masked sum by a count, the fused path hands the library pre-divided weights)
    def _stage_rows(self, inside, camera_only):
        """``inside`` (N,) narrowed to the labelled rows this stage fits: still if camera-only, else moving (trainer.py:467-471)"""
        if not self.has_still:
            return inside
        n = self.still_mask.shape[0]
        out = inside.clone()
        out[:n] = (self.still_mask if camera_only else ~self.still_mask) & out[:n]
        return out

    def _still_selection(self, lambda_still):
        """(last_still_mask, the positions those rows are held at), or None without a still term"""
        if not (lambda_still and self.has_still):
            return None
        m = self.last_still_mask
        return m, self.last_xyz[:m.shape[0]]

    def _flow_selection(self, lambda_flow, camera_only):
        """(the rows of ``last_uv`` the flow term counts, the ground-truth flow at ``last_uv``), or None without a flow term"""
        if not (lambda_flow and self.gt_flow is not None and self.last_uv is not None):
            return None
        W, H = self.W, self.H
        and_mask = self._stage_rows(geometry.within(self.last_uv, W, H), camera_only)
        yx = self.last_uv.long()
        return and_mask, self.gt_flow[yx[:, 1].clamp(0, H - 1), yx[:, 0].clamp(0, W - 1)]

    # ------------------------------------------------------- fused (native) path
    def _new_engine(self, capacity, K_cap=None):
        from .fused import FitEngine
        return FitEngine(self.W, self.H, capacity, self.device, K_cap=K_cap, bg=self.bg, cu_count=self.cu_count,
                         deterministic=self.deterministic)

    def _engine_for(self, n):
        if self.engine is None:
            self.engine = self._new_engine(max(8 * int(self.num_points), 2 * n, 65536))
        self.engine.ensure_capacity(n)
        return self.engine

    def _pack_to_engine(self):
        """Copy the attribute tensors into the engine's packed rows and re-point
        ``_attributes`` at live views of them."""
        eng = self._engine_for(self.current_pts_num())
        if not self.engine_live:
            eng.set_splats(self._attributes)         # (already live views of the engine's rows: nothing to copy)
        self._attributes = eng.views()
        self._engine_live = True
        return eng

    def train(self, *a, **kw):
        """``train_steps`` run to the end (the generator exists so that several fits can take turns on one device,
        fit_video.fit_clips_concurrent); same arguments, returns what it returns."""
        return run_to_end(self.train_steps(*a, **kw))

    def train_steps(self, iterations=500, save_ckpt=False, ckpt_name="ckpt", snapshot_interval=10, render_parts=True,
                    lazy_images=False, chunk=None, move_seg=False, **kw):
        """A generator: yields after every ``chunk`` iterations (None: never), returns train()'s tuple.
        One call = the optimisation of one frame (trainer.py:332-711); keyword arguments
        as ``make_stepper``.  Returns (frames, frames_center, frames_depth, still_rgb,
        still_center, move_rgb, move_center, move_seg) like the reference; the frame lists
        hold (H,W,3) uint8 snapshots taken every ``snapshot_interval`` iterations (0 = none).
        ``move_seg``: also build ``self.move_seg`` / ``self.move_seg_erode`` (trainer.py:604-609; off by default, see below).
        ``render_parts``: the four images of the still / moving splats the reference renders at the end of EVERY train()
        (trainer.py:632-677); False skips them (None in the tuple).  ``lazy_images``: return without waiting for the
        images -- they are views of page-locked memory that the device fills behind the queued work; read them after
        ``torch.cuda.synchronize()``.  (A caller that drops them, like fit_clip, saves one full stop of the host per call.)"""
        st = self.make_stepper(iterations=iterations, snapshot_interval=snapshot_interval, **kw)
        if chunk:
            # (several fits taking turns on one device from ONE host thread: a fit that would have to WAIT for its look at the
            #  overflow words hands the turn on instead -- run() returns early -- so that the others' queues do not run dry)
            st.yielding = True
            while st.iteration < iterations:
                st.run(min(int(chunk), iterations - st.iteration))
                yield
        else:
            st.run(iterations)
        self.train_log = st.log
        # (``fused and engine is not None`` here and in _project_appended, not ``engine_current``: the question is which path
        #  has just run the stage -- the engine's row count is the truth then, and nothing is compared with it)
        if self.fused and self.engine is not None:
            # Dropped (splat, tile) pairs must neither go unnoticed nor end the fit: the lists are grown and the iterations
            # that stepped nothing are run again (FitEngine.settle_overflow).  One read of two words per train() call.
            # (Round 6 measured what this full stop costs: the pause between two stages is 1.4-1.5 ms of DEVICE time with it and
            #  1.2 ms without -- an "exact tail" of 24 iterations behind a watch, the words read from that copy --, because the
            #  boundary's ~70 small torch kernels are a chain of launch latencies on the device whoever waits for whom; the tail's
            #  exact binning cost the 0.25 ms back.  tools/stage_times.py, tools/experiments/README.md.)
            st.settle()
            st.sink.watch_overflow()
        move_mask = kw.get("move_mask")
        if move_mask is not None:
            move_mask = move_mask.to(self.device).bool()

        # ---- post-update (trainer.py:588-625)
        self._project_appended(st)
        uv_d, depth_d = st.uv.clone(), st.depth.clone()
        if not st.camera_only:
            self._relabel_after_stage(uv_d, depth_d, move_mask, move_seg)
        parts, parts_block = (None, None, None, None), None
        if self.has_still and render_parts:
            parts, parts_block = self._render_parts(st.sink)
            self.rasterisations_done += 2
        self.last_render = st.last_render.clone()
        if save_ckpt:
            self.save_checkpoint(ckpt_name=ckpt_name)
        st.sink.flush(lazy_images)
        if parts_block is not None:
            parts = PINNED.hand_out(parts_block, [parts[0, 0], parts[0, 2], parts[1, 0], parts[1, 2]])
            PINNED.release(parts_block)
        frames, frames_depth, frames_center = st.sink.images()
        return (frames, frames_center, frames_depth, *parts, self.move_seg)

    def _project_appended(self, st):
        # splats were appended after the last render (densification on the final iteration; the
        # reference would fail on the shape mismatch at trainer.py:596): project them once more
        if st.uv.shape[0] == self.current_pts_num():
            return
        with torch.no_grad():
            if self.fused and self.engine is not None:
                self.engine.forward()
                st.uv, st.depth, st.last_render = self.engine.uv, self.engine.depth, self.engine.render
            else:
                st.uv, st.depth, st.last_render, _ = self._render_rgbd(want_extras=False)
            self.rasterisations_done += 1

    def _relabel_after_stage(self, uv_d, depth_d, move_mask, move_seg):
        """trainer.py:590-625: still / moving labels from where the splats project now, hull masks, the ``last_*`` state"""
        W, H, dev = self.W, self.H, self.device
        within = geometry.within(uv_d, W, H)
        yx = uv_d.long()
        labels = ~move_mask[yx[:, 1].clamp(0, H - 1), yx[:, 0].clamp(0, W - 1)]
        n_now = self.current_pts_num()
        still = torch.ones(n_now, dtype=torch.bool, device=dev)
        still[:uv_d.shape[0]] = torch.where(within, labels, still[:uv_d.shape[0]])
        self.still_mask = still
        self.still_mask_tentative = still.clone()
        if self.last_still_mask is not None:
            self.still_mask[:self.last_still_mask.shape[0]] = self.last_still_mask
        if move_seg:
            # trainer.py:604-609: the moving region as the smoothed concave hull of the moving splats' projections
            # (gflow_amd/hull.py).  Host work on a few thousand points -- the reference does it after every joint
            # train(); here only on request, because it reads uv back and stops the host (visualisation and
            # trajectory seeds use it, the optimisation does not).
            from .hull import FastConcaveHull2D
            from scipy.ndimage import minimum_filter
            sel = within & ~self.still_mask[:uv_d.shape[0]]
            pts = uv_d[sel].cpu().numpy()
            if pts.shape[0] > 5:
                self.move_seg = (FastConcaveHull2D(pts).mask(W, H) * 255).astype(np.uint8)
                # cv2.erode(move_seg, ones((20, 20))): minimum over x-10 .. x+9, nothing eroded from the border
                self.move_seg_erode = minimum_filter(self.move_seg, size=20, mode="constant", cval=255)
        if self.seg_recorder is not None:
            # the same two tensors, kept for the end of the clip: the masks of every frame are built then, from one copy
            self.seg_recorder.record(uv_d, within & ~self.still_mask[:uv_d.shape[0]])
        if self.mask_prompt_pts is not None:
            # trainer.py:611-619: the first frame's mask prompt, carried by the splats that lay under it: the smoothed
            # concave hull of where THOSE splats project now (the reference builds it after every joint train() once
            # init_mask_prompt_pts has been called; host work, like move_seg)
            from .hull import FastConcaveHull2D
            m = self.mask_prompt_pts
            p_uv = uv_d[:m.shape[0]][m]
            p_uv = p_uv[geometry.within(p_uv, W, H)]
            if p_uv.shape[0] > 4:
                self.propagate_seg = (FastConcaveHull2D(p_uv.cpu().numpy()).mask(W, H) * 255).astype(np.uint8)
        self.last_still_mask = self.still_mask.detach()
        self.last_uv = uv_d
        self.last_depth = depth_d
        self.last_xyz = self.get_attribute("xyz").detach()
        self.last_num = self.last_xyz.shape[0]

    def _render_parts(self, sink):
        """trainer.py:632-677: ((still_rgb, still_center, move_rgb, move_center), None), or -- through the fused kernels --
        (the (2, 3, H, W, 3) page-locked array the device is filling, its block: handed out once the sink is flushed)"""
        # (``engine.N == still_mask.shape[0]``, not ``engine_current``: SecondEngine.parts_u8 hides a row by its label, so every
        #  row of the engine needs one -- after a camera-only stage on a checkpoint's labels, say, they may be fewer)
        if self.fused and self.engine is not None and self.engine.N == self.still_mask.shape[0]:
            # both renders through the fused kernels on a second engine, the images converted on the device and on
            # their way to page-locked memory without stopping the host (four operator-path renders and four
            # blocking copies took ~3 ms per train() call: 4 % of a clip fit)
            block, pin = sink.copy_out(self.second.parts_u8(self.engine, self.bg, self.still_mask))
            return pin, block
        with torch.no_grad():
            o = render_mod.render_multiple(self._input_group(sel=self.still_mask, detach=True), ["rgb", "center"])
            still_rgb, still_center = render_mod.render2img(o["rgb"]), render_mod.render2img(o["center"])
            o = render_mod.render_multiple(self._input_group(sel=~self.still_mask, detach=True), ["rgb", "center"])
            move_rgb, move_center = render_mod.render2img(o["rgb"]), render_mod.render2img(o["center"])
        return (still_rgb, still_center, move_rgb, move_center), None

    # ------------------------------------------------------------ densification
    def densify_weights(self, error_map, error_threshold=1e-3, mask=None):
        """The sampling weights of trainer.py:880-897 on the device: (masked error map with the uniform floor, the
        boolean mask).  Nothing here reads back."""
        dev = self.device
        err = error_map.detach().float()
        inf = torch.full_like(err, float("inf"))
        pos_min = torch.where(err > 0, err, inf).min()
        # (no positive entry at all: np.nanmin of an empty selection -- the reference fails there; sample the mask
        # uniformly instead)
        err = err + torch.where(torch.isinf(pos_min), torch.ones_like(pos_min), pos_min)      # uniform floor (:884)
        if mask is None:
            m = err > error_threshold
        else:
            m = mask.detach().to(dev).squeeze()
            if m.dim() == 3:
                m = m[..., 0] if m.shape[-1] in (1, 3) else m[0]
            m = m > 0
        m = m[:, :err.shape[1]]
        return err * m, m

    def new_splats_at(self, ys, xs):
        """Raw attributes of the splats densification creates at the pixels (ys, xs) (trainer.py:910-934): at the
        ground-truth depth, isotropic scale depth / min(sampled depths) / num_points, the pixel's colour, identity
        rotation, opacity 0.99."""
        dev = self.device
        k = ys.shape[0]
        xys = torch.stack([xs, ys], dim=1).float()
        depths = self.gt_depth[ys, xs].reshape(-1, 1).float()
        scales = (depths / depths.min()).squeeze(1) * (1.0 / self.num_points)
        new_xyz = geometry.pix2world(xys, depths, self.intr, self.get_extr().detach())
        new_scale = torch.abs(scales.unsqueeze(1).repeat(1, 3))
        new_rgb = torch.logit(torch.clamp(self.gt_image[ys, xs].contiguous(), 1e-15, 1 - 1e-15))
        new_rot = torch.zeros(k, 4, device=dev)
        new_rot[:, 0] = 1.0
        new_op = torch.logit(0.99 * torch.ones(k, 1, device=dev)) / 10.0
        return new_xyz, new_scale, new_rot, new_op, new_rgb

    def densify_by_pixels(self, error_map, error_threshold=1e-3, percent=0.1, mask=None, n_masked=None):
        """trainer.py:878-939 on the device.  ONE host read per call -- the number of masked pixels, which fixes how
        many rows are appended (launch sizes and tensor shapes live on the host); the reference moves the whole error
        map to the host and samples with numpy.  ``n_masked``: that number, when the caller knows it already (the
        occlusion mask is an INPUT of the frame: fit_video counts it once when the clip is uploaded) -- no read at all."""
        W = self.W
        if n_masked == 0:
            return self.current_pts_num(), self.current_pts_num()
        err, m = self.densify_weights(error_map, error_threshold, mask)
        if n_masked is None:
            n_masked = int(m.sum())                                        # the host read
            if self.fused and self.engine is not None:          # (whatever rows it holds: its graphs are meant)
                self.engine.reap_graphs()            # (the device is idle right now: the one place per frame where retired graphs cost nothing to destroy)
        densify_num = int(self.num_points * (n_masked / m.numel()) * percent)     # float64 like numpy (:896-901)
        num_before = self.current_pts_num()
        if densify_num > 0:
            idx = self.sample_pixels(err, densify_num)
            self.last_densify_idx = idx
            self.densification_postfix(*self.new_splats_at(idx // W, idx % W))
        return num_before, self.current_pts_num()

    def sample_pixels(self, weights, count):
        """``count`` independent draws (with replacement) of flat pixel indices with probability weights / sum --
        np.random.choice(H*W, size, p) of trainer.py:905 -- by inverse-CDF lookup on the device (torch.multinomial
        over 4e5 categories took ~25 ms).  The deterministic mode forms the CDF with the library's scan."""
        from .sampling import cdf_device
        cdf = cdf_device(weights, self.deterministic)
        u = torch.rand(count, generator=self.gen, device=self.device, dtype=torch.float64) * cdf[-1]
        return torch.searchsorted(cdf, u, right=True).clamp_(max=cdf.numel() - 1)

    def densification_postfix(self, new_xyz, new_scale, new_rotate, new_opacity, new_rgb):
        """trainer.py:941-951 -- including the quirk that the new optimiser covers only the attributes, with a
        constant lr and fresh moments (the fused stepper turns that into flags, stage.py: FusedStage.one_iteration).  On the fused path
        the rows are appended IN PLACE behind the engine's live rows (capacity-based buffers: no concatenation, no
        re-packing, the parameter views are simply re-cut)."""
        new = {"xyz": new_xyz, "scale": new_scale, "rotate": new_rotate, "opacity": new_opacity, "rgb": new_rgb}
        eng = self.engine
        if self.engine_live:
            from .fused import COLS
            n0, k = eng.N, new_xyz.shape[0]
            eng.ensure_capacity(n0 + k)
            rows = eng.params[n0:n0 + k]
            for name, (a, b) in COLS.items():
                rows[:, a:b] = new[name].detach().reshape(k, b - a)
            rows[:, 14:] = 0
            eng.set_count(n0 + k)
            self._attributes = eng.views()
            return
        for k in self._attributes:
            cat = torch.cat((self._attributes[k].detach(), new[k]), dim=0).contiguous()
            self._attributes[k] = nn.Parameter(cat).requires_grad_(True)
        self.optimizer = Adam(list(self._attributes.values()), lr=self.lr)

    # -------------------------------------------------------------- checkpoint
    def save_checkpoint(self, ckpt_name=None):
        """Same dict keys as trainer.py:252-272."""
        if self.dir is None:
            raise RuntimeError("save_checkpoint: this trainer was built without log_dir")
        ckpt = {
            # contiguous clones: on the fused path the attributes are column views of the engine's
            # [capacity][16] buffer, and torch.save would serialise the whole storage
            "attributes": {k: v.detach().clone().contiguous() for k, v in self._attributes.items()},
            "intr": self.intr,
            "extr": self.get_extr().detach().clone(),
            "still_mask": self.still_mask,
            "move_seg": self.move_seg,
            "last_uv": self.last_uv,
            "width": self.W,
            "height": self.H,
        }
        os.makedirs(os.path.join(self.dir, "ckpt"), exist_ok=True)
        self.checkpoint_path = os.path.join(self.dir, "ckpt", f"{ckpt_name or 'ckpt'}.tar")
        torch.save(ckpt, self.checkpoint_path)

    def load_checkpoint(self, checkpoint_path):
        ckpt = torch.load(checkpoint_path, map_location=self.device, weights_only=False)
        self._engine_live = False                    # the attributes are replaced: no longer views of the engine's rows
        self._attributes = {k: v.to(self.device) for k, v in ckpt["attributes"].items()}
        self.intr = ckpt["intr"].to(self.device)
        self.load_camera(extr=ckpt["extr"])
        for k in ("still_mask", "move_seg", "last_uv"):
            if ckpt.get(k) is not None:
                setattr(self, k, ckpt[k])

    # -------------------------------------------------------- trajectory render
    def eval(self, traj_index=None, line_scale=0.1, point_scale=0.3, alpha=0.5, split_interval=None):
        """trainer.py:713-811: render the current splats (rgb, center, depth_map_color) and the trajectories of the
        splats ``traj_index`` (poly-lines from their previous to their current positions, older segments fading by
        ``alpha`` per frame), plus the screen blend of both.  Returns five (H,W,3) uint8 images:
        (rgb, center, depth_colour, trajectories, rgb with the trajectories on top)."""
        traj_index = torch.as_tensor(traj_index, device=self.device).long()
        current_xyz = self.get_attribute("xyz")[traj_index].detach().float()
        with torch.no_grad():
            out_traj = self.eval_trajectories(current_xyz, self.get_extr().detach(), line_scale, point_scale, alpha, split_interval)
            out = render_mod.render_multiple(self._input_group(detach=True), ["rgb", "center", "depth_map_color"])
            self.rasterisations_done += 1
        out_img = render_mod.render2img(out["rgb"])
        out_img_center = render_mod.render2img(out["center"])
        out_img_depth = render_mod.render2img(out["depth_map_color"])
        out_img_traj = render_mod.render2img(out_traj)
        # screen blending
        result = 1 - (1 - np.array(out_img) / 255.0) * (1 - np.array(out_img_traj) / 255.0)
        return out_img, out_img_center, out_img_depth, out_img_traj, (result * 255).astype(np.uint8)

    def eval_trajectories(self, current_xyz, extr, line_scale=0.1, point_scale=0.3, alpha=0.5, split_interval=None):
        """The trajectory half of ``eval`` (trainer.py:716-762, 779-794) as a function of what it needs of a frame: where the
        tracked splats are (``current_xyz`` (n, 3)) and the frame's camera (``extr`` (3, 4)).  Advances the trajectory state
        (all poly-line points so far, their fading opacities and colours) by one frame and returns the overlay (3, H, W) float.
        fit_video.fit_clip records the two inputs after every frame and calls this for all frames once the clip is fitted:
        the poly-lines' point counts are data (a read-back per frame) and the operator path sizes its lists on the host."""
        from .color import apply_float_colormap
        from .trajectory import gen_line_set
        dev = self.device
        num_traj = current_xyz.shape[0]
        op_inv = self._activations_inv["opacity"]
        if self.traj_xyz is None:                                       # the first frame
            self.traj_xyz = current_xyz
            self.traj_scale = torch.ones((num_traj, 3), device=dev)
            self.traj_rotate = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(num_traj, 1)
            self.traj_opacity = op_inv(0.99 * torch.ones((num_traj, 1), device=dev))
            if split_interval is None or num_traj == split_interval:
                traj_rgb = torch.arange(0, 1, 1 / num_traj, device=dev).float().unsqueeze(1)
            else:
                still = torch.arange(0, 1, 1 / split_interval, device=dev).float().unsqueeze(1)
                move = torch.arange(0, 1, 1 / (num_traj - split_interval), device=dev).float().unsqueeze(1)
                traj_rgb = torch.cat([still, move], dim=0)
            traj_rgb = apply_float_colormap(traj_rgb, colormap="gist_rainbow")
            # The reference keeps logit(colour) and hands it to the rasteriser RAW (:735, :784-790): table entries that
            # are exactly 0 or 1 become -inf / +inf, i.e. "saturate wherever the blob has any weight".  A branch-free
            # compositor multiplies skipped splats by weight 0, and 0 * inf is NaN: keep the saturation, finite.
            self.traj_rgb = torch.nan_to_num(self._activations_inv["rgb"](traj_rgb), posinf=1e6, neginf=-1e6)
            self.last_traj_xyz = self.traj_xyz
            self.last_traj_rgb = self.traj_rgb
        else:                                                              # the following frames
            line_xyz, line_rgb = gen_line_set(self.last_traj_xyz, current_xyz, self.last_traj_rgb, device=dev)
            num_in_line = line_xyz.shape[0]
            self.traj_xyz = torch.cat([self.traj_xyz, line_xyz], dim=0)
            num_total = self.traj_xyz.shape[0]
            self.traj_scale = torch.ones((num_total, 3), device=dev) * 1e-6
            self.traj_rotate = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(num_total, 1)
            self.traj_opacity = torch.cat([self.traj_opacity * alpha,       # gradually fade out (raw values, :761)
                                           op_inv(0.99 * torch.ones((num_in_line, 1), device=dev))], dim=0)
            self.traj_rgb = torch.cat([self.traj_rgb, line_rgb], dim=0)
            self.last_traj_xyz = current_xyz
        # (the reference hands the RAW trajectory opacity / colour to the rasteriser, :784-790)
        traj_group = [self.traj_xyz, self.traj_scale, self.traj_rotate, self.traj_opacity, self.traj_rgb, self.intr, extr,
                      self.bg, self.W, self.H]
        self.last_traj_group = traj_group
        self.rasterisations_done += 1
        return render_mod.render_traj(traj_group, num_traj, line_scale, point_scale)

    def project_points(self, points):
        return msplat.project_point(points, self.intr, self.get_extr(), self.W, self.H)

    def psnr(self):
        return self.psnr_of(self.last_render)

    def psnr_of(self, render4):
        """PSNR of a rendered frame against the ground truth, on what the reference evaluates (benchmark.py:191-230): the
        SAVED image -- render2img's clamp, x 255, truncation to uint8 (render.py:158-166) -- read back as uint8 / 255."""
        img = torch.floor(torch.clamp(render4[:3].permute(1, 2, 0), 0.0, 1.0) * 255.0) / 255.0
        mse = ((img - self.gt_image) ** 2).mean()
        return -10.0 * torch.log10(mse)
