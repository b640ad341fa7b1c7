"""One ``train`` call of the per-frame optimiser (SimpleGaussian.make_stepper): what happens at which iteration (StagePlan),
where the snapshots go (RingSink on a SnapshotRing / ListSink), the iteration loop on the fused and on the operator path."""
from types import SimpleNamespace

import torch

from . import geometry, losses
from . import render as render_mod
from .optim import LinearLR
from .pinned import PINNED, copy_stream


class StagePlan(SimpleNamespace):
    """``make_stepper``'s arguments (and ``occlusion``: a later frame's joint stage that was given an occlusion mask), and
    what they make happen in iteration i besides the iteration itself (trainer.py:560-582).  Rules on the index, not a
    table: a stepper may be driven past ``iterations`` (bench.py does; the snapshot sink grows then)."""

    def snapshot(self, i):
        return bool(self.snapshot_interval) and i % self.snapshot_interval == 0

    def log(self, i):
        return bool(self.log_interval) and i % self.log_interval == 0

    def occ_densify(self, i):
        """splats are added under the occlusion mask, behind iteration i's update (trainer.py:562-565)"""
        return bool(self.occlusion) and i == 0

    def err_densify(self, i):
        """splats are added where iteration i's error map is large, behind its update (trainer.py:566-571)"""
        return bool(not self.camera_only and self.densify_interval and (i + 1) % self.densify_interval == 0
                    and (i + 1) // self.densify_interval <= self.densify_times)

    def plain(self, i):
        """nothing but the library's iteration happens in iteration i (no snapshot, log entry or densification)"""
        return not (self.snapshot(i) or self.log(i) or self.occ_densify(i) or self.err_densify(i))


class ListSink:
    """The operator path's snapshots: lists (rgb, depth colour, centre) of uint8 device images, copied at the end."""
    copy_stream = None

    def __init__(self):
        self.lists = ([], [], [])

    def put(self, *images):
        for lst, img in zip(self.lists, images):
            lst.append(img)

    def flush(self, lazy=False):
        pass

    def images(self):
        """[frames, depths, centers]: lists of (H, W, 3) uint8 host arrays"""
        return [[f for f in torch.stack(lst).cpu().numpy()] if lst else [] for lst in self.lists]


class SnapshotRing:
    """(rows, 3, H, W, 3) uint8 on the device: where a train() call keeps its snapshots until its end (RingSink).  One ring per
    trainer, reused by its train() calls and grown on demand; ``done``: the event of the copy that emptied it last."""

    def __init__(self, H, W, dev):
        self.H, self.W, self.dev = H, W, dev
        self.buf = self.done = None

    def rows(self, n):
        """the first ``n`` rows; the current stream waits for the copy that emptied the ring last (``copied``)"""
        if self.buf is None or self.buf.shape[0] < n:
            self.buf = torch.empty(int(n), 3, self.H, self.W, 3, dtype=torch.uint8, device=self.dev)
        if self.done is not None:
            torch.cuda.current_stream().wait_event(self.done)
        return self.buf[:n]

    def copied(self):
        """call on the stream that has just been given the ring's device-to-host copy"""
        self.done = torch.cuda.Event()
        self.done.record()


class RingSink(ListSink):
    """The fused path's snapshots: the lists hold views of a page-locked block, one per snapshot taken."""
    # They stay on the DEVICE until the end of this train() call (a ring of uint8 images in HBM: 3.7 MB each at
    # 480p, 50 per call) and leave for page-locked memory in ONE copy then.  A copy to the host while the
    # iterations run holds up whatever kernel is running beside it for as long as it lasts -- 65 us, every
    # tenth iteration (tools/snapshot_timeline.sh, tools/d2h_probe.py: a chain of short kernels gets +57 us
    # per 74 us copy); at the end of the call it runs beside the host's set-up of the next stage, when the
    # device has little else to do.  (The reference blocks on three device-to-host copies right here.)

    def __init__(self, store, shadow, plan, H, W, dev):
        """``store``: the trainer's SnapshotRing; ``shadow``: its companion.SnapshotShadow, or None where the snapshots are
        taken inside the iteration's own launch"""
        super().__init__()
        self.store, self.shadow, self.plan, self.H, self.W, self.dev = store, shadow, plan, H, W, dev
        self.pin = self.pin_block = self.pin_hold = self.ring = None
        self.copy_stream = None          # the stream of the copies to the host, once there is one to wait for
        self.composed = False            # the shadow engine has written into the ring, on its side stream, in this call

    def slot(self, k):
        """(3, H, W, 3) uint8 on the device: where the three images of snapshot ``k`` (the next one) are to be written"""
        if self.pin is None or k >= self.pin.shape[0]:
            self._grow(k)
        self.put(*self.pin[k])
        return self.ring[k]

    def compose(self, main, dst, n):
        """the images of the forward ``main`` has just run (``n`` rows) into ``dst`` (this snapshot's ``slot``), beside what
        the current stream does next (companion.SnapshotShadow.compose)"""
        self.shadow.compose(main, dst, n)
        self.composed = True

    def watch_overflow(self):
        """the end of the call: the shadow engine's overflow watch behind its snapshots, if it took any in this call"""
        if self.composed:
            self.shadow.watch_overflow()

    def _grow(self, k):
        H, W, p = self.H, self.W, self.plan
        # (k >= rows: a stepper that is run for more than ``iterations`` steps gets larger blocks)
        n_snaps = max((p.iterations + p.snapshot_interval - 1) // p.snapshot_interval, 2 * k, 1)
        block = PINNED.take(n_snaps * 3 * H * W * 3)
        pin = block[0][:n_snaps * 3 * H * W * 3].view(n_snaps, 3, H, W, 3)
        hold = PINNED.hold(block, self)                      # ... while this sink (its stepper) lives
        PINNED.release(block)
        ring = self.store.rows(n_snaps)                      # (waits, on the stream, for the last call's copy)
        if self.pin is not None:
            if self.composed:
                torch.cuda.current_stream().wait_stream(self.shadow.stream)     # (the shadow engine writes the old ring)
            ring[:k].copy_(self.ring[:k])
            self.lists = tuple([pin[j, c] for j in range(k)] for c in range(3))
            self.pin_hold()
        self.pin_block, self.pin, self.pin_hold, self.ring = block, pin, hold, ring
        self.copy_stream = copy_stream(self.dev)

    def copy_out(self, t):
        """``t`` (on the device) leaves for a page-locked block of its own behind the current stream's work: (block, view)"""
        block = PINNED.take(t.numel())
        pin = block[0][:t.numel()].view(t.shape)
        cs = copy_stream(self.dev)
        cs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cs):
            pin.copy_(t, non_blocking=True)
        PINNED.copied(block, cs)
        t.record_stream(cs)
        if self.copy_stream is None:
            self.copy_stream = cs
        return block, pin

    def flush(self, lazy=False):
        # the snapshots stayed on the device as uint8 images: ONE copy to the host here, not three
        # blocking copies every 10th iteration (trainer.py:573-582)
        k = len(self.lists[0])
        if self.pin is not None and k:
            self.copy_stream.wait_stream(torch.cuda.current_stream())
            if self.composed:
                self.copy_stream.wait_stream(self.shadow.stream)     # (the shadow engine's last images)
            with torch.cuda.stream(self.copy_stream):
                self.pin[:k].copy_(self.ring[:k], non_blocking=True)
                self.store.copied()                                  # (an event: the ring is free again after it)
            PINNED.copied(self.pin_block, self.copy_stream)
            self.ring.record_stream(self.copy_stream)                # (should the store replace it by a larger one)
        if self.copy_stream is not None and not lazy:
            self.copy_stream.synchronize()           # fused path: the images are already in pinned host memory

    def images(self):
        out = [PINNED.hand_out(self.pin_block, lst) if lst else [] for lst in self.lists]
        if self.pin_hold is not None:
            self.lists, self.pin = ([], [], []), None
            self.pin_hold()                          # (do not wait for the stepper to be collected)
        return out


class _Stage:
    """State of one ``train`` call; calling it runs one iteration, ``run(n)`` the next n."""

    def __init__(self, tr, p, sink):
        self.tr, self.plan, self.sink = tr, p, sink
        self.log = []
        self.iteration = 0
        self.move_mask, self.camera_only = p.move_mask, p.camera_only
        self.uv = self.depth = self.last_render = None       # of the last forward
        self.yielding = False            # run() returns early rather than wait for a look (train_steps with ``chunk``)

    @property
    def frames(self):
        return self.sink.lists[0]

    def __call__(self):
        self.one_iteration()

    def run(self, n):
        for _ in range(n):
            self.one_iteration()


class OperatorStage(_Stage):
    """One iteration of trainer.py:387-582 per call, through the autograd operators (pre-update done, fresh Adam +
    LinearLR: trainer.py:347-384)."""

    def __init__(self, tr, p):
        super().__init__(tr, p, ListSink())
        tr.add_optimizer(p.lr, p.lr_camera, depth_invariant=True)
        tr.scheduler = LinearLR(tr.optimizer, start_factor=1.0, end_factor=0.1, total_iters=p.iterations)
        self.later_frame = tr.later_frame

    def one_iteration(self):
        tr, p, iteration, camera_only = self.tr, self.plan, self.iteration, self.camera_only
        snap = p.snapshot(iteration)
        uv, depth, render4, extras = tr._render_rgbd(want_extras=snap)
        within = geometry.within(uv.detach(), tr.W, tr.H)
        tr.within_index = within
        mm = p.move_mask
        if tr.still_mask_tentative is not None and camera_only:
            # moving-splat footprint joins the move mask (trainer.py:427-451)
            with torch.no_grad():
                grp = tr._input_group(sel=~tr.still_mask_tentative, detach=True)
                mrgb = render_mod.render_multiple(grp, ["rgb"])["rgb"]
                tr.rasterisations_done += 1
                grey = 0.299 * mrgb[0] + 0.587 * mrgb[1] + 0.114 * mrgb[2]
                mm = (grey > 0.0) | self.move_mask       # running union (trainer.py:451 rebinds move_mask)
            self.move_mask = mm
        loss, loss_rgb_pixel, l_rgb, l_depth = losses.image_loss(
            render4, tr.gt_image, tr.gt_depth if p.lambda_depth > 0 else None, tr.depth_ab,
            p.lambda_rgb if p.lambda_rgb > 0 else 0.0, p.lambda_depth if p.lambda_depth > 0 else 0.0,
            mm if camera_only else None)
        terms = {"rgb": l_rgb, "depth": l_depth}

        valid = tr._stage_rows(within, camera_only)
        if p.lambda_var:
            l_var = losses.var_loss(tr.get_attribute("scale"))
            loss = loss + p.lambda_var * l_var
            terms["var"] = l_var
        if p.lambda_scale:
            # trainer.py:495-502: the reference's within_index ALIASES valid_uv_index, which :467-471 narrow in
            # place, so scale and depth are both taken over `valid`
            l_scale = losses.scale_loss(tr.get_attribute("scale"), valid, depth[valid])
            loss = loss + p.lambda_scale * l_scale
            terms["scale"] = l_scale
        still = tr._still_selection(p.lambda_still)
        if still is not None:
            m, last_xyz = still
            diff = torch.norm(tr.get_attribute("xyz")[:m.shape[0]] - last_xyz, dim=1)
            # (an empty selection gives the reference a NaN LOSS VALUE but finite gradients: the
            # clamp keeps both finite here)
            l_still = (diff * m).sum() / m.sum().clamp(min=1)
            loss = loss + p.lambda_still * l_still
            terms["still"] = l_still
        flow = tr._flow_selection(p.lambda_flow, camera_only)
        if flow is not None:
            and_mask, gt_f = flow
            d = (uv[:tr.last_num] - tr.last_uv - gt_f) ** 2
            l_flow = (d * and_mask.unsqueeze(1)).sum() / (2.0 * and_mask.sum().clamp(min=1))   # mse over selected rows
            loss = loss + p.lambda_flow * l_flow
            terms["flow"] = l_flow

        tr.optimizer.zero_grad()
        loss.backward()
        # ---- gradient control (trainer.py:535-551)
        if self.later_frame and tr._attributes["rgb"].grad is not None:
            tr._attributes["rgb"].grad.zero_()
        if tr.has_still and tr._attributes["xyz"].grad is not None:
            tr._attributes["xyz"].grad[:tr.still_mask.shape[0]] *= (~tr.still_mask).unsqueeze(1)
        if camera_only:
            for q in tr._attributes.values():
                if q.grad is not None:
                    q.grad.zero_()
        tr.optimizer.step()
        tr.scheduler.step()
        tr.iterations_done += 1
        if p.log(iteration):
            self.log.append({k: float(v.detach()) for k, v in terms.items()}
                            | {"total": float(loss.detach()), "it": iteration})

        # ---- densification (trainer.py:560-571)
        if p.occ_densify(iteration):
            if p.mask.sum() > 0:
                tr.densify_by_pixels(torch.ones_like(loss_rgb_pixel), error_threshold=0.0,
                                     percent=p.densify_occ_percent, mask=p.mask)
        if p.err_densify(iteration):
            tr.densify_by_pixels(loss_rgb_pixel, error_threshold=p.densify_err_thre, percent=p.densify_err_percent,
                                 mask=None)
        if snap:
            self.sink.put(render_mod.render2img_device(render4[:3]), render_mod.render2img_device(extras[0]),
                          render_mod.render2img_device(extras[1]))
        self.uv, self.depth, self.last_render = uv.detach(), depth.detach(), render4.detach()
        self.iteration += 1


class FusedStage(_Stage):
    """Same iteration as ``OperatorStage`` but every step is ONE call into
    libgflow_hip (gfl_fit_iteration): no autograd graph, no torch kernels, no host sync."""

    def __init__(self, tr, p):
        tr.lr, tr.lr_camera = p.lr, p.lr_camera
        eng = self.eng = tr._pack_to_engine()
        # (a lone fit composes its snapshots on the shadow engine's side stream; with ``async_snapshots`` off: _launch)
        super().__init__(tr, p, RingSink(tr.ring, tr.shadow if tr.async_snapshots else None, p, tr.H, tr.W, tr.device))
        eng.drop_pending()                         # (a watch the last stage queued and never read is not this stage's)
        eng.pose.copy_(tr.pose.detach())
        eng.invalidate_regions()                   # (new pose, new frame's warp of the moving splats: the first iteration bins exactly)
        tr.pose = eng.pose                         # live: get_extr() follows the optimised pose
        eng.depth_ab.zero_()                                         # trainer.py:145-146: (a, b) = (1, 0) on every train()
        eng.depth_ab[0:1].fill_(1.0)                                 # (fills, not torch.tensor(..., device=): that copy blocks)
        tr.depth_ab = eng.depth_ab
        eng.intr.copy_(tr.intr)
        eng.reset_optimizer()
        hp = eng.hp
        hp.bg = tr.bg
        hp.lambda_rgb = p.lambda_rgb if p.lambda_rgb > 0 else 0.0
        hp.lambda_depth = p.lambda_depth if p.lambda_depth > 0 else 0.0
        hp.lambda_var, hp.lr, hp.lr_camera = p.lambda_var, p.lr, p.lr_camera
        hp.lambda_scale = float(p.lambda_scale or 0.0)
        hp.lr_end_factor, hp.total_iters = 0.1, p.iterations        # LinearLR(1.0 -> 0.1), trainer.py:384
        hp.freeze_rgb = 1 if tr.later_frame else 0
        hp.freeze_all_splats = 1 if p.camera_only else 0
        hp.step_camera = 1
        hp.lambda_flow = hp.lambda_still = 0.0
        self._set_regularisers()
        move_mask, camera_only = p.move_mask, p.camera_only
        eng.set_targets(tr.gt_image, tr.gt_depth if p.lambda_depth > 0 else None,
                        (~move_mask) if (camera_only and move_mask is not None) else None)
        self.tentative = tr.still_mask_tentative is not None and camera_only
        if self.tentative:
            # the footprint of the tentative moving splats joins the move mask in every iteration
            # (trainer.py:426-451): the library rebuilds ``keep`` inside its forward
            eng.set_footprint_mask(move_mask if move_mask is not None else torch.zeros(tr.H, tr.W, dtype=torch.bool),
                                   ~tr.still_mask_tentative)
        self.unchecked = 0               # iterations on reserved regions since the last look at the overflow words

    def _set_regularisers(self):
        tr, p, eng, dev = self.tr, self.plan, self.eng, self.tr.device
        n, hp = eng.N, eng.hp
        flow_target = flow_w = still_target = still_w = row_flags = None
        if tr.has_still:
            row_flags = torch.zeros(n, dtype=torch.uint8, device=dev)
            # bit0: still (xyz frozen, trainer.py:543-546); bit1: the row has a label (scale term, :467-471)
            row_flags[:tr.still_mask.shape[0]] = tr.still_mask.to(torch.uint8) | 2
        still = tr._still_selection(p.lambda_still)
        if still is not None:
            m, last_xyz = still
            still_target = torch.zeros(n, 3, device=dev)
            still_target[:m.shape[0]] = last_xyz
            still_w = torch.zeros(n, device=dev)
            still_w[:m.shape[0]] = m.float() / m.sum().clamp(min=1)      # empty selection: weights 0, not 0/0
            hp.lambda_still = p.lambda_still
        flow = tr._flow_selection(p.lambda_flow, p.camera_only)
        if flow is not None:
            and_mask, gt_f = flow
            flow_target = torch.zeros(n, 2, device=dev)
            flow_target[:tr.last_num] = tr.last_uv + gt_f
            flow_w = torch.zeros(n, device=dev)
            flow_w[:tr.last_num] = and_mask.float() / (2.0 * and_mask.sum().clamp(min=1))
            hp.lambda_flow = p.lambda_flow
        eng.set_regularisers(flow_target, flow_w, still_target, still_w, row_flags)

    def note_forward(self, n_rendered, rec=None):
        """the engine has just run a forward of ``n_rendered`` rows (``rec``: its records, should the engine have grown since)"""
        rec = self.eng.rec if rec is None else rec
        self.uv, self.depth, self.last_render = rec[:n_rendered, 0:2], rec[:n_rendered, 9:10], self.eng.render

    def settle(self, last=None):
        """Iterations that stepped NOTHING since the last look (the pair lists overflowed: they are grown first; or a tile
        outgrew its reserved region: that one iteration was void) are run again, so that the fit is where one that never
        skipped an update is.  ``last``: what to run as the LAST of them instead of a plain iteration (an iteration
        whose forward the host looks at is taken again: one_iteration).  One blocking read of two words."""
        while True:
            k = self.eng.settle_overflow()
            if not k:
                return
            for _ in range(k - 1 if last else k):
                self.eng.iteration(use_graph=False)
            if last:
                last()

    def account(self):
        """run()'s watch, read (FitEngine.take_pending): iterations that stepped nothing are run now, on the exact path (they
        cannot be void again); pair lists that overflowed or are more than half full (a looked-at iteration must not be the
        one that overflows them) go the blocking way -- grown, made up for."""
        k = self.eng.take_pending()
        if k is None:
            # (iterations run one at a time, st() instead of st.run(n): nothing was queued in between -- the blocking look)
            if self.unchecked:
                self.settle()
        elif k < 0:
            self.settle()
        else:
            for _ in range(k):
                self.eng.iteration(use_graph=False, reserved=False)

    def _launch(self, dst, n_rendered, looked_at):
        """the library's iteration; ``dst``: the sink's slot for its snapshot (None: no snapshot)"""
        tr, eng = self.tr, self.eng
        if dst is not None and self.sink.shadow is None:
            # (several fits sharing the device -- fit_clips_concurrent -- already fill each other's gaps, and a side
            #  stream and a shadow engine per clip cost them more than they give: 12.7 -> 10.9 frames/s with two clips.
            #  There the snapshot stays behind the iteration, in the same graph launch; an elementwise kernel moves it
            #  into the ring: ``copy_`` goes through the runtime's blit kernel, 47 us for these 3.7 MB)
            imgs = eng.iteration(use_graph=tr.use_graph, snapshot=True, reserved=False)
            torch.bitwise_or(imgs, 0, out=dst)
        else:
            # one call (or one hipGraph replay)
            eng.iteration(use_graph=tr.use_graph, reserved=None if not looked_at else False)
            if dst is not None:
                self.sink.compose(eng, dst, n_rendered)

    def one_iteration(self):
        tr, eng, p, iteration = self.tr, self.eng, self.plan, self.iteration
        n_rendered = eng.N                       # rows this iteration projects (densification appends afterwards)
        # Somebody LOOKS at this iteration's forward (snapshot, log entry, the error map of a densification).  An iteration
        # can step nothing (settle, above) -- its forward is then a render of truncated lists, and while it waits to be made
        # up for, the splats are a step behind the reference's at every later index (5 such iterations in the 27 050 of a
        # 60-frame clip, all in the first steps of the first frame).  So (a) a looked-at iteration bins on the exact path,
        # where no tile can outgrow a region, and so does the plain iteration in front of it; (b) BEFORE it is launched,
        # the iterations up to the one before that are accounted for (run(): watch_pending behind them, one more iteration
        # queued, then the look -- the host waits for work that is already done while the device runs that iteration; a
        # blocking look behind every looked-at iteration cost a clip fit 2 %, tools/ab_trainer_flag.py) and made up for on
        # the exact path.  The forward the host then looks at is the forward of the splats after exactly ``iteration``
        # optimiser steps, as in the reference (trainer.py:573-582).
        looked_at = not p.plain(iteration)
        if looked_at and tr.exact_snapshots:
            self.account()
        if self.tentative:
            tr.rasterisations_done += 1                  # the reference's extra render of the moving set
        dst = None
        if p.snapshot(iteration):
            # The three images of THIS iteration's forward are composed on a stream of their own, from a COPY of what the
            # forward left behind (records, sorted ids, tile ranges, the render, the tile queues: 9 MB, one launch --
            # gfl_fit_snapshot_stage -- into a shadow engine), BESIDE the next iterations instead of between them.  Inside
            # the iteration's own graph the snapshot cost 115-140 us every tenth iteration, 4-5 % of a clip fit; two
            # independent chains of launches share the chip well (two clips on one GPU: 1.43x), a fork inside a graph
            # does not (docs/history.md section 7).  Where they stay until the end of the call: RingSink.
            dst = self.sink.slot(len(self.frames))
        launch = lambda: self._launch(dst, n_rendered, looked_at)
        launch()
        if looked_at and tr.exact_snapshots == "blocking":
            self.settle(last=launch)                 # (the look BEHIND the iteration, and the iteration again: tests, A/B)
        self.unchecked = 0 if looked_at else self.unchecked + 1
        tr.rasterisations_done += 1
        tr.iterations_done += 1
        rec_now = eng.rec                        # (densification may re-allocate the engine's buffers below)
        if p.log(iteration):
            self.log.append(self._log_entry(iteration))
        densified = self._densify(iteration, launch)
        self.note_forward(n_rendered, rec_now)
        if densified:
            # trainer.py:941-951: the optimiser is replaced by Adam(attributes, lr): moments and step restart,
            # lr stays constant, pose / depth affine are no longer stepped.  Flags only: the new rows already
            # sit behind the old ones in the engine (densification_postfix), their regulariser weights and row
            # flags are the zeros the capacity-sized buffers were padded with.
            self.uv, self.depth = self.uv.clone(), self.depth.clone()
            eng.reset_optimizer(splats=True, camera=False)
            eng.hp.total_iters = 0
            eng.hp.step_camera = 0
        self.iteration += 1

    def _log_entry(self, iteration):
        eng, hp, lambda_var = self.eng, self.eng.hp, self.plan.lambda_var
        l_rgb, l_depth = eng.loss_terms()
        total = hp.lambda_rgb * l_rgb + hp.lambda_depth * l_depth
        entry = {"rgb": float(l_rgb), "depth": float(l_depth), "it": iteration}
        if lambda_var:
            entry["var"] = float(losses.var_loss(torch.abs(eng.views()["scale"])))
            total = total + lambda_var * entry["var"]
        entry["total"] = float(total)
        return entry

    def _densify(self, iteration, launch):
        """densification behind iteration ``iteration`` (trainer.py:560-571); True if rows were appended"""
        tr, eng, p = self.tr, self.eng, self.plan
        densified = False
        if not tr.exact_snapshots and p.err_densify(iteration):
            self.settle(last=launch)                 # (the error map below must be the scene's; this event reads back anyway)
        if p.occ_densify(iteration):
            # (an empty mask appends nothing: densify_by_pixels's own single host read decides, there is no
            #  separate ``mask.sum() > 0`` read as in trainer.py:563)
            b, n = tr.densify_by_pixels(torch.ones_like(eng.err_px), error_threshold=0.0,
                                        percent=p.densify_occ_percent, mask=p.mask, n_masked=p.mask_count)
            densified |= n > b
        if p.err_densify(iteration):
            b, n = tr.densify_by_pixels(eng.err_px, error_threshold=p.densify_err_thre,
                                        percent=p.densify_err_percent, mask=None)
            densified |= n > b          # the reference swaps the optimiser only inside `if densify_num > 0` (:903-936)
        return densified

    def _plain(self, b, **how):
        """``b`` plain iterations in one launch"""
        n_rendered = self.eng.N
        self.eng.iteration(count=b, **how)
        self.note_forward(n_rendered)
        self.tr.rasterisations_done += (2 * b) if self.tentative else b
        self.tr.iterations_done += b
        self.iteration += b

    def run(self, n):
        """the next n iterations; runs of plain ones go into ONE graph launch, two or four at a time (2-6 us pass
        between two graph launches, tools/graph_gap.py)"""
        tr, eng, plain, iterations = self.tr, self.eng, self.plan.plain, self.plan.iterations
        end = self.iteration + n
        while self.iteration < end:
            i = self.iteration
            if self.yielding and not plain(i) and tr.exact_snapshots and not eng.pending_ready():
                return                           # (the caller comes back: train_steps)
            if plain(i) and not plain(i + 1) and i + 1 < iterations and tr.exact_snapshots:
                # the plain iteration in front of a looked-at one: what ran before it is accounted for while IT runs
                # (one_iteration: account) -- on the exact path, so that nothing is left unaccounted for.  Not the LAST
                # iteration of the stage: index ``iterations`` is never run, so a watch queued there would be read by
                # the next stage's first iteration -- after the end-of-stage settle() has already made up for the same
                # void iterations (they were made up twice, under the next stage's hyper-parameters)
                if self.unchecked:
                    eng.watch_pending()
                    self.unchecked = 0
                self._plain(1, use_graph=tr.use_graph, reserved=False)
                continue
            k = 0
            while (k < 4 and i + k < end and plain(i + k)
                   and (plain(i + k + 1) or i + k + 1 >= iterations or not tr.exact_snapshots)):
                k += 1
            if k < 2 or not tr.use_graph:
                self.one_iteration()
                continue
            self._plain(4 if k == 4 else 2, use_graph=True)
            self.unchecked += 4 if k == 4 else 2
