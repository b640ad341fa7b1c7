"""The two engines a trainer keeps beside ``SimpleGaussian.engine``, each with one owner.

``SecondEngine`` renders the CURRENT splats without disturbing the fit, on the fit's stream: the part images at the end of
``train()``, the scene image of the trajectories, the frame's shared final forward for the tracker and the flow recorder.
``SnapshotShadow`` composes the asynchronous snapshots on a side stream, from a copy of the forward the fit has just run.
They stay TWO engines: the shadow's buffers are read on the side stream while the second engine is written on the fit's
stream -- one engine for both would need every use of the second engine to wait for the last snapshot.
Both are made by the trainer's engine factory ``make(capacity, K_cap=None)``, which carries W, H, bg, cu_count and the
deterministic mode, and exist only from their first use on."""
import torch

HIDDEN = -1000.0         # raw opacity of a splat that is not to be drawn: sigmoid(-10^4) = 0 < 1/255


def fits(eng, n, K_cap=None):
    """``eng`` (an engine, or None) has room for ``n`` rows and ``K_cap`` pairs"""
    return eng is not None and eng.cap >= n and (K_cap is None or eng.K_cap >= K_cap)


class SecondEngine:
    """``engine``: None until first use, replaced by a larger one when the main engine's rows no longer fit."""

    def __init__(self, make):
        self.make, self.engine = make, None

    def follow(self, main, bg):
        """The engine, with room for ``main``'s rows and primed with its count, camera and background."""
        if not fits(self.engine, main.N):
            self.engine = self.make(max(main.cap, main.N))
        eng = self.engine
        eng.set_count(main.N)
        eng.pose.copy_(main.pose)
        eng.intr.copy_(main.intr)
        eng.hp.bg = bg
        return eng

    def _forward_rows(self, main, hide=None, hidden=None):
        """``main``'s live rows copied into the primed engine and run forward.  ``hide`` ((N,) bool): those rows get the raw
        opacity ``hidden`` (HIDDEN as a device scalar) -- the preprocess kernel never bins them -- instead of being gathered
        out: no boolean gather (that is a host read of the count), the depth order of the others is unchanged."""
        eng, n = self.engine, main.N
        eng.params[:n].copy_(main.params[:n])
        if hide is not None:
            eng.params[:n, 10] = torch.where(hide, hidden, main.params[:n, 10])
        eng.forward()

    def forward(self, main, bg):
        """One forward of ``main``'s CURRENT splats and camera; returns the engine, its records (``rec``: uv in columns 0:2,
        depth in column 9) and ``render`` (rgb, depth_map) holding the result.  The caller watches its overflow flag."""
        eng = self.follow(main, bg)
        self._forward_rows(main)
        return eng

    def scene_u8(self, main, bg):
        """(3, H, W, 3) uint8 on the device: rgb, depth colour, centre blobs of the CURRENT splats and camera (what
        render_multiple(["rgb", "center", "depth_map_color"]) + render2img give, trainer.py:765-777) through the fused
        kernels: one forward, one gfl_fit_snapshot, the overflow watch; nothing is read back."""
        eng = self.forward(main, bg)
        out = eng.snapshot()
        eng.watch_overflow()
        return out

    def parts_u8(self, main, bg, still_mask):
        """(2, 3, H, W, 3) uint8 on the device: [still splats, moving splats] x [rgb, depth colour, centre blobs] of the
        current state (trainer.py:632-677 renders rgb and centre of both sets), the other set hidden (``_forward_rows``); the engine
        is primed and the scalar made once for both."""
        eng = self.follow(main, bg)
        out = []
        hidden = torch.full((), HIDDEN, device=eng.dev)
        for hide in (~still_mask, still_mask):
            self._forward_rows(main, hide, hidden)
            out.append(eng.snapshot())
        eng.watch_overflow()
        return torch.stack(out)


class SnapshotShadow:
    """The shadow engine of the asynchronous snapshots, its side stream (``stream``: None before the first ``compose``, the
    SAME object from then on) and the event of its last snapshot."""

    def __init__(self, make, device):
        self.make, self.device = make, device
        self.engine = self.stream = self.done = None

    def compose(self, main, out, n):
        """The snapshot images of the forward ``main`` has just run (``n`` rows) into ``out`` ((3, H, W, 3) uint8 on the
        device), composed by the shadow engine on the side stream from a copy of that forward's state; returns at once."""
        cur = torch.cuda.current_stream()
        if not fits(self.engine, n, main.K_cap):
            if self.engine is not None:
                # the engine grew.  The side stream may still be composing the previous snapshot from the old shadow's
                # buffers (allocated on the fit stream, used over there): let it finish before they are freed -- a rare
                # event, a wait of one snapshot -- and keep the SAME stream, so that everything that waits on it (the
                # ring's growth, the final copy to the host: stage.RingSink) still sees its last write
                self.stream.synchronize()
            else:
                self.stream = torch.cuda.Stream(device=self.device)
            self.engine = self.make(max(main.cap, n), main.K_cap)
            self.done = None
        shadow, side = self.engine, self.stream
        if self.done is not None:
            cur.wait_event(self.done)                # the previous snapshot has read the shadow's buffers (ten iterations ago)
        # (count and compositing constants only: gfl_fit_snapshot_stage copies the camera with the rest of the forward's state)
        shadow.set_count(n)
        shadow.hp.bg, shadow.hp.nearest, shadow.hp.extent = main.hp.bg, main.hp.nearest, main.hp.extent
        main.stage_forward_to(shadow)                # (on the current stream, behind the forward)
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            shadow.snapshot(out=out)
            self.done = torch.cuda.Event()
            self.done.record(side)

    def watch_overflow(self):
        """the shadow's overflow watch, queued on its own stream (behind its snapshots)"""
        with torch.cuda.stream(self.stream):
            self.engine.watch_overflow()
