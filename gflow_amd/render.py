"""Render orchestrator -- the counterpart of gflow/utils/render.py.

``render_multiple`` / ``render_traj`` / ``render2img`` keep the reference's
signatures and semantics (render.py:6-166) on top of ``gflow_amd.msplat``.
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib as L
from . import msplat
from .color import apply_float_colormap
from .fused import tile_count
from .pinned import DeferredRead

FUSED_TYPES = frozenset(("rgb", "uv", "depth", "depth_map"))
USE_FUSED = True        # render_multiple routes {"rgb","uv","depth","depth_map"} requests through the fused operator

# ------------------------------------------------------------ fused differentiable operator
_POOL = {}              # (W, H, device) -> [_Slot]; a slot's engine is checked out from forward until backward


class _Slot:
    """A pooled engine and what the pool keeps about it: ``busy`` / ``owner`` (the reservation token, _checkout) and ``pad2``,
    the two zero columns that complete a parameter row."""

    def __init__(self, eng):
        self.eng, self.busy, self.owner, self.pad2 = eng, False, None, None


def _checkout(W, H, n, dev):
    """A slot of the pool, reserved for the caller: returns (slot, token).  The token is the reservation --
    ``_release`` frees the slot only for the token it was checked out with, so a stale finalizer of an earlier
    forward (its graph node is collected AFTER the next forward took the same engine) cannot free it under the
    forward / backward pair that owns it now."""
    from .fused import FitEngine
    key = (int(W), int(H), str(dev))
    for slot in _POOL.setdefault(key, []):
        if not slot.busy:
            break
    else:
        slot = _Slot(FitEngine(W, H, max(2 * n, 65536), dev))
        _POOL[key].append(slot)
    eng = slot.eng
    # the pair-list overflow flag of this engine's PREVIOUS call, copied to pinned memory behind that call: read it
    # here without waiting for the device (an overflow drops splat-tile pairs silently otherwise)
    eng.poll_overflow()
    eng.ensure_capacity(n)
    if slot.pad2 is None or slot.pad2.shape[0] < eng.cap:
        slot.pad2 = torch.zeros(eng.cap, 2, dtype=torch.float32, device=eng.dev)
    # the deterministic mode follows torch's switch at the time of the forward (the backward reads the same state word)
    eng.deterministic = torch.are_deterministic_algorithms_enabled()
    slot.busy = True
    slot.owner = object()
    return slot, slot.owner


def _release(slot, token):
    if slot.owner is token:
        slot.owner = None
        slot.busy = False


def check_overflow():
    """Blocking: raises if ANY render of the fused operator -- or any batched call (render_views / render_jobs / render_block / render_composed) --
    so far dropped splat-tile pairs (the operator itself looks at
    the flag without stopping the host: at the backward of the same render, and at the next render on the same engine).
    Call it after the last render of a program whose result matters."""
    for slots in _POOL.values():
        for slot in slots:
            slot.eng.check_overflow()
    for ws in _BATCH_WS.values():
        ws.check(blocking=True)


class _FusedRender(torch.autograd.Function):
    """render(gaussians, camera) -> (rgb, depth_map, uv, depth): gfl_render_fwd / gfl_render_bwd of
    include/gflow_hip.h -- projection, covariance, EWA, binning, sort and the 4-channel composite in the fused
    kernels, one library call per direction (render.py:6-108 makes six operator calls).  The library writes straight
    into the tensors that are returned (fresh render / record buffers per call, the caller's intr / extr are read in
    place): per direction the host issues one concatenation, two allocations and the call."""

    @staticmethod
    def forward(ctx, xyz, scale, rotate, opacity, rgb, intr, extr, bg, W, H):
        dev = xyz.device
        n = xyz.shape[0]
        slot, token = _checkout(W, H, n, dev)
        eng = slot.eng
        try:
            if n:
                f = lambda t, c: t.detach().float().reshape(n, c)
                torch.cat([f(xyz, 3), f(scale, 3), f(rotate, 4), f(opacity, 1), f(rgb, 3), slot.pad2[:n]], dim=1,
                          out=eng.params[:n])
            intr_c = intr.detach().float().contiguous().reshape(4)
            extr_c = extr.detach().float().contiguous().reshape(12)
            out = torch.empty(4, eng.H, eng.W, dtype=torch.float32, device=dev)
            rec = torch.empty(max(n, 1), 12, dtype=torch.float32, device=dev)
            st = eng.state()
            st.N, st.intr, st.extr, st.render, st.rec = n, intr_c.data_ptr(), extr_c.data_ptr(), out.data_ptr(), rec.data_ptr()
            eng.hp.bg = float(bg)
            L.check(eng.lib.gfl_render_fwd(ctypes.byref(st), ctypes.byref(eng.hp), L.stream()), "render")
            eng.watch_overflow()
        except Exception:
            _release(slot, token)
            raise
        if any(ctx.needs_input_grad):
            ctx.slot, ctx.n, ctx.keep, ctx.token = slot, n, (intr_c, extr_c, out, rec), token
            ctx.intr_shape = intr.shape
            # a graph that is dropped without backward frees the engine too; backward() calls this same finalizer,
            # which runs at most once
            ctx.fin = weakref.finalize(ctx, _release, slot, token)
        else:
            _release(slot, token)
        return out[:3], out[3:4], rec[:n, 0:2], rec[:n, 9:10]

    @staticmethod
    def backward(ctx, d_rgb, d_depth_map, d_uv, d_depth):
        eng, n = ctx.slot.eng, ctx.n
        if ctx.slot.owner is not ctx.token:
            # (the tile lists, records and checkpoints of the forward live in the pooled engine, which went back to the
            # pool with the first backward)
            raise RuntimeError("gflow_amd.render: backward through the fused render operator a second time "
                               "(retain_graph) is not supported; call render() again")
        eng.poll_overflow()          # (the forward of this very render: by now its flag has usually reached the host)
        dev = eng.dev
        H, W = eng.H, eng.W
        z = lambda c: torch.zeros(c, H, W, dtype=torch.float32, device=dev)
        d_render = torch.cat([z(3) if d_rgb is None else d_rgb.float(), z(1) if d_depth_map is None else d_depth_map.float()])
        d_uv = None if d_uv is None else d_uv.float().contiguous()
        d_depth = None if d_depth is None else d_depth.float().contiguous()
        d_params = torch.empty(max(n, 1), 16, dtype=torch.float32, device=dev)
        d_extr = torch.empty(12, dtype=torch.float32, device=dev)
        d_intr = None
        if ctx.needs_input_grad[5]:
            # asked for (intr.requires_grad_()): the entry whose per-splat launch also reduces the four intrinsics sums
            d_intr = torch.empty(4, dtype=torch.float32, device=dev)
            L.check(eng.lib.gfl_render_bwd_cam(ctypes.byref(eng.state()), ctypes.byref(eng.hp), L.ptr(d_render), L.ptr(d_uv),
                                               L.ptr(d_depth), L.ptr(d_params), L.ptr(d_extr), L.ptr(d_intr), L.stream()),
                    "render backward")
            d_intr = d_intr.reshape(ctx.intr_shape)
        else:
            L.check(eng.lib.gfl_render_bwd(ctypes.byref(eng.state()), ctypes.byref(eng.hp), L.ptr(d_render), L.ptr(d_uv),
                                           L.ptr(d_depth), L.ptr(d_params), L.ptr(d_extr), L.stream()), "render backward")
        ctx.fin()
        g = d_params[:n]
        return (g[:, 0:3], g[:, 3:6], g[:, 6:10], g[:, 10:11], g[:, 11:14], d_intr, d_extr.reshape(3, 4), None, None, None)


def render(gaussians, camera, bg=0.0):
    """The rasteriser as ONE differentiable operator.  gaussians: dict with the ACTIVATED attributes xyz (N,3),
    scale (N,3), rotate (N,4, unit, wxyz), opacity (N,1), rgb (N,3); camera: dict with intr (4,), extr (3,4),
    W, H.  Returns dict(rgb (3,H,W), depth_map (1,H,W), uv (N,2), depth (N,1)) -- what
    render_multiple(input_group, ["rgb", "uv", "depth", "depth_map"]) returns (render.py:6-108), with gradients to
    the five attributes, to extr and to intr.  The gradient of intr (4,) is computed when the caller asks for it
    (``intr.requires_grad_()``) and costs nothing otherwise; culling, radius and tile rectangles are not differentiated.
    Under torch.use_deterministic_algorithms(True) the call runs in the library's deterministic mode (GFL_FIT_DETERMINISTIC,
    include/gflow_hip.h): forward and backward give bit-identical results for identical inputs."""
    L.need_device(gaussians["xyz"])
    rgb, depth_map, uv, depth = _FusedRender.apply(
        gaussians["xyz"], gaussians["scale"], gaussians["rotate"], gaussians["opacity"], gaussians["rgb"],
        camera["intr"], camera["extr"], float(bg), int(camera["W"]), int(camera["H"]))
    return {"rgb": rgb, "depth_map": depth_map, "uv": uv, "depth": depth}


def render_multiple(input_group,
                    return_type=("rgb", "uv", "depth", "depth_map", "depth_map_color", "center"),
                    center_scale=10.0):
    """input_group = [xyz, scale, rotate, opacity, rgb, intr, extr, bg, W, H]
    (render.py:9).  Returns a dict with the requested entries:
    rgb (3,H,W), uv (N,2), depth (N,1), depth_map (1,H,W), depth_map_color (3,H,W),
    center (3,H,W)."""
    xyz, scale, rotate, opacity, rgb, intr, extr, bg, W, H = input_group
    if USE_FUSED and xyz.is_cuda and set(return_type) <= FUSED_TYPES and ("rgb" in return_type or "depth_map" in return_type):
        # the training call (trainer.py:404-407 minus the two snapshot images): one fused operator
        full = render(dict(xyz=xyz, scale=scale, rotate=rotate, opacity=opacity, rgb=rgb),
                      dict(intr=intr, extr=extr, W=W, H=H), bg)
        return {k: full[k] for k in return_type}
    out = {}
    uv, depth = msplat.project_point(xyz, intr, extr, W, H)
    visible = depth != 0
    if "uv" in return_type:
        out["uv"] = uv
    if "depth" in return_type:
        out["depth"] = depth
    cov3d = msplat.compute_cov3d(scale, rotate, visible)
    conic, radius, tiles_touched = msplat.ewa_project(xyz, cov3d, intr, extr, uv, W, H, visible)
    ids, tile_range = msplat.sort_gaussian(uv, depth, W, H, radius, tiles_touched)
    if "rgb" in return_type:
        out["rgb"] = msplat.alpha_blending(uv, conic, opacity, rgb, ids, tile_range, bg, W, H)
    if "depth_map" in return_type:
        out["depth_map"] = msplat.alpha_blending(uv, conic, opacity, depth, ids, tile_range, bg, W, H)
    if "depth_map_color" in return_type:
        depth_color = apply_float_colormap(depth, colormap="turbo", non_zero=True)
        out["depth_map_color"] = msplat.alpha_blending(uv, conic, opacity, depth_color, ids, tile_range, bg, W, H)
    if "center" in return_type:
        # unit-variance blobs at the splat centres, same sorted lists (render.py:93-106)
        unit = torch.tensor([1.0, 0.0, 1.0], device=conic.device)
        out["center"] = msplat.alpha_blending(uv, torch.ones_like(conic) * unit, torch.ones_like(opacity), rgb, ids,
                                              tile_range, bg, W, H)
    return out


def render_traj(input_group, point_num, line_scale=1.0, point_scale=2.0):
    """Trajectory overlay (render.py:110-156): isotropic blobs, the last
    ``point_num`` splats drawn with ``line_scale``, the others with ``point_scale``."""
    xyz, scale, rotate, opacity, rgb, intr, extr, bg, W, H = input_group
    uv, depth = msplat.project_point(xyz, intr, extr, W, H)
    visible = depth != 0
    cov3d = msplat.compute_cov3d(scale, rotate, visible)
    conic, radius, tiles_touched = msplat.ewa_project(xyz, cov3d, intr, extr, uv, W, H, visible)
    ids, tile_range = msplat.sort_gaussian(uv, depth, W, H, radius, tiles_touched)
    unit = torch.tensor([1.0, 0.0, 1.0], device=conic.device)
    conic = torch.ones_like(conic) * unit * line_scale
    conic[:-point_num] = torch.ones_like(conic[:-point_num]) * unit * point_scale
    return msplat.alpha_blending(uv, conic, opacity, rgb, ids, tile_range, bg, W, H)


def render2img_device(rendered):
    """(3,H,W) float -> (H,W,3) uint8 tensor ON THE DEVICE: the clamp / x255 / truncation of render.py:158-166
    without the host round trip (a snapshot used to cost ~6 ms of numpy arithmetic on three 1.2 M-element
    float images; the iteration it interrupts takes 0.22 ms).  Nothing here waits for the GPU."""
    return (torch.clamp(rendered.detach(), 0.0, 1.0) * 255.0).to(torch.uint8).permute(1, 2, 0).contiguous()


def render2img(rendered):
    """(3,H,W) float -> (H,W,3) uint8 numpy (render.py:158-166)."""
    return render2img_device(rendered).cpu().numpy()


# ------------------------------------------------------------ batched inference rasteriser
# gfl_render_batch (include/gflow_hip.h): many (row range, camera) jobs per library call, no backward state, uint8 written by
# the blend.  A long job list is split into calls; each call stays under these limits (module attributes: set them before a call):
BATCH_MAX_JOBS = 256                 # jobs per library call
BATCH_MAX_TILES = 1 << 20            # (job, tile) pairs per call: 647 jobs of 480 x 854
BATCH_MAX_PAIRS = 1 << 28            # splat-tile pairs of a call's pool (12 bytes apiece: 3.2 GB)
_BATCH_WS = {}                       # (W, H, device) -> _BatchWorkspace


def batch_k_cap(n):
    """splat-tile pairs a job of n rows gets by default: what a pooled engine of render() has (FitEngine: capacity
    max(2 n, 65536), K_cap max(4 M, 8 x capacity))"""
    return max(4_000_000, 8 * max(2 * int(n), 65536))


class _BatchWorkspace:
    """The library workspace of the batched calls on one (W, H, device): grows, never shrinks.  ``pending``: the overflow
    flags of earlier calls, each a watched DeferredRead with the call's K_cap (what FitEngine.watch_overflow / poll_overflow
    do per engine); ``captured``: the device flags of calls that were captured into a graph (nothing can be
    copied to the host behind a replay: check_overflow() reads them)."""

    def __init__(self, dev):
        self.dev = dev
        self.buf = None
        self.pending = []
        self.captured = []

    def room(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.dev)
        return self.buf

    def watch(self, ovf, k_cap):
        if torch.cuda.is_current_stream_capturing():
            self.captured.append((ovf, k_cap))
            return
        read = DeferredRead(ovf.numel())
        read.watch(ovf)
        self.pending.append((read, k_cap))

    def check(self, blocking=False):
        """raises if a finished (blocking: any) earlier call dropped pairs or had a row range outside its block"""
        if torch.cuda.is_current_stream_capturing():
            return
        keep, bad = [], None
        for read, k_cap in self.pending:
            flags = read.read() if blocking else read.poll()
            if flags is None:
                keep.append((read, k_cap))
            elif bad is None and any(flags):
                bad = (flags, k_cap)
        self.pending = keep
        if blocking and bad is None:
            for ovf, k_cap in self.captured:
                flags = ovf.tolist()
                if any(flags):
                    ovf.zero_()
                    bad = (flags, k_cap)
                    break
        if bad is not None:
            flags, k_cap = bad
            jobs = [j for j, f in enumerate(flags) if f]
            if 2 in flags:
                raise RuntimeError(f"gflow_amd.render: jobs {jobs} of a batched call had a row range outside the row block")
            raise RuntimeError(f"gflow_amd.render: jobs {jobs} of a batched call lost splat-tile pairs (the call's pool of "
                               f"K_cap={k_cap} pairs was full); raise K_cap")


def _batch_ws(W, H, dev):
    key = (int(W), int(H), str(dev))
    ws = _BATCH_WS.get(key)
    if ws is None:
        ws = _BATCH_WS[key] = _BatchWorkspace(dev)
    return ws


def rows_block(gaussians):
    """One activated splat set (dict xyz, scale, rotate, opacity, rgb) as the [N][16] float32 row block the library reads
    (xyz | scale | unit quaternion wxyz | opacity | rgb | pad pad).  Detached."""
    n = gaussians["xyz"].shape[0]
    f = lambda t, c: t.detach().float().reshape(n, c)
    xyz = f(gaussians["xyz"], 3)
    return torch.cat([xyz, f(gaussians["scale"], 3), f(gaussians["rotate"], 4), f(gaussians["opacity"], 1),
                      f(gaussians["rgb"], 3), torch.zeros(n, 2, dtype=torch.float32, device=xyz.device)], dim=1)


def _job_cams(J, intr, extr, bg, dev):
    """[J][17] = intr | extr | bg, built on the device (inside a graph capture: from the caller's tensors at every replay)"""
    intr = intr.detach().float().to(dev).reshape(-1, 4)
    extr = extr.detach().float().to(dev).reshape(-1, 12)
    if intr.shape[0] == 1 and J > 1:
        intr = intr.expand(J, 4)
    if torch.is_tensor(bg):
        bgc = bg.detach().float().to(dev).reshape(-1, 1)
    elif isinstance(bg, (int, float)):
        bgc = torch.full((J, 1), float(bg), dtype=torch.float32, device=dev)
    else:
        vals = [float(b) for b in bg]
        if len(set(vals)) == 1:
            bgc = torch.full((J, 1), vals[0], dtype=torch.float32, device=dev)
        else:
            bgc = torch.tensor(vals, dtype=torch.float32).reshape(-1, 1).to(dev)
    if intr.shape[0] != J or extr.shape[0] != J or bgc.shape[0] != J:
        raise ValueError(f"gflow_amd.render: {J} jobs, but {intr.shape[0]} intrinsics, {extr.shape[0]} extrinsics, "
                         f"{bgc.shape[0]} backgrounds")
    return torch.cat([intr, extr, bgc], dim=1).contiguous()


def render_block(block, ranges, intr, extr, bg, W, H, uint8=False, records=False, K_cap=None):
    """The batched inference rasteriser on a row block.  block: [R][16] float32 ACTIVATED rows (rows_block); ranges: J pairs
    (first row, row count) -- they may overlap or repeat --, or (J, 2) int32 on the device; intr (4,) or (J, 4); extr
    (J, 3, 4); bg a float, a sequence or a tensor of J.  Returns dict(rgb (J,3,H,W), depth_map (J,1,H,W)), or with
    ``uint8`` dict(img (J,H,W,3) uint8) = render2img of the rgb planes; with ``records`` also rec (sum of counts, 12), the
    jobs' records one after the other (uv = columns 0:2, depth = column 9).  NOT differentiable.  Nothing here waits for
    the device; dropped pairs raise at the next batched call or in check_overflow().  ``K_cap``: pairs per library call
    (default: batch_k_cap(longest job) x jobs of the call)."""
    L.need_device(block)
    lib = L.load()
    dev = block.device
    W, H = int(W), int(H)
    block = block.detach()
    if block.dtype != torch.float32 or not block.is_contiguous() or block.dim() != 2 or block.shape[1] != 16:
        raise ValueError("gflow_amd.render: the row block is [R][16] float32, contiguous")
    if torch.is_tensor(ranges):
        rows_dev = ranges.to(dev).to(torch.int32).reshape(-1, 2).contiguous()
        counts = None                        # (device values: every job may be the whole block)
        J = rows_dev.shape[0]
    else:
        counts = [int(c) for _, c in ranges]
        J = len(counts)
        rows_dev = None
    ws = _batch_ws(W, H, dev)
    ws.check()
    img = torch.empty(J, H, W, 3, dtype=torch.uint8, device=dev) if uint8 else None
    out = None if uint8 else torch.empty(J, 4, H, W, dtype=torch.float32, device=dev)
    R = block.shape[0]
    per_job = [R] * J if counts is None else counts
    rec = torch.empty(max(sum(per_job), 1), 12, dtype=torch.float32, device=dev) if records else None
    if J:
        cams = _job_cams(J, intr, extr, bg, dev)
        if rows_dev is None:
            firsts = [int(a) for a, _ in ranges]
            if len(set(firsts)) == 1 and len(set(counts)) == 1:      # (fills: nothing is copied from the host)
                rows_dev = torch.zeros(J, 2, dtype=torch.int32, device=dev)
                if firsts[0]:
                    rows_dev[:, 0].fill_(firsts[0])
                if counts[0]:
                    rows_dev[:, 1].fill_(counts[0])
            else:
                host = torch.tensor([[a, c] for a, c in zip(firsts, counts)], dtype=torch.int32).pin_memory()
                rows_dev = host.to(dev, non_blocking=True)
        ovf = torch.empty(J, dtype=torch.int32, device=dev)
        T = tile_count(W, H)
        k_job = batch_k_cap(max(per_job))
        step = max(1, min(int(BATCH_MAX_JOBS), int(BATCH_MAX_TILES) // T, int(BATCH_MAX_PAIRS) // k_job))
        k_used = 0
        rec_at = 0
        for a in range(0, J, step):
            b = min(J, a + step)
            rows_total = sum(per_job[a:b])
            k_cap = int(K_cap) if K_cap is not None else k_job * (b - a)
            k_used = max(k_used, k_cap)
            buf = ws.room(lib.gfl_render_batch_workspace_bytes(b - a, rows_total, k_cap, W, H))
            L.check(lib.gfl_render_batch(L.ptr(block), R, L.ptr(rows_dev[a:b]), L.ptr(cams[a:b]), b - a, rows_total, W, H, k_cap,
                                         L.ptr(out[a:b]) if out is not None else None,
                                         L.ptr(img[a:b]) if img is not None else None,
                                         L.ptr(rec[rec_at:]) if rec is not None else None,
                                         L.ptr(ovf[a:b]), L.ptr(buf), buf.numel(), L.stream()), "render_batch")
            rec_at += rows_total
        ws.watch(ovf, k_used)
    res = {"img": img} if uint8 else {"rgb": out[:, :3], "depth_map": out[:, 3:4]}
    if records:
        res["rec"] = rec[:sum(per_job)]
    return res


def _job_table(values, dtype, width, dev):
    """A small per-job table on the device: a device tensor is taken as it is; host values whose rows are all alike are made
    with fills (nothing is copied from the host: such a call can be captured), others go through page-locked memory."""
    if torch.is_tensor(values):
        return values.detach().to(dev).to(dtype).reshape(-1, width).contiguous()
    rows = [tuple(r) if width > 1 else (r,) for r in values]
    if len(set(rows)) <= 1:
        out = torch.zeros(len(rows), width, dtype=dtype, device=dev)
        for k, x in enumerate(rows[0] if rows else ()):
            if x:
                out[:, k].fill_(x)
        return out
    return torch.tensor(rows, dtype=dtype).pin_memory().to(dev, non_blocking=True)


def render_composed(block, labels, job_src, job_s, job_edit, intr, extr, bg, W, H, rows_max, uint8=False, rows=False):
    """In-between frames, layers and group edits of a clip's row block, rendered: gfl_compose_rows (include/gflow_hip.h) makes
    every job's rows on the device -- frame a blended with frame b at s, the group edits applied, invisible rows dropped --
    and gfl_render_batch renders them where the composer left them.  block: [R][16] float32 ACTIVATED rows (rows_block);
    labels: (R,) uint8 on the device, a group per row (0 still, 1 moving), or None; job_src: J rows (first_a, count_a, first_b,
    count_b) or (J, 4) int32 on the device; job_s: J floats in [0, 1] or a tensor; job_edit: (J, G, 16) float32 on the device
    (viewer.Edit.table) or None; intr, extr, bg as render_block takes them; rows_max: room per job, at least the longest
    range.  Returns what render_block returns, and with ``rows`` also out_rows (J * rows_max, 16) and out_job_rows (J, 2) =
    (j * rows_max, rows kept).  NOT differentiable.  Nothing here waits for the device; a source range outside the block, or
    longer than rows_max, and dropped pairs raise at the next batched call or in check_overflow()."""
    L.need_device(block)
    lib = L.load()
    dev = block.device
    W, H, rows_max = int(W), int(H), int(rows_max)
    block = block.detach()
    if block.dtype != torch.float32 or not block.is_contiguous() or block.dim() != 2 or block.shape[1] != 16:
        raise ValueError("gflow_amd.render: the row block is [R][16] float32, contiguous")
    R = block.shape[0]
    if labels is not None:
        L.need_device(labels)
        if labels.dtype != torch.uint8 or labels.numel() != R or not labels.is_contiguous():
            raise ValueError("gflow_amd.render: labels are (R,) uint8, contiguous")
    src = _job_table(job_src, torch.int32, 4, dev)
    J = src.shape[0]
    s = _job_table(job_s, torch.float32, 1, dev)
    G = 1
    if job_edit is not None:
        L.need_device(job_edit)
        if job_edit.dtype != torch.float32 or not job_edit.is_contiguous() or job_edit.dim() != 3 or job_edit.shape[0] != J \
                or job_edit.shape[2] != 16:
            raise ValueError("gflow_amd.render: the edit table is [J][G][16] float32, contiguous")
        G = job_edit.shape[1]
    if s.shape[0] != J:
        raise ValueError(f"gflow_amd.render: {J} jobs, but {s.shape[0]} blend weights")
    ws = _batch_ws(W, H, dev)
    ws.check()
    img = torch.empty(J, H, W, 3, dtype=torch.uint8, device=dev) if uint8 else None
    out = None if uint8 else torch.empty(J, 4, H, W, dtype=torch.float32, device=dev)
    out_rows = torch.empty(max(J * rows_max, 1), 16, dtype=torch.float32, device=dev)
    job_rows = torch.empty(J, 2, dtype=torch.int32, device=dev)
    if J:
        cams = _job_cams(J, intr, extr, bg, dev)
        flags = torch.empty(J, dtype=torch.int32, device=dev)
        ovf = torch.empty(J, dtype=torch.int32, device=dev)
        buf = ws.room(lib.gfl_compose_rows_workspace_bytes(J, rows_max))
        L.check(lib.gfl_compose_rows(L.ptr(block), L.ptr(labels), R, L.ptr(src), L.ptr(s), L.ptr(job_edit), G, J, rows_max,
                                     L.ptr(out_rows), L.ptr(job_rows), L.ptr(flags), L.ptr(buf), buf.numel(), L.stream()),
                "compose_rows")
        # the composer's rows are the rasteriser's block: R = J * rows_max, job j's range is out_job_rows[j]
        T = tile_count(W, H)
        k_job = batch_k_cap(rows_max)
        step = max(1, min(int(BATCH_MAX_JOBS), int(BATCH_MAX_TILES) // T, int(BATCH_MAX_PAIRS) // k_job))
        k_used = 0
        for a in range(0, J, step):
            b = min(J, a + step)
            rows_total = (b - a) * rows_max
            k_cap = k_job * (b - a)
            k_used = max(k_used, k_cap)
            buf = ws.room(lib.gfl_render_batch_workspace_bytes(b - a, rows_total, k_cap, W, H))
            L.check(lib.gfl_render_batch(L.ptr(out_rows), J * rows_max, L.ptr(job_rows[a:b]), L.ptr(cams[a:b]), b - a, rows_total,
                                         W, H, k_cap, L.ptr(out[a:b]) if out is not None else None,
                                         L.ptr(img[a:b]) if img is not None else None, None, L.ptr(ovf[a:b]), L.ptr(buf),
                                         buf.numel(), L.stream()), "render_batch")
        torch.maximum(ovf, flags, out=ovf)           # (one watched word per job: 2 from either side is a refused range)
        ws.watch(ovf, k_used)
    res = {"img": img} if uint8 else {"rgb": out[:, :3], "depth_map": out[:, 3:4]}
    if rows:
        res["out_rows"], res["out_job_rows"] = out_rows[:J * rows_max], job_rows
    return res


def _stack_cameras(cameras):
    """cameras: a list of dict(intr, extr) plus W, H in each (or in the first), or a dict of stacked tensors intr (V, 4) /
    (4,), extr (V, 3, 4), W, H.  Returns intr, extr (V, 3, 4), W, H."""
    if isinstance(cameras, dict):
        extr = cameras["extr"]
        return cameras["intr"], extr.reshape(-1, 3, 4), int(cameras["W"]), int(cameras["H"])
    if not len(cameras):
        raise ValueError("gflow_amd.render: no cameras")
    W, H = int(cameras[0]["W"]), int(cameras[0]["H"])
    return (torch.stack([c["intr"].detach().float().reshape(4) for c in cameras]),
            torch.stack([c["extr"].detach().float().reshape(3, 4) for c in cameras]), W, H)


def render_views(gaussians, cameras, bg=0.0, uint8=False, records=False, K_cap=None):
    """ONE activated splat set (as render() takes it) from V cameras in batched library calls.  cameras: a list of
    dict(intr, extr, W, H) or dict(intr (V,4) or (4,), extr (V,3,4), W, H).  Returns dict(rgb (V,3,H,W), depth_map
    (V,1,H,W)); with ``uint8`` dict(img (V,H,W,3) uint8 on the device) = render2img of rgb; with ``records`` also uv (V,N,2)
    and depth (V,N,1).  Per camera the numbers are render()'s.  NOT differentiable: inputs are detached -- render() is the
    differentiable operator.  A call with stacked camera tensors can be captured into a graph on one stream (run it once
    before, so that the workspace exists): a replay reads the camera tensors as they are then."""
    intr, extr, W, H = _stack_cameras(cameras)
    V = extr.shape[0]
    block = rows_block(gaussians)
    n = block.shape[0]
    res = render_block(block, [(0, n)] * V, intr, extr, bg, W, H, uint8=uint8, records=records, K_cap=K_cap)
    if records:
        rec = res.pop("rec").reshape(V, n, 12)
        res["uv"], res["depth"] = rec[:, :, 0:2], rec[:, :, 9:10]
    return res


def render_jobs(sets, cameras, bg=0.0, uint8=False, records=False, K_cap=None):
    """The ragged form: a list of activated splat sets with one camera each (cameras as render_views takes them), ``bg`` a
    float or one per job.  Returns what render_views returns, stacked over the jobs; with ``records`` uv and depth are LISTS
    of (N_j, 2) and (N_j, 1).  NOT differentiable: inputs are detached."""
    intr, extr, W, H = _stack_cameras(cameras)
    if extr.shape[0] != len(sets):
        raise ValueError(f"gflow_amd.render: {len(sets)} splat sets, {extr.shape[0]} cameras")
    blocks = [rows_block(g) for g in sets]
    ranges, at = [], 0
    for b in blocks:
        ranges.append((at, b.shape[0]))
        at += b.shape[0]
    dev = blocks[0].device if blocks else torch.device("cuda")
    block = torch.cat(blocks) if blocks else torch.zeros(0, 16, dtype=torch.float32, device=dev)
    res = render_block(block, ranges, intr, extr, bg, W, H, uint8=uint8, records=records, K_cap=K_cap)
    if records:
        rec = res.pop("rec")
        res["uv"] = [rec[a:a + c, 0:2] for a, c in ranges]
        res["depth"] = [rec[a:a + c, 9:10] for a, c in ranges]
    return res
