"""Depth and camera from the flows ("Depth and camera from the flows").

What a clip fit reads as ``<seq>_depth_mast3r_s2/*.npy`` and ``<seq>_camera_mast3r_s2/*.json`` -- a depth map and a
world-to-camera pose per frame, one focal length -- estimated here from the forward and backward flows instead of by
MASt3R's network: classical two-view geometry per pair of consecutive frames (a robust refit of the fundamental matrix, the
essential matrix's pose, triangulation), the baselines chained through the frames by the median ratio of a frame's two inverse
depths, the two fused, and what has no parallax-supported depth filled from its surroundings (pull-push, then weighted
Jacobi sweeps).  All pairs of a clip go through every stage in ONE library call (csrc/gfl_sfm.hip); only the starting
matrices come from the existing gfl_epi_fundamental, one call per pair (most of a clip's time: DESIGN.md, "Depth and camera
kernels").

It is NOT MASt3R and is unpinned against it: depth is recovered only where the camera translates (a pair without parallax
is flagged ``degenerate`` and contributes nothing), moving and occluded regions are filled from their surroundings, the
focal length is an ASSUMPTION (``max(W, H)`` unless given), and it has never been run on real video here.
include/gflow_hip.h ("depth and camera from the flows") holds the definitions, tests/sfm_ref.py restates them in float64.

    python -m gflow_amd.sfm --img_dir SEQ [--focal F] [--overwrite]
"""
import argparse
import json
import os
import warnings

import numpy as np
import torch

from . import _lib as L

MAX_PIXELS = 2 ** 30


def _device_of(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.sfm: needs a HIP (cuda) device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _check_shape(P, H, W):
    if H < 8 or W < 8 or H > 16384 or W > 16384 or P < 1 or P > 65535 or P * H * W > MAX_PIXELS:
        raise ValueError(f"sfm: {P} problems of {H} x {W} are refused (8 <= H, W <= 16384, 1 <= P <= 65535, P H W <= 2^30)")


def _workspace(lib, P, H, W, dev):
    need = lib.gfl_sfm_workspace_bytes(P, H, W)
    if need == 0:
        raise ValueError(f"sfm: {P} problems of {H} x {W} are refused by the library")
    return L.scratch(need, dev)


def _intr(intr):
    intr = tuple(float(v) for v in intr)
    if len(intr) != 4 or not all(np.isfinite(intr)) or intr[0] <= 0 or intr[1] <= 0:
        raise ValueError(f"sfm: intr must be finite (fx, fy, cx, cy) with positive focal lengths, got {intr}")
    return intr


def default_camera(H, W, focal=None, pp=None):
    """(focal, pp): the ASSUMED focal length max(W, H) and the principal point (round(W / 2), round(H / 2)) unless given"""
    focal = float(max(W, H)) if focal is None else float(focal)
    pp = [round(W / 2), round(H / 2)] if pp is None else [pp[0], pp[1]]
    return focal, pp


def initial_F(flow, exclude=None, hypotheses=256, seed=0):
    """The starting fundamental matrices ``(P, 9)`` float64 in pixel coordinates (x2 = x + flow) of ``flow (P, H, W, 2)`` on
    the device, from gfl_epi_fundamental (the least-median-of-squares fit of gflow_amd.move_seg), one call per pair.  That
    routine maps view 1 by N(x) = 2 (x + 0.5) / W - 1 and adds 2 flow / (W - 1): fed the flow scaled by (W - 1) / W and
    (H - 1) / H, both views are mapped by N and F_pix = N^T F N.  Excluded pixels are made unknown (their flow set to inf).
    The eight pixels of a hypothesis are drawn from all pixels: one that hits an unknown pixel is dropped by the routine."""
    from .move_seg import draw_samples
    P, H, W, _ = flow.shape
    dev = flow.device
    lib = L.load()
    K = int(hypotheses)
    samples = torch.tensor(draw_samples(np.ones(H * W, dtype=bool), K, seed), device=dev)
    scaled = flow * torch.tensor([(W - 1) / W, (H - 1) / H], dtype=torch.float32, device=dev)
    if exclude is not None:
        scaled = torch.where((exclude != 0).unsqueeze(-1), scaled.new_tensor(float("inf")), scaled)
    scaled = scaled.contiguous()
    ws = L.scratch(lib.gfl_epi_workspace_bytes(W, H, K), dev)
    Fn = torch.empty((P, 9), dtype=torch.float64, device=dev)
    best = torch.empty(1, dtype=torch.int32, device=dev)
    for p in range(P):
        L.check(lib.gfl_epi_fundamental(L.ptr(scaled[p]), W, H, L.ptr(samples), K, None, None, L.ptr(Fn[p]), L.ptr(best),
                                        L.ptr(ws), ws.numel(), L.stream()), "sfm initial F")
    N = torch.tensor([[2.0 / W, 0.0, 1.0 / W - 1.0], [0.0, 2.0 / H, 1.0 / H - 1.0], [0.0, 0.0, 1.0]], dtype=torch.float64,
                     device=dev)
    return (N.T @ Fn.reshape(P, 3, 3) @ N).reshape(P, 9).contiguous()


def two_view(flow, intr, exclude=None, *, F_init=None, rounds=2, e_floor=0.25 ** 2, min_parallax=0.1, min_share=0.2,
             hypotheses=256, seed=0):
    """Stages a - c of one pair ``(H, W, 2)`` or of P pairs ``(P, H, W, 2)``: ``flow`` in pixels (view 2 sees pixel x of view 1
    at x + flow; a pixel whose flow is not finite is unknown), ``intr = (fx, fy, cx, cy)`` of both views, ``exclude`` an
    optional mask of the flow's leading shape (nonzero: leave the pixel out -- a move mask, an occlusion mask).  Returns
    device tensors of the matching leading shape: dict(F (.., 3, 3), R (.., 3, 3), t (.., 3) float64 with x2 ~ R x1 + t,
    parallax (..) float64 px, degenerate (..) bool, inlier (.., H, W) uint8 0 / 1, rho, weight (.., H, W) float32 -- the
    inverse depth in units of 1 / baseline and sin^2 of the parallax angle --, votes (.., 4), counts (.., 2) int32 = usable
    pixels and inliers, median (..) float64).  ``F_init``: the starting matrices (default: ``initial_F``).  A degenerate pair
    (too few pixels or inliers, an F that is not finite, parallax below ``min_parallax`` px) has t = 0 and no weight.
    Everything is enqueued on the current stream; nothing is read back."""
    flow = torch.as_tensor(flow)
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError(f"sfm: flow must be (H, W, 2) or (P, H, W, 2), got {tuple(flow.shape)}")
    single = flow.dim() == 3
    dev = _device_of(flow)
    flow = flow.detach().to(dev, torch.float32).reshape((-1,) + tuple(flow.shape[-3:])).contiguous()
    P, H, W, _ = flow.shape
    _check_shape(P, H, W)
    fx, fy, cx, cy = _intr(intr)
    if exclude is not None:
        exclude = torch.as_tensor(exclude)
        if tuple(exclude.shape) != ((H, W) if single else (P, H, W)):
            raise ValueError(f"sfm: exclude must have the flow's leading shape, got {tuple(exclude.shape)}")
        exclude = (exclude.to(dev) != 0).to(torch.uint8).reshape(P, H, W).contiguous()
    if int(rounds) != rounds or not 0 <= rounds <= 16:
        raise ValueError(f"sfm: rounds must be an integer in 0 .. 16, got {rounds!r}")
    for k, v in dict(e_floor=e_floor, min_parallax=min_parallax, min_share=min_share).items():
        if not np.isfinite(v) or v < 0:
            raise ValueError(f"sfm: {k} must be finite and not negative, got {v}")
    lib = L.load()
    with torch.cuda.device(dev):
        if F_init is None:
            F_init = initial_F(flow, exclude, hypotheses, seed)
        F_init = torch.as_tensor(F_init).detach().to(dev, torch.float64).reshape(P, 9).contiguous()
        ws = _workspace(lib, P, H, W, dev)
        F = torch.empty((P, 9), dtype=torch.float64, device=dev)
        counts = torch.empty((P, 2), dtype=torch.int32, device=dev)
        median, parallax = (torch.empty(P, dtype=torch.float64, device=dev) for _ in range(2))
        inlier = torch.empty((P, H, W), dtype=torch.uint8, device=dev)
        R = torch.empty((P, 9), dtype=torch.float64, device=dev)
        t = torch.empty((P, 3), dtype=torch.float64, device=dev)
        votes = torch.empty((P, 4), dtype=torch.int32, device=dev)
        degenerate = torch.empty(P, dtype=torch.int32, device=dev)
        rho, weight = (torch.empty((P, H, W), dtype=torch.float32, device=dev) for _ in range(2))
        L.check(lib.gfl_sfm_refit(L.ptr(flow), L.ptr(F_init), L.ptr(exclude), P, H, W, int(rounds), float(e_floor), L.ptr(F),
                                  L.ptr(counts), L.ptr(median), L.ptr(inlier), L.ptr(ws), ws.numel(), L.stream()), "sfm refit")
        L.check(lib.gfl_sfm_pose(L.ptr(flow), L.ptr(F), L.ptr(inlier), L.ptr(counts), P, H, W, fx, fy, cx, cy,
                                 float(min_parallax), float(min_share), L.ptr(R), L.ptr(t), L.ptr(votes), L.ptr(parallax),
                                 L.ptr(degenerate), L.ptr(ws), ws.numel(), L.stream()), "sfm pose")
        L.check(lib.gfl_sfm_triangulate(L.ptr(flow), L.ptr(inlier), L.ptr(R), L.ptr(t), L.ptr(degenerate), P, H, W, fx, fy, cx,
                                        cy, L.ptr(rho), L.ptr(weight), L.stream()), "sfm triangulate")
    out = dict(F=F.reshape(P, 3, 3), R=R.reshape(P, 3, 3), t=t, parallax=parallax, degenerate=degenerate != 0, inlier=inlier,
               rho=rho, weight=weight, votes=votes, counts=counts, median=median)
    return {k: v[0] for k, v in out.items()} if single else out


def masked_median(a, b=None, wa=None, wb=None, w_min=0.0):
    """Per row of ``a (M, H, W)`` float32 on the device: the exact lower median of a / b (``b`` None: of a) over the pixels
    with wa > w_min and wb > w_min (None passes) -- (median (M,) float64, NaN for none; count (M,) int32), on the device."""
    M, H, W = a.shape
    _check_shape(M, H, W)
    dev = a.device
    lib = L.load()
    prep = lambda x: None if x is None else x.detach().to(dev, torch.float32).contiguous()
    a, b, wa, wb = prep(a), prep(b), prep(wa), prep(wb)
    med = torch.empty(M, dtype=torch.float64, device=dev)
    cnt = torch.empty(M, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(lib, M, H, W, dev)
        L.check(lib.gfl_sfm_median(L.ptr(a), L.ptr(b), L.ptr(wa), L.ptr(wb), float(w_min), M, H, W, L.ptr(med), L.ptr(cnt),
                                   L.ptr(ws), ws.numel(), L.stream()), "sfm median")
    return med, cnt


def fuse_fill(rho_f, w_f, rho_b, w_b, scale_f, scale_b, *, sweeps=20, lam=0.05, rho_min=1e-6):
    """Stage e for T frames ``(T, H, W)`` float32 on the device: the two inverse depths fused with the scales ``(T,)`` float64
    (1 / baseline), the pull-push fill and ``sweeps`` Jacobi sweeps with lambda = ``lam`` times the exact lower median of the
    frame's positive weights.  Returns dict(depth = 1 / max(rho, rho_min), rho0, weight (T, H, W), pixels (T,) int32 = the
    number of pixels with weight)."""
    T, H, W = rho_f.shape
    _check_shape(T, H, W)
    dev = rho_f.device
    lib = L.load()
    if int(sweeps) != sweeps or sweeps < 0 or not (np.isfinite(lam) and lam >= 0) or not (np.isfinite(rho_min) and rho_min > 0):
        raise ValueError(f"sfm: sweeps >= 0, lam >= 0 and rho_min > 0 are needed, got {sweeps!r}, {lam}, {rho_min}")
    rho0, weight, depth = (torch.empty((T, H, W), dtype=torch.float32, device=dev) for _ in range(3))
    scale_f, scale_b = (s.detach().to(dev, torch.float64).contiguous() for s in (scale_f, scale_b))
    with torch.cuda.device(dev):
        L.check(lib.gfl_sfm_fuse(L.ptr(rho_f), L.ptr(w_f), L.ptr(rho_b), L.ptr(w_b), L.ptr(scale_f), L.ptr(scale_b), T, H, W,
                                 L.ptr(rho0), L.ptr(weight), L.stream()), "sfm fuse")
        med_w, pixels = masked_median(weight, wa=weight)
        lam_t = torch.nan_to_num(med_w * float(lam), nan=0.0).contiguous()
        ws = _workspace(lib, T, H, W, dev)
        L.check(lib.gfl_sfm_fill(L.ptr(rho0), L.ptr(weight), L.ptr(lam_t), T, H, W, int(sweeps), float(rho_min), L.ptr(depth),
                                 L.ptr(ws), ws.numel(), L.stream()), "sfm fill")
    return dict(depth=depth, rho0=rho0, weight=weight, pixels=pixels)


def warn_unreliable(unreliable, median_depth=1.0):
    """the ONE warning that names the frames without any parallax-supported depth"""
    if np.any(unreliable):
        warnings.warn("gflow_amd.sfm: no parallax-supported depth in frame(s) " + ", ".join(str(i) for i in np.flatnonzero(unreliable))
                      + f": they get the constant depth {median_depth}")


def _frame_stacks(tv, n):
    """the pairs' (rho, weight) as the frames see them: frame i's forward pair is i (none for the last frame), its backward
    pair n + i - 1 (none for frame 0)"""
    zero = torch.zeros_like(tv["rho"][:1])
    rf, wf = torch.cat([tv["rho"][:n], zero]), torch.cat([tv["weight"][:n], zero])
    if tv["rho"].shape[0] == n:                                     # (no backward flows)
        return rf, wf, torch.zeros_like(rf), torch.zeros_like(wf)
    rb, wb = torch.cat([zero, tv["rho"][n:]]), torch.cat([zero, tv["weight"][n:]])
    return rf, wf, rb, wb


def clip_depth_camera(fwd, bwd, focal=None, pp=None, exclude_fwd=None, exclude_bwd=None, median_depth=1.0, *, w_min=1e-7,
                      sweeps=20, lam=0.05, rho_min=1e-6, warn=True, **kw):
    """Depth and camera of a clip of T frames from its flows: ``fwd[i]`` is the flow i -> i + 1 on frame i's grid, ``bwd[i]``
    the flow i + 1 -> i on frame i + 1's grid, both ``(T - 1, H, W, 2)`` in pixels; ``exclude_fwd`` / ``exclude_bwd``
    ``(T - 1, H, W)`` masks on the same grids (nonzero: not used for the geometry).  ``bwd`` may be None: the frames then have
    their forward depth alone and no ratio, so every baseline comes from the medians (below).  ``focal`` defaults to max(W, H) -- an
    ASSUMPTION, nothing here estimates it -- and ``pp`` to (round(W / 2), round(H / 2)).  ``kw``: the keywords of ``two_view``.

    Returns dict(depth (T, H, W) float32 and extr (T, 3, 4) float64 world-to-camera on the device, focal, pp, baseline
    (T - 1,) float64 on the device, degenerate (T - 1,) and unreliable (T,) host bool arrays).  extr_0 = I and
    extr_{i+1} = [R_i | b_i t_i] o extr_i; b_i / b_{i-1} is the median ratio of frame i's two inverse depths over the pixels
    where both weights exceed ``w_min``; where there is no ratio, b_i makes the frame's median forward depth equal the
    previous frame's median filled depth.  The global scale makes the median filled depth of the FIRST FRAME THAT HAS WEIGHT
    ``median_depth`` -- frame 0, unless it is unreliable (it then holds the constant, and the scale comes from the next
    frame with parallax; a clip without any keeps its baselines as chained).  A frame
    with no weight anywhere gets the constant ``median_depth`` and is ``unreliable`` (one warning names them, unless ``warn``
    is off: ``warn_unreliable``).

    Every stage is one batched call; the flags are read back ONCE, at the end.  Only a clip with a missing ratio then costs
    more: its scales are settled one missing ratio after the other, each with a batched pass of stage e."""
    fwd = torch.as_tensor(fwd)
    bwd = None if bwd is None else torch.as_tensor(bwd)
    if fwd.dim() != 4 or fwd.shape[-1] != 2 or fwd.shape[0] < 1 or (bwd is not None and fwd.shape != bwd.shape):
        raise ValueError(f"sfm: fwd and bwd must both be (T - 1 >= 1, H, W, 2), got {tuple(fwd.shape)} and "
                         f"{None if bwd is None else tuple(bwd.shape)}")
    if not (np.isfinite(median_depth) and median_depth > 0):
        raise ValueError(f"sfm: median_depth must be finite and > 0, got {median_depth}")
    dev = _device_of(fwd, bwd)
    n, H, W = int(fwd.shape[0]), int(fwd.shape[1]), int(fwd.shape[2])
    T = n + 1
    focal, pp = default_camera(H, W, focal, pp)
    intr = (focal, focal, float(pp[0]), float(pp[1]))
    exclude = None
    if exclude_fwd is not None or (exclude_bwd is not None and bwd is not None):
        zeros = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
        as_mask = lambda m: zeros if m is None else (torch.as_tensor(m).to(dev) != 0).to(torch.uint8)
        exclude = torch.cat([as_mask(exclude_fwd)] + ([] if bwd is None else [as_mask(exclude_bwd)]))
    flows = fwd.detach().to(dev, torch.float32)
    if bwd is not None:
        flows = torch.cat([flows, bwd.detach().to(dev, torch.float32)])
    with torch.cuda.device(dev):
        tv = two_view(flows, intr, exclude, **kw)
        rf, wf, rb, wb = _frame_stacks(tv, n)
        ratio, count = masked_median(rf, rb, wf, wb, w_min)
        inner = torch.zeros(T, dtype=torch.bool, device=dev)
        inner[1:n] = True                                           # the frames 1 .. T - 2 have a ratio
        have = inner & (count > 0) & torch.isfinite(ratio) & (ratio > 0)
        step = torch.where(have, ratio, torch.ones_like(ratio))

        def stage_e(step):
            b = torch.cumprod(step[:n], 0)                          # b_0 = 1 (step[0] = 1), b_i = b_{i-1} step_i
            one = b.new_ones(1)
            res = fuse_fill(rf, wf, rb, wb, torch.cat([1.0 / b, one]), torch.cat([one, 1.0 / b]), sweeps=sweeps, lam=lam,
                            rho_min=rho_min)
            return b, res, masked_median(res["depth"])[0]

        b, res, med_depth = stage_e(step)
        flags = torch.cat([tv["degenerate"][:n].to(torch.int32), have.to(torch.int32), res["pixels"]]).cpu().numpy()
        degenerate, have_h, has = flags[:n] != 0, flags[n:n + T] != 0, flags[n + T:] > 0
        missing = [i for i in range(1, n) if not have_h[i]]
        if missing:
            med_inv = masked_median(torch.ones_like(rf), rf, wf, None, w_min)[0]
            for i in missing:
                prev = max((j for j in range(i) if has[j]), default=None)      # the last frame before i with weight
                carry = med_depth[prev] if prev is not None else med_depth.new_ones(())
                ok = torch.isfinite(med_inv[i]) & (med_inv[i] > 0)
                step = step.clone()
                step[i] = torch.where(ok, carry / med_inv[i] / b[i - 1], torch.ones_like(carry))
                b, res, med_depth = stage_e(step)
        has_d = torch.as_tensor(has, device=dev)
        first = int(np.argmax(has)) if has.any() else None
        scale = float(median_depth) / med_depth[first] if first is not None else med_depth.new_ones(())
        depth = torch.where(has_d[:, None, None], res["depth"] * scale.float(), res["depth"].new_tensor(float(median_depth)))
        baseline = b * scale
        extr = [torch.eye(4, dtype=torch.float64, device=dev)]
        for i in range(n):
            M = torch.eye(4, dtype=torch.float64, device=dev)
            M[:3, :3] = tv["R"][i]
            M[:3, 3] = baseline[i] * tv["t"][i]
            extr.append(M @ extr[-1])
        extr = torch.stack(extr)[:, :3].contiguous()
    unreliable = ~has
    if warn:
        warn_unreliable(unreliable, median_depth)
    return dict(depth=depth, extr=extr, focal=focal, pp=pp, baseline=baseline, degenerate=degenerate, unreliable=unreliable,
                ratio=ratio, count=count, pairs=tv)


# ---------------------------------------------------------------------------------------------------------------- files
def write_depth_camera(result, depth_dir, camera_dir, names, overwrite=False):
    """Write ``<depth_dir>/<name>.npy`` (float32 (H, W)) and ``<camera_dir>/<name>.json`` ({"focal", "pose": 4 x 4
    world-to-camera, "pp"}: what io.read_depth and io.read_camera read) for the frames of a ``clip_depth_camera`` result (or
    any dict with depth (T, H, W), extr (T, 3, 4), focal, pp).  Returns the paths, depth files first."""
    host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    depth, extr = host(result["depth"]).astype(np.float32), host(result["extr"]).astype(np.float64)
    if len(names) != depth.shape[0] or extr.shape[0] != depth.shape[0]:
        raise ValueError(f"sfm: {len(names)} names for {depth.shape[0]} depth maps and {extr.shape[0]} poses")
    targets = [os.path.join(depth_dir, n + ".npy") for n in names] + [os.path.join(camera_dir, n + ".json") for n in names]
    there = [t for t in targets if os.path.exists(t)]
    if there and not overwrite:
        raise FileExistsError(f"{there[0]} exists ({len(there)} of {len(targets)} files do): pass overwrite to replace them")
    os.makedirs(depth_dir, exist_ok=True)
    os.makedirs(camera_dir, exist_ok=True)
    T = depth.shape[0]
    for i, name in enumerate(names):
        np.save(targets[i], depth[i])
        pose = np.eye(4)
        pose[:3] = extr[i]
        with open(targets[T + i], "w") as f:
            json.dump({"focal": float(result["focal"]), "pose": pose.tolist(),
                       "pp": [float(result["pp"][0]), float(result["pp"][1])]}, f)
    return targets


def _read_masks(paths, shape):
    """(len(paths), H, W) bool from mask files of the flows' shape; None when there is none or a shape differs"""
    from .io import read_mask
    if not paths:
        return None
    masks = [read_mask(p) for p in paths]
    if any(tuple(m.shape) != tuple(shape) for m in masks):
        return None
    return torch.stack(masks)


def main(argv=None):
    ap = argparse.ArgumentParser(description="depth and camera of a sequence from its forward and backward flows, written as "
                                             "<img_dir>_depth_mast3r_s2/<name>.npy and <img_dir>_camera_mast3r_s2/<name>.json "
                                             "(classical two-view geometry on the device, not MASt3R)")
    ap.add_argument("--img_dir", type=str, required=True, help="images folder path")
    ap.add_argument("--focal", type=float, default=None, help="focal length in pixels (default: max(W, H), an assumption)")
    ap.add_argument("--overwrite", action="store_true", help="replace files that are already there")
    args = ap.parse_args(argv)
    from . import io as gio
    sp = args.img_dir.rstrip("/")
    p = gio.sequence_paths(sp, frame_range=1 << 30)
    images = p["img"]
    n = len(images) - 1
    if n < 1:
        raise SystemExit(f"{sp}: {len(images)} images (*.png, *.jpg), depth and camera need two")
    if len(p["flow"]) < n or len(p["flow_bwd"]) < n:
        raise SystemExit(f"{sp}: {len(images)} images need {n} forward and {n} backward flows, found {len(p['flow'])} and "
                         f"{len(p['flow_bwd'])} (python -m gflow_amd.optflow makes them)")
    read = lambda fs: [gio._read_flo(f) for f in fs[:n]]
    fwd, bwd = read(p["flow"]), read(p["flow_bwd"])
    if any(f is None for f in fwd + bwd):
        raise SystemExit(f"{sp}: a flow file is not a .flo file")
    fwd, bwd = torch.from_numpy(np.stack(fwd)), torch.from_numpy(np.stack(bwd))
    shape = fwd.shape[1:3]
    move = _read_masks(p["move"][:n], shape) if len(p["move"]) >= n else None
    occ = _read_masks(p["occ"][:n], shape) if len(p["occ"]) >= n else None
    names = [os.path.basename(str(ip)).split(".")[0] for ip in images]
    targets = [os.path.join(sp + "_depth_mast3r_s2", nm + ".npy") for nm in names] + \
              [os.path.join(sp + "_camera_mast3r_s2", nm + ".json") for nm in names]
    there = [t for t in targets if os.path.exists(t)]
    if there and not args.overwrite:
        raise SystemExit(f"{there[0]} exists ({len(there)} of {len(targets)} files do): pass --overwrite to replace them")
    res = clip_depth_camera(fwd, bwd, focal=args.focal, exclude_fwd=move, exclude_bwd=occ)
    write_depth_camera(res, sp + "_depth_mast3r_s2", sp + "_camera_mast3r_s2", names, overwrite=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
