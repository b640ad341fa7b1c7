"""Move masks from the flow ("Move masks from the flow").

What the reference's ``utility/move_seg.py`` prepares for every frame of a sequence -- the only preprocessing step that
is not a neural network: a fundamental matrix fitted to the forward flow by least median of squares, the per-pixel Sampson
error normalised by its maximum, its threshold, and the opened / eroded / dilated masks, written as
``<seq>_epipolar/<name>_{epipolar_error,open,erode,dilate}.png``.  The ``_open`` mask is the ``move_mask`` a clip fit
reads.

Here the fit and the mask run on the device (csrc/gfl_epi.hip: gfl_epi_fundamental, gfl_epi_mask).  The LMedS is this
project's own and deterministic -- K hypotheses of eight pixels drawn on the host from ``numpy.random.default_rng(seed)``,
each scored by the exact lower median of its Sampson errors -- and is unpinned against cv2.findFundamentalMat, whose
sampler cannot be observed here; the morphology is skimage's as recalled, unpinned too.  tests/move_seg_ref.py restates
both in float64 numpy.

    python -m gflow_amd.move_seg --img_dir SEQ [--threshold 0.01] [--hypotheses 512] [--seed 0]
"""
import argparse
import os

import numpy as np
import torch

from . import _lib as L

SUFFIXES = ("epipolar_error", "open", "erode", "dilate")
MAX_HYPOTHESES = 65535


def _check_flow(flow):
    shape = tuple(getattr(flow, "shape", ()))
    if len(shape) != 3 or shape[2] != 2:
        raise ValueError(f"move_seg: flow must be (H, W, 2), got {shape}")
    H, W = int(shape[0]), int(shape[1])
    if H < 2 or W < 2 or H * W < 8 or H * W > 2 ** 30:
        raise ValueError(f"move_seg: an image of {H} x {W} is refused (H, W >= 2 and 8 <= H W <= 2^30)")
    return H, W


def known_pixels(flow):
    """(H W,) bool: the pixels whose correspondence is finite in float32 (include/gflow_hip.h: a flow that is not finite, or
    so large that 2 flow overflows, is unknown)."""
    f = np.asarray(torch.as_tensor(flow).detach().cpu(), dtype=np.float32)
    H, W = f.shape[:2]
    f32 = np.float32
    xx = (f32(2) * (np.arange(W, dtype=f32) + f32(0.5))) / f32(W) - f32(1)
    yy = (f32(2) * (np.arange(H, dtype=f32) + f32(0.5))) / f32(H) - f32(1)
    with np.errstate(over="ignore", invalid="ignore"):
        x2 = xx[None, :] + (f32(2) * f[..., 0]) / f32(W - 1)
        y2 = yy[:, None] + (f32(2) * f[..., 1]) / f32(H - 1)
    return (np.isfinite(x2) & np.isfinite(y2)).reshape(-1)


def draw_samples(known, hypotheses=512, seed=0):
    """(hypotheses, 8) int32: eight distinct known pixels per hypothesis from numpy.random.default_rng(seed) -- every row
    is eight draws with replacement from the known pixels, drawn again while two of them are equal."""
    known = np.asarray(known, dtype=bool).reshape(-1)
    idx = np.flatnonzero(known)
    if idx.size < 8:
        raise ValueError(f"move_seg: {idx.size} known pixels, a hypothesis needs 8")
    K = int(hypotheses)
    if K < 1 or K > MAX_HYPOTHESES:
        raise ValueError(f"move_seg: hypotheses must be in [1, {MAX_HYPOTHESES}], got {hypotheses}")
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, idx.size, size=(K, 8))
    while True:
        s = np.sort(rows, axis=1)
        again = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
        if again.size == 0:
            break
        rows[again] = rng.integers(0, idx.size, size=(again.size, 8))
    return idx[rows].astype(np.int32)


def epipolar_move_mask(flow, *, hypotheses=512, seed=0, threshold=0.01, samples=None):
    """The move mask of one frame from its forward flow ``(H, W, 2)`` (tensor on any device, or array).  Returns device
    tensors: dict(F (3, 3) float64, best () int32, median () float64, err_norm (H, W) float32, mask, open, erode, dilate
    (H, W) uint8 0 / 255).  ``samples``: (K, 8) pixel indices y W + x, else ``draw_samples`` of the known pixels.
    Everything is enqueued on the current stream; nothing is read back."""
    H, W = _check_flow(flow)
    if not np.isfinite(threshold):
        raise ValueError(f"move_seg: threshold must be finite, got {threshold}")
    if samples is None:
        samples = draw_samples(known_pixels(flow), hypotheses, seed)
    samples = np.ascontiguousarray(np.asarray(samples.cpu() if torch.is_tensor(samples) else samples), dtype=np.int32)
    if samples.ndim != 2 or samples.shape[1] != 8 or not 1 <= samples.shape[0] <= MAX_HYPOTHESES:
        raise ValueError(f"move_seg: samples must be (K, 8) with 1 <= K <= {MAX_HYPOTHESES}, got {samples.shape}")
    K = samples.shape[0]
    flow = torch.as_tensor(flow)
    if not flow.is_cuda and not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.move_seg: needs a HIP (cuda) device; there is no CPU fallback")
    dev = flow.device if flow.is_cuda else torch.device("cuda", torch.cuda.current_device())
    flow = flow.detach().to(dev, torch.float32).contiguous()
    smp = torch.tensor(samples, device=dev)
    lib = L.load()
    ws = L.scratch(lib.gfl_epi_workspace_bytes(W, H, K), dev)
    F = torch.empty(9, dtype=torch.float64, device=dev)
    med = torch.empty(K, dtype=torch.float64, device=dev)
    best = torch.empty(1, dtype=torch.int32, device=dev)
    err_norm = torch.empty((H, W), dtype=torch.float32, device=dev)
    mask, opened, eroded, dilated = (torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(4))
    with torch.cuda.device(dev):
        L.check(lib.gfl_epi_fundamental(L.ptr(flow), W, H, L.ptr(smp), K, None, L.ptr(med), L.ptr(F), L.ptr(best), L.ptr(ws),
                                        ws.numel(), L.stream()), "epi fundamental")
        L.check(lib.gfl_epi_mask(L.ptr(flow), W, H, L.ptr(F), float(threshold), L.ptr(err_norm), L.ptr(mask), L.ptr(opened),
                                 L.ptr(eroded), L.ptr(dilated), L.ptr(ws), ws.numel(), L.stream()), "epi mask")
        best = best.reshape(())
        median = torch.where(best >= 0, med[best.clamp(min=0).long()], med.new_tensor(float("inf")))
    return dict(F=F.reshape(3, 3), best=best, median=median, err_norm=err_norm, mask=mask, open=opened, erode=eroded,
                dilate=dilated)


def clip_move_masks(frames, n_flows=None, **kw):
    """Fill ``fr["move_mask"]`` (the opened mask, bool, on the device of the frame's image) of the first ``n_flows`` frames
    from ``fr["flow"]``; the others keep zeros.  Default: the frames 0 .. T - 2 -- the last frame of a clip has no forward
    flow (io.load_sequence passes the number of flow files: the reference's file lists drop the last image, so every frame
    it loads may have one).  ``kw``: the keywords of ``epipolar_move_mask``.  Returns ``frames``."""
    n_flows = len(frames) - 1 if n_flows is None else min(int(n_flows), len(frames))
    for i, fr in enumerate(frames):
        image = torch.as_tensor(fr["image"])
        if i < n_flows:
            mm = epipolar_move_mask(fr["flow"], **kw)["open"] != 0
        else:
            mm = torch.zeros(image.shape[:2], dtype=torch.bool)
        fr["move_mask"] = mm.to(image.device)
    return frames


def result_images(result):
    """{suffix: (H, W) uint8 array} with the reference's byte conversions (move_seg.py:242-259): the error image is
    (err_norm * 255.0) in float32, truncated; a mask is 0 or 255."""
    host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    out = {"epipolar_error": (host(result["err_norm"]).astype(np.float32) * np.float32(255.0)).astype(np.uint8)}
    for k in ("open", "erode", "dilate"):
        out[k] = ((host(result[k]) != 0) * 255.0).astype(np.uint8)
    return out


def write_result(result, out_dir, name):
    """Write ``<out_dir>/<name>_{epipolar_error,open,erode,dilate}.png``; returns the paths in SUFFIXES' order."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    images = result_images(result)
    paths = []
    for k in SUFFIXES:
        paths.append(os.path.join(out_dir, f"{name}_{k}.png"))
        Image.fromarray(images[k]).save(paths[-1])
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description="move masks of a prepared sequence from its forward flows (<img_dir>_epipolar)")
    ap.add_argument("--img_dir", type=str, required=True, help="images folder path")
    ap.add_argument("--threshold", type=float, default=0.01, help="epipolar error threshold for motion mask")
    ap.add_argument("--hypotheses", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.move_seg needs a HIP device (there is no CPU fallback)")
    from . import io as gio
    sp = args.img_dir.rstrip("/")
    p = gio.sequence_paths(sp)
    if len(p["flow"]) != len(p["img"]):
        raise SystemExit(f"{sp}: {len(p['img']) + 1} images need {len(p['img'])} forward flows, found {len(p['flow'])}")
    for ip, fp in zip(p["img"], p["flow"]):
        flow = gio.read_flow(fp)
        if flow is None:
            raise SystemExit(f"{fp}: not a .flo file")
        res = epipolar_move_mask(flow, hypotheses=args.hypotheses, seed=args.seed, threshold=args.threshold)
        write_result(res, sp + "_epipolar", os.path.splitext(os.path.basename(ip))[0])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
