"""Frame preparation on the device ("Frame preparation").

What the reference's readers do to every decoded file of a sequence -- to float, ``Resize(n, antialias=True)``, optionally
``GaussianBlur(7, 5.0)``, then depth's scale and offset or the mask test (gflow/utils/conversion.py:6-19, read.py:7-70) --
for a whole stack of frames in one library call (csrc/gfl_prep.hip: gfl_prep_frames).  The resize is torchvision's filter with
weights formed in float64 (include/gflow_hip.h, "frame preparation", holds the definition); torch's CPU kernel is the same
filter with float32 weights, so values agree to a few 1e-6 and masks at non-dyadic scales in all but 1-3 % of their pixels.
tests/prep_ref.py restates the definition in float64.
"""
import math

import torch

from . import _lib as L

MAX_FRAMES_PER_CALL = 16            # a long batch is cut into calls of this many frames: the workspace stays that small
MAX_EXTENT = 16384
_workspaces = {}                    # device index -> the one cached workspace of that device (grown when a call needs more)


def out_shape(h, w, resize):
    """(H', W') of torchvision.transforms.Resize(resize): the shorter side becomes ``resize`` (io._resize_chw)."""
    if resize is None:
        return int(h), int(w)
    if h <= w:
        return int(resize), int(resize * w / h)
    return int(resize * h / w), int(resize)


def _workspace(nbytes, device):
    key = torch.device(device).index
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[key] = L.scratch(nbytes, device)
    return ws


def prep_frames(src, resize=None, *, div=1.0, mul=1.0, add=0.0, blur=False, blur_kernel_size=7, blur_sigma=5.0,
                as_mask=False):
    """Prepare a stack of decoded frames on the device.  ``src``: a contiguous device tensor (T, H, W, C), (H, W, C) or
    (H, W), uint8 or float32, C <= 4.  In this order: ``v = src / div``; the antialiased resize of the shorter side to
    ``resize`` (None or a size that changes nothing: skipped); with ``blur`` the Gaussian blur (reflect padding); then
    ``v * mul + add`` -- or with ``as_mask`` the test "sum over the channels > 0".  Returns float32 of src's rank, or with
    ``as_mask`` a bool tensor without the channel axis ((T, H', W'); (H', W') for a single frame).  Enqueued on the current
    stream; nothing is read back.  The calls on one device share one workspace: enqueue them on one stream.  ValueError for
    what the library would refuse; no CPU fallback."""
    if not torch.is_tensor(src) or src.dtype not in (torch.uint8, torch.float32):
        raise ValueError("prep_frames: src must be a uint8 or float32 tensor")
    if src.dim() not in (2, 3, 4):
        raise ValueError(f"prep_frames: src must be (T, H, W, C), (H, W, C) or (H, W), got {tuple(src.shape)}")
    if not src.is_contiguous():
        raise ValueError("prep_frames: src must be contiguous")
    rank = src.dim()
    x = src if rank == 4 else src.unsqueeze(0) if rank == 3 else src.unsqueeze(0).unsqueeze(-1)
    T, Hs, Ws, C = (int(v) for v in x.shape)
    if resize is not None and (int(resize) != resize or not 1 <= resize <= MAX_EXTENT):
        raise ValueError(f"prep_frames: resize must be an integer in 1 .. {MAX_EXTENT}, got {resize!r}")
    Hd, Wd = out_shape(Hs, Ws, resize) if min(Hs, Ws) >= 1 else (0, 0)
    div, mul, add, blur_sigma = float(div), float(mul), float(add), float(blur_sigma)
    k = int(blur_kernel_size) if blur else 0
    if blur and (k != blur_kernel_size or k < 3 or k > 31 or k % 2 == 0 or not (0.0 < blur_sigma < math.inf)):
        raise ValueError(f"prep_frames: blur needs an odd kernel size in 3 .. 31 and a finite sigma > 0, got "
                         f"{blur_kernel_size!r}, {blur_sigma!r}")
    if not (0.0 < div < math.inf and math.isfinite(mul) and math.isfinite(add)):
        raise ValueError(f"prep_frames: div must be finite and > 0, mul and add finite; got {div}, {mul}, {add}")
    if as_mask and (blur or mul != 1.0 or add != 0.0):
        raise ValueError("prep_frames: as_mask takes no blur, mul or add")
    lib = L.load()
    chunk = min(T, MAX_FRAMES_PER_CALL)
    need = lib.gfl_prep_workspace_bytes(chunk, C, Hs, Ws, Hd, Wd, k) if T >= 1 else 0
    if need == 0:
        raise ValueError(f"prep_frames: {T} frames of {Hs} x {Ws} x {C} to {Hd} x {Wd}" + (f" with a blur of {k}" if k else "")
                         + f" are refused (T >= 1, C <= 4, extents 1 .. {MAX_EXTENT}, at most 64 to 1, 2^31 - 1 elements per "
                         "call, blur_kernel_size / 2 < min(H', W'))")
    if not src.is_cuda:
        raise RuntimeError("gflow_amd.prep: tensors must be on a HIP (cuda) device; there is no CPU fallback")
    dev = src.device
    if as_mask:
        out = torch.empty((T, Hd, Wd), dtype=torch.uint8, device=dev)
    else:
        out = torch.empty((T, Hd, Wd, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(need, dev)
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)                 # (a shorter last call needs no more workspace than a full one)
            L.check(lib.gfl_prep_frames(L.ptr(x[t0:t0 + n]), int(src.dtype == torch.uint8), n, C, Hs, Ws, Hd, Wd, div, mul, add,
                                        k, blur_sigma, int(bool(as_mask)), L.ptr(out[t0:t0 + n]), L.ptr(ws), ws.numel(),
                                        L.stream()), "prep_frames")
    if as_mask:
        out = out.view(torch.bool)
        return out if rank == 4 else out[0]
    return out if rank == 4 else out[0] if rank == 3 else out[0, ..., 0]
