"""Optical flow from the images ("Flows from the images").

What a clip fit reads as ``<seq>_flow_unimatch/*pred.flo`` and ``*pred_bwd.flo`` -- the flow between consecutive frames,
forward and backward -- estimated here instead of by UniMatch's network: a classical coarse-to-fine variational estimate
(grey value constancy with a robust penalty, robust isotropic smoothness, a 5-tap binomial pyramid, Jacobi sweeps), on the
device for all pairs of a clip and both directions in ONE library call (csrc/gfl_optflow.hip: gfl_optflow).  It is NOT
UniMatch and is unpinned against it on real video; include/gflow_hip.h ("optical flow") holds the definition,
tests/optflow_ref.py restates it in float64.  The move masks (gflow_amd.move_seg) and the occlusion masks
(gflow_amd.occlusion) follow from these flows, so a sequence with images, depth and cameras needs nothing else.

    python -m gflow_amd.optflow --img_dir SEQ [--out DIR] [--overwrite] [--alpha 5] [--warps 5] [--outer 3] [--sweeps 50]
                                [--min-side 16]
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _lib as L

MAX_PIXELS = 2 ** 30
DEFAULTS = dict(alpha=5.0, warps=5, outer=3, sweeps=50, min_side=16)
_workspaces = {}                    # device index -> the one cached workspace of that device (grown when a call needs more)


def _workspace(nbytes, device):
    key = torch.device(device).index
    if key not in _workspaces or _workspaces[key].numel() < nbytes:
        _workspaces.pop(key, None)                 # (a clip's workspace is GBs: let go of it before the larger one comes)
        _workspaces[key] = L.scratch(nbytes, device)
    return _workspaces[key]


def _as_images(x, name):
    x = torch.as_tensor(x)
    if x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise ValueError(f"optflow: {name} must be (H, W, 3) or (P, H, W, 3), got {tuple(x.shape)}")
    return x


def _check_params(alpha, warps, outer, sweeps, min_side):
    alpha = float(alpha)
    if not (0.0 < alpha < math.inf):
        raise ValueError(f"optflow: alpha must be finite and > 0, got {alpha}")
    counts = dict(warps=warps, outer=outer, sweeps=sweeps)
    for k, v in counts.items():
        if int(v) != v or v < 1:
            raise ValueError(f"optflow: {k} must be an integer >= 1, got {v!r}")
    if int(min_side) != min_side or min_side < 2:
        raise ValueError(f"optflow: min_side must be an integer >= 2, got {min_side!r}")
    return alpha, int(warps), int(outer), int(sweeps), int(min_side)


def estimate_flow(a, b, *, alpha=5.0, warps=5, outer=3, sweeps=50, min_side=16):
    """The flow a -> b on a's grid, in pixels, of one pair ``(H, W, 3)`` or of P pairs ``(P, H, W, 3)`` (tensors on any
    device, or arrays): uint8 (divided by 255) or float in [0, 1].  Returns a device float32 tensor ``(..., H, W, 2)`` of the
    matching leading shape.  ``alpha``: the weight of the smoothness term; ``warps`` linearisations per pyramid level,
    ``outer`` re-weightings per linearisation, ``sweeps`` Jacobi sweeps per re-weighting; pyramid levels are added while
    half the shorter side is at least ``min_side``.  Everything is enqueued on the current stream; nothing is read back.
    The calls on one device share one workspace: enqueue them on one stream.  A problem's result does not depend on the
    others of its call, and the same inputs give the same bits."""
    a, b = _as_images(a, "a"), _as_images(b, "b")
    if a.shape != b.shape:
        raise ValueError(f"optflow: a is {tuple(a.shape)}, b is {tuple(b.shape)}")
    if (a.dtype == torch.uint8) != (b.dtype == torch.uint8):
        raise ValueError(f"optflow: a is {a.dtype}, b is {b.dtype} (both uint8 or both float)")
    lead = tuple(a.shape[:-1])
    H, W = int(lead[-2]), int(lead[-1])
    P = int(lead[0]) if len(lead) == 3 else 1
    if H < 8 or W < 8 or P < 1 or P * H * W > MAX_PIXELS:
        raise ValueError(f"optflow: {P} pairs of {H} x {W} are refused (H, W >= 8, P >= 1, P H W <= 2^30)")
    alpha, warps, outer, sweeps, min_side = _check_params(alpha, warps, outer, sweeps, min_side)
    if not (a.is_cuda or b.is_cuda or torch.cuda.is_available()):
        raise RuntimeError("gflow_amd.optflow: needs a HIP (cuda) device; there is no CPU fallback")
    dev = a.device if a.is_cuda else b.device if b.is_cuda else torch.device("cuda", torch.cuda.current_device())
    is_u8 = a.dtype == torch.uint8
    dt = torch.uint8 if is_u8 else torch.float32
    a = a.detach().to(dev, dt).contiguous()
    b = b.detach().to(dev, dt).contiguous()
    out = torch.empty(lead + (2,), dtype=torch.float32, device=dev)
    lib = L.load()
    need = lib.gfl_optflow_workspace_bytes(P, H, W, min_side)
    if need == 0:
        raise ValueError(f"optflow: {P} pairs of {H} x {W} with min_side {min_side} are refused by the library")
    with torch.cuda.device(dev):
        ws = _workspace(need, dev)
        L.check(lib.gfl_optflow(L.ptr(a), L.ptr(b), int(is_u8), P, H, W, alpha, warps, outer, sweeps, min_side, L.ptr(out),
                                L.ptr(ws), ws.numel(), L.stream()), "optflow")
    return out


def clip_flows(images, pairs=None, **kw):
    """The flows between consecutive images of a clip, from ONE batched call: ``images`` (T, H, W, 3) (or a list of (H, W, 3)),
    uint8 or float.  Returns ``(fwd, bwd)``, device tensors (T - 1, H, W, 2): ``fwd[i]`` is the flow i -> i + 1 on image i's
    grid, ``bwd[i]`` the flow i + 1 -> i on image i + 1's grid.  ``pairs``: only these i, in this order (the result then has
    len(pairs) rows).  ``kw``: the keywords of ``estimate_flow``."""
    if not torch.is_tensor(images):
        images = torch.stack([torch.as_tensor(im) for im in images])
    if images.dim() != 4 or images.shape[-1] != 3 or images.shape[0] < 2:
        raise ValueError(f"optflow: a clip must be (T >= 2, H, W, 3), got {tuple(images.shape)}")
    T = int(images.shape[0])
    idx = list(range(T - 1)) if pairs is None else [int(i) for i in pairs]
    if any(i < 0 or i >= T - 1 for i in idx):
        raise ValueError(f"optflow: pairs must lie in 0 .. {T - 2}")
    n = len(idx)
    if n == 0:
        dev = images.device if images.is_cuda else torch.device("cuda", torch.cuda.current_device())
        empty = torch.empty((0,) + tuple(images.shape[1:3]) + (2,), dtype=torch.float32, device=dev)
        return empty, empty.clone()
    first = torch.as_tensor(idx, device=images.device)
    a, b = images.index_select(0, first), images.index_select(0, first + 1)
    flow = estimate_flow(torch.cat([a, b]), torch.cat([b, a]), **kw)
    return flow[:n], flow[n:]


def _decode(path):
    """(H, W, 3): uint8 as PIL reads an 8-bit file, else float32 in [0, 1] (io.image_path_to_tensor's conversion)"""
    from .io import _decode_image
    img, div = _decode_image(path)
    if img.shape[-1] == 1:
        img = np.repeat(img, 3, axis=-1)
    elif img.shape[-1] != 3:
        raise ValueError(f"optflow: {path} has {img.shape[-1]} channels")
    return img if img.dtype == np.uint8 else (img / np.float32(div)).astype(np.float32)


def pair_flows(image_paths, pairs=None, device=None, **kw):
    """``clip_flows`` of the image files ``image_paths`` (in clip order, all of one shape): only the images that the pairs
    touch are decoded.  Returns ``(fwd, bwd)`` on ``device`` (default: the current HIP device)."""
    paths = list(image_paths)
    idx = list(range(len(paths) - 1)) if pairs is None else [int(i) for i in pairs]
    if any(i < 0 or i >= len(paths) - 1 for i in idx):
        raise ValueError(f"optflow: pairs must lie in 0 .. {len(paths) - 2}")
    if not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.optflow: needs a HIP (cuda) device; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    used = sorted({i for i in idx} | {i + 1 for i in idx})
    if not used:
        return clip_flows(torch.zeros(2, 8, 8, 3, device=dev), pairs=[], **kw)
    where = {i: j for j, i in enumerate(used)}
    arrays = [_decode(paths[i]) for i in used]
    if len({(a.shape, a.dtype.str) for a in arrays}) != 1:
        raise ValueError("optflow: the images of a sequence must have one shape and one bit depth")
    stack = torch.from_numpy(np.stack(arrays)).to(dev)
    return clip_flows(stack, pairs=[where[i] for i in idx], **kw)       # (i and i + 1 are neighbours in the stack too)


def main(argv=None):
    ap = argparse.ArgumentParser(description="forward and backward optical flow of a sequence's consecutive images, written as "
                                             "<img_dir>_flow_unimatch/<name>_pred.flo and <name>_pred_bwd.flo (a classical "
                                             "variational estimate on the device, not UniMatch)")
    ap.add_argument("--img_dir", type=str, required=True, help="images folder path")
    ap.add_argument("--out", type=str, default=None, help="where the flows go (default: <img_dir>_flow_unimatch)")
    ap.add_argument("--overwrite", action="store_true", help="replace flows that are already there")
    ap.add_argument("--alpha", type=float, default=DEFAULTS["alpha"], help="weight of the smoothness term")
    ap.add_argument("--warps", type=int, default=DEFAULTS["warps"], help="linearisations per pyramid level")
    ap.add_argument("--outer", type=int, default=DEFAULTS["outer"], help="re-weightings per linearisation")
    ap.add_argument("--sweeps", type=int, default=DEFAULTS["sweeps"], help="Jacobi sweeps per re-weighting")
    ap.add_argument("--min-side", type=int, default=DEFAULTS["min_side"],
                    help="pyramid levels are added while half the shorter side is at least this")
    args = ap.parse_args(argv)
    from . import io as gio
    sp = args.img_dir.rstrip("/")
    out_dir = args.out or sp + "_flow_unimatch"
    images = gio.sequence_paths(sp, frame_range=1 << 30)["img"]               # every image, not the fit's slice
    if len(images) < 2:
        raise SystemExit(f"{sp}: {len(images)} images (*.png, *.jpg), a flow needs two")
    names = [os.path.basename(str(p)).split(".")[0] for p in images[:-1]]
    targets = [os.path.join(out_dir, f"{n}_{k}.flo") for n in names for k in ("pred", "pred_bwd")]
    there = [t for t in targets if os.path.exists(t)]
    if there and not args.overwrite:
        raise SystemExit(f"{there[0]} exists ({len(there)} of {len(targets)} flows do): pass --overwrite to replace them")
    fwd, bwd = pair_flows(images, alpha=args.alpha, warps=args.warps, outer=args.outer, sweeps=args.sweeps,
                          min_side=args.min_side)
    fwd, bwd = fwd.cpu().numpy(), bwd.cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    for i, n in enumerate(names):
        gio.write_flow(os.path.join(out_dir, n + "_pred.flo"), fwd[i])
        gio.write_flow(os.path.join(out_dir, n + "_pred_bwd.flo"), bwd[i])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
