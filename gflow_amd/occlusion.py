"""Occlusion masks from the forward and the backward flow ("Occlusion masks from the flows").

What UniMatch writes under ``--pred_bidir_flow --fwd_bwd_check`` for every pair of frames: a pixel is occluded where the
flow a -> b and the flow b -> a, sampled where the first one points, do not cancel --
``|a + S(bwd, x + a)| > alpha (|a| + |b|) + beta``.  ``<name>_occ_bwd.png`` of pair i is the ``occ_mask`` a clip fit reads
for frame i + 1 (the occlusion-driven densification samples from it).

Here the check runs on the device (csrc/gfl_occ.hip: gfl_flow_occlusion, one launch for all pairs and both directions).
The definition, its defaults alpha = 0.01, beta = 0.5 and the file name ``*pred_bwd.flo`` are UniMatch's as recalled and
unpinned: that code cannot be observed here.  tests/occ_ref.py restates the check in float64.

    python -m gflow_amd.occlusion --img_dir SEQ [--out DIR] [--alpha 0.01] [--beta 0.5] [--overwrite]
"""
import argparse
import os

import torch

from . import _lib as L

MAX_PIXELS = 2 ** 30


def _as_flow(flow, name):
    flow = torch.as_tensor(flow)
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError(f"occlusion: {name} must be (H, W, 2) or (P, H, W, 2), got {tuple(flow.shape)}")
    return flow


def flow_occlusion(fwd, bwd, *, alpha=0.01, beta=0.5, maps=False):
    """The forward-backward check of one pair ``(H, W, 2)`` or of P pairs ``(P, H, W, 2)`` (tensors on any device, or
    arrays): ``fwd[p]`` is the flow a -> b on a's grid, ``bwd[p]`` the flow b -> a on b's grid, in pixels.  Returns device
    tensors of the matching leading shape: dict(occ, occ_bwd (..., H, W) uint8 0 / 255) -- occ on a's grid, occ_bwd on b's
    -- and with ``maps`` also dict(diff, diff_bwd (..., H, W) float32), the two differences.  A pixel whose difference or
    threshold is not finite is 0 in both.  Everything is enqueued on the current stream; nothing is read back."""
    fwd, bwd = _as_flow(fwd, "fwd"), _as_flow(bwd, "bwd")
    if fwd.shape != bwd.shape:
        raise ValueError(f"occlusion: fwd is {tuple(fwd.shape)}, bwd is {tuple(bwd.shape)}")
    lead = tuple(fwd.shape[:-1])
    H, W = int(lead[-2]), int(lead[-1])
    P = int(lead[0]) if len(lead) == 3 else 1
    if H < 2 or W < 2 or P < 1 or P * H * W > MAX_PIXELS:
        raise ValueError(f"occlusion: {P} pairs of {H} x {W} are refused (H, W >= 2, P >= 1, P H W <= 2^30)")
    alpha, beta = float(alpha), float(beta)
    if not (0.0 <= alpha < float("inf") and 0.0 <= beta < float("inf")):
        raise ValueError(f"occlusion: alpha and beta must be finite and not negative, got {alpha}, {beta}")
    if not (fwd.is_cuda or bwd.is_cuda or torch.cuda.is_available()):
        raise RuntimeError("gflow_amd.occlusion: needs a HIP (cuda) device; there is no CPU fallback")
    dev = fwd.device if fwd.is_cuda else bwd.device if bwd.is_cuda else torch.device("cuda", torch.cuda.current_device())
    fwd = fwd.detach().to(dev, torch.float32).contiguous()
    bwd = bwd.detach().to(dev, torch.float32).contiguous()
    out = dict(occ=torch.empty(lead, dtype=torch.uint8, device=dev), occ_bwd=torch.empty(lead, dtype=torch.uint8, device=dev))
    if maps:
        out.update(diff=torch.empty(lead, dtype=torch.float32, device=dev),
                   diff_bwd=torch.empty(lead, dtype=torch.float32, device=dev))
    lib = L.load()
    with torch.cuda.device(dev):
        L.check(lib.gfl_flow_occlusion(L.ptr(fwd), L.ptr(bwd), P, W, H, alpha, beta, L.ptr(out.get("diff")),
                                       L.ptr(out.get("diff_bwd")), L.ptr(out["occ"]), L.ptr(out["occ_bwd"]), L.stream()),
                "flow occlusion")
    return out


def clip_occ_masks(frames, bwd_flows, fwd_flows=None, resize=None, **kw):
    """Fill ``fr["occ_mask"]`` of the frames 1 .. from the flows: ``bwd_flows[i]`` is the flow i + 1 -> i on frame i + 1's
    grid (None: there is none), the forward flow of pair i is ``fwd_flows[i]``, by default ``frames[i]["flow"]``.  ONE batched
    call for the whole clip; frame i + 1 gets occ_bwd of pair i as (H, W, 1) float32 in {0, 1} on the device of its image
    -- what io.image_path_to_tensor makes of a written ``*_occ_bwd.png``.  A frame whose pair lacks a flow is left as it is.
    ``resize``: the mask is resized as io.load_sequence resizes a mask file (the check itself must see the flows at their
    native resolution: resizing a flow does not rescale its values).  ``kw``: alpha, beta.  Returns ``frames``."""
    from .io import _resize_chw
    if fwd_flows is None:
        fwd_flows = [fr.get("flow") for fr in frames]
    pairs = [i for i in range(min(len(frames) - 1, len(bwd_flows), len(fwd_flows)))
             if bwd_flows[i] is not None and fwd_flows[i] is not None]
    if not pairs:
        return frames
    fwd = torch.stack([torch.as_tensor(fwd_flows[i]).float() for i in pairs])
    bwd = torch.stack([torch.as_tensor(bwd_flows[i]).float().to(fwd.device) for i in pairs])
    occ = flow_occlusion(fwd, bwd, **kw)["occ_bwd"]
    for j, i in enumerate(pairs):
        image = torch.as_tensor(frames[i + 1]["image"])
        m = (occ[j] != 0).to(image.device, torch.float32).unsqueeze(0)
        frames[i + 1]["occ_mask"] = _resize_chw(m, resize).permute(1, 2, 0)
    return frames


def write_masks(result, out_dir, name, overwrite=False):
    """Write ``<out_dir>/<name>_occ.png`` and ``<name>_occ_bwd.png`` (mode L, 0 / 255) from one pair's ``flow_occlusion``;
    an existing file is replaced only with ``overwrite``.  Returns the two paths."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    paths = [os.path.join(out_dir, f"{name}_{k}.png") for k in ("occ", "occ_bwd")]
    for p in paths:
        if os.path.exists(p) and not overwrite:
            raise FileExistsError(f"{p} exists (pass --overwrite to replace it)")
    for p, k in zip(paths, ("occ", "occ_bwd")):
        m = torch.as_tensor(result[k]).detach().cpu().numpy()
        Image.fromarray(((m != 0) * 255).astype("uint8")).save(p)          # (2-D uint8: mode L)
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description="occlusion masks of a prepared sequence from its forward and backward flows "
                                             "(<img_dir>_flow_unimatch/*pred.flo, *pred_bwd.flo)")
    ap.add_argument("--img_dir", type=str, required=True, help="images folder path")
    ap.add_argument("--out", type=str, default=None, help="where the masks go (default: <img_dir>_flow_unimatch)")
    ap.add_argument("--alpha", type=float, default=0.01, help="threshold = alpha (|fwd| + |bwd|) + beta")
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--overwrite", action="store_true", help="replace masks that are already there")
    args = ap.parse_args(argv)
    from . import io as gio
    sp = args.img_dir.rstrip("/")
    out_dir = args.out or sp + "_flow_unimatch"
    # every flow file, not the fit's slice of them (io.sequence_paths drops the last image's)
    p = gio.sequence_paths(sp, frame_range=1 << 30)
    if len(p["flow"]) != len(p["flow_bwd"]):
        raise SystemExit(f"{sp}_flow_unimatch: {len(p['flow'])} forward flows (*pred.flo) but {len(p['flow_bwd'])} backward "
                         "flows (*pred_bwd.flo)")
    if not p["flow"]:
        raise SystemExit(f"{sp}_flow_unimatch: no *pred.flo")
    names = [os.path.basename(str(f))[:-len("pred.flo")].rstrip("_") for f in p["flow"]]
    targets = [os.path.join(out_dir, f"{n}_{k}.png") for n in names for k in ("occ", "occ_bwd")]
    there = [t for t in targets if os.path.exists(t)]
    if there and not args.overwrite:
        raise SystemExit(f"{there[0]} exists ({len(there)} of {len(targets)} masks do): pass --overwrite to replace them")
    if not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.occlusion needs a HIP device (there is no CPU fallback)")
    flows = []
    for fp in list(p["flow"]) + list(p["flow_bwd"]):
        flow = gio.read_flow(fp)
        if flow is None:
            raise SystemExit(f"{fp}: not a .flo file")
        flows.append(flow)
    n = len(names)
    res = flow_occlusion(torch.stack(flows[:n]), torch.stack(flows[n:]), alpha=args.alpha, beta=args.beta)
    for i, name in enumerate(names):
        write_masks({k: res[k][i] for k in ("occ", "occ_bwd")}, out_dir, name, overwrite=args.overwrite)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
