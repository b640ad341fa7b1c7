"""Readers for a prepared GFlow sequence and a writer that lays a clip out the same way.

Mirrors ``gflow/utils/read.py`` and ``gflow/utils/conversion.py`` and the directory convention of
``gflow/fit_video.py:79-96``: next to the image folder ``<seq>/`` sit

    <seq>_depth_mast3r_s2/*.npy      per-frame depth                     (read.py:60-70)
    <seq>_flow_unimatch/*pred.flo    forward flow i -> i+1, Middlebury    (read.py:7-38)
    <seq>_flow_unimatch/*occ_bwd.png occlusion mask of frame i+1          (fit_video.py:88-89,248)
    <seq>_flow_unimatch/*pred_bwd.flo backward flow i+1 -> i (optional; UniMatch's name as recalled: gflow_amd.occlusion)
                                     (both kinds of .flo can be made from the images: gflow_amd.optflow)
    <seq>_epipolar/*_open.png        move mask                           (fit_video.py:96-97)
    <seq>_camera_mast3r_s2/*.json    {"focal", "pp", "pose"}              (read.py:72-89)
    <seq>_mask/*.png                 object ids per pixel (DAVIS annotations; fit_video.py's mask prompt; optional)

A clip can also be ONE video file: a ``sequence_path`` that is a file ending in ``.avi`` (Motion-JPEG, as gflow_amd.video
writes it) stands for the folder of its frames, named ``frame_00000``, ``frame_00001``, ...; the sibling folders are then
``<path without .avi>_flow_unimatch`` and so on.  Its frames are decoded on the device (gflow_amd.video.read_avi_frames).

``Resize(n, antialias=True)`` of torchvision (shorter side to n, bilinear with antialiasing) is
``torch.nn.functional.interpolate(..., mode="bilinear", antialias=True)``; imageio / torchvision are
not needed, PIL reads and writes the PNGs.
"""
import json
import os
import warnings
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

FLO_MAGIC = 202021.25


def _resize_target(h, w, resize):
    """the size torchvision.transforms.Resize(int) gives an (h, w) image: the shorter side becomes ``resize``"""
    if resize is None:
        return h, w
    return (resize, int(resize * w / h)) if h <= w else (int(resize * h / w), resize)


def _resize_chw(t, resize):
    """torchvision.transforms.Resize(int, antialias=True) on a (C,H,W) float tensor."""
    _, h, w = t.shape
    nh, nw = _resize_target(h, w, resize)
    if (nh, nw) == (h, w):
        return t
    return F.interpolate(t.unsqueeze(0), size=(nh, nw), mode="bilinear", antialias=True, align_corners=False).squeeze(0)


def _blur_chw(t, blur, kernel_size=7, sigma=5.0):
    """torchvision.transforms.GaussianBlur(kernel_size, sigma) on a (C,H,W) float tensor: reflect padding, then the
    outer-product kernel as a grouped conv2d (the reference's ``blur`` option: conversion.py:13-14, read.py:32-33)."""
    if not blur:
        return t
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k1 = (pdf / pdf.sum()).to(t.dtype)
    k2 = torch.mm(k1[:, None], k1[None, :]).expand(t.shape[0], 1, kernel_size, kernel_size)
    r = kernel_size // 2
    return F.conv2d(F.pad(t.unsqueeze(0), [r, r, r, r], mode="reflect"), k2, groups=t.shape[0]).squeeze(0)


def _image_div(dtype):
    if isinstance(dtype, torch.dtype):             # (decoded on the device: uint8)
        return 255.0 if dtype == torch.uint8 else 1.0
    return 255.0 if dtype == np.uint8 else 65535.0 if dtype == np.uint16 else 1.0


def image_path_to_tensor(image_path, resize=None, blur=False):
    """conversion.py:6-19 -> (H,W,3) float in [0,1]."""
    from PIL import Image
    img = np.asarray(Image.open(image_path))
    t = torch.from_numpy(img.copy())
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    t = t.permute(2, 0, 1).float() / _image_div(img.dtype)
    return _blur_chw(_resize_chw(t, resize), blur).permute(1, 2, 0)[..., :3]


def _read_flo(fn):
    """The (h, w, 2) float32 array of a Middlebury .flo file (little endian); None on a bad magic number."""
    with open(fn, "rb") as f:
        magic = np.fromfile(f, np.float32, count=1)
        if magic.size != 1 or magic[0] != np.float32(FLO_MAGIC):
            print("Magic number incorrect. Invalid .flo file")
            return None
        w = int(np.fromfile(f, np.int32, count=1)[0])
        h = int(np.fromfile(f, np.int32, count=1)[0])
        data = np.fromfile(f, np.float32, count=2 * w * h)
    return np.resize(data, (h, w, 2)).copy()


def _flow_to_tensor(flow, resize=None, blur=False):
    """what read_flow makes of a file's (h, w, 2) array (None stays None): the resize does not rescale the values"""
    if flow is None:
        return None
    return _blur_chw(_resize_chw(torch.from_numpy(flow).permute(2, 0, 1), resize), blur).permute(1, 2, 0)


def read_flow(fn, resize=None, blur=False):
    """read.py:7-38: Middlebury .flo (little endian) -> (H,W,2); None on a bad magic number."""
    return _flow_to_tensor(_read_flo(fn), resize, blur)


def write_flow(fn, flow):
    flow = np.asarray(flow, dtype=np.float32)
    h, w, _ = flow.shape
    with open(fn, "wb") as f:
        np.array([FLO_MAGIC], np.float32).tofile(f)
        np.array([w, h], np.int32).tofile(f)
        flow.tofile(f)


def read_mask(mask_path, resize=None):
    """read.py:41-57 -> (H,W) bool (any non-zero channel)."""
    from PIL import Image
    mask = np.asarray(Image.open(mask_path))
    if mask.ndim == 3:
        t = torch.tensor(mask.copy(), dtype=torch.float32).permute(2, 0, 1)
    elif mask.ndim == 2:
        t = torch.tensor(mask.copy(), dtype=torch.float32).unsqueeze(0)
    else:
        raise ValueError("The mask should be 2D or 3D")
    t = _resize_chw(t, resize)
    if t.shape[-1] > 1:
        t = t.sum(dim=0)
    return t.squeeze() > 0


def _resize_ids(ids, resize):
    """_resize_chw's target size, nearest neighbour: an id is never interpolated"""
    nh, nw = _resize_target(*ids.shape, resize)
    if (nh, nw) == tuple(ids.shape):
        return ids
    return F.interpolate(ids[None, None].float(), size=(nh, nw), mode="nearest")[0, 0].to(torch.uint8)


def _object_ids(img):
    """(H, W) uint8 ids of an opened PIL image: a palette image's indices; any other mode 1 where read_mask's rule says
    set (a non-zero channel)"""
    a = np.asarray(img)
    if img.mode != "P":
        a = (a.reshape(a.shape[0], a.shape[1], -1) != 0).any(axis=-1)
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8)))


def read_object_mask(mask_path, resize=None):
    """An object annotation -> (H, W) uint8 ids, 0 = background: the indices of a palette PNG (DAVIS-2017), else 1 where
    ``read_mask`` says set.  ``resize``: the loader's target size, nearest neighbour."""
    from PIL import Image
    return _resize_ids(_object_ids(Image.open(mask_path)), resize)


def read_depth(depth_path, resize=None, depth_scale=1.0, depth_offset=0.0):
    """read.py:60-70 -> (H,W) float."""
    t = torch.tensor(np.load(depth_path), dtype=torch.float32).unsqueeze(0)
    return _resize_chw(t, resize).squeeze(0) * depth_scale + depth_offset


def read_camera(camera_paths):
    """read.py:72-89 -> (mean focal, rounded principal point of the last file, poses[:, :3])."""
    focal_list, pose_list, pp = [], [], None
    for camera_path in camera_paths:
        with open(camera_path, "r") as f:
            d = json.load(f)
        focal_list.append(d["focal"])
        pose_list.append(d["pose"][:3])
        pp = [round(d["pp"][0]), round(d["pp"][1])]
    return float(np.array(focal_list).mean()), pp, np.array(pose_list)


# ----------------------------------------------------------------- sequence level
class AviFrame:
    """frame ``index`` of the Motion-JPEG AVI ``path``: what stands in a clip's image list where a file's path would"""

    def __init__(self, path, index, data=None):
        self.path, self.index = str(path), int(index)
        self.name = f"frame_{self.index:05d}"
        self.data = data                           # the frame's JPEG bytes, as sequence_paths took them from the parsed file

    def __repr__(self):
        return f"{self.path}:{self.name}"


def is_video(sequence_path):
    """is the sequence ONE video file (a file ending in .avi) instead of a folder of images?"""
    sp = str(sequence_path)
    return sp.lower().endswith(".avi") and os.path.isfile(sp)


def _frame_name(ip):
    return ip.name if isinstance(ip, AviFrame) else os.path.basename(ip).split(".")[0]


def _every_path(sequence_path):
    """the file lists of a sequence before they are sliced; a video file is parsed here, once"""
    sp = str(sequence_path).rstrip("/")
    if is_video(sp):
        from .video import read_avi
        img = [AviFrame(sp, i, data) for i, data in enumerate(read_avi(sp)["frames"])]
        sp = sp[:-4]
    else:
        img = sorted(Path(sp).glob("*.png")) + sorted(Path(sp).glob("*.jpg"))
    flow_dir = Path(sp + "_flow_unimatch")
    return dict(
        img=img,
        depth=sorted(Path(sp + "_depth_mast3r_s2").glob("*.npy")),
        occ=sorted(flow_dir.glob("*occ_bwd.png")) + sorted(flow_dir.glob("*occ_bwd.jpg")),
        flow=sorted(flow_dir.glob("*pred.flo")),
        flow_bwd=sorted(flow_dir.glob("*pred_bwd.flo")),
        move=sorted(Path(sp + "_epipolar").glob("*_open.png")),
        camera=sorted(Path(sp + "_camera_mast3r_s2").glob("*.json")),
        objects=sorted(Path(sp + "_mask").glob("*.png")),
    )


def _slicer(n_images, frame_start, frame_range, skip_interval):
    """the slice fit_video.py:79-99 takes of every list (``less``: the occlusion masks' list is one shorter)"""
    if frame_range == -1:
        frame_range = n_images - 1
    return lambda lst, less=0: lst[frame_start:frame_start + frame_range - less][::skip_interval]


def sequence_paths(sequence_path, frame_start=0, frame_range=-1, skip_interval=1):
    """The file lists of fit_video.py:79-99, same globbing, slicing and ordering.  For a video file ``img`` lists its frames
    (AviFrame) and the sibling folders hang on the path without its ``.avi``."""
    every = _every_path(sequence_path)
    cut = _slicer(len(every["img"]), frame_start, frame_range, skip_interval)
    return {k: cut(v, k == "occ") for k, v in every.items()}


_OPTIONS = dict(decode=("host", "device", "device-all"), occ_masks=("files", "flow"), move_masks=("files", "epipolar"),
                flows=("files", "estimate"), depth_camera=("files", "estimate"))


def load_sequence(sequence_path, resize=None, frame_start=0, frame_range=-1, skip_interval=1, depth_offset=0.0,
                  move_masks="files", occ_masks="files", blur=False, device=None, flows="files", depth_camera="files",
                  focal=None, decode="host", object_masks="none"):
    """Frames in the dict form ``gflow_amd.fit_video.fit_clip`` takes.  Frame i carries the flow
    i -> i+1 (fit_video.py:249: frame i+1 is fitted with flow_paths[i]) and the occlusion mask that
    fit_video.py:248 reads for it (img_occ_paths[i-1]).
    ``move_masks``: "files" reads ``<seq>_epipolar/*_open.png`` (a frame without a file gets zeros); "epipolar" ignores
    that folder and computes the mask of every frame that has a flow file from that flow, on the device
    (gflow_amd.move_seg.clip_move_masks; a frame without one gets zeros).
    ``occ_masks``: "files" reads ``*occ_bwd.*``; "flow" ignores those files and computes the mask of frame i + 1 from the
    flows i -> i + 1 and i + 1 -> i (``*pred_bwd.flo``) at the flows' NATIVE resolution, on the device
    (gflow_amd.occlusion.clip_occ_masks), then resizes the mask as a mask file would be.  Either way a frame without its
    file(s) gets no ``occ_mask``.
    ``flows``: "files" reads ``*pred.flo`` (and for occ_masks="flow" ``*pred_bwd.flo``); "estimate" ignores both and estimates
    the forward and the backward flow of every pair the files would cover from the decoded images at their NATIVE
    resolution, on the device (gflow_amd.optflow.pair_flows: ONE batched call).  An estimated flow then goes exactly the way
    a file's array goes (the resize that does not rescale the values, the blur), and move_masks="epipolar" and
    occ_masks="flow" run on the estimated flows.  A frame without a following image gets zeros, as a frame without a file.
    ``depth_camera``: "files" reads ``<seq>_depth_mast3r_s2/*.npy`` and ``<seq>_camera_mast3r_s2/*.json``; "estimate" ignores
    both folders and estimates the depth maps, the poses and the principal point from the flows at their NATIVE resolution,
    on the device (gflow_amd.sfm.clip_depth_camera: classical two-view geometry, NOT MASt3R; the flows from the files or,
    with flows="estimate", from the images; the move and occlusion masks, read or computed as ``move_masks`` and
    ``occ_masks`` say, keep their pixels out of the geometry).  ``focal`` is then the focal length in pixels of the native
    images (default: max(W, H), an assumption); the depth arrays, focal, pp and poses go exactly the way the files' values
    go.  It needs consecutive frames (skip_interval = 1) and a forward flow between every two of them.
    ``blur``: the reference's option -- GaussianBlur(7, 5.0) after the resize on the image, the occlusion mask and the flow
    (fit_video.py:245-248), not on the depth or the move mask.
    ``device``: None prepares every file on the host with torch, one file at a time, and returns host tensors.  With a
    device the files are only decoded on the host: the raw arrays of one kind are stacked, uploaded once and prepared there
    (gflow_amd.prep.prep_frames), and the frames hold device tensors of the same shapes and dtypes (``extr`` stays on the
    host, ``occ_count`` is set from one read-back for the whole clip).  The device's resize is the same filter with exact
    weights ("Frame preparation"): without ``resize`` and ``blur`` both paths give the same bits.
    ``decode``: "host" opens every image file with PIL; "device" (needs ``device``) decodes the JPEG files that
    gflow_amd.video.parse_jpeg accepts in one gflow_amd.video.decode_jpeg call per shape -- the same bits, so the frames are
    the same tensors -- and leaves PNGs and refused JPEGs to PIL, with one warning per clip that says how many.
    "device-all" (needs ``device`` too) does that and also decodes the PNG files gflow_amd.png.parse_png accepts -- images,
    move masks, occlusion masks and object masks -- with gflow_amd.png.decode_png, one call per kind and shape, again the
    same bits; whatever is left (16-bit or interlaced PNGs, other formats) is opened by PIL, with one warning per clip that
    counts those files.  A video
    file's frames (``sequence_path`` a ``.avi`` file) are always decoded on the device: without ``device`` it raises.
    ``object_masks``: "none" (the default) leaves the frames as they are; "files" reads ``<seq>_mask/*.png``, sliced like
    the other per-frame files, into ``frames[i]["object_mask"]`` -- (H, W) uint8 ids (``read_object_mask``: resized nearest
    neighbour, never blurred; on ``device`` if there is one) -- which is None for a frame without a file."""
    given = dict(decode=decode, occ_masks=occ_masks, move_masks=move_masks, flows=flows, depth_camera=depth_camera)
    for name, allowed in _OPTIONS.items():
        if given[name] not in allowed:
            (a, b), more = allowed[:2], "".join(f" or \"{c}\"" for c in allowed[2:])
            raise ValueError(f"load_sequence: {name} must be \"{a}\" or \"{b}\"{more}, got {given[name]!r}")
    if object_masks not in ("none", "files"):
        raise ValueError(f"load_sequence: object_masks must be \"none\" or \"files\", got {object_masks!r}")
    if decode != "host" and device is None:
        raise ValueError(f"load_sequence: decode=\"{decode}\" needs device=")
    if is_video(sequence_path) and device is None:
        raise RuntimeError(f"gflow_amd.io: {sequence_path}: a video file is decoded on a HIP (cuda) device, pass device=; there "
                           "is no CPU fallback")
    if depth_camera == "files" and focal is not None:
        raise ValueError("load_sequence: focal is the assumption of depth_camera=\"estimate\"; the files carry their own")
    if depth_camera == "estimate" and skip_interval != 1:
        raise ValueError("load_sequence: depth_camera=\"estimate\" needs consecutive frames (skip_interval = 1)")
    # the device everything below works on: the frames', or the current one where only an estimate needs it
    dev = None
    if device is not None or "estimate" in (flows, depth_camera):
        if not torch.cuda.is_available() or (device is not None and torch.device(device).type != "cuda"):
            raise RuntimeError("gflow_amd.io: load_sequence with device=, flows=\"estimate\" or depth_camera=\"estimate\" needs a "
                               "HIP (cuda) device; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    tally = [0, 0]                                 # decode="device-all": files PIL had to open, files in all
    clip = _resolve(sequence_path, frame_start, frame_range, skip_interval, move_masks, occ_masks, flows, depth_camera, focal,
                    decode, dev, tally)
    prep = _HostPrep(resize, blur, depth_offset) if device is None else _DevicePrep(dev, resize, blur, depth_offset)
    frames = _assemble(clip, prep)
    if object_masks == "files":
        paths = [path for _, path in zip(frames, clip.objects)]
        on_device, colour = [None] * len(paths), [None] * len(paths)
        if decode == "device-all":
            on_device, colour = _device_pngs(paths, dev)
            _count(tally, sum(a is None for a in on_device), len(paths))
        for fr, path, a, c in zip(frames, paths + [None] * len(frames), on_device + [None] * len(frames),
                                  colour + [None] * len(frames)):
            if a is not None:                      # _object_ids' rule on the decoded tensor
                ids = a if c == 3 else (a.reshape(a.shape[0], a.shape[1], -1) != 0).any(dim=-1).to(torch.uint8)
                fr["object_mask"] = _resize_ids(ids.contiguous(), resize)
                continue
            ids = None if path is None else read_object_mask(path, resize)
            fr["object_mask"] = ids if ids is None or device is None else ids.to(dev)
    if move_masks == "epipolar":
        from .move_seg import clip_move_masks
        clip_move_masks(frames, n_flows=len(clip.fwd))
    if decode == "device-all" and tally[0]:
        warnings.warn(f"load_sequence(decode=\"device-all\"): {tally[0]} of {tally[1]} image and mask files were decoded on the "
                      "host (files outside the device decoders' scope)")
    return frames


# ---- 1. resolve: the clip's sources at their native resolution, every file opened once
@dataclass
class _Clip:
    """The n frames' sources as arrays -- or device tensors, where something was decoded or estimated there."""
    names: list
    images: list                                   # ((H, W, C <= 3) uint8 or float32, the divisor that makes it [0, 1])
    fwd: list                                      # (h, w, 2) of pair i, None for a bad file; shorter than n: no more pairs
    bwd: list
    depth: list                                    # (H, W)
    move: list                                     # (H, W, C) as _decode_mask gives it, None without a file
    occ: list                                      # of PAIR i, as an image with its divisor; None without one
    focal: float
    pp: list
    poses: np.ndarray
    objects: list = None                           # the slice's <seq>_mask files (paths; read only when asked for)


def _resolve(sequence_path, frame_start, frame_range, skip_interval, move_masks, occ_masks, flows, depth_camera, focal, decode,
             dev, tally):
    """In dependency order: images -> flows -> native occlusion -> the geometry's exclusion masks -> depth and camera."""
    every = _every_path(sequence_path)
    cut = _slicer(len(every["img"]), frame_start, frame_range, skip_interval)
    p = {k: cut(v, k == "occ") for k, v in every.items()}
    n = len(p["img"])
    # images: the slice's and, for estimated flows, the ones its pairs touch (the last pair reaches one image past the slice)
    mine = cut(list(range(len(every["img"]))))
    pairs = cut(list(range(max(len(every["img"]) - 1, 0)))) if flows == "estimate" else []
    touched = sorted(set(pairs) | {i + 1 for i in pairs})
    used = sorted(set(mine) | set(touched))
    decoded = dict(zip(used, _decode_images([every["img"][i] for i in used], decode, dev, tally)))
    # flows: pair k of the list is (image k, image k + 1), as in a folder that holds the flows of EVERY pair
    if flows == "files":
        fwd = [_read_flo(f) for f in p["flow"][:n]]
        bwd = [_read_flo(f) for f in p["flow_bwd"][:n]] if occ_masks == "flow" or depth_camera == "estimate" else []
    elif pairs:
        from .optflow import clip_flows
        where = {i: j for j, i in enumerate(touched)}              # (i and i + 1 stay neighbours in the stack)
        stack = _image_stack([decoded[i] for i in touched], dev, decode != "host" or is_video(sequence_path))
        fwd, bwd = (list(f[:n]) for f in clip_flows(stack, pairs=[where[i] for i in pairs]))
    else:
        fwd, bwd = [], []
    m = len(fwd)
    estimate = depth_camera == "estimate"
    if estimate and n < 1:
        raise ValueError("load_sequence: depth_camera=\"estimate\" needs at least one frame")
    if estimate and (m < max(n - 1, 1) or any(f is None for f in fwd)):
        raise ValueError(f"load_sequence: depth_camera=\"estimate\" needs a forward flow between the {n} frames, found {m}")
    # the frames need the occlusion of the pairs 0 .. n - 2.  The geometry takes every pair there is (a flow into an image
    # behind the slice adds one), and the backward flows only if each of them has one
    both = estimate and len(bwd) >= m and all(b is not None for b in bwd[:m])
    frames_reach = max(n - 1, 0)
    occ, checked, occ_files = [], None, []
    if occ_masks == "flow":
        # the check sees the flows at their NATIVE resolution (resizing a flow does not rescale its values)
        from .occlusion import flow_occlusion
        idx = [i for i in range(min(m if both else frames_reach, m, len(bwd))) if fwd[i] is not None and bwd[i] is not None]
        if idx:
            checked = flow_occlusion(_stack([fwd[i] for i in idx], dev), _stack([bwd[i] for i in idx], dev))
            masks = (checked["occ_bwd"] != 0).to(torch.uint8).unsqueeze(-1)
            occ = [None] * (idx[-1] + 1)
            for j, i in enumerate(idx):
                occ[i] = (masks[j], 1.0)
    else:
        occ_files = _open_images(p["occ"][:m if estimate else frames_reach], decode, dev, tally)
        occ = [_image_array(a) for a in occ_files]
    move = [None] * n
    if move_masks == "files":
        move = [_mask_array(a) for a in _open_images(p["move"][:n], decode, dev, tally)] + [None] * max(n - len(p["move"]), 0)
    if estimate:
        f_dev, b_dev = _stack(fwd, dev), _stack(bwd[:m], dev) if both else None
        ex_f, ex_b = _exclusions(f_dev, move[:m], [_mask_array(a) for a in occ_files], checked if both else None,
                                 move_masks == "epipolar")
        from .sfm import clip_depth_camera, warn_unreliable
        res = clip_depth_camera(f_dev, b_dev, focal=focal, exclude_fwd=ex_f, exclude_bwd=ex_b, warn=False)
        warn_unreliable(res["unreliable"][:n])
        depth, focal, pp, poses = list(res["depth"][:n]), float(res["focal"]), list(res["pp"]), res["extr"][:n].cpu().numpy()
    else:
        depth = [np.load(p["depth"][i]) for i in range(n)]
        focal, pp, poses = read_camera(p["camera"])
    return _Clip([_frame_name(ip) for ip in p["img"]], [decoded[i] for i in mine], fwd, bwd, depth, move, occ, focal, pp, poses,
                 list(p["objects"][:n]))


def _exclusions(fwd, move, occ, checked, epipolar):
    """(exclude_fwd, exclude_bwd) (m, h, w) bool for gflow_amd.sfm.clip_depth_camera: the move masks keep pixels of the forward
    grids out of the geometry, the occlusion masks (occ_bwd) pixels of the backward grids and, from a check, (occ) of the
    forward ones.  ``move`` / ``occ``: the mask files' arrays, used where one has the flows' shape; ``checked``: the
    flow_occlusion result of all m pairs; ``epipolar``: the move masks are computed from the native flows instead."""
    shape, dev = tuple(fwd.shape[1:3]), fwd.device
    ex_f, ex_b = (torch.zeros(tuple(fwd.shape[:3]), dtype=torch.bool, device=dev) for _ in range(2))
    if epipolar:
        from .move_seg import epipolar_move_mask
        for i in range(len(fwd)):
            ex_f[i] = epipolar_move_mask(fwd[i])["open"] != 0
    for ex, arrays in ((ex_f, move), (ex_b, occ)):
        for i, a in enumerate(arrays):
            mask = None if a is None else _mask_to_tensor(a)
            if mask is not None and tuple(mask.shape) == shape:
                ex[i] = mask.to(dev)
    if checked is not None:
        ex_f |= checked["occ"] != 0
        ex_b |= checked["occ_bwd"] != 0
    return ex_f, ex_b


def _stack(arrays, device):
    """one (T, ...) tensor of arrays of one shape, with ONE upload to ``device`` (None: it stays on the host); tensors that
    are on the device already are not uploaded again"""
    if any(torch.is_tensor(a) for a in arrays):
        return torch.stack([a if torch.is_tensor(a) else torch.from_numpy(np.array(a)).to(device) for a in arrays])
    stack = torch.from_numpy(np.stack(arrays))
    return stack if device is None else stack.to(device)


def _kind(a):
    return tuple(a.shape), "|u1" if a.dtype == torch.uint8 else str(a.dtype) if torch.is_tensor(a) else a.dtype.str


def _image_stack(images, dev, device_decode):
    """the (T, H, W, 3) stack gflow_amd.optflow.clip_flows takes, from decoded images: uint8, or float in [0, 1]"""
    arrays = [a if torch.is_tensor(a) or a.dtype == np.uint8 else (a / np.float32(div)).astype(np.float32) for a, div in images]
    kinds = {_kind(a) for a in arrays}
    if device_decode and (len(kinds) != 1 or _kind(arrays[0])[1] != "|u1"):
        raise ValueError("load_sequence: flows=\"estimate\" from device-decoded images needs 8-bit images of one shape")
    if len(kinds) != 1:
        raise ValueError("optflow: the images of a sequence must have one shape and one bit depth")
    stack = _stack(arrays, dev)
    return stack.expand(-1, -1, -1, 3).contiguous() if stack.shape[-1] == 1 else stack


def _open_image(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _device_pngs(paths, device):
    """([a device tensor with the shape and the bits of np.asarray(Image.open(path)), or None], [the file's colour type, or
    None]): the PNG files gflow_amd.png.parse_png accepts, decoded by gflow_amd.png.decode_png in one call per shape"""
    from .png import decode_png, parse_png
    out, colour, groups = [None] * len(paths), [None] * len(paths), {}
    for i, ip in enumerate(paths):
        if isinstance(ip, AviFrame) or not str(ip).lower().endswith(".png"):
            continue
        with open(ip, "rb") as f:
            data = f.read()
        try:
            p = parse_png(data, str(ip))
        except ValueError:
            continue
        colour[i] = p["colour_type"]
        groups.setdefault((p["width"], p["height"], p["bpp"]), []).append((i, p))
    for members in groups.values():
        stack = decode_png([p for _, p in members], device, names=[str(paths[i]) for i, _ in members])
        for j, (i, _) in enumerate(members):
            out[i] = stack[j, :, :, 0] if stack.shape[-1] == 1 else stack[j]
    return out, colour


def _open_images(paths, decode, device, tally):
    """_open_image of every path; with decode="device-all" the PNG files the device decoder takes come from it, as device
    tensors.  ``tally``: [files PIL opened, files in all], counted under "device-all" only."""
    if decode != "device-all":
        return [_open_image(ip) for ip in paths]
    on_device = _device_pngs(paths, device)[0]
    _count(tally, sum(a is None for a in on_device), len(paths))
    return [_open_image(ip) if a is None else a for ip, a in zip(paths, on_device)]


def _count(tally, on_host, files):
    """decode="device-all": ``on_host`` of ``files`` more files were left to PIL"""
    tally[0] += on_host
    tally[1] += files


def _mask_array(mask):
    """(H, W, C) uint8 or float32 as read_mask takes a file's array"""
    if mask.ndim == 2:
        mask = mask[..., None]
    elif mask.ndim != 3:
        raise ValueError("The mask should be 2D or 3D")
    if torch.is_tensor(mask):                      # (decoded on the device: uint8)
        return mask.contiguous()
    return np.ascontiguousarray(mask if mask.dtype == np.uint8 else mask.astype(np.float32))


def _image_array(img):
    """(array (H, W, C <= 3) uint8 or float32, the divisor that makes it [0, 1]) as image_path_to_tensor takes a file's array"""
    rgb = _mask_array(img)[..., :3]
    return rgb.contiguous() if torch.is_tensor(rgb) else np.ascontiguousarray(rgb), _image_div(img.dtype)


def _decode_image(path):
    """(array (H, W, C <= 3) uint8 or float32, the divisor that makes it [0, 1]) as image_path_to_tensor reads the file"""
    return _image_array(_open_image(path))


def _decode_mask(path):
    """(H, W, C) uint8 or float32 as read_mask reads the file"""
    return _mask_array(_open_image(path))


def _decode_images(paths, decode, device, tally=None):
    """[(array or device tensor (H, W, C <= 3), divisor)] of a clip's images, as _decode_image gives them.  A video file's
    frames, and with decode="device" the JPEG files the device decoder takes, come from gflow_amd.video.decode_jpeg as
    device tensors (one call per shape); every other file from PIL, with one warning that counts them.  With
    decode="device-all" the PNG files gflow_amd.png.parse_png accepts come from gflow_amd.png.decode_png as well, and the
    files left to PIL are counted into ``tally`` for the clip's one warning."""
    from .video import decode_jpeg, parse_jpeg
    out = [None] * len(paths)
    groups, rest = {}, []                          # JPEG data by shape; the indices of every other file
    for i, ip in enumerate(paths):
        if isinstance(ip, AviFrame):
            data, name = ip.data, repr(ip)
        elif decode != "host" and str(ip).lower().endswith((".jpg", ".jpeg")):
            with open(ip, "rb") as f:
                data, name = f.read(), str(ip)
        else:
            data = None
        if data is not None:
            try:
                p = parse_jpeg(data, name)
                groups.setdefault((p["width"], p["height"], p["components"], p["hs"], p["vs"]), []).append((i, data, name))
                continue
            except ValueError:
                if isinstance(ip, AviFrame):
                    raise
        rest.append(i)
    if decode == "device-all":
        on_device = _device_pngs([paths[i] for i in rest], device)[0]
        for i, a in zip(rest, on_device):
            out[i] = _image_array(_open_image(paths[i]) if a is None else a)
        _count(tally, sum(a is None for a in on_device), len(paths))
    else:
        for i in rest:
            out[i] = _decode_image(paths[i])
    on_host = len(rest) if decode == "device" else 0
    for members in groups.values():
        stack = decode_jpeg([d for _, d, _ in members], device, names=[n for _, _, n in members])
        for j, (i, _, _) in enumerate(members):
            out[i] = (stack[j], 255.0)
    if on_host:
        warnings.warn(f"load_sequence(decode=\"device\"): {on_host} of {len(paths)} images were decoded on the host (PNG files, "
                      "or JPEG files outside the device decoder's scope)")
    return out


# ---- 2. prepare: native arrays -> the frames' tensors (None passes through); a host and a device preparer, one interface
def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _mask_to_tensor(mask, resize=None):
    """what read_mask makes of a file's (H, W, C) array"""
    t = _resize_chw(torch.from_numpy(np.array(_np(mask))).float().permute(2, 0, 1), resize)
    if t.shape[-1] > 1:
        t = t.sum(dim=0)
    return t.squeeze() > 0


class _HostPrep:
    """the readers' torch code on one decoded array at a time -> host tensors"""

    def __init__(self, resize, blur, depth_offset):
        self.resize, self.blur, self.depth_offset = resize, blur, depth_offset

    def _each(self, fn, arrays):
        return [None if a is None else fn(a) for a in arrays]

    def image(self, images):
        to_chw = lambda a, div: torch.from_numpy(np.array(_np(a))).permute(2, 0, 1).float() / div
        return self._each(lambda x: _blur_chw(_resize_chw(to_chw(*x), self.resize), self.blur).permute(1, 2, 0), images)

    occ_mask = image

    def flow(self, flows):
        return self._each(lambda a: _flow_to_tensor(_np(a), self.resize, self.blur), flows)

    def depth(self, depths):
        to_chw = lambda a: torch.tensor(_np(a), dtype=torch.float32).unsqueeze(0)
        return self._each(lambda a: (_resize_chw(to_chw(a), self.resize).squeeze(0) + self.depth_offset).unsqueeze(-1), depths)

    def move_mask(self, masks):
        return self._each(lambda a: _mask_to_tensor(a, self.resize), masks)

    def occ_counts(self, masks):
        return [None] * len(masks)                 # (fit_video.upload_clip counts them when it uploads the frames)


class _DevicePrep:
    """whole stacks on the device (gflow_amd.prep.prep_frames) -> device tensors of the host preparer's shapes and dtypes"""

    def __init__(self, device, resize, blur, depth_offset):
        self.device, self.resize, self.blur, self.depth_offset = device, resize, blur, depth_offset

    def _stacks(self, arrays, keys=None, **kw):
        """prep_frames over a list of (H, W, C) arrays: those of one shape and dtype (and ``keys`` entry, the divisor) go up
        as ONE stack and come back as views of one result"""
        from .prep import prep_frames
        out = [None] * len(arrays)
        groups = {}
        for i, a in enumerate(arrays):
            if a is not None:
                groups.setdefault(_kind(a) + (None if keys is None else keys[i],), []).append(i)
        for (_, _, key), idx in groups.items():
            res = prep_frames(_stack([arrays[i] for i in idx], self.device), self.resize,
                              **(kw if key is None else dict(kw, div=key)))
            for j, i in enumerate(idx):
                out[i] = res[j]
        return out

    def image(self, images):
        split = lambda k: [None if x is None else x[k] for x in images]
        return self._stacks(split(0), keys=split(1), blur=self.blur)

    occ_mask = image

    def flow(self, flows):
        return self._stacks(flows, blur=self.blur)

    def depth(self, depths):
        hw1 = lambda a: a.unsqueeze(-1) if torch.is_tensor(a) else np.asarray(a, dtype=np.float32)[..., None]
        return self._stacks([hw1(a) for a in depths], mul=1.0, add=self.depth_offset)

    def move_mask(self, masks):
        return self._stacks(masks, as_mask=True)

    def occ_counts(self, masks):
        """what upload_clip counts on the host, one frame at a time: here one read-back for the clip"""
        sums = [(m[..., 0] > 0).sum() for m in masks if m is not None]
        counts = iter(torch.stack(sums).cpu().tolist() if sums else [])
        return [None if m is None else int(next(counts)) for m in masks]


# ---- 3. assemble: the per-frame rules, here and only here
def _assemble(clip, prep):
    n = len(clip.names)
    image, depth = prep.image(clip.images), prep.depth(clip.depth)
    flow = prep.flow([clip.fwd[i] if i < len(clip.fwd) else None for i in range(n)])
    move = prep.move_mask(clip.move)
    occ = prep.occ_mask([clip.occ[i - 1] if 1 <= i <= len(clip.occ) else None for i in range(n)])     # frame i: pair i - 1
    counts = prep.occ_counts(occ)
    frames = []
    for i in range(n):
        fr = dict(image=image[i], focal=clip.focal, pp=clip.pp, name=clip.names[i], depth=depth[i])
        H, W = fr["image"].shape[:2]
        fr["move_mask"] = move[i] if move[i] is not None else fr["image"].new_zeros((H, W), dtype=torch.bool)   # (no file)
        # a pair without a flow: zeros; a file with a bad magic number: None, as read_flow gives
        fr["flow"] = flow[i] if i < len(clip.fwd) else fr["image"].new_zeros((H, W, 2))
        if occ[i] is not None:
            fr["occ_mask"] = occ[i]
        if i < len(clip.poses):
            fr["extr"] = torch.tensor(clip.poses[i], dtype=torch.float32)                           # (stays on the host)
        if counts[i] is not None:
            fr["occ_count"] = counts[i]
        frames.append(fr)
    return frames


def write_sequence(frames, sequence_path):
    """Lay a clip (e.g. gflow_amd.synthetic.make_clip) out on disk in the reference's convention, so
    that the same folder can be read back here or handed to the reference's fit_video.py."""
    from PIL import Image
    sp = str(sequence_path).rstrip("/")
    dirs = {k: sp + s for k, s in (("img", ""), ("depth", "_depth_mast3r_s2"), ("flow", "_flow_unimatch"),
                                   ("move", "_epipolar"), ("camera", "_camera_mast3r_s2"))}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    u8 = lambda t: (torch.as_tensor(t).float().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
    for i, fr in enumerate(frames):
        name = f"{i:05d}"
        Image.fromarray(u8(fr["image"])).save(os.path.join(dirs["img"], name + ".png"))
        np.save(os.path.join(dirs["depth"], name + ".npy"), torch.as_tensor(fr["depth"]).squeeze(-1).cpu().numpy())
        Image.fromarray(u8(torch.as_tensor(fr["move_mask"]).float())).save(os.path.join(dirs["move"], name + "_open.png"))
        if i + 1 < len(frames):
            write_flow(os.path.join(dirs["flow"], name + "_pred.flo"), torch.as_tensor(fr["flow"]).cpu().numpy())
        if i >= 1:
            occ = fr.get("occ_mask")
            occ = torch.zeros(fr["image"].shape[:2]) if occ is None else torch.as_tensor(occ).float()
            if occ.dim() == 3:
                occ = occ[..., 0]
            Image.fromarray(u8(occ)).save(os.path.join(dirs["flow"], f"{i - 1:05d}_occ_bwd.png"))
        pose = torch.eye(4)
        if fr.get("extr") is not None:
            pose[:3] = torch.as_tensor(fr["extr"]).float()
        with open(os.path.join(dirs["camera"], name + ".json"), "w") as f:
            json.dump({"focal": float(fr["focal"]), "pp": [float(fr["pp"][0]), float(fr["pp"][1])], "pose": pose.tolist()}, f)
    return sp
