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
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

FLO_MAGIC = 202021.25


def _resize_chw(t, resize):
    """torchvision.transforms.Resize(int, antialias=True) on a (C,H,W) float tensor."""
    if resize is None:
        return t
    _, h, w = t.shape
    if h <= w:
        nh, nw = resize, int(resize * w / h)
    else:
        nh, nw = int(resize * h / w), resize
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


def read_depth(depth_path, resize=None, depth_scale=1.0, depth_offset=0.0):
    """read.py:60-70 -> (H,W) float."""
    t = torch.tensor(_depth_array(depth_path), dtype=torch.float32).unsqueeze(0)
    return _resize_chw(t, resize).squeeze(0) * depth_scale + depth_offset


def _depth_array(src):
    """a frame's depth at its native resolution, wherever it comes from: the array of a .npy file, or an estimate's array"""
    return src if isinstance(src, np.ndarray) else np.load(src)


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

    def __init__(self, path, index):
        self.path, self.index = str(path), int(index)
        self.name = f"frame_{self.index:05d}"

    def __repr__(self):
        return f"{self.path}:{self.name}"


def is_video(sequence_path):
    """is the sequence ONE video file (a file ending in .avi) instead of a folder of images?"""
    sp = str(sequence_path)
    return sp.lower().endswith(".avi") and os.path.isfile(sp)


def _frame_name(ip):
    return ip.name if isinstance(ip, AviFrame) else os.path.basename(ip).split(".")[0]


def sequence_paths(sequence_path, frame_start=0, frame_range=-1, skip_interval=1):
    """The file lists of fit_video.py:79-99, same globbing, slicing and ordering.  For a video file ``img`` lists its frames
    (AviFrame) and the sibling folders hang on the path without its ``.avi``."""
    sp = str(sequence_path).rstrip("/")
    if is_video(sp):
        from .video import read_avi
        img = [AviFrame(sp, i) for i in range(len(read_avi(sp)["frames"]))]
        sp = sp[:-4]
    else:
        img = sorted(Path(sp).glob("*.png")) + sorted(Path(sp).glob("*.jpg"))
    if frame_range == -1:
        frame_range = len(img) - 1
    cut = lambda lst, n=frame_range: lst[frame_start:frame_start + n][::skip_interval]
    flow_dir = Path(sp + "_flow_unimatch")
    return dict(
        img=cut(img),
        depth=cut(sorted(Path(sp + "_depth_mast3r_s2").glob("*.npy"))),
        occ=cut(sorted(flow_dir.glob("*occ_bwd.png")) + sorted(flow_dir.glob("*occ_bwd.jpg")), frame_range - 1),
        flow=cut(sorted(flow_dir.glob("*pred.flo"))),
        flow_bwd=cut(sorted(flow_dir.glob("*pred_bwd.flo"))),
        move=cut(sorted(Path(sp + "_epipolar").glob("*_open.png"))),
        camera=cut(sorted(Path(sp + "_camera_mast3r_s2").glob("*.json"))),
    )


def load_sequence(sequence_path, resize=None, frame_start=0, frame_range=-1, skip_interval=1, depth_offset=0.0,
                  move_masks="files", occ_masks="files", blur=False, device=None, flows="files", depth_camera="files",
                  focal=None, decode="host"):
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
    the same tensors -- and leaves PNGs and refused JPEGs to PIL, with one warning per clip that says how many.  A video
    file's frames (``sequence_path`` a ``.avi`` file) are always decoded on the device: without ``device`` it raises."""
    if decode not in ("host", "device"):
        raise ValueError(f"load_sequence: decode must be \"host\" or \"device\", got {decode!r}")
    if decode == "device" and device is None:
        raise ValueError("load_sequence: decode=\"device\" needs device=")
    if is_video(sequence_path) and device is None:
        raise RuntimeError(f"gflow_amd.io: {sequence_path}: a video file is decoded on a HIP (cuda) device, pass device=; there "
                           "is no CPU fallback")
    if occ_masks not in ("files", "flow"):
        raise ValueError(f"load_sequence: occ_masks must be \"files\" or \"flow\", got {occ_masks!r}")
    if move_masks not in ("files", "epipolar"):
        raise ValueError(f"load_sequence: move_masks must be \"files\" or \"epipolar\", got {move_masks!r}")
    if flows not in ("files", "estimate"):
        raise ValueError(f"load_sequence: flows must be \"files\" or \"estimate\", got {flows!r}")
    if depth_camera not in ("files", "estimate"):
        raise ValueError(f"load_sequence: depth_camera must be \"files\" or \"estimate\", got {depth_camera!r}")
    if depth_camera == "files" and focal is not None:
        raise ValueError("load_sequence: focal is the assumption of depth_camera=\"estimate\"; the files carry their own")
    p = sequence_paths(sequence_path, frame_start, frame_range, skip_interval)
    n = len(p["img"])
    if flows == "estimate":
        fwd, bwd = _estimated_flows(sequence_path, frame_start, frame_range, skip_interval, device, decode)
    else:
        fwd, bwd = [_FloFile(f) for f in p["flow"]], [_FloFile(f) for f in p["flow_bwd"]]
    fwd, bwd = fwd[:n], bwd[:n]
    if depth_camera == "estimate":
        if skip_interval != 1:
            raise ValueError("load_sequence: depth_camera=\"estimate\" needs consecutive frames (skip_interval = 1)")
        depth, focal, pp, poses = _estimated_depth_camera(p, fwd, bwd, n, move_masks, occ_masks, focal, device)
        p = dict(p, depth=depth)
    else:
        focal, pp, poses = read_camera(p["camera"])
    if device is not None:
        frames = _load_frames_device(p, fwd, bwd, focal, pp, poses, resize, depth_offset, move_masks, occ_masks, blur,
                                     torch.device(device), decode)
    else:
        frames = _load_frames_host(p, fwd, bwd, focal, pp, poses, resize, depth_offset, move_masks, occ_masks, blur)
    if move_masks == "epipolar":
        from .move_seg import clip_move_masks
        clip_move_masks(frames, n_flows=len(fwd))
    return frames


class _FloFile:
    """a frame's flow at its native resolution, wherever it comes from: read() is the (h, w, 2) float32 array of a .flo
    file (None on a bad magic number) or of an estimate"""

    def __init__(self, path=None, array=None):
        self.path, self.array = path, array

    def read(self):
        return _read_flo(self.path) if self.array is None else self.array


def _estimated_flows(sequence_path, frame_start, frame_range, skip_interval, device, decode="host"):
    """(forward, backward) _FloFile lists as sequence_paths would list the files of a folder that holds the flows of EVERY
    pair of consecutive images (the one ``python -m gflow_amd.optflow`` writes): file k is the pair (image k, image k + 1)."""
    from .optflow import clip_flows, pair_flows
    sp = str(sequence_path).rstrip("/")
    img = sequence_paths(sp, frame_range=1 << 30)["img"]
    if frame_range == -1:
        frame_range = len(img) - 1
    pairs = list(range(max(len(img) - 1, 0)))[frame_start:frame_start + frame_range][::skip_interval]
    if not pairs:
        return [], []
    if decode == "device" or is_video(sp):
        # the decoded stack instead of paths: only the images the pairs touch (i and i + 1 stay neighbours in it)
        used = sorted(set(pairs) | {i + 1 for i in pairs})
        where = {i: j for j, i in enumerate(used)}
        dev = torch.device(device)
        arrays = [a if torch.is_tensor(a) else torch.from_numpy(np.array(a)).to(dev)
                  for a, _ in _decode_images([img[i] for i in used], decode, dev)]
        if len({(tuple(a.shape), a.dtype) for a in arrays}) != 1 or arrays[0].dtype != torch.uint8:
            raise ValueError("load_sequence: flows=\"estimate\" from device-decoded images needs 8-bit images of one shape")
        stack = torch.stack(arrays)
        stack = stack.expand(-1, -1, -1, 3).contiguous() if stack.shape[-1] == 1 else stack
        fwd, bwd = clip_flows(stack, pairs=[where[i] for i in pairs])
    else:
        fwd, bwd = pair_flows(img, pairs, device=device)
    fwd, bwd = fwd.cpu().numpy(), bwd.cpu().numpy()
    return ([_FloFile(array=np.ascontiguousarray(f)) for f in fwd], [_FloFile(array=np.ascontiguousarray(f)) for f in bwd])


def _estimated_depth_camera(p, fwd_src, bwd_src, n, move_masks, occ_masks, focal, device):
    """(depth arrays, focal, pp, poses) of the n frames as the files would give them, from gflow_amd.sfm.clip_depth_camera on
    the native flows.  The backward flows are used when every pair has one; the exclusions are the move masks (on the forward
    flows' grids) and the occlusion masks (``occ_bwd`` on the backward flows' grids, and with occ_masks="flow" ``occ`` on the
    forward ones'), read where a file of the flows' shape is there, computed where the loader computes them."""
    from .sfm import clip_depth_camera, warn_unreliable
    if n < 1:
        raise ValueError("load_sequence: depth_camera=\"estimate\" needs at least one frame")
    fwd = [f.read() for f in fwd_src[:n]]
    if len(fwd) < max(n - 1, 1) or any(f is None for f in fwd):
        raise ValueError(f"load_sequence: depth_camera=\"estimate\" needs a forward flow between the {n} frames, found {len(fwd)}")
    m = len(fwd)
    bwd = [f.read() for f in bwd_src[:m]]
    bwd = None if len(bwd) < m or any(b is None for b in bwd) else bwd
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.io: depth_camera=\"estimate\" needs a HIP (cuda) device; there is no CPU fallback")
    f_dev = torch.from_numpy(np.stack(fwd)).to(dev)
    b_dev = None if bwd is None else torch.from_numpy(np.stack(bwd)).to(dev)
    shape = tuple(f_dev.shape[1:3])
    ex_f = torch.zeros((m,) + shape, dtype=torch.bool, device=dev)
    ex_b = torch.zeros((m,) + shape, dtype=torch.bool, device=dev)
    if move_masks == "epipolar":
        from .move_seg import epipolar_move_mask
        for i in range(m):
            ex_f[i] = epipolar_move_mask(f_dev[i])["open"] != 0
    else:
        for i, path in enumerate(p["move"][:m]):
            mask = read_mask(path)
            if tuple(mask.shape) == shape:
                ex_f[i] = mask.to(dev)
    if occ_masks == "flow" and b_dev is not None:
        from .occlusion import flow_occlusion
        occ = flow_occlusion(f_dev, b_dev)
        ex_f |= occ["occ"] != 0
        ex_b |= occ["occ_bwd"] != 0
    elif occ_masks == "files":
        for i, path in enumerate(p["occ"][:m]):
            mask = read_mask(path)
            if tuple(mask.shape) == shape:
                ex_b[i] = mask.to(dev)
    res = clip_depth_camera(f_dev, b_dev, focal=focal, exclude_fwd=ex_f, exclude_bwd=ex_b, warn=False)
    warn_unreliable(res["unreliable"][:n])                       # (a flow into an image behind the slice adds a frame)
    depth = res["depth"][:n].cpu().numpy()
    poses = res["extr"][:n].cpu().numpy()
    return [np.ascontiguousarray(d) for d in depth], float(res["focal"]), list(res["pp"]), poses


def _load_frames_host(p, flow_src, bwd_src, focal, pp, poses, resize, depth_offset, move_masks, occ_masks, blur):
    frames = []
    for i, ip in enumerate(p["img"]):
        fr = dict(image=image_path_to_tensor(ip, resize, blur), focal=focal, pp=pp, name=_frame_name(ip))
        fr["depth"] = read_depth(p["depth"][i], resize, depth_offset=depth_offset).unsqueeze(-1)
        H, W = fr["image"].shape[:2]
        from_file = move_masks == "files" and i < len(p["move"])
        fr["move_mask"] = read_mask(p["move"][i], resize) if from_file else torch.zeros(H, W, dtype=torch.bool)
        fr["flow"] = _flow_to_tensor(flow_src[i].read(), resize, blur) if i < len(flow_src) else torch.zeros(H, W, 2)
        if occ_masks == "files" and i >= 1 and i - 1 < len(p["occ"]):
            fr["occ_mask"] = image_path_to_tensor(p["occ"][i - 1], resize, blur)
        if i < len(poses):
            fr["extr"] = torch.tensor(poses[i], dtype=torch.float32)
        frames.append(fr)
    if occ_masks == "flow":
        from .occlusion import clip_occ_masks
        n_pairs = min(len(frames) - 1, len(flow_src), len(bwd_src))
        # (the reference resizes a flow without rescaling its values: the check must not see fr["flow"] of a resized clip)
        native = resize is None and not blur
        fwd = [frames[i]["flow"] if native else _flow_to_tensor(flow_src[i].read()) for i in range(n_pairs)]
        bwd = [_flow_to_tensor(bwd_src[i].read()) for i in range(n_pairs)]
        clip_occ_masks(frames, bwd, fwd_flows=fwd, resize=resize)
        if blur:                                   # (no frame had a mask before: the files are ignored)
            for fr in frames:
                if "occ_mask" in fr:
                    fr["occ_mask"] = _blur_chw(fr["occ_mask"].permute(2, 0, 1), True).permute(1, 2, 0)
    return frames


# ---- the device path: decode on the host, prepare whole stacks on the device
def _decode_image(path):
    """(array (H, W, C <= 3) uint8 or float32, the divisor that makes it [0, 1]) as image_path_to_tensor reads the file"""
    from PIL import Image
    img = np.asarray(Image.open(path))
    div = _image_div(img.dtype)
    if img.ndim == 2:
        img = img[..., None]
    img = img[..., :3]
    return np.ascontiguousarray(img if img.dtype == np.uint8 else img.astype(np.float32)), div


def _decode_images(paths, decode, device):
    """[(array or device tensor (H, W, C <= 3), divisor)] of a clip's images, as _decode_image gives them.  A video file's
    frames, and with decode="device" the JPEG files the device decoder takes, come from gflow_amd.video.decode_jpeg as
    device tensors (one call per shape); every other file from PIL, with one warning that counts them."""
    from .video import decode_jpeg, parse_jpeg, read_avi
    out = [None] * len(paths)
    groups, avi, on_host = {}, {}, 0
    for i, ip in enumerate(paths):
        if isinstance(ip, AviFrame):
            if ip.path not in avi:
                avi[ip.path] = read_avi(ip.path)["frames"]
            data, name = avi[ip.path][ip.index], repr(ip)
        elif decode == "device" and str(ip).lower().endswith((".jpg", ".jpeg")):
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
        out[i] = _decode_image(ip)
        on_host += decode == "device"
    for members in groups.values():
        stack = decode_jpeg([d for _, d, _ in members], device, names=[n for _, _, n in members])
        for j, (i, _, _) in enumerate(members):
            out[i] = (stack[j], 255.0)
    if on_host:
        warnings.warn(f"load_sequence(decode=\"device\"): {on_host} of {len(paths)} images were decoded on the host (PNG files, "
                      "or JPEG files outside the device decoder's scope)")
    return out


def _decode_mask(path):
    """(H, W, C) uint8 or float32 as read_mask reads the file"""
    from PIL import Image
    mask = np.asarray(Image.open(path))
    if mask.ndim == 2:
        mask = mask[..., None]
    elif mask.ndim != 3:
        raise ValueError("The mask should be 2D or 3D")
    return np.ascontiguousarray(mask if mask.dtype == np.uint8 else mask.astype(np.float32))


def _prep_stacks(arrays, device, resize, keys=None, **kw):
    """prep_frames over a list of (H, W, C) arrays (None: no file): the arrays of one shape and dtype (and ``keys`` entry,
    the divisor) go up as ONE stack and come back as views of one result.  Returns the list of device tensors."""
    from .prep import prep_frames
    out = [None] * len(arrays)
    groups = {}
    for i, a in enumerate(arrays):
        if a is not None:
            kind = "|u1" if a.dtype == torch.uint8 else str(a.dtype) if torch.is_tensor(a) else a.dtype.str
            groups.setdefault((tuple(a.shape), kind, None if keys is None else keys[i]), []).append(i)
    for (_, _, key), idx in groups.items():
        if any(torch.is_tensor(arrays[i]) for i in idx):       # (decoded on the device: already there)
            stack = torch.stack([arrays[i] if torch.is_tensor(arrays[i]) else torch.from_numpy(np.array(arrays[i])).to(device)
                                 for i in idx])
        else:
            stack = torch.from_numpy(np.stack([arrays[i] for i in idx])).to(device)
        res = prep_frames(stack, resize, **(kw if key is None else dict(kw, div=key)))
        for j, i in enumerate(idx):
            out[i] = res[j]
    return out


def _load_frames_device(p, flow_src, bwd_src, focal, pp, poses, resize, depth_offset, move_masks, occ_masks, blur, device,
                        decode="host"):
    if device.type != "cuda":
        raise RuntimeError("gflow_amd.io: load_sequence(device=...) needs a HIP (cuda) device; there is no CPU fallback")
    n = len(p["img"])
    images = _decode_images(p["img"], decode, device)
    image = _prep_stacks([a for a, _ in images], device, resize, keys=[d for _, d in images], blur=blur)
    depth = _prep_stacks([np.asarray(_depth_array(p["depth"][i]), dtype=np.float32)[..., None] for i in range(n)], device, resize,
                         mul=1.0, add=depth_offset)
    flows = [flow_src[i].read() if i < len(flow_src) else None for i in range(n)]
    flow = _prep_stacks(flows, device, resize, blur=blur)
    move = [None] * n
    if move_masks == "files":
        move = _prep_stacks([_decode_mask(p["move"][i]) if i < len(p["move"]) else None for i in range(n)], device, resize,
                            as_mask=True)
    occ = [None] * n
    if occ_masks == "files":
        files = [_decode_image(p["occ"][i - 1]) if 1 <= i <= len(p["occ"]) else (None, None) for i in range(n)]
        occ = _prep_stacks([a for a, _ in files], device, resize, keys=[d for _, d in files], blur=blur)
    else:
        from .occlusion import flow_occlusion
        from .prep import prep_frames
        # the check sees the flows at their native resolution (resizing a flow does not rescale its values)
        bwd = [bwd_src[i].read() for i in range(min(n - 1, len(flow_src), len(bwd_src)))]
        pairs = [i for i, b in enumerate(bwd) if b is not None and flows[i] is not None]
        if pairs:
            res = flow_occlusion(torch.from_numpy(np.stack([flows[i] for i in pairs])).to(device),
                                 torch.from_numpy(np.stack([bwd[i] for i in pairs])).to(device))["occ_bwd"]
            masks = prep_frames((res != 0).to(torch.uint8).unsqueeze(-1).contiguous(), resize, blur=blur)
            for j, i in enumerate(pairs):
                occ[i + 1] = masks[j]
    frames = []
    for i, ip in enumerate(p["img"]):
        fr = dict(image=image[i], focal=focal, pp=pp, name=_frame_name(ip), depth=depth[i])
        H, W = fr["image"].shape[:2]
        fr["move_mask"] = move[i] if move[i] is not None else torch.zeros(H, W, dtype=torch.bool, device=device)
        if i < len(flow_src):
            fr["flow"] = flow[i]                   # (None for a file with a bad magic number, as read_flow gives)
        else:
            fr["flow"] = torch.zeros(H, W, 2, device=device)
        if occ[i] is not None:
            fr["occ_mask"] = occ[i]
        if i < len(poses):
            fr["extr"] = torch.tensor(poses[i], dtype=torch.float32)
        frames.append(fr)
    # what upload_clip counts on the host, one frame at a time: here one read-back for the clip
    with_occ = [fr for fr in frames if "occ_mask" in fr]
    if with_occ:
        counts = torch.stack([(fr["occ_mask"][..., 0] > 0).sum() for fr in with_occ]).cpu()
        for fr, c in zip(with_occ, counts.tolist()):
            fr["occ_count"] = int(c)
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
