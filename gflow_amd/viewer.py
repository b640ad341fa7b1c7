"""Free-viewpoint playback of a saved fit -- the counterpart of gflow/viewer.py, headless.

The reference's viewer loads the per-frame checkpoints of a log folder (viewer.py:38-64), and in a loop renders the
current frame from the camera of a web client on a white background and hands the uint8 image over (viewer.py:201-228).
Here the same pieces are functions: ``log_loader`` / ``load_ckpt`` with the reference's semantics, the camera-to-world
quaternion / position conversion of viewer.py:66-82 on the project's own pose algebra (geometry.py), a ``ViewerSession``
that keeps every checkpoint on the device as ONE activated row block and renders through the batched inference rasteriser
(render.render_block: uint8 written by the blend kernel), camera paths as pure functions of the training cameras, and a
command line that writes a path's images with PIL:

    python -m gflow_amd.viewer --folder LOG --path follow|fixed:T|offset:dx,dy,dz|orbit:T,N,R|lerp:A,B,N --out DIR
                               [--format png|jpeg] [--gpu 0]

A live web server is not part of this module ("Viewer and batched views": the reference's
``while True`` loop is ten lines around ``ViewerSession.frame``).
"""
import argparse
import math
import os

import torch

from .geometry import pose_to_extr, rotmat_to_unitquat_xyzw

# viewer.py:28-36 (the trainer's own, trainer.py:64-69)
ACTIVATIONS = {
    "scale": torch.abs,
    "rotate": torch.nn.functional.normalize,
    "opacity": lambda x: torch.sigmoid(x * 10.0),
    "rgb": torch.sigmoid,
}


def log_loader(folder):
    """(sorted checkpoint paths of ``folder``/ckpt/*.tar, width, height of the first one) -- viewer.py:38-48."""
    ckpt_dir = os.path.join(folder, "ckpt")
    files = sorted(os.path.join(ckpt_dir, f) for f in os.listdir(ckpt_dir) if f.endswith(".tar"))
    if not files:
        raise FileNotFoundError(f"gflow_amd.viewer: no ckpt/*.tar in {folder}")
    first = torch.load(files[0], map_location="cpu", weights_only=False)
    return files, int(first["width"]), int(first["height"])


def load_ckpt(path, device):
    """A checkpoint of SimpleGaussian.save_checkpoint as ACTIVATED attributes: (xyz, |scale|, normalised rotate,
    sigmoid(10 opacity), sigmoid(rgb), intr, extr) on ``device`` -- viewer.py:50-64."""
    ckpt = torch.load(path, map_location=device, weights_only=False)
    a = ckpt["attributes"]
    return (a["xyz"].detach(), ACTIVATIONS["scale"](a["scale"].detach()), ACTIVATIONS["rotate"](a["rotate"].detach()),
            ACTIVATIONS["opacity"](a["opacity"].detach()), ACTIVATIONS["rgb"](a["rgb"].detach()),
            ckpt["intr"].detach().to(device), ckpt["extr"].detach().to(device))


# ------------------------------------------------------------------ pose conversion (viewer.py:66-82)
def extr_to_quat_pos(extr):
    """extr (3,4) world -> camera  ->  (q, pos): the CAMERA-TO-WORLD rotation as a unit quaternion in xyzw order (4,) and the
    camera's position (3,), tensors of extr's dtype and device.  (The web client's wxyz is q[[3, 0, 1, 2]].)  The inverse of
    a rigid [R | t] is [R^T | -R^T t]: no 4x4 inversion."""
    extr = extr.detach()
    Rt = extr[:3, :3].T
    return rotmat_to_unitquat_xyzw(Rt), -(Rt @ extr[:3, 3])


def quat_pos_to_extr(q_xyzw, pos):
    """(camera-to-world quaternion xyzw, camera position) -> extr (3,4) world -> camera.  q need not be normalised; q and -q
    give the same matrix."""
    q = torch.as_tensor(q_xyzw)
    q = q if q.is_floating_point() else q.float()
    pos = torch.as_tensor(pos, dtype=q.dtype, device=q.device)
    c2w = pose_to_extr(torch.cat([q, pos]))                  # [R(q) | pos]
    Rt = c2w[:, :3].T
    return torch.cat([Rt, -(Rt @ pos).unsqueeze(1)], dim=1)


# ------------------------------------------------------------------ camera paths: pure functions of the training cameras
def follow(extrs):
    """the training view of every frame: (T,3,4) -> the same"""
    return extrs


def fixed(extrs, t0):
    """every frame from the training camera of frame t0"""
    return extrs[int(t0)].unsqueeze(0).expand(extrs.shape[0], 3, 4).clone()


def offset(extrs, dx, dy, dz):
    """every training camera moved by (dx, dy, dz) in ITS OWN frame (x right, y down, z forward), looking the same way:
    x_cam = R (x - C), so C -> C + R^T d is t -> t - d.  A stereo baseline b is offset(b, 0, 0)."""
    out = extrs.clone()
    out[..., 3] = out[..., 3] - torch.as_tensor([dx, dy, dz], dtype=extrs.dtype, device=extrs.device)
    return out


def look_at(centre, target, down):
    """extr (3,4) of a camera at ``centre`` whose optical axis passes through ``target``; ``down`` fixes the roll (the
    image's y axis is ``down`` made orthogonal to the axis)."""
    z = target - centre
    z = z / torch.linalg.norm(z)
    x = torch.linalg.cross(down, z)
    x = x / torch.linalg.norm(x)
    y = torch.linalg.cross(z, x)
    R = torch.stack([x, y, z])
    return torch.cat([R, -(R @ centre).unsqueeze(1)], dim=1)


def orbit(extr, n, radius, look_at_depth):
    """n cameras on a circle of ``radius`` around the position of the camera ``extr`` (3,4), in the plane across its optical
    axis, all looking at the point ``look_at_depth`` ahead of it on that axis: the point stays on every camera's axis and at
    one distance, sqrt(depth^2 + radius^2).  Returns (n,3,4)."""
    R, t = extr[:, :3], extr[:, 3]
    C = -(R.T @ t)
    ax, ay, az = R[0], R[1], R[2]                            # the camera's axes in the world
    P = C + float(look_at_depth) * az
    out = []
    for k in range(int(n)):
        a = 2.0 * math.pi * k / int(n)
        out.append(look_at(C + float(radius) * (math.cos(a) * ax + math.sin(a) * ay), P, ay))
    return torch.stack(out)


def slerp(q0, q1, s):
    """unit quaternions (4,), s in [0, 1]: the shorter great arc from q0 to q1"""
    d = torch.dot(q0, q1)
    if d < 0:
        q1, d = -q1, -d
    d = torch.clamp(d, -1.0, 1.0)
    theta = torch.acos(d)
    if float(theta) < 1e-6:
        q = (1.0 - s) * q0 + s * q1
    else:
        q = (torch.sin((1.0 - s) * theta) * q0 + torch.sin(s * theta) * q1) / torch.sin(theta)
    return q / torch.linalg.norm(q)


def lerp(extr_a, extr_b, n):
    """n cameras from ``extr_a`` to ``extr_b`` (both ends included): slerp of the rotation, lerp of the position.  (n,3,4)"""
    qa, pa = extr_to_quat_pos(extr_a)
    qb, pb = extr_to_quat_pos(extr_b)
    n = int(n)
    out = []
    for k in range(n):
        s = k / (n - 1) if n > 1 else 0.0
        out.append(quat_pos_to_extr(slerp(qa, qb, s), (1.0 - s) * pa + s * pb))
    return torch.stack(out)


def parse_path(text):
    """'follow' | 'fixed:T' | 'offset:dx,dy,dz' | 'orbit:T,N,R' | 'lerp:A,B,N' -> (kind, args tuple); ValueError naming the
    text otherwise."""
    kind, sep, rest = str(text).partition(":")
    forms = {"follow": (), "fixed": (int,), "offset": (float, float, float), "orbit": (int, int, float), "lerp": (int, int, int)}
    try:
        types = forms[kind]
        parts = rest.split(",") if rest else []
        if len(parts) != len(types) or (not types and sep):
            raise ValueError
        args = tuple(t(p) for t, p in zip(types, parts))
    except (KeyError, ValueError):
        raise ValueError(f"--path {text!r}: expected follow | fixed:T | offset:dx,dy,dz | orbit:T,N,R | lerp:A,B,N") from None
    if (kind in ("orbit", "lerp") and args[-2 if kind == "orbit" else -1] < 1) or (kind == "orbit" and args[2] < 0):
        raise ValueError(f"--path {text!r}: the number of cameras must be at least 1 and a radius not negative")
    return kind, args


# ------------------------------------------------------------------ session
class ViewerSession:
    """Every checkpoint of a log folder on the device, as one concatenated [R][16] ACTIVATED row block and a row range per
    frame; images come out of the batched inference rasteriser as uint8 on the device.  ``bg``: the reference's viewer
    shows a white background (viewer.py:93-94)."""

    def __init__(self, folder, device="cuda", bg=1.0):
        from . import render as R
        self._R = R
        self.device = torch.device(device)
        self.files, self.W, self.H = log_loader(folder)
        self.bg = float(bg)
        blocks, intrs, extrs, self.ranges = [], [], [], []
        at = 0
        for f in self.files:
            xyz, scale, rotate, opacity, rgb, intr, extr = load_ckpt(f, self.device)
            blocks.append(R.rows_block(dict(xyz=xyz, scale=scale, rotate=rotate, opacity=opacity, rgb=rgb)))
            self.ranges.append((at, xyz.shape[0]))
            at += xyz.shape[0]
            intrs.append(intr.float().reshape(4))
            extrs.append(extr.float().reshape(3, 4))
        self.block = torch.cat(blocks).contiguous()
        self.intrs = torch.stack(intrs)
        self.extrs = torch.stack(extrs)              # the training cameras (T,3,4): what the camera paths are functions of
        self._timing = None
        self._shown = 0

    def __len__(self):
        return len(self.files)

    @property
    def n_gaussians(self):
        """splats of the frame shown last (the reference's "Number of Gaussians")"""
        return self.ranges[self._shown][1]

    @property
    def fps(self):
        """images per second of the last call, from device events around it (waits for that call; 0.0 before the first)"""
        if self._timing is None:
            return 0.0
        start, end, n = self._timing
        end.synchronize()
        ms = start.elapsed_time(end)
        return 1000.0 * n / ms if ms > 0 else float("inf")

    def look_at_depth(self, t):
        """median depth of frame t's splats in front of its training camera: the orbit's centre lies there on the axis"""
        a, c = self.ranges[t]
        z = self.block[a:a + c, 0:3] @ self.extrs[t][2, :3] + self.extrs[t][2, 3]
        z = z[z > 0]
        return float(z.median()) if z.numel() else 1.0

    def _render(self, frames, extrs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        frames = [int(t) for t in frames]
        img = self._R.render_block(self.block, [self.ranges[t] for t in frames], self.intrs[frames], extrs.to(self.device).float(),
                                   self.bg, self.W, self.H, uint8=True)["img"]
        end.record()
        self._timing = (start, end, len(frames))
        if frames:
            self._shown = frames[-1]
        return img

    def frame(self, t, extr=None):
        """frame t from ``extr`` (3,4) world -> camera, or from its training view (None: the reference's "follow"):
        (H,W,3) uint8 on the device.  One job."""
        e = self.extrs[int(t)] if extr is None else extr
        return self._render([t], e.reshape(1, 3, 4))[0]

    def play(self, extrs):
        """frame i from extrs[i], for all T frames: (T,3,4) -> (T,H,W,3) uint8, in batched calls"""
        if extrs.shape[0] != len(self):
            raise ValueError(f"gflow_amd.viewer: {len(self)} frames, {extrs.shape[0]} cameras")
        return self._render(range(len(self)), extrs)

    def views(self, t, extrs):
        """frame t from V cameras: (V,3,4) -> (V,H,W,3) uint8"""
        return self._render([int(t)] * extrs.shape[0], extrs)

    def path(self, kind, args=()):
        """(frame indices, cameras (n,3,4)) of a parsed --path"""
        T = len(self)
        if kind == "follow":
            return list(range(T)), follow(self.extrs)
        if kind == "fixed":
            return list(range(T)), fixed(self.extrs, args[0])
        if kind == "offset":
            return list(range(T)), offset(self.extrs, *args)
        if kind == "orbit":
            t, n, radius = args
            return [t] * n, orbit(self.extrs[t], n, radius, self.look_at_depth(t))
        if kind == "lerp":
            a, b, n = args
            return [int(round(a + (b - a) * (k / (n - 1) if n > 1 else 0.0))) for k in range(n)], lerp(self.extrs[a], self.extrs[b], n)
        raise ValueError(f"gflow_amd.viewer: unknown path {kind!r}")


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(description="render a camera path through a saved fit to image files")
    ap.add_argument("--folder", required=True, help="log folder (holds ckpt/*.tar)")
    ap.add_argument("--path", default="follow", help="follow | fixed:T | offset:dx,dy,dz | orbit:T,N,R | lerp:A,B,N")
    ap.add_argument("--out", required=True, help="directory the images are written to")
    ap.add_argument("--format", default="png", choices=("png", "jpeg"))
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
    kind, pargs = parse_path(args.path)
    session = ViewerSession(args.folder, torch.device("cuda", args.gpu))
    frames, extrs = session.path(kind, pargs)
    imgs = session._render(frames, extrs).cpu().numpy()
    session._R.check_overflow()
    os.makedirs(args.out, exist_ok=True)
    for k, im in enumerate(imgs):
        Image.fromarray(im).save(os.path.join(args.out, f"{k:06d}.{args.format}"))
    print(f"{len(imgs)} images of {session.W}x{session.H} -> {args.out}  ({session.fps:.0f} images/s on the device)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
