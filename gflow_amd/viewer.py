"""Free-viewpoint playback of a saved fit -- the counterpart of gflow/viewer.py, headless.

The reference's viewer loads the per-frame checkpoints of a log folder (viewer.py:38-64), and in a loop renders the
current frame from the camera of a web client on a white background and hands the uint8 image over (viewer.py:201-228).
Here the same pieces are functions: ``log_loader`` / ``load_ckpt`` with the reference's semantics, the camera-to-world
quaternion / position conversion of viewer.py:66-82 on the project's own pose algebra (geometry.py), a ``ViewerSession``
that keeps every checkpoint on the device as ONE activated row block and renders through the batched inference rasteriser
(render.render_block: uint8 written by the blend kernel), camera paths as pure functions of the training cameras, and a
command line that writes a path's images with PIL:

    python -m gflow_amd.viewer --folder LOG --path follow|fixed:T|offset:dx,dy,dz|orbit:T,N,R|lerp:A,B,N --out DIR
                               [--format png|jpeg] [--gpu 0] [--slowmo K] [--layer all|still|moving] [--edit TEXT ...]
                               [--video FILE.avi [--fps 5] [--quality 90]]      (one Motion-JPEG AVI; --out is then optional)

The rows of a clip fit keep their index from frame to frame and carry a still / moving label, so the session also shows the
clip BETWEEN its frames, one layer of it, or a group of it moved, turned, resized, tinted or hidden (``frame_at`` / ``play_at``,
``Edit``, ``slowmo``, ``camera_at``): the row composer gfl_compose_rows makes those rows on the device in front of the same
rasteriser (render.render_composed).

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
    return _activated(torch.load(path, map_location=device, weights_only=False), device)


def _activated(ckpt, device):
    a = ckpt["attributes"]
    return (a["xyz"].detach(), ACTIVATIONS["scale"](a["scale"].detach()), ACTIVATIONS["rotate"](a["rotate"].detach()),
            ACTIVATIONS["opacity"](a["opacity"].detach()), ACTIVATIONS["rgb"](a["rgb"].detach()),
            ckpt["intr"].detach().to(device), ckpt["extr"].detach().to(device))


def load_labels(ckpt, n):
    """The group of each of a checkpoint's ``n`` rows, uint8 (n,) on the CPU, from the checkpoint dict's ``still_mask`` (the
    still / moving split of the joint stages, trainer.py:468-471): 0 = still, 1 = moving.  No mask: all still.  A mask
    shorter than ``n`` (rows densified after the last joint stage) is padded as still."""
    n = int(n)
    out = torch.zeros(n, dtype=torch.uint8)
    mask = ckpt.get("still_mask")
    if mask is not None:
        m = min(n, int(mask.shape[0]))
        out[:m] = (~mask.detach().reshape(-1)[:m].to("cpu").bool()).to(torch.uint8)
    return out


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


# ------------------------------------------------------------------ time: in-between cameras and frames
def split_time(tau, T):
    """time tau in [0, T - 1] -> (a, b, s): the frames around it and the weight of b.  An integral tau is (tau, tau, 0.0)."""
    tau = float(tau)
    if not 0.0 <= tau <= T - 1:
        raise ValueError(f"gflow_amd.viewer: time {tau} outside [0, {T - 1}]")
    a = int(math.floor(tau))
    s = tau - a
    return a, (min(a + 1, T - 1) if s > 0.0 else a), s


def camera_at(extrs, intrs, tau):
    """The camera of time tau between the cameras (T,3,4) / (T,4) of the frames: ``slerp`` of the camera-to-world rotation, lerp
    of the position and of the intrinsics, a = floor(tau), b = min(a + 1, T - 1), s = tau - a.  An integral tau returns
    frame tau's own values.  Returns (extr (3,4), intr (4,))."""
    a, b, s = split_time(tau, extrs.shape[0])
    if s == 0.0:
        return extrs[a], intrs[a]
    qa, pa = extr_to_quat_pos(extrs[a])
    qb, pb = extr_to_quat_pos(extrs[b])
    return quat_pos_to_extr(slerp(qa, qb, s), (1.0 - s) * pa + s * pb), (1.0 - s) * intrs[a] + s * intrs[b]


def slowmo(T, k):
    """the (T - 1) k + 1 times 0, 1/k, ..., T - 1 of a clip of T frames slowed k times; the integral ones are exact (i // k)"""
    T, k = int(T), int(k)
    if T < 1 or k < 1:
        raise ValueError(f"gflow_amd.viewer: slowmo({T}, {k})")
    return [float(i // k) if i % k == 0 else i // k + (i % k) / k for i in range((T - 1) * k + 1)]


# ------------------------------------------------------------------ group edits
GROUPS = {"still": 0, "moving": 1}
MAX_GROUPS = 8
_AXES = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}


class Edit:
    """What happens to the rows of one group (gfl_compose_rows, include/gflow_hip.h): opacity x ``gain`` (0 hides the group);
    about ``pivot`` -- None: the centroid of the group's rows in frame a -- a scaling by ``size`` and a turn by ``turn`` =
    (axis, degrees), the axis 'x' | 'y' | 'z' or a 3-vector; then ``shift``; the colour moved towards ``tint`` by ``mix``."""

    __slots__ = ("gain", "size", "turn", "pivot", "shift", "tint", "mix")

    def __init__(self, gain=1.0, size=1.0, turn=("y", 0.0), pivot=None, shift=(0.0, 0.0, 0.0), tint=(0.0, 0.0, 0.0), mix=0.0):
        axis, degrees = turn
        axis = _AXES[axis] if isinstance(axis, str) else tuple(float(x) for x in axis)
        if len(axis) != 3 or not any(axis):
            raise ValueError(f"gflow_amd.viewer: the axis of a turn is x, y, z or a non-zero 3-vector, not {turn[0]!r}")
        self.gain, self.size, self.turn = float(gain), float(size), (axis, float(degrees))
        self.pivot = None if pivot is None else tuple(float(x) for x in pivot)
        self.shift, self.tint, self.mix = tuple(float(x) for x in shift), tuple(float(x) for x in tint), float(mix)
        if len(self.shift) != 3 or len(self.tint) != 3 or (self.pivot is not None and len(self.pivot) != 3):
            raise ValueError("gflow_amd.viewer: pivot, shift and tint have three components")

    def key(self):
        return (self.gain, self.size, self.turn, self.pivot, self.shift, self.tint, self.mix)

    def hidden(self):
        """this edit with gain 0: how a layer hides the other group"""
        return Edit(0.0, self.size, self.turn, self.pivot, self.shift, self.tint, self.mix)

    def quat(self):
        """the turn as a unit quaternion wxyz; no turn is (1, 0, 0, 0) exactly"""
        axis, degrees = self.turn
        if degrees == 0.0:
            return (1.0, 0.0, 0.0, 0.0)
        n = math.sqrt(sum(x * x for x in axis))
        h = math.radians(degrees) / 2.0
        return (math.cos(h),) + tuple(math.sin(h) * x / n for x in axis)

    def moves(self):
        return self.size != 1.0 or self.turn[1] != 0.0 or any(self.shift)

    def row(self):
        """the 16 floats of the table: gain | size | q wxyz | pivot | shift | tint | mix (a None pivot as zeros)"""
        return [self.gain, self.size, *self.quat(), *(self.pivot or (0.0, 0.0, 0.0)), *self.shift, *self.tint, self.mix]

    @staticmethod
    def table(session, frames, edits):
        """[J][G][16] float32 on the session's device for the jobs whose frame a is frames[j]; ``edits``: {group: Edit}, G =
        the largest group + 1.  The rows of the groups come from the host once per distinct set of edits (the session keeps
        them); a None pivot is filled in with torch on the device, from frame a's rows: nothing is read back."""
        edits = {int(g): e for g, e in edits.items()}
        if not edits or min(edits) < 0 or max(edits) >= MAX_GROUPS:
            raise ValueError(f"gflow_amd.viewer: edits are for the groups 0 .. {MAX_GROUPS - 1}")
        G = max(edits) + 1
        key = tuple((g, edits[g].key()) for g in sorted(edits))
        base = session._tables.get(key)
        if base is None:
            rows = [(edits[g] if g in edits else Edit()).row() for g in range(G)]
            base = session._tables[key] = torch.tensor(rows, dtype=torch.float32).to(session.device)
        frames = [int(t) for t in frames]
        table = base.unsqueeze(0).repeat(len(frames), 1, 1)
        for g, e in edits.items():
            if e.pivot is None and e.moves():
                for t in sorted(set(frames)):
                    first, count = session.ranges[t]
                    w = (session.labels[first:first + count] == g).float().unsqueeze(1)
                    centre = (session.block[first:first + count, 0:3] * w).sum(0) / w.sum().clamp(min=1.0)
                    if len(set(frames)) == 1:
                        table[:, g, 6:9] = centre
                    else:
                        table[[j for j, f in enumerate(frames) if f == t], g, 6:9] = centre
        return table.contiguous()


def parse_edit(text):
    """'GROUP:key=value;key=value...' -> (group, Edit).  GROUP: still | moving | 0 .. 7; keys: gain=G, size=S, turn=AXIS,DEGREES
    (AXIS x | y | z) or turn=ax,ay,az,DEGREES, pivot=x,y,z, shift=x,y,z, tint=r,g,b,MIX.  ValueError naming the text otherwise."""
    try:
        head, sep, rest = str(text).partition(":")
        if not sep or not rest:
            raise ValueError
        group = GROUPS[head] if head in GROUPS else int(head)
        if not 0 <= group < MAX_GROUPS or (head not in GROUPS and head != str(group)):
            raise ValueError
        kw = {}
        for part in rest.split(";"):
            k, eq, val = part.partition("=")
            vals = val.split(",")
            if not eq or k in kw:
                raise ValueError
            if k in ("gain", "size"):
                (x,) = vals
                kw[k] = float(x)
            elif k in ("pivot", "shift"):
                x, y, z = vals
                kw[k] = (float(x), float(y), float(z))
            elif k == "tint":
                r, g, b, m = vals
                kw["tint"], kw["mix"] = (float(r), float(g), float(b)), float(m)
            elif k == "turn":
                if len(vals) == 2 and vals[0] in _AXES:
                    kw[k] = (vals[0], float(vals[1]))
                else:
                    x, y, z, d = vals
                    kw[k] = ((float(x), float(y), float(z)), float(d))
            else:
                raise ValueError
        edit = Edit(**kw)
        if not all(math.isfinite(x) for x in edit.row()):
            raise ValueError
        return group, edit
    except (KeyError, ValueError):
        raise ValueError(f"--edit {text!r}: expected GROUP:key=value;... with GROUP still | moving | 0..7 and the keys gain=G, "
                         "size=S, turn=AXIS,DEGREES, pivot=x,y,z, shift=x,y,z, tint=r,g,b,MIX") from None


LAYERS = {"all": None, "still": 1, "moving": 0}          # a layer hides the OTHER group: layer -> the group with gain 0


def _with_layer(layer, edits):
    """{group: Edit} of a layer and the caller's edits (a dict or (group, Edit) pairs); None when nothing is to be done"""
    if layer not in LAYERS:
        raise ValueError(f"gflow_amd.viewer: layer {layer!r}: expected all | still | moving")
    out = {}
    for g, e in (edits.items() if isinstance(edits, dict) else edits or ()):
        g = GROUPS[g] if g in GROUPS else int(g)
        if g in out:
            raise ValueError(f"gflow_amd.viewer: two edits for group {g}")
        out[g] = e
    hide = LAYERS[layer]
    if hide is not None:
        out[hide] = out.get(hide, Edit()).hidden()
        out.setdefault(1 - hide, Edit())
    return out or None


# ------------------------------------------------------------------ session
class ViewerSession:
    """Every checkpoint of a log folder on the device, as one concatenated [R][16] ACTIVATED row block and a row range per
    frame; images come out of the batched inference rasteriser as uint8 on the device.  ``bg``: the reference's viewer
    shows a white background (viewer.py:93-94).  ``labels`` (R,) uint8 holds every row's group beside the block -- 0 still,
    1 moving, from the checkpoints' ``still_mask`` (load_labels), or from ``labels=``, one tensor per frame."""

    def __init__(self, folder, device="cuda", bg=1.0, labels=None):
        from . import render as R
        self._R = R
        self.device = torch.device(device)
        self.files, self.W, self.H = log_loader(folder)
        self.bg = float(bg)
        if labels is not None and len(labels) != len(self.files):
            raise ValueError(f"gflow_amd.viewer: {len(self.files)} frames, {len(labels)} label tensors")
        blocks, intrs, extrs, groups, self.ranges = [], [], [], [], []
        at = 0
        for k, f in enumerate(self.files):
            ckpt = torch.load(f, map_location=self.device, weights_only=False)
            xyz, scale, rotate, opacity, rgb, intr, extr = _activated(ckpt, self.device)
            n = xyz.shape[0]
            blocks.append(R.rows_block(dict(xyz=xyz, scale=scale, rotate=rotate, opacity=opacity, rgb=rgb)))
            if labels is None:
                groups.append(load_labels(ckpt, n))
            else:
                if labels[k].numel() != n:
                    raise ValueError(f"gflow_amd.viewer: frame {k} has {n} rows, its labels {labels[k].numel()}")
                groups.append(labels[k].detach().reshape(n).to("cpu").to(torch.uint8))
            self.ranges.append((at, n))
            at += n
            intrs.append(intr.float().reshape(4))
            extrs.append(extr.float().reshape(3, 4))
        self.block = torch.cat(blocks).contiguous()
        self.labels = torch.cat(groups).to(self.device).contiguous()
        self.rows_max = max(c for _, c in self.ranges)
        self.intrs = torch.stack(intrs)
        self.extrs = torch.stack(extrs)              # the training cameras (T,3,4): what the camera paths are functions of
        self._cameras = (self.extrs.cpu(), self.intrs.cpu())      # (host copies: camera_at's slerp branches on values)
        self._camera_cache = {}                      # time -> camera_at's (extr, intr) on the device
        self._tables = {}                            # Edit.table's group rows on the device, per distinct set of edits
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

    def _compose(self, taus, extrs, intrs, layer, edits, rows=False):
        """the jobs of the times ``taus`` through render.render_composed: cameras (n,3,4) / (n,4) on the device"""
        timed = not torch.cuda.is_current_stream_capturing()         # (a captured call has no events of its own: fps stays)
        if timed:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
        T = len(self)
        src, weights, frames = [], [], []
        for tau in taus:
            a, b, s = split_time(tau, T)
            src.append(self.ranges[a] + self.ranges[b])
            weights.append(s)
            frames.append(a)
        edits = _with_layer(layer, edits)
        table = Edit.table(self, frames, edits) if edits and frames else None
        res = self._R.render_composed(self.block, self.labels, src, weights, table, intrs, extrs, self.bg, self.W, self.H,
                                      self.rows_max, uint8=True, rows=rows)
        if timed:
            end.record()
            self._timing = (start, end, len(frames))
        if frames:
            self._shown = frames[-1]
        return res

    def frame_at(self, tau, extr=None, layer="all", edits=None, rows=False):
        """The clip at time tau in [0, T - 1]: the rows of frames floor(tau) and the next one blended (gfl_compose_rows), from
        ``extr`` (3,4) or from the camera ``camera_at`` gives; ``layer``: all | still | moving (the other group gets gain 0);
        ``edits``: {group: Edit} or (group, Edit) pairs, groups 0 .. 7 or 'still' / 'moving'.  (H,W,3) uint8 on the device, one
        job; with ``rows`` the whole dict of render.render_composed.  After a first call with the same time and edits (and
        with ``extr``, if given, on the device) nothing is copied from the host: such a call can be captured into a graph."""
        a, b, s = split_time(tau, len(self))
        if extr is None:
            e, i = self._camera(tau)
        else:
            e, i = extr, (self.intrs[a] if s == 0.0 else (1.0 - s) * self.intrs[a] + s * self.intrs[b])
        res = self._compose([tau], e.reshape(1, 3, 4).to(self.device).float(), i.reshape(1, 4).to(self.device).float(), layer, edits, rows)
        return res if rows else res["img"][0]

    def _camera(self, tau):
        """``camera_at`` of the training cameras on the device, kept per time: the slerp runs on the host (it branches on
        values) once per distinct tau, a replayed path costs a lookup"""
        tau = float(tau)
        cam = self._camera_cache.get(tau)
        if cam is None:
            if len(self._camera_cache) >= 1 << 16:
                self._camera_cache.clear()
            e, i = camera_at(*self._cameras, tau)
            cam = self._camera_cache[tau] = (e.float().to(self.device), i.float().to(self.device))
        return cam

    def play_at(self, taus, extrs=None, layer="all", edits=None):
        """the clip at every time of ``taus`` (``slowmo``), time i from extrs[i] or from ``camera_at``: (n,H,W,3) uint8, in
        batched calls"""
        taus = [float(t) for t in taus]
        cams = [self._camera(t) for t in taus]
        intrs = torch.stack([c[1] for c in cams]) if cams else torch.zeros(0, 4, device=self.device)
        if extrs is None:
            extrs = torch.stack([c[0] for c in cams]) if cams else torch.zeros(0, 3, 4, device=self.device)
        elif extrs.shape[0] != len(taus):
            raise ValueError(f"gflow_amd.viewer: {len(taus)} times, {extrs.shape[0]} cameras")
        return self._compose(taus, extrs.to(self.device).float(), intrs, layer, edits)["img"]

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
    ap.add_argument("--out", default=None, help="directory the images are written to (needed unless --video is given)")
    ap.add_argument("--format", default="png", choices=("png", "jpeg"))
    ap.add_argument("--video", default=None, metavar="FILE.avi",
                    help="write the path as ONE Motion-JPEG AVI, coded on the device (gflow_amd.video), instead of images")
    ap.add_argument("--fps", type=float, default=5, help="with --video: frames per second of the file")
    ap.add_argument("--quality", type=int, default=90, help="with --video: JPEG quality, 1 .. 100")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--slowmo", type=int, default=0, metavar="K",
                    help="K images per frame step: the times 0, 1/K, ... of the clip, rows and cameras blended in between "
                         "(with --path follow | fixed:T | offset:dx,dy,dz)")
    ap.add_argument("--layer", default="all", choices=tuple(LAYERS), help="show only the still or only the moving splats")
    ap.add_argument("--edit", action="append", default=[], metavar="TEXT",
                    help="GROUP:key=value;... with GROUP still | moving | 0..7 and the keys gain, size, turn=AXIS,DEGREES, "
                         "pivot=x,y,z, shift=x,y,z, tint=r,g,b,MIX; may be given several times")
    args = ap.parse_args(argv)
    if not args.out and not args.video:
        ap.error("one of --out and --video is needed")
    kind, pargs = parse_path(args.path)
    edits = [parse_edit(t) for t in args.edit]
    if args.slowmo < 0 or (args.slowmo and kind not in ("follow", "fixed", "offset")):
        raise ValueError(f"--slowmo {args.slowmo}: expected K >= 1 with --path follow | fixed:T | offset:dx,dy,dz")
    session = ViewerSession(args.folder, torch.device("cuda", args.gpu))
    frames, extrs = session.path(kind, pargs)
    if args.slowmo:
        # the path gives a camera per frame: the cameras of the times in between are interpolated like the training cameras
        taus = slowmo(len(session), args.slowmo)
        path_cpu = extrs.cpu()
        imgs = session.play_at(taus, torch.stack([camera_at(path_cpu, session._cameras[1], t)[0] for t in taus]), args.layer, edits)
    elif edits or args.layer != "all":
        imgs = session.play_at(frames, extrs, args.layer, edits)
    else:
        imgs = session._render(frames, extrs)
    if args.video:
        # the images stay on the device until they are the file's bytes
        from . import video
        session._R.check_overflow()
        d = os.path.dirname(args.video)
        if d:
            os.makedirs(d, exist_ok=True)
        info = video.write_avi(args.video, imgs, fps=args.fps, quality=args.quality)
        print(f"{info['frames']} frames of {session.W}x{session.H} at {args.fps:g} fps -> {args.video}  ({info['bytes']} bytes)")
        if not args.out:
            return 0
    imgs = imgs.cpu().numpy()
    session._R.check_overflow()
    os.makedirs(args.out, exist_ok=True)
    for k, im in enumerate(imgs):
        Image.fromarray(im).save(os.path.join(args.out, f"{k:06d}.{args.format}"))
    print(f"{len(imgs)} images of {session.W}x{session.H} -> {args.out}  ({session.fps:.0f} images/s on the device)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
