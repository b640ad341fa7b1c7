"""Back-projection helpers on the hot path (reference: gflow/utils/geometry.py:95-120), the pose algebra of the camera
(trainer.py:115-121) and two small tensor helpers of the trainer."""
import torch


def inv(mat):
    """torch.linalg.inv without its error check (the check reads a status word back from the device: a full stop of
    the host in the middle of a fit; a singular extrinsic does not occur -- it is a rotation and a translation)."""
    return torch.linalg.inv_ex(mat, check_errors=False).inverse


def depth2pts3d(depth, xys, focal, pp):
    """depth (N,1), xys (N,2) pixels -> camera-space points (N,3) (geometry.py:118-119)."""
    return torch.cat((depth * (xys - pp) / focal, depth), dim=-1)


def geotrf(Trf, pts):
    """Apply a 4x4 rigid transform to (N,3) points (the only case pix2world uses)."""
    return pts @ Trf[:3, :3].T + Trf[:3, 3]


def pix2world(uv, depth, intr, extr):
    """uv (N,2), depth (N,1), intr (4,) [fx,fy,cx,cy], extr (3,4) world->camera.
    Like the reference (geometry.py:105-106) the single focal intr[0] is used for both
    axes."""
    rel = depth2pts3d(depth, uv, intr[0], intr[2:])
    # camera -> world of the rigid world -> camera transform [R | t]: [R^T | -R^T t].  The reference inverts the 4x4
    # numerically (geometry.py:107); for a rotation + translation that is the same matrix up to rounding, and the
    # closed form is three small kernels instead of an LU factorisation in the middle of a fit
    Rt = extr[:3, :3].T
    return rel @ Rt.T + (-(Rt @ extr[:3, 3]))


def pose_to_extr(pose):
    """pose [qx,qy,qz,qw,tx,ty,tz] (XYZW, identity [0,0,0,1,0,0,0]) -> (3,4) world->camera:
    what roma.RigidUnitQuat(Q,T).normalize().to_homogeneous()[:3] gives
    (trainer.py:115-121; signed_expm1 is the identity, utils/__init__.py:11-15)."""
    # R is linear in the ten products q_i q_j: ONE outer product and ONE (9 x 16) matrix-vector product instead of ~40
    # scalar kernels (this runs at every frame boundary and densification event of a fit, between two graph launches)
    q = pose[:4] / torch.linalg.norm(pose[:4])
    qq = (q.unsqueeze(1) * q.unsqueeze(0)).reshape(16)                  # [xx xy xz xw | yx yy yz yw | zx zy zz zw | wx wy wz ww]
    C, I9 = _quat_to_rot_constants(pose.device, pose.dtype)
    R = (I9 + C @ qq).reshape(3, 3)
    return torch.cat([R, pose[4:7].unsqueeze(1)], dim=1)


_Q2R = {}


def _quat_to_rot_constants(device, dtype):
    key = (str(device), dtype)
    if key not in _Q2R:
        xx, xy, xz, xw, yy, yz, yw, zz, zw = 0, 1, 2, 3, 5, 6, 7, 10, 11
        C = torch.zeros(9, 16, dtype=torch.float64)
        for row, terms in enumerate((
                ((yy, -2), (zz, -2)), ((xy, 2), (zw, -2)), ((xz, 2), (yw, 2)),
                ((xy, 2), (zw, 2)), ((xx, -2), (zz, -2)), ((yz, 2), (xw, -2)),
                ((xz, 2), (yw, -2)), ((yz, 2), (xw, 2)), ((xx, -2), (yy, -2)))):
            for col, val in terms:
                C[row, col] = val
        I9 = torch.eye(3, dtype=torch.float64).reshape(9)
        _Q2R[key] = (C.to(dtype).to(device), I9.to(dtype).to(device))
    return _Q2R[key]


def rotmat_to_unitquat_xyzw(R):
    """roma.rotmat_to_unitquat restated (XYZW, w >= 0 branch-free variant)."""
    m = R.double()
    t = m[0, 0] + m[1, 1] + m[2, 2]
    cands = torch.stack([
        torch.stack([m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + t]),
        torch.stack([1 + m[0, 0] - m[1, 1] - m[2, 2], m[0, 1] + m[1, 0], m[0, 2] + m[2, 0], m[2, 1] - m[1, 2]]),
        torch.stack([m[0, 1] + m[1, 0], 1 - m[0, 0] + m[1, 1] - m[2, 2], m[1, 2] + m[2, 1], m[0, 2] - m[2, 0]]),
        torch.stack([m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], 1 - m[0, 0] - m[1, 1] + m[2, 2], m[1, 0] - m[0, 1]]),
    ])
    best = torch.argmax(torch.stack([1 + t, 1 + m[0, 0] - m[1, 1] - m[2, 2], 1 - m[0, 0] + m[1, 1] - m[2, 2],
                                     1 - m[0, 0] - m[1, 1] + m[2, 2]]))
    q = cands[best]
    return (q / torch.linalg.norm(q)).to(R.dtype)


def device_constant(values, device, dtype=torch.float32):
    """A small constant tensor WITHOUT a host-to-device copy: ``torch.tensor([...], device=)`` copies from pageable memory,
    which stops the host until everything queued on the device has run (7 ms apiece at the start of a fit, right behind the
    zero-filling of the engine's buffers: six of them were 4.6 % of an 8-frame clip fit).  Fills are just launches."""
    out = torch.zeros(len(values), dtype=dtype, device=device)
    for i, v in enumerate(values):
        if v != 0:
            out[i:i + 1].fill_(float(v))
    return out


def within(uv, W, H):
    """rows of uv (N,2) that lie strictly inside the (W, H) image"""
    return (uv[:, 0] > 0) & (uv[:, 0] < W - 1) & (uv[:, 1] > 0) & (uv[:, 1] < H - 1)
