"""gfl_label_frame and gfl_label_assign restated in numpy (include/gflow_hip.h; gflow_amd/propagation.py), and the inputs
the host and GPU tests share.

``label_frame_ref`` walks every tile's list per pixel.  The alpha of a (pixel, splat) is formed in float32 exactly as
splat_alpha (csrc/gfl_splat_alpha.hpp) states it -- the same products, the two fused multiply-adds, alpha = min(cap, o G) --
and the transmittance the stop is decided on is the float32 product chain, so the skip and stop decisions are the
kernel's (up to the last bit of exp); the class sums are kept in ``dtype``: float64 for the reference, float32 for the
restatement that shows how far float32 sums can move a label."""
import numpy as np
import torch

from oracle import msplat_oracle as MO

REC = 12
NONE = 255
TIE = 1e-5                         # margin / |den - min_weight| below this: the label hangs on the last bits of the sums
TIE_SHARE = 0.005                  # at most this share of the image may be left out for it
CONF_BOUND = 1e-5

f32 = np.float32


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum is rounded once there and once to
    float32 (a double rounding that differs from fmaf in about one case in 2^29)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def label_frame_ref(rec, ids, tile_range, labels, n_labels, K, W, H, min_weight=0.5, unknown=NONE, dtype=np.float64):
    """dict(label (H, W) uint8, den, margin (best minus runner-up class sum), conf, acc (K, H, W): in ``dtype``;
    stopped (H, W) bool: the walk ended at the T_MIN stop; walked (H, W) int: list entries looked at)."""
    rec = np.asarray(rec, f32).reshape(-1, REC)
    n = rec.shape[0]
    ids = np.asarray(ids).reshape(-1)
    tr = np.asarray(tile_range).reshape(-1, 2)
    labels = np.asarray(labels, np.uint8).reshape(-1)
    gx = (W + MO.TILE - 1) // MO.TILE
    acc = np.zeros((K, H, W), dtype)
    stopped = np.zeros((H, W), bool)
    walked = np.zeros((H, W), np.int64)
    a_min, a_max, t_min = f32(MO.ALPHA_MIN), f32(MO.ALPHA_MAX), f32(MO.T_MIN)
    for tile in range(len(tr) if n else 0):
        x0, y0 = (tile % gx) * MO.TILE, (tile // gx) * MO.TILE
        ys, xs = np.mgrid[y0:min(y0 + MO.TILE, H), x0:min(x0 + MO.TILE, W)]
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        fx, fy = xs.astype(f32) + f32(MO.PIXEL_CENTER), ys.astype(f32) + f32(MO.PIXEL_CENTER)
        T = np.ones(len(xs), f32)
        live = np.ones(len(xs), bool)
        a = np.zeros((K, len(xs)), dtype)
        for pos in range(int(tr[tile, 0]), int(tr[tile, 1])):
            if not live.any():
                break
            walked[ys[live], xs[live]] += 1
            g = int(ids[pos])
            if not 0 <= g < n:
                continue
            u, v, A, B, C, o = (f32(x) for x in rec[g, 0:6])
            dx, dy = u - fx, v - fy
            q = _fma32(A * dx, dx, (C * dy) * dy)
            power = _fma32(np.full_like(q, -0.5), q, -((B * dx) * dy))
            with np.errstate(over="ignore", under="ignore"):
                G = np.exp(power, dtype=f32)
            alpha = np.minimum(a_max, o * G)
            keep = live & (power <= 0) & (alpha >= a_min)
            test_T = T * (f32(1) - alpha)
            stop = keep & (test_T < t_min)
            stopped[ys[stop], xs[stop]] = True
            live &= ~stop
            keep &= ~stop
            lab = int(labels[g]) if g < n_labels else NONE
            if lab < K:
                w = alpha.astype(dtype) * T.astype(dtype)
                a[lab, keep] += w[keep]
            T = np.where(keep, test_T, T)
        acc[:, ys, xs] = a
    den = acc[0].copy()
    for k in range(1, K):
        den = den + acc[k]
    best = acc.max(axis=0)
    arg = acc.argmax(axis=0)                               # (the first among equals: the smallest k)
    order = np.sort(acc, axis=0)
    margin = order[-1] - order[-2]
    known = den >= dtype(min_weight)
    with np.errstate(divide="ignore", invalid="ignore"):
        conf = np.where(known, best / den, 0).astype(dtype)
    label = np.where(known, arg, unknown).astype(np.uint8)
    return dict(label=label, den=den, margin=margin, conf=conf, acc=acc, stopped=stopped, walked=walked)


def label_assign_ref(rec, map_, W, H, labels):
    """labels (n,) uint8 after gfl_label_assign: plain integer logic, row by row"""
    rec = np.asarray(rec, f32).reshape(-1, REC)
    out = np.array(labels, np.uint8, copy=True)
    m = np.asarray(map_, np.uint8).reshape(H, W)
    for j in range(len(out)):
        if out[j] != NONE:
            continue
        u, v, d = rec[j, 0], rec[j, 1], rec[j, 9]
        if d != 0 and 0 < u < f32(W - 1) and 0 < v < f32(H - 1):       # (a NaN fails every comparison)
            got = m[int(v), int(u)]
            if got != NONE:
                out[j] = got
    return out


def comparable(ref, min_weight=0.5):
    """(H, W) bool: pixels whose label does not hang on the last bits -- the float64 margin and |den - min_weight| both
    above TIE"""
    return (ref["margin"] > TIE) & (np.abs(ref["den"] - min_weight) > TIE)


def compare(label, conf, ref, min_weight=0.5, what=""):
    """The parity check of the issue: equal labels on the comparable pixels, conf within CONF_BOUND there, at most
    TIE_SHARE of the image left out.  Returns (left-out share, worst conf error)."""
    ok = comparable(ref, min_weight)
    share = 1.0 - float(ok.mean())
    bad = int((np.asarray(label)[ok] != ref["label"][ok]).sum())
    worst = float(np.abs(np.asarray(conf, np.float64) - ref["conf"])[ok].max()) if ok.any() else 0.0
    print(f"label parity {what}: left out {share:.4%}, mismatched labels {bad}, worst |conf - ref| {worst:.3g}, "
          f"unknown {float((ref['label'] == NONE).mean()):.3f}, stopped {float(ref['stopped'].mean()):.3f}, "
          f"longest walk {int(ref['walked'].max())}")
    assert share <= TIE_SHARE, (what, share)
    assert bad == 0, (what, bad)
    assert worst <= CONF_BOUND, (what, worst)
    return share, worst


# ------------------------------------------------------------------------------------------------------ shared inputs
W, H = 40, 24                      # 3 x 2 tiles, the last tile column and the last tile row partial
N_FAINT, N_OPAQUE, N_REST = 300, 60, 240
N_UNLISTED = 50                    # rows beyond n_labels


def label_scene(seed=0):
    """dict(xyz, scale, rotate, opacity, rgb, intr, extr, W, H) of float32 tensors, 600 splats under the identity camera:
    300 small faint ones piled on tile 0 (its list crosses the 256-record staging batch and no pixel stops before the
    second batch), 60 opaque ones piled on tile 1 (pixels reach the T_MIN stop), 240 scattered over and beyond the image,
    a few of them behind the camera."""
    from tests import scenes
    s = scenes.random_scene(N_REST, W, H, seed=seed + 1, sigma_px=2.5, spread=1.3, tilt=False, behind=0.05)
    g = torch.Generator().manual_seed(seed)
    f = float(s["intr"][0])

    def pile(n, cu, cv, spread, sigma, o_lo, o_hi):
        z = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
        u = cu + (torch.rand(n, generator=g, dtype=torch.float64) - 0.5) * spread
        v = cv + (torch.rand(n, generator=g, dtype=torch.float64) - 0.5) * spread
        xyz = torch.stack([(u - W / 2) / f * z, (v - H / 2) / f * z, z], dim=1)
        scale = (sigma / f * z).unsqueeze(1) * (0.8 + 0.4 * torch.rand(n, 3, generator=g, dtype=torch.float64))
        rot = torch.nn.functional.normalize(torch.randn(n, 4, generator=g, dtype=torch.float64), dim=1)
        op = o_lo + (o_hi - o_lo) * torch.rand(n, 1, generator=g, dtype=torch.float64)
        return xyz.float(), scale.float(), rot.float(), op.float(), torch.rand(n, 3, generator=g).float()

    parts = [pile(N_FAINT, 7.5, 7.5, 9.0, 1.2, 0.02, 0.08), pile(N_OPAQUE, 24.0, 8.0, 6.0, 2.5, 0.9, 0.999),
             (s["xyz"], s["scale"], s["rotate"], s["opacity"], s["rgb"])]
    cat = lambda i: torch.cat([p[i] for p in parts]).contiguous()
    return dict(xyz=cat(0), scale=cat(1), rotate=cat(2), opacity=cat(3), rgb=cat(4), intr=s["intr"], extr=s["extr"], W=W, H=H)


def scene_labels(n, K, seed=0):
    """(labels (n_labels,) uint8, n_labels): every class 0 .. K - 1 in use, a tenth of the rows 255, one row with the label
    K (>= K: unlabelled), one with 200, the last N_UNLISTED rows beyond n_labels"""
    rng = np.random.default_rng(seed + 11 * K)
    n_labels = n - N_UNLISTED
    lab = rng.integers(0, K, n_labels).astype(np.uint8)
    lab[rng.random(n_labels) < 0.1] = NONE
    lab[N_FAINT + N_OPAQUE + 3] = K
    lab[N_FAINT + N_OPAQUE + 4] = 200
    return lab, n_labels


def assign_case():
    """(rec (n, 12), map (H, W), labels (n,), W, H) of the edge rows of gfl_label_assign, W x H = 12 x 9"""
    w, h = 12, 9
    m = (np.arange(w * h).reshape(h, w) % 7).astype(np.uint8)
    m[4, 6] = NONE                                         # a map pixel that is not inherited
    nan = float("nan")
    rows = [  # u, v, depth, label before
        (0.0, 3.0, 1.0, NONE), (w - 1.0, 3.0, 1.0, NONE), (5.0, 0.0, 1.0, NONE), (5.0, h - 1.0, 1.0, NONE),   # on the border
        (-2.5, 3.0, 1.0, NONE), (4.0, -0.5, 1.0, NONE), (nan, 3.0, 1.0, NONE), (4.0, nan, 1.0, NONE),
        (4.0, 3.0, 0.0, NONE),                                                                             # depth 0
        (4.0, 3.0, 1.0, 3), (4.0, 3.0, 1.0, 0), (-3.0, 2.0, 0.0, 5),                                       # labelled already
        (6.2, 4.9, 1.0, NONE),                                                                             # the map says 255
        (3.6, 2.7, 1.0, NONE), (7.5, 5.5, 1.0, NONE), (10.99, 7.99, 1.0, NONE), (0.01, 0.01, 1.0, NONE),    # truncation
        (np.nextafter(f32(w - 1), f32(0)), np.nextafter(f32(h - 1), f32(0)), 2.0, NONE),
        (4.0, 3.0, -1.0, NONE),                                                                            # depth != 0
    ]
    rec = np.zeros((len(rows), REC), f32)
    rec[:, 0], rec[:, 1], rec[:, 9] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    return rec, m, np.array([r[3] for r in rows], np.uint8), w, h
