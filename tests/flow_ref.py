"""The flow score restated on the oracle (gfl_flow_pair, include/gflow_hip.h; gflow_amd/flow.py): the motion field is ONE
call of oracle.msplat_oracle.alpha_blending with the features [has dx, has dy, has] and a zero background -- that yields
num and den under the blend's own rule --, the masks and sums follow in numpy float64.  Also the inputs the host and GPU
tests share: the known-answer cases, and frame pairs made from tests/scenes.py."""
import numpy as np
import torch

from oracle import msplat_oracle as MO

REC = 12
BOUND = 1e-4                       # the project's parity figure: |F - F_ref| <= BOUND * max(1, max|d|) pixels per component
FRAGILE_DEN = 1e-4                 # |den_ref - min_weight| below this: validity hangs on the last bits of the sums
FRAGILE_SHARE = 0.01


def compact_lists(ids, tile_range):
    """The tile lists moved to the front of a new ids array, in tile order (the lists may lie anywhere in ``ids``, with
    anything between them, which the oracle's gather does not expect)."""
    ids, tr = np.asarray(ids).reshape(-1), np.asarray(tile_range).reshape(-1, 2).astype(np.int64)
    out, new = [], np.zeros_like(tr)
    pos = 0
    for t, (a, b) in enumerate(tr):
        if b > a:
            out.append(ids[a:b])
            new[t] = (pos, pos + (b - a))
            pos += b - a
    cat = np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)
    return cat, new.astype(np.int32)


def flow_pair(rec_a, ids, tile_range, uv_b, depth_b, gt_flow, move_mask, W, H, min_weight=0.5, dtype=torch.float64):
    """dict(num (2, H, W), den (H, W), flow (H, W, 2), valid (H, W) bool, sums (3, 6) float64, dmax) of one frame pair.
    ``rec_a`` (n_a, 12) float32 fit records, ``uv_b`` (n_b, 2) and ``depth_b`` (n_b,) float32: numpy arrays.  The blend
    runs in ``dtype`` on the float32 inputs; d = uv_b - uv_a is one float32 subtraction, as in the kernel."""
    rec_a = np.asarray(rec_a, np.float32).reshape(-1, REC)
    n_a = rec_a.shape[0]
    uv_b, depth_b = np.asarray(uv_b, np.float32).reshape(-1, 2), np.asarray(depth_b, np.float32).reshape(-1)
    n_b = uv_b.shape[0]
    gt = np.asarray(gt_flow, np.float32).reshape(H, W, 2)
    num, den = np.zeros((2, H, W)), np.zeros((H, W))
    dmax = 0.0
    if n_a > 0:
        m = min(n_a, n_b)
        has = np.zeros(n_a, bool)
        has[:m] = depth_b[:m] != 0
        d = np.zeros((n_a, 2), np.float32)
        d[:m] = uv_b[:m] - rec_a[:m, 0:2]
        d[~has] = 0
        dmax = float(np.abs(d).max()) if has.any() else 0.0
        feat = np.concatenate([d.astype(np.float64), has[:, None].astype(np.float64)], axis=1)
        cids, ctr = compact_lists(ids, tile_range)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        out = MO.alpha_blending(t(rec_a[:, 0:2]), t(rec_a[:, 2:5]), t(rec_a[:, 5:6]), t(feat), torch.from_numpy(cids),
                                torch.from_numpy(ctr), 0.0, W, H).double().numpy()
        num, den = out[0:2], out[2]
    valid = (den >= min_weight) & np.isfinite(gt).all(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        flow = np.where(valid[..., None], np.moveaxis(num, 0, -1) / den[..., None], 0.0)
    return dict(num=num, den=den, flow=flow, valid=valid, sums=sums_from_maps(flow, valid, gt, move_mask), dmax=dmax)


def sums_from_maps(flow, valid, gt_flow, move_mask):
    """The 18 numbers of gfl_flow_pair, float64, from a flow map, its valid mask, the given flow and the move mask (or
    None): per class (all, still, moving) {n_pixels, n_valid, epe_sum, n(epe < 1), n(epe < 3), n(epe < 5)}."""
    flow, gt = np.asarray(flow), np.asarray(gt_flow)
    valid = np.asarray(valid, bool)
    ex = flow[..., 0].astype(np.float64) - gt[..., 0].astype(np.float64)
    ey = flow[..., 1].astype(np.float64) - gt[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        epe = np.sqrt(ex * ex + ey * ey)
    out = np.zeros((3, 6))
    classes = [np.ones(valid.shape, bool)]
    if move_mask is not None:
        mm = np.asarray(move_mask) != 0
        classes += [~mm, mm]
    for c, sel in enumerate(classes):
        v = sel & valid
        e = epe[v]
        out[c] = [sel.sum(), v.sum(), e.sum(), (e < 1).sum(), (e < 3).sum(), (e < 5).sum()]
    return out


def fragile(ref64, ref32, min_weight=0.5):
    """(H, W) bool: pixels whose comparison says nothing about the kernel -- the reference's den within FRAGILE_DEN of the
    threshold, or the restatement in float32 and in float64 apart by more than the bound (validity included)."""
    bound = BOUND * max(1.0, ref64["dmax"])
    f = np.abs(ref64["den"] - min_weight) < FRAGILE_DEN
    f |= ref64["valid"] != ref32["valid"]
    f |= (np.abs(ref64["flow"] - ref32["flow"]) > bound).any(axis=-1)
    return f


def compare(flow, valid, ref64, ref32, min_weight=0.5, what=""):
    """The parity check: outside the fragile pixels (at most FRAGILE_SHARE of them) ``valid`` equals the reference's and
    every component of ``flow`` lies within BOUND * max(1, max|d|) of it.  Returns (worst error, fragile share)."""
    bound = BOUND * max(1.0, ref64["dmax"])
    fr = fragile(ref64, ref32, min_weight)
    share = float(fr.mean())
    ok = ~fr
    err = np.abs(np.asarray(flow, np.float64) - ref64["flow"])[ok]
    worst = float(err.max()) if err.size else 0.0
    print(f"flow parity {what}: worst |F - F_ref| {worst:.3g} px (bound {bound:.3g}), fragile {share:.4f}, "
          f"valid share {float(ref64['valid'].mean()):.3f}, max|d| {ref64['dmax']:.3g}")
    assert share <= FRAGILE_SHARE, (what, share)
    np.testing.assert_array_equal(np.asarray(valid, bool)[ok], ref64["valid"][ok], err_msg=what)
    assert worst <= bound, (what, worst, bound)
    return worst, share


# ------------------------------------------------------------------------------------------------------ known answers
def known_case(name):
    """Inputs of the 18 x 18 known-answer cases (2 x 2 tiles; every splat at integer pixel (8, 8), inside tile 0):
    dict(rec_a, ids, tile_range, uv_b, depth_b, W, H).  "one": conic [1, 0, 1], opacity 1, d = (2, -1).  "two": two
    splats, opacity 0.8, depths 1 and 2, d1 = (2, 0), d2 = (0, 4).  "two_culled": the far one has no future."""
    W = H = 18
    if name == "one":
        rows, d, depth_b = [(8.0, 8.0, 1.0)], [(2.0, -1.0)], [1.0]
    elif name in ("two", "two_culled"):
        rows, d = [(8.0, 8.0, 0.8), (8.0, 8.0, 0.8)], [(2.0, 0.0), (0.0, 4.0)]
        depth_b = [1.0, 2.0 if name == "two" else 0.0]
    else:
        raise ValueError(name)
    n = len(rows)
    rec = np.zeros((n, REC), np.float32)
    for j, (u, v, o) in enumerate(rows):
        rec[j, 0:6] = [u, v, 1.0, 0.0, 1.0, o]
        rec[j, 9] = 1.0 + j
    uv_b = rec[:, 0:2] + np.asarray(d, np.float32)
    depth_b = np.asarray(depth_b, np.float32)
    uv_b[depth_b == 0] = 0                              # (a culled row projects to (0, 0))
    tr = np.zeros((4, 2), np.int32)
    tr[0] = (0, n)
    return dict(rec_a=rec, ids=np.arange(n, dtype=np.int32), tile_range=tr, uv_b=uv_b, depth_b=depth_b, W=W, H=H,
                gt_flow=np.zeros((H, W, 2), np.float32), d=np.asarray(d, np.float64))


# ------------------------------------------------------------------------------------------------------ scene pairs
CAM_SHIFT = (0.04, -0.02, 0.03)
ROW_SHIFT = (0.03, 0.01, -0.02)


def front_end(xyz, scale, rotate, opacity, intr, extr, W, H):
    """Projection, EWA and the sorted lists of the oracle in float32: dict(uv, depth, conic, ids, tile_range, rec)."""
    f = lambda a: a.detach().float()
    xyz, scale, rotate, opacity, intr, extr = f(xyz), f(scale), f(rotate), f(opacity), f(intr), f(extr)
    uv, depth = MO.project_point(xyz, intr, extr, W, H)
    vis = depth != 0
    conic, radius, tiles = MO.ewa_project(xyz, MO.compute_cov3d(scale, rotate, vis), intr, extr, uv, W, H, vis)
    ids, tr = MO.sort_gaussian(uv, depth, W, H, radius, tiles)
    rec = np.zeros((xyz.shape[0], REC), np.float32)
    rec[:, 0:2], rec[:, 2:5] = uv.numpy(), conic.numpy()
    rec[:, 5], rec[:, 9] = opacity.reshape(-1).numpy(), depth.reshape(-1).numpy()
    return dict(uv=uv.numpy(), depth=depth.reshape(-1).numpy(), ids=ids.numpy().astype(np.int32),
                tile_range=tr.numpy().astype(np.int32), rec=rec)


def scene_pair(activated, intr, extr, W, H, seed=0, drop=True):
    """A frame pair from activated rows [xyz, scale, rotate, opacity, rgb]: frame B is the same rows under the camera
    translated by CAM_SHIFT with 30 % of the rows moved by ROW_SHIFT; with ``drop`` only the first N - N / 10 rows exist in
    B.  Returns dict(rec_a, ids, tile_range, uv_b, depth_b, W, H)."""
    xyz, scale, rotate, opacity = (a.detach().float() for a in activated[:4])
    N = xyz.shape[0]
    a = front_end(xyz, scale, rotate, opacity, intr, extr, W, H)
    rng = np.random.default_rng(seed + 77)
    moved = torch.from_numpy(rng.random(N) < 0.3)
    xyz_b = xyz + moved[:, None].float() * torch.tensor(ROW_SHIFT)
    extr_b = extr.detach().float().clone()
    extr_b[:, 3] += torch.tensor(CAM_SHIFT)
    uv_b, depth_b = MO.project_point(xyz_b, intr.detach().float(), extr_b, W, H)
    n_b = N - N // 10 if drop else N
    return dict(rec_a=a["rec"], ids=a["ids"], tile_range=a["tile_range"], uv_b=uv_b.numpy()[:n_b].copy(),
                depth_b=depth_b.reshape(-1).numpy()[:n_b].copy(), W=W, H=H)


def random_pair(N, W, H, seed, **kw):
    from tests import scenes
    s = scenes.random_scene(N, W, H, seed=seed, **kw)
    return scene_pair([s["xyz"], s["scale"], s["rotate"], s["opacity"], s["rgb"]], s["intr"], s["extr"], W, H, seed=seed)


def pile_pair():
    from oracle import fit_oracle as FO
    from tests import scenes
    s = scenes.capped_pile_scene()
    return scene_pair(FO.activate(s["raw"]), s["intr"], s["extr"], s["W"], s["H"], seed=5)


def shuffled_lists(ids, tile_range, seed=0, garbage=0x7fffffff):
    """The same lists at shuffled positions of a larger ids buffer with ``garbage`` between them (what reserved regions
    leave behind): (ids, tile_range)."""
    tr = np.asarray(tile_range).astype(np.int64)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(tr))
    total = int((tr[:, 1] - tr[:, 0]).sum())
    out = np.full(2 * total + 64 * len(tr) + 64, garbage, np.int32)
    new = np.zeros_like(tr)
    pos = 7
    for t in order:
        n = int(tr[t, 1] - tr[t, 0])
        pos += int(rng.integers(1, 40))
        new[t] = (pos, pos + n)                         # (an empty list keeps a position too: start == end)
        out[pos:pos + n] = np.asarray(ids)[tr[t, 0]:tr[t, 1]]
        pos += n
    return out, new.astype(np.int32)


def test_targets(ref_flow, W, H, seed=0):
    """(gt_flow, move_mask) of the sums test: gt = F_ref + (1.5 sin(x / 9), 4 cos(y / 7)) -- errors on both sides of all
    three thresholds --, a few NaN pixels, a disc mask."""
    y, x = np.mgrid[0:H, 0:W]
    gt = np.asarray(ref_flow, np.float64) + np.stack([1.5 * np.sin(x / 9.0), 4.0 * np.cos(y / 7.0)], axis=-1)
    gt = gt.astype(np.float32)
    rng = np.random.default_rng(seed)
    for _ in range(6):
        gt[rng.integers(0, H), rng.integers(0, W), rng.integers(0, 2)] = np.nan
    mask = ((x - 0.55 * W) ** 2 + (y - 0.45 * H) ** 2 <= (0.3 * min(W, H)) ** 2).astype(np.uint8)
    return gt, mask


test_targets.__test__ = False
