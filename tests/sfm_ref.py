"""Float64 numpy restatement of gflow_amd.sfm / csrc/gfl_sfm.hip (include/gflow_hip.h, "depth and camera from the flows"):
the refit of the fundamental matrix, the relative pose, the triangulation, the baseline ratios, fusion, pull-push fill, the
Jacobi sweeps and the pose chain -- plain and slow, with LAPACK where the device runs cyclic Jacobi.  Also the analytic scenes
the tests share."""
import numpy as np

from tests.epipolar_ref import canonical as normalise_F, sampson  # noqa: F401  (the tests call R.normalise_F)
from tests import epipolar_ref as E

K2 = (2.5 * 2.5) * (1.4826 * 1.4826)
E_FLOOR = 0.25 ** 2


# ------------------------------------------------------------------------------------------------------------- helpers
def lower_median(v):
    """the exact lower median (rank (n - 1) // 2) of the finite values, NaN for none; also their number"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    return (E.lower_median(v) if v.size else float("nan")), int(v.size)


def points(flow):
    """x1, y1, x2, y2 (H, W) float64 and the known pixels: centres at integer coordinates, x2 = x + flow"""
    flow = np.asarray(flow, dtype=np.float32)
    H, W = flow.shape[:2]
    y1, x1 = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    known = np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1])
    f = np.where(known[..., None], flow, 0).astype(np.float64)
    return x1, y1, x1 + f[..., 0], y1 + f[..., 1], known


def fit8(x1, y1, x2, y2):
    """the Hartley-normalised 8-point fit of the given correspondences (1-D arrays)"""
    def hartley(x, y):
        cx, cy = x.mean(), y.mean()
        s = np.sqrt(2.0) / np.sqrt((x - cx) ** 2 + (y - cy) ** 2).mean()
        return (x - cx) * s, (y - cy) * s, np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])
    u1, v1, T1 = hartley(x1, y1)
    u2, v2, T2 = hartley(x2, y2)
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=1)
    _, vecs = np.linalg.eigh(A.T @ A)
    f = vecs[:, 0].reshape(3, 3)
    U, S, Vt = np.linalg.svd(f)
    f = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    return normalise_F(T2.T @ f @ T1)


def initial_F(flow, exclude=None, hypotheses=64, seed=0):
    """a small least-median-of-squares start for the CPU tests (the device starts from gfl_epi_fundamental)"""
    x1, y1, x2, y2, known = points(flow)
    use = known if exclude is None else known & (np.asarray(exclude) == 0)
    idx = np.flatnonzero(use.reshape(-1))
    if idx.size < 8:
        return np.zeros((3, 3))
    X = [a.reshape(-1) for a in (x1, y1, x2, y2)]
    rng = np.random.default_rng(seed)
    best, best_med = np.zeros((3, 3)), np.inf
    for _ in range(hypotheses):
        s = rng.choice(idx, 8, replace=False)
        with np.errstate(all="ignore"):
            F = fit8(*(a[s] for a in X))
        if not np.isfinite(F).all():
            continue
        med = lower_median(sampson(F, *(a[idx] for a in X)))[0]
        if med < best_med:
            best, best_med = F, med
    return best


# ------------------------------------------------------------------------------------------------------- a. the refit
def refit(flow, F_init, exclude=None, rounds=2, e_floor=E_FLOOR):
    """dict(F (3, 3), counts (usable, inliers), median, inlier (H, W) uint8, err (H, W) with NaN where not usable, thr)"""
    x1, y1, x2, y2, known = points(flow)
    use = known if exclude is None else known & (np.asarray(exclude) == 0)
    F = np.asarray(F_init, dtype=np.float64).reshape(3, 3).copy()

    def evaluate(F):
        if not np.isfinite(F).all():
            return np.full(x1.shape, np.nan), float("nan"), 0, -1.0
        e = sampson(F, x1, y1, x2, y2)
        e = np.where(use & np.isfinite(e), e, np.nan)
        med, n = lower_median(e)
        return e, med, n, (max(K2 * med, e_floor) if n else -1.0)

    for _ in range(rounds):
        e, med, n, thr = evaluate(F)
        with np.errstate(invalid="ignore"):
            inl = e <= thr
        if inl.sum() >= 8:
            with np.errstate(all="ignore"):
                Fn = fit8(x1[inl], y1[inl], x2[inl], y2[inl])
            if np.isfinite(Fn).all():
                F = Fn
    e, med, n, thr = evaluate(F)
    with np.errstate(invalid="ignore"):
        inl = e <= thr
    return dict(F=F, counts=(n, int(inl.sum())), median=med, inlier=inl.astype(np.uint8), err=e, thr=thr)


def threshold_margin(res):
    """the smallest relative distance of a usable pixel's error from the inlier threshold"""
    e = res["err"][np.isfinite(res["err"])]
    if e.size == 0 or not res["thr"] > 0:
        return float("inf")
    return float(np.abs(e - res["thr"]).min() / res["thr"])


# --------------------------------------------------------------------------------------------------------- b. the pose
def bearings(x, y, intr):
    fx, fy, cx, cy = intr
    return np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], axis=-1)


def depths(a, b, t):
    """z1 a + t = z2 b by least squares, and sin^2 of the angle between a and b"""
    c = np.cross(a, b)
    cc = (c * c).sum(-1)
    tt = np.broadcast_to(np.asarray(t, dtype=np.float64), a.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        z1 = (c * np.cross(b, tt)).sum(-1) / cc
        z2 = (c * np.cross(a, tt)).sum(-1) / cc
        w = cc / ((a * a).sum(-1) * (b * b).sum(-1))
    return z1, z2, w


def essential_candidates(F, intr):
    """(Ra, Rb, t0): numpy.linalg.svd of E = K^T F K, singular values (1, 1, 0); the rotation with the larger trace first, t0
    with its entry of largest magnitude positive"""
    fx, fy, cx, cy = intr
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    E = K.T @ np.asarray(F, dtype=np.float64).reshape(3, 3) @ K
    U, _, Vt = np.linalg.svd(E)
    u1, u2, v1, v2 = U[:, 0], U[:, 1], Vt[0], Vt[1]
    u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
    s = np.outer(u2, v1) - np.outer(u1, v2)
    z = np.outer(u3, v3)
    Ra, Rb = s + z, z - s
    if np.trace(Rb) > np.trace(Ra):
        Ra, Rb = Rb, Ra
    big = u3[np.argmax(np.abs(u3))]
    return Ra, Rb, u3 * (-1.0 if big < 0 else 1.0)


def pose(flow, F, inlier, counts, intr, min_parallax=0.1, min_share=0.2):
    """dict(R, t, votes (4,), parallax, degenerate)"""
    x1, y1, x2, y2, _ = points(flow)
    inl = np.asarray(inlier) != 0
    R, t, votes, par = np.eye(3), np.zeros(3), np.zeros(4, dtype=np.int64), 0.0
    ok = bool(np.isfinite(np.asarray(F)).all())
    if ok:
        with np.errstate(all="ignore"):
            Ra, Rb, t0 = essential_candidates(F, intr)
        b1, b2 = bearings(x1[inl], y1[inl], intr), bearings(x2[inl], y2[inl], intr)
        for c in range(4):
            Rc, tc = (Ra, Rb)[c // 2], (t0 if c % 2 == 0 else -t0)
            with np.errstate(all="ignore"):
                z1, z2, _ = depths(b1 @ Rc.T, b2, tc)
                votes[c] = int(((z1 > 0) & (z2 > 0)).sum())
        best = int(np.argmax(votes))                               # (the first of equal counts)
        R, t = (Ra, Rb)[best // 2], (t0 if best % 2 == 0 else -t0)
        with np.errstate(all="ignore"):
            a = b1 @ R.T
            fx, fy, cx, cy = intr
            d = np.sqrt((fx * (a[:, 0] / a[:, 2]) + cx - x2[inl]) ** 2 + (fy * (a[:, 1] / a[:, 2]) + cy - y2[inl]) ** 2)
        par = lower_median(d)[0]
        if not np.isfinite(par):
            par = 0.0
    usable, n_inl = counts
    r_ok = bool(np.isfinite(R).all())
    bad = (not ok) or usable < 8 or n_inl < min_share * usable or not par >= min_parallax or not r_ok or not np.isfinite(t).all()
    if bad:
        t = np.zeros(3)
        if not r_ok:
            R = np.eye(3)
    return dict(R=R, t=t, votes=votes, parallax=par, degenerate=bool(bad))


# ------------------------------------------------------------------------------------------------ c. the triangulation
def triangulate(flow, inlier, R, t, degenerate, intr):
    """(rho, weight) (H, W) float64"""
    x1, y1, x2, y2, known = points(flow)
    rho, w = np.zeros(x1.shape), np.zeros(x1.shape)
    if degenerate:
        return rho, w
    a, b = bearings(x1, y1, intr) @ np.asarray(R).T, bearings(x2, y2, intr)
    z1, z2, ww = depths(a, b, t)
    with np.errstate(all="ignore"):
        r = 1.0 / z1
        good = known & (np.asarray(inlier) != 0) & (z1 > 0) & (z2 > 0) & np.isfinite(r) & np.isfinite(ww)
    rho[good], w[good] = r[good], ww[good]
    return rho, w


def two_view(flow, intr, F_init, exclude=None, rounds=2, e_floor=E_FLOOR, min_parallax=0.1, min_share=0.2):
    """stages a - c of one pair"""
    fit = refit(flow, F_init, exclude, rounds, e_floor)
    ps = pose(flow, fit["F"], fit["inlier"], fit["counts"], intr, min_parallax, min_share)
    rho, w = triangulate(flow, fit["inlier"], ps["R"], ps["t"], ps["degenerate"], intr)
    return dict(fit, **ps, rho=rho, weight=w)


# ------------------------------------------------------------------------------------------------------ d. the ratios
def median_quotient(a, b=None, wa=None, wb=None, w_min=0.0):
    """(median, count) of a / b over the pixels whose weights exceed w_min"""
    a = np.asarray(a, dtype=np.float64)
    ok = np.ones(a.shape, dtype=bool)
    for w in (wa, wb):
        if w is not None:
            ok &= np.asarray(w) > w_min
    with np.errstate(all="ignore"):
        q = a if b is None else a / np.asarray(b, dtype=np.float64)
    return lower_median(np.where(ok & np.isfinite(q), q, np.nan))


# --------------------------------------------------------------------------------------------------- e. fusion and fill
def fuse(rf, wf, rb, wb, sf, sb):
    w = wf + wb
    num = wf * (rf * sf) + wb * (rb * sb)
    with np.errstate(all="ignore"):
        return np.where(w > 0, num / np.where(w > 0, w, 1.0), 0.0), w


def pull_push(v, w):
    """the fill: pixels without weight take the bilinear sample of the filled coarser level"""
    vs, ws = [np.asarray(v, dtype=np.float64)], [np.asarray(w, dtype=np.float64)]
    while vs[-1].shape != (1, 1):
        pv, pw = vs[-1], ws[-1]
        H, W = pv.shape
        ys, xs = np.arange((H + 1) // 2), np.arange((W + 1) // 2)
        y0, y1, x0, x1 = 2 * ys, np.minimum(2 * ys + 1, H - 1), 2 * xs, np.minimum(2 * xs + 1, W - 1)
        g = lambda a, yy, xx: a[yy[:, None], xx[None, :]]
        sw = ((g(pw, y0, x0) + g(pw, y0, x1)) + g(pw, y1, x0)) + g(pw, y1, x1)
        num = ((g(pw, y0, x0) * g(pv, y0, x0) + g(pw, y0, x1) * g(pv, y0, x1)) + g(pw, y1, x0) * g(pv, y1, x0)) \
            + g(pw, y1, x1) * g(pv, y1, x1)
        vs.append(np.where(sw > 0, num / np.where(sw > 0, sw, 1.0), 0.0))
        ws.append(0.25 * sw)
    filled = vs[-1]
    for l in range(len(vs) - 2, -1, -1):
        H, W = vs[l].shape
        Hc, Wc = filled.shape
        cy = np.clip(0.5 * np.arange(H) - 0.25, 0, Hc - 1)
        cx = np.clip(0.5 * np.arange(W) - 0.25, 0, Wc - 1)
        y0, x0 = cy.astype(np.int64), cx.astype(np.int64)
        y1, x1 = np.minimum(y0 + 1, Hc - 1), np.minimum(x0 + 1, Wc - 1)
        ty, tx = (cy - y0)[:, None], (cx - x0)[None, :]
        g = lambda yy, xx: filled[yy[:, None], xx[None, :]]
        top = (1 - tx) * g(y0, x0) + tx * g(y0, x1)
        bot = (1 - tx) * g(y1, x0) + tx * g(y1, x1)
        filled = np.where(ws[l] > 0, vs[l], (1 - ty) * top + ty * bot)
    return filled


def jacobi(rho0, w, lam, x, sweeps):
    """weighted Jacobi sweeps of min sum w (rho - rho0)^2 + lam sum_pq (rho_p - rho_q)^2 from x"""
    x = np.asarray(x, dtype=np.float64).copy()
    H, W = x.shape
    cnt = np.zeros((H, W))
    cnt[:, 1:] += 1; cnt[:, :-1] += 1; cnt[1:, :] += 1; cnt[:-1, :] += 1
    for _ in range(sweeps):
        S = np.zeros((H, W))
        S[:, 1:] += x[:, :-1]
        S[:, :-1] += x[:, 1:]
        S[1:, :] += x[:-1, :]
        S[:-1, :] += x[1:, :]
        with np.errstate(all="ignore"):
            data = rho0 + (lam * (S - cnt * rho0)) / (w + lam * cnt)
            x = np.where(w > 0, data, (S / cnt) if lam > 0 else x)
    return x


def fill(rho0, w, lam, sweeps=20, rho_min=1e-6):
    """(depth, rho) of one frame"""
    x = jacobi(rho0, w, lam, pull_push(rho0, w), sweeps)
    return 1.0 / np.maximum(x, rho_min), x


# ------------------------------------------------------------------------------------------------------------ the chain
def clip_depth_camera(fwd, bwd, intr, F_fwd=None, F_bwd=None, exclude_fwd=None, exclude_bwd=None, median_depth=1.0, w_min=1e-7,
                      sweeps=20, lam=0.05, rho_min=1e-6, **kw):
    """the clip: depth (T, H, W), extr (T, 3, 4), baseline (T - 1), ratio, count (T), degenerate (T - 1), unreliable (T) and
    the per-pair results.  F_fwd / F_bwd: the starting matrices per pair (default: initial_F)."""
    n = len(fwd)
    T = n + 1
    H, W = np.asarray(fwd[0]).shape[:2]
    pick = lambda lst, i: None if lst is None else lst[i]
    start = lambda Fs, flow, ex, i: initial_F(flow, ex) if Fs is None else Fs[i]
    pf = [two_view(fwd[i], intr, start(F_fwd, fwd[i], pick(exclude_fwd, i), i), pick(exclude_fwd, i), **kw) for i in range(n)]
    pb = [] if bwd is None else \
        [two_view(bwd[i], intr, start(F_bwd, bwd[i], pick(exclude_bwd, i), i), pick(exclude_bwd, i), **kw) for i in range(n)]
    zero = np.zeros((H, W))
    rf = [pf[i]["rho"] if i < n else zero for i in range(T)]
    wf = [pf[i]["weight"] if i < n else zero for i in range(T)]
    rb = [pb[i - 1]["rho"] if i >= 1 and pb else zero for i in range(T)]
    wb = [pb[i - 1]["weight"] if i >= 1 and pb else zero for i in range(T)]
    ratio, count = zip(*[median_quotient(rf[i], rb[i], wf[i], wb[i], w_min) for i in range(T)])
    has = [bool((wf[i] + wb[i] > 0).any()) for i in range(T)]

    def frame(i, b):
        r0, w = fuse(rf[i], wf[i], rb[i], wb[i], 1.0 / b[i] if i < n else 1.0, 1.0 / b[i - 1] if i >= 1 else 1.0)
        med_w = lower_median(np.where(w > 0, w, np.nan))[0]
        return fill(r0, w, lam * med_w if np.isfinite(med_w) else 0.0, sweeps, rho_min)[0]

    b = np.ones(max(n, 1))
    carry = 1.0                                                    # the median filled depth of the last frame with weight
    depth = [None] * T
    for i in range(T):
        if 1 <= i < n:
            if count[i] > 0 and np.isfinite(ratio[i]) and ratio[i] > 0:
                b[i] = b[i - 1] * ratio[i]
            else:
                with np.errstate(all="ignore"):
                    med_inv = median_quotient(np.ones((H, W)), rf[i], wf[i], None, w_min)[0]
                b[i] = carry / med_inv if np.isfinite(med_inv) and med_inv > 0 else b[i - 1]
        depth[i] = frame(i, b)
        if has[i]:
            carry = lower_median(depth[i])[0]
    first = next((i for i in range(T) if has[i]), None)
    s = median_depth / lower_median(depth[first])[0] if first is not None else 1.0
    depth = np.stack([depth[i] * s if has[i] else np.full((H, W), float(median_depth)) for i in range(T)])
    b = b[:n] * s
    extr = [np.eye(4)]
    for i in range(n):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = pf[i]["R"], b[i] * pf[i]["t"]
        extr.append(M @ extr[-1])
    return dict(depth=depth, extr=np.stack(extr)[:, :3], baseline=b, ratio=np.array(ratio), count=np.array(count),
                degenerate=np.array([p["degenerate"] for p in pf]), unreliable=~np.array(has), pairs_fwd=pf, pairs_bwd=pb)


# ----------------------------------------------------------------------------------------------------------- the scenes
def rodrigues(r):
    r = np.asarray(r, dtype=np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def surface(x, y, W):
    """the scenes' depth at the (continuous) pixel (x, y)"""
    return 2.0 + 0.5 * np.sin(0.2 * x) * np.cos(0.15 * y) + 0.4 * x / W


def scene_depth(H, W):
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return surface(x, y, W)


def depth_seen_from(H, W, intr, R, t, iterations=60):
    """the depth map of the view x' = R x + t of the surface that the first view sees as ``surface``: for every pixel p of the
    new view the surface point that projects to it, by the fixed-point iteration u <- u - (project(u) - p) (the views are
    close: the map's Jacobian is near the identity)"""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fx, fy, cx, cy = intr
    ux, uy = x.copy(), y.copy()
    for _ in range(iterations):
        X2 = (bearings(ux, uy, intr) * surface(ux, uy, W)[..., None]) @ np.asarray(R).T + np.asarray(t)
        ux -= fx * X2[..., 0] / X2[..., 2] + cx - x
        uy -= fy * X2[..., 1] / X2[..., 2] + cy - y
    return ((bearings(ux, uy, intr) * surface(ux, uy, W)[..., None]) @ np.asarray(R).T + np.asarray(t))[..., 2]


def make_scene3(H=36, W=48, f=40.0, rvec=(0.01, -0.02, 0.005), tdir=(0.08, 0.02, 0.03), baselines=(0.08, 0.12)):
    """three views of one static surface (the middle view sees it as ``surface``): x_{i+1} = R x_i + baselines[i] tdir / |tdir|.
    dict(fwd [2], bwd [2] float32 flows, intr, extr (3, 3, 4) true world-to-camera with view 0 the world, R, tdir, baselines)"""
    intr = (float(f), float(f), float(round(W / 2)), float(round(H / 2)))
    R = rodrigues(rvec)
    tdir = np.asarray(tdir, dtype=np.float64) / np.linalg.norm(tdir)
    t01, t12 = baselines[0] * tdir, baselines[1] * tdir
    d1 = scene_depth(H, W)
    d0 = depth_seen_from(H, W, intr, R.T, -R.T @ t01)               # view 0 from view 1: x0 = R^T (x1 - t01)
    d2 = depth_seen_from(H, W, intr, R, t12)
    fwd = [exact_flow(d0, intr, R, t01)[0], exact_flow(d1, intr, R, t12)[0]]
    bwd = [exact_flow(d1, intr, R.T, -R.T @ t01)[0], exact_flow(d2, intr, R.T, -R.T @ t12)[0]]
    extr = [np.eye(4)]
    for t in (t01, t12):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, t
        extr.append(M @ extr[-1])
    return dict(fwd=fwd, bwd=bwd, intr=intr, extr=np.stack(extr)[:, :3], R=R, tdir=tdir, baselines=np.asarray(baselines),
                depth=[d0, d1, d2])


def exact_flow(depth, intr, R, t):
    """the float32 flow of a static scene of the given depth under x' = R x + t (no occlusion handling), and the depth in
    the second view"""
    H, W = depth.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fx, fy, cx, cy = intr
    X = bearings(x, y, intr) * depth[..., None]
    X2 = X @ np.asarray(R).T + np.asarray(t)
    u, v = fx * X2[..., 0] / X2[..., 2] + cx, fy * X2[..., 1] / X2[..., 2] + cy
    return np.stack([u - x, v - y], axis=-1).astype(np.float32), X2[..., 2]


def make_scene(H=36, W=48, f=40.0, rvec=(0.01, -0.02, 0.005), t=(0.08, 0.02, 0.03)):
    """the analytic static scene of the tests: dict(flow, depth, intr, R, t)"""
    intr = (float(f), float(f), float(round(W / 2)), float(round(H / 2)))
    depth = scene_depth(H, W)
    R = rodrigues(rvec)
    flow, _ = exact_flow(depth, intr, R, t)
    return dict(flow=flow, depth=depth, intr=intr, R=R, t=np.asarray(t, dtype=np.float64))


def add_block(flow, y0=10, x0=14, size=12, offset=(3.0, -2.0)):
    """the scene's flow with a size x size block moved by `offset` pixels; also the block's mask"""
    flow = flow.copy()
    flow[y0:y0 + size, x0:x0 + size] += np.asarray(offset, dtype=np.float32)
    mask = np.zeros(flow.shape[:2], dtype=bool)
    mask[y0:y0 + size, x0:x0 + size] = True
    return flow, mask


def angle_deg(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


def rotation_angle_deg(Ra, Rb):
    D = np.asarray(Ra, dtype=np.float64).T @ np.asarray(Rb, dtype=np.float64)
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(s, (np.trace(D) - 1.0) / 2.0)))   # (arccos alone loses small angles)
