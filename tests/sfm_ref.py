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


def fit8(x1, y1, x2, y2, perturb=None):
    """the Hartley-normalised 8-point fit of the given correspondences (1-D arrays); ``perturb`` maps the normalised A^T A to
    the matrix whose null vector is taken (the sensitivity probe)"""
    def hartley(x, y):
        cx, cy = x.mean(), y.mean()
        s = np.sqrt(2.0) / np.sqrt((x - cx) ** 2 + (y - cy) ** 2).mean()
        return (x - cx) * s, (y - cy) * s, np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])
    u1, v1, T1 = hartley(x1, y1)
    u2, v2, T2 = hartley(x2, y2)
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=1)
    M = A.T @ A
    _, vecs = np.linalg.eigh(M if perturb is None else perturb(M))
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
def _margin(e, thr):
    """the smallest relative distance of a usable pixel's error e from the inlier threshold thr"""
    e = e[np.isfinite(e)]
    if e.size == 0 or not thr > 0:
        return float("inf")
    return float(np.abs(e - thr).min() / thr)


def refit(flow, F_init, exclude=None, rounds=2, e_floor=E_FLOOR, perturb=None):
    """dict(F (3, 3), counts (usable, inliers), median, inlier (H, W) uint8, err (H, W) with NaN where not usable, thr, margins
    [rounds + 1]: the threshold margin of every round's inlier decision, the final F's last)"""
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

    margins = []
    for _ in range(rounds):
        e, med, n, thr = evaluate(F)
        margins.append(_margin(e, thr))
        with np.errstate(invalid="ignore"):
            inl = e <= thr
        if inl.sum() >= 8:
            with np.errstate(all="ignore"):
                Fn = fit8(x1[inl], y1[inl], x2[inl], y2[inl], perturb)
            if np.isfinite(Fn).all():
                F = Fn
    e, med, n, thr = evaluate(F)
    margins.append(_margin(e, thr))
    with np.errstate(invalid="ignore"):
        inl = e <= thr
    return dict(F=F, counts=(n, int(inl.sum())), median=med, inlier=inl.astype(np.uint8), err=e, thr=thr, margins=margins)


def threshold_margin(res):
    """the smallest relative distance of a usable pixel's error from the inlier threshold, over every round of the refit: an
    inlier that flips in an intermediate round moves F at the 1e-4 level"""
    return min(res["margins"])


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


def two_view(flow, intr, F_init, exclude=None, rounds=2, e_floor=E_FLOOR, min_parallax=0.1, min_share=0.2, perturb=None):
    """stages a - c of one pair"""
    fit = refit(flow, F_init, exclude, rounds, e_floor, perturb)
    ps = pose(flow, fit["F"], fit["inlier"], fit["counts"], intr, min_parallax, min_share)
    rho, w = triangulate(flow, fit["inlier"], ps["R"], ps["t"], ps["degenerate"], intr)
    return dict(fit, **ps, rho=rho, weight=w)


def cheirality(flow, tv, intr):
    """what the exact comparison of a pair's votes and weights rests on -- dict(margin, sin2, sin2_any (H, W), NaN off the
    inliers).  margin: the smallest min(|z1|, |z2|) / max(|z1|, |z2|) over the inliers and the four candidates (R, t): no depth
    may sit on zero, where its sign is the rounding's.  sin2: sin^2 of the angle between the two bearings under the pair's R
    (the weight before the cheirality test); sin2_any: the smaller of the two candidate rotations'.  Both depths are quotients
    by it, so their relative error is 2^-52 / sin2: at the epipole itself sin2 is the rounding's, and so is the vote.  Depths
    that are not finite vote for nothing on either side and are left out of the margin."""
    x1, y1, x2, y2, _ = points(flow)
    inl = np.asarray(tv["inlier"]) != 0
    sin2, sin2_any = np.full(x1.shape, np.nan), np.full(x1.shape, np.nan)
    if not np.isfinite(tv["F"]).all() or not inl.any():
        return dict(margin=float("inf"), sin2=sin2, sin2_any=sin2_any)
    clean = lambda w: np.where(np.isfinite(w), w, 0.0)
    with np.errstate(all="ignore"):
        Ra, Rb, t0 = essential_candidates(tv["F"], intr)
        b1, b2 = bearings(x1[inl], y1[inl], intr), bearings(x2[inl], y2[inl], intr)
        margin, w = np.inf, np.full(b1.shape[0], np.inf)
        for Rc in (Ra, Rb):
            z1, z2, wc = depths(b1 @ Rc.T, b2, t0)                  # (-t0 gives the same depths with the other sign)
            w = np.fmin(w, clean(wc))
            z = np.stack([np.abs(z1), np.abs(z2)])
            ok = np.isfinite(z).all(0) & (z.max(0) > 0)
            if ok.any():
                margin = min(margin, float((z.min(0)[ok] / z.max(0)[ok]).min()))
        sin2[inl] = clean(depths(b1 @ np.asarray(tv["R"]).T, b2, t0)[2])
    sin2_any[inl] = w
    return dict(margin=margin, sin2=sin2, sin2_any=sin2_any)


def sensitivity(flow, intr, F_init, exclude=None, repeats=8, seed=0, **kw):
    """how far the restatement's own answer moves under another summation order and another eigen-solver: ``two_view`` again
    ``repeats`` times with every entry of the normalised A^T A (kept symmetric) multiplied by 1 + d, d uniform in +-2^-50.
    dict(F, R, t, parallax): the largest change of the normalised F, of R, of t and of the parallax.  It sets the float64
    bounds of the device comparison and never sees the device."""
    rng = np.random.default_rng(seed)

    def perturb(M):
        d = np.triu(rng.uniform(-2.0 ** -50, 2.0 ** -50, M.shape))
        return M * (1.0 + d + np.triu(d, 1).T)

    base = two_view(flow, intr, F_init, exclude, **kw)
    out = dict(F=0.0, R=0.0, t=0.0, parallax=0.0)
    for _ in range(repeats):
        tv = two_view(flow, intr, F_init, exclude, perturb=perturb, **kw)
        out["F"] = max(out["F"], float(np.abs(normalise_F(tv["F"]) - normalise_F(base["F"])).max()))
        out["R"] = max(out["R"], float(np.abs(tv["R"] - base["R"]).max()))
        out["t"] = max(out["t"], float(np.abs(tv["t"] - base["t"]).max()))
        out["parallax"] = max(out["parallax"], abs(tv["parallax"] - base["parallax"]))
    return out


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


def make_scene3(H=36, W=48, f=40.0, rvec=(0.01, -0.02, 0.005), tdir=(0.08, 0.02, 0.03), baselines=(0.08, 0.12), pp=None):
    """three views of one static surface (the middle view sees it as ``surface``): x_{i+1} = R x_i + baselines[i] tdir / |tdir|.
    dict(fwd [2], bwd [2] float32 flows, intr, extr (3, 3, 4) true world-to-camera with view 0 the world, R, tdir, baselines);
    ``pp``: the principal point (default: the rounded centre)"""
    cx, cy = (round(W / 2), round(H / 2)) if pp is None else pp
    intr = (float(f), float(f), float(cx), float(cy))
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


def flow64(depth, intr, R, t):
    """the float64 flow of a static scene of the given depth under x' = R x + t (no occlusion handling), and the depth in
    the second view"""
    H, W = depth.shape
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fx, fy, cx, cy = intr
    X = bearings(x, y, intr) * depth[..., None]
    X2 = X @ np.asarray(R).T + np.asarray(t)
    u, v = fx * X2[..., 0] / X2[..., 2] + cx, fy * X2[..., 1] / X2[..., 2] + cy
    return np.stack([u - x, v - y], axis=-1), X2[..., 2]


def exact_flow(depth, intr, R, t):
    """``flow64`` rounded to float32"""
    flow, z2 = flow64(depth, intr, R, t)
    return flow.astype(np.float32), z2


def make_scene_general(H, W, intr, rvec, t, noise=None):
    """the analytic static scene under any camera ``intr = (fx, fy, cx, cy)`` and motion: dict(flow, depth, intr, R, t).
    ``noise = (sigma, seed)``: seeded Gaussian noise of sigma px, added to the float64 flow before it is rounded to float32."""
    intr = tuple(float(v) for v in intr)
    depth = scene_depth(H, W)
    R = rodrigues(rvec)
    flow, _ = flow64(depth, intr, R, t)
    if noise is not None:
        sigma, seed = noise
        flow = flow + np.random.default_rng(seed).normal(scale=sigma, size=flow.shape)
    return dict(flow=flow.astype(np.float32), depth=depth, intr=intr, R=R, t=np.asarray(t, dtype=np.float64))


def make_scene(H=36, W=48, f=40.0, rvec=(0.01, -0.02, 0.005), t=(0.08, 0.02, 0.03)):
    """the analytic static scene of the tests: dict(flow, depth, intr, R, t)"""
    return make_scene_general(H, W, (f, f, round(W / 2), round(H / 2)), rvec, t)


# ---------------------------------------------------------------------------------------- motions, cameras, sizes: the cases
# what each motion reaches in gfl_sfm.hip (asserted on the restatement by tests/test_sfm_host.py and again, with the device's
# starting matrix, by tests/test_gpu_sfm.py): the winner of the cheirality vote, or the flag
ROT = (0.01, -0.02, 0.005)
MOTIONS = {                      # tag: (rvec, t, winner)
    "base": (ROT, (0.08, 0.02, 0.03), 0),
    "neg-x": (ROT, (-0.08, 0.02, 0.03), 1),
    "pos-y": (ROT, (0.02, 0.08, 0.03), 0),
    "neg-y": (ROT, (0.02, -0.08, 0.03), 1),
    "fwd": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.1), 0),                  # the epipole is the principal point
    "back": (ROT, (0.01, 0.0, -0.1), 1),                           # the epipole is inside the image as well
    "roll": ((0.0, 0.0, 3.0), (0.08, 0.02, 0.03), 2),              # 172 degrees about the axis: the true R has the smaller trace
    "roll-neg": ((0.0, 0.0, 3.0), (-0.08, 0.02, 0.03), 3),
    "small": (ROT, (0.004, 0.001, 0.0015), 0),                     # parallax under min_parallax: degenerate, R kept, t = 0
    "noisy": (ROT, (0.08, 0.02, 0.03), 0),                         # sigma = 0.3 px: thr = K2 median, above the floor
}
NOISE = (0.3, 7)
SIZES = ((8, 8), (33, 47), (64, 65), (91, 91))                    # 64 x 65: two workgroups of 4096 pixels, the second with 64;
PER_WORKGROUP = 4096                                              # 91 x 91: three
EPIPOLE_W = 1e-6                   # below this sin^2 the kernels' stated 1 / sin <= 1e3 fails: rho is not compared there
# Two rotations that differ by 1e-11 (the bound of the comparison) turn a = R x1 by as much, and a x b by a relative
# 1e-11 / sin: below sin^2 = 1e-14 by more than 1e-4.  There -- at the epipole's own pixel, where sin^2 is 1e-17 .. 1e-21, the
# square of R's distance from the truth -- the sign of a depth is the rounding's: the pixel's vote and weight are not pinned.
UNDECIDED_W = 1e-14
MIN_PARALLAX = 0.1


def camera(kind, H, W):
    """"centred": f = 40 max(H, W) / 48 and the rounded centre; "general": fx != fy and a principal point off the centre and off
    the pixel grid"""
    f = 40.0 * max(H, W) / 48.0
    if kind == "centred":
        return (f, f, float(round(W / 2)), float(round(H / 2)))
    return (1.3 * f, 0.9 * f, W / 2 - 3.25, H / 2 + 2.5)


CASES = [(m, H, W, cam) for (m, sizes, cam) in (
    ("base", SIZES, "centred"), ("base", SIZES[1:2], "general"), ("noisy", SIZES, "general"),
    ("roll", (SIZES[0], SIZES[3]), "centred"), ("roll", SIZES[2:3], "general"),
    ("roll-neg", SIZES[1:2], "general"), ("roll-neg", SIZES[2:3], "centred"),
    ("neg-x", SIZES[1:2], "centred"), ("neg-x", SIZES[2:3], "general"),
    ("pos-y", SIZES[0:1], "centred"), ("pos-y", SIZES[1:2], "general"),
    ("neg-y", SIZES[0:1], "centred"), ("neg-y", SIZES[2:3], "general"),
    ("back", SIZES[1:2], "centred"), ("back", SIZES[2:3], "general"),
    ("small", SIZES[1:2], "centred"), ("small", SIZES[2:3], "general"),
    ("fwd", SIZES, "centred"), ("fwd", (SIZES[1], SIZES[3]), "general")) for (H, W) in sizes]


def case_id(case):
    return "{}-{}x{}-{}".format(*case)


def case_scene(case):
    """the scene of (motion, H, W, camera kind)"""
    motion, H, W, cam = case
    rvec, t, _ = MOTIONS[motion]
    return make_scene_general(H, W, camera(cam, H, W), rvec, t, NOISE if motion == "noisy" else None)


def case_kw(case):
    """the keywords of ``two_view`` for the case: ``small`` moves the image by 0.074 px at 33 x 47, under the default
    min_parallax of 0.1 px, and by 0.10 - 0.13 px at 64 x 65 with its longer focal lengths, where the threshold is 0.2 px"""
    motion, H, W, _ = case
    return dict(min_parallax=0.2) if motion == "small" and (H, W) == (64, 65) else {}


def epipole_cap(H, W):
    """how many inliers may lie so near the epipole that sin^2 < EPIPOLE_W"""
    return max(1, int(0.005 * H * W))


def check_case(case, flow, intr, ref):
    """asserts on the restatement's result ``ref`` that the case reaches what it is there for; returns dict(left_out (H, W)
    bool: the inliers with sin^2 < EPIPOLE_W, undecided (H, W) bool: those with sin^2 < UNDECIDED_W)"""
    motion, H, W, cam = case
    tag = case_id(case)
    n = H * W
    assert flow.shape == (H, W, 2) and (n + PER_WORKGROUP - 1) // PER_WORKGROUP == {64: 1, 1551: 1, 4160: 2, 8281: 3}[n], tag
    assert (intr[0] != intr[1] and intr[2] != round(W / 2) and intr[3] != round(H / 2)) == (cam == "general"), tag
    assert threshold_margin(ref) > 1e-9, (tag, ref["margins"])
    ch = cheirality(flow, ref, intr)
    assert ch["margin"] > 1e-9, (tag, ch["margin"])
    assert np.isfinite(ref["F"]).all() and ref["counts"][0] == n, tag
    winner = MOTIONS[motion][2]
    votes = ref["votes"]
    if motion == "noisy":
        assert ref["thr"] > E_FLOOR and ref["thr"] == K2 * ref["median"], (tag, ref["thr"])
        if n > 64:
            assert 8 <= n - ref["counts"][1] <= n // 20, (tag, ref["counts"])       # a scattered subset is left out
    else:
        assert ref["thr"] == E_FLOOR and ref["counts"][1] == n, (tag, ref["thr"], ref["counts"])
    min_parallax = case_kw(case).get("min_parallax", MIN_PARALLAX)
    assert abs(ref["parallax"] / min_parallax - 1.0) > 0.01, (tag, ref["parallax"])      # the flag does not hang on a rounding
    if motion == "small":                                          # degenerate by parallax alone: a finite F, every pixel kept
        assert ref["degenerate"] and 0.05 < ref["parallax"] < min_parallax and not ref["t"].any(), (tag, ref["parallax"])
        assert np.isfinite(ref["R"]).all() and not ref["weight"].any(), tag
    else:
        assert not ref["degenerate"], (tag, ref["parallax"])
    if not (motion == "noisy" and n == 64):                        # (8 x 8 under 0.3 px of noise: the votes may split)
        assert int(np.argmax(votes)) == winner and votes[winner] > 2 * np.delete(votes, winner).max(), (tag, votes)
    with np.errstate(invalid="ignore"):
        left_out, undecided = ch["sin2"] < EPIPOLE_W, ch["sin2_any"] < UNDECIDED_W
    if motion in ("fwd", "back"):
        assert left_out.sum() <= epipole_cap(H, W), (tag, left_out.sum())
        assert undecided.sum() <= 1 and not (undecided & ~left_out).any(), (tag, undecided.sum())
    elif motion == "small":                                        # (no parallax: sin^2 is small everywhere, and nothing has weight)
        assert not undecided.any(), tag
    else:
        assert not left_out.any() and not undecided.any(), (tag, left_out.sum())
    return dict(left_out=left_out, undecided=undecided)


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
