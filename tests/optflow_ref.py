"""The optical-flow estimator of gflow_amd.optflow restated with torch on the CPU ("Flows from the images"):
a coarse-to-fine variational estimate -- grey, a 5-tap binomial pyramid, per level `warps` linearisations, per linearisation
`outer` re-weightings of a robust data and a robust smoothness term, per re-weighting `sweeps` Jacobi sweeps of the 2 x 2
per-pixel systems.  Written from the definition, not from the kernels; every step is batched over the leading axis P.
``dtype``: torch.float64 is the reference, torch.float32 the same arithmetic in the kernels' precision and order.
"""
import torch

EPS2 = 1e-6                        # epsilon^2, epsilon = 1e-3


def _sqrt(x):
    """the correctly rounded square root in x's precision.  torch.sqrt of a float32 tensor is not that on every CPU (measured:
    one in five roots an ulp off on one machine, none on another); the float64 root rounded to float32 is, everywhere."""
    return torch.sqrt(x.double()).to(x.dtype)


def grey(img, dtype=torch.float64):
    """(..., H, W, 3) uint8 (divided by 255) or float in [0, 1] -> (..., H, W) in [0, 255]"""
    img = torch.as_tensor(img)
    x = img.to(dtype) / 255 if img.dtype == torch.uint8 else img.to(dtype)
    return 255 * ((0.299 * x[..., 0] + 0.587 * x[..., 1]) + 0.114 * x[..., 2])


def _take(f, idx, axis):
    return f.index_select(axis, idx)


def _nb(f, d, axis):
    """f at index + d along ``axis`` (-1: x, -2: y), border replicated"""
    n = f.shape[axis]
    return _take(f, (torch.arange(n) + d).clamp(0, n - 1), axis)


def _cd(f, axis):
    """central difference 1/2 (f(+1) - f(-1)), border replicated"""
    return 0.5 * (_nb(f, 1, axis) - _nb(f, -1, axis))


def level_sizes(H, W, min_side=16):
    sizes = [(H, W)]
    while min(sizes[-1]) // 2 >= min_side:
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def _binomial_down(f, axis):
    n = f.shape[axis]
    c = torch.arange(0, n, 2)
    t = lambda d: _take(f, (c + d).clamp(0, n - 1), axis)
    return ((((t(-2) + 4 * t(-1)) + 6 * t(0)) + 4 * t(1)) + t(2)) * 0.0625


def pyr_down(I):
    """(..., H, W) -> (..., ceil(H / 2), ceil(W / 2)): [1 4 6 4 1] / 16 along the rows, then along the columns, at (2x, 2y)"""
    return _binomial_down(_binomial_down(I, -1), -2)


def bilinear(img, xc, yc):
    """img (P, H, W) at the (already clamped) coordinates xc, yc (P, h, w)"""
    P, H, W = img.shape
    x0, y0 = xc.floor(), yc.floor()
    tx, ty = xc - x0, yc - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    flat = img.reshape(P, H * W)
    g = lambda yy, xx: flat.gather(1, (yy * W + xx).reshape(P, -1)).reshape(xc.shape)
    top = (1 - tx) * g(y0, x0) + tx * g(y0, x1)
    bot = (1 - tx) * g(y1, x0) + tx * g(y1, x1)
    return (1 - ty) * top + ty * bot


def upsample_flow(flow, H, W):
    """(P, h, w, 2) -> (P, H, W, 2): 2 bilinear(flow, x / 2, y / 2), coordinates clamped to the coarse grid"""
    P, h, w, _ = flow.shape
    dt = flow.dtype
    ys, xs = torch.meshgrid((torch.arange(H, dtype=dt) / 2).clamp(0, h - 1), (torch.arange(W, dtype=dt) / 2).clamp(0, w - 1),
                            indexing="ij")
    xs, ys = xs.expand(P, H, W), ys.expand(P, H, W)
    return torch.stack([2 * bilinear(flow[..., c], xs, ys) for c in range(2)], -1)


def warp_terms(Ia, Ib, u, v):
    """dict(Ix, Iy, It, inside) of one linearisation"""
    P, H, W = Ia.shape
    dt = Ia.dtype
    Y, X = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    xs, ys = X + u, Y + v
    inside = ((xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)).to(dt)
    Iw = bilinear(Ib, xs.clamp(0, W - 1), ys.clamp(0, H - 1))
    return dict(Ix=0.5 * (_cd(Iw, -1) + _cd(Ia, -1)), Iy=0.5 * (_cd(Iw, -2) + _cd(Ia, -2)), It=Iw - Ia, inside=inside)


def coefficients(t, u, v, du, dv, alpha):
    """The nine planes the sweeps read: wl, wr, wt, wb, a11, a22, a12, c1 = pd Ix It, c2 = pd Iy It"""
    Ix, Iy, It = t["Ix"], t["Iy"], t["It"]
    H, W = Ix.shape[-2:]
    dt = Ix.dtype
    r = (It + Ix * du) + Iy * dv
    pd = t["inside"] / _sqrt(r * r + EPS2)
    U, V = u + du, v + dv
    ux, uy, vx, vy = _cd(U, -1), _cd(U, -2), _cd(V, -1), _cd(V, -2)
    root = _sqrt(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + EPS2)
    ps = torch.full_like(root, alpha) / root       # (a true division: torch forms `scalar / tensor` as scalar * (1 / tensor))
    x, y = torch.arange(W), torch.arange(H)[:, None]
    wl = 0.5 * (ps + _nb(ps, -1, -1)) * (x > 0).to(dt)
    wr = 0.5 * (ps + _nb(ps, 1, -1)) * (x < W - 1).to(dt)
    wt = 0.5 * (ps + _nb(ps, -1, -2)) * (y > 0).to(dt)
    wb = 0.5 * (ps + _nb(ps, 1, -2)) * (y < H - 1).to(dt)
    ws = ((wl + wr) + wt) + wb
    pix, piy = pd * Ix, pd * Iy
    return dict(wl=wl, wr=wr, wt=wt, wb=wb, a11=pix * Ix + ws, a22=piy * Iy + ws, a12=pix * Iy, c1=pix * It, c2=piy * It)


def jacobi_sweep(c, u, v, du, dv):
    """One sweep: reads only the given (du, dv).  A neighbour outside the array is read replicated (its weight is zero at
    an image border; on a cut-out tile it makes the outermost ring wrong, which is what the halo is for)."""
    U, V = u + du, v + dv
    ws = ((c["wl"] + c["wr"]) + c["wt"]) + c["wb"]
    lap = lambda F: ((c["wl"] * _nb(F, -1, -1) + c["wr"] * _nb(F, 1, -1)) + c["wt"] * _nb(F, -1, -2)) + c["wb"] * _nb(F, 1, -2)
    b1 = (lap(U) - ws * u) - c["c1"]
    b2 = (lap(V) - ws * v) - c["c2"]
    det = c["a11"] * c["a22"] - c["a12"] * c["a12"]
    return (c["a22"] * b1 - c["a12"] * b2) / det, (c["a11"] * b2 - c["a12"] * b1) / det


def flow_level(Ia, Ib, flow, alpha=5.0, warps=5, outer=3, sweeps=50):
    """Step 4 on grey images (P, H, W) from the starting flow (P, H, W, 2); returns the new flow"""
    dt = Ia.dtype
    u, v = flow[..., 0].to(dt).clone(), flow[..., 1].to(dt).clone()
    for _ in range(warps):
        t = warp_terms(Ia, Ib, u, v)
        du, dv = torch.zeros_like(u), torch.zeros_like(v)
        for _ in range(outer):
            c = coefficients(t, u, v, du, dv, alpha)
            for _ in range(sweeps):
                du, dv = jacobi_sweep(c, u, v, du, dv)
        u, v = u + du, v + dv
    return torch.stack([u, v], -1)


def pyramid(I, min_side=16):
    levels = [I]
    for _ in level_sizes(I.shape[-2], I.shape[-1], min_side)[1:]:
        levels.append(pyr_down(levels[-1]))
    return levels


def estimate_flow(a, b, alpha=5.0, warps=5, outer=3, sweeps=50, min_side=16, dtype=torch.float64):
    """a, b (P, H, W, 3) or (H, W, 3) -> the flow a -> b on a's grid, (P, H, W, 2) or (H, W, 2), in ``dtype``"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    single = a.dim() == 3
    if single:
        a, b = a[None], b[None]
    pa, pb = pyramid(grey(a, dtype), min_side), pyramid(grey(b, dtype), min_side)
    flow = torch.zeros(pa[-1].shape + (2,), dtype=dtype)
    for l in range(len(pa) - 1, -1, -1):
        if l < len(pa) - 1:
            flow = upsample_flow(flow, pa[l].shape[-2], pa[l].shape[-1])
        flow = flow_level(pa[l], pb[l], flow, alpha, warps, outer, sweeps)
    return flow[0] if single else flow
