"""The image loss restated in plain torch with every intermediate map returned, the seeded images and masks the loss
tests run on, and the ONE tolerance rule they all use.

``loss_ref`` is ``oracle/loss_oracle.py``'s arithmetic (2-D 11 x 11 window, zero padding, autograd) with ``dtype`` as a
parameter: float64 is the reference, float32 the yardstick.  The rule (``Rule``): a result is held to float64 within
``FACTOR`` times the error E32 of the float32 run of this very file -- never to a constant, because on a smooth image the
SSIM term is a difference of nearly equal float32 numbers and the float32 oracle itself is off by 4e-3 relative on the loss,
and never to anything measured on the code under test.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from oracle import loss_oracle as LO

TILE = 16
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2
FACTOR = 4.0                     # the kernel is another sample of float32 rounding, not another algorithm
FLOOR = 2.0 ** -22               # of the quantity's own float64 scale, where E32 would be (next to) zero


# ------------------------------------------------------------------ the restatement
def blur2d(x, dtype):
    """(1,3,H,W) through the 11 x 11 window of ``LO.ssim``: the float32 outer product of the float32 1-D window."""
    w1 = LO.ssim_window(11, 1.5, torch.float32)
    win = (w1.unsqueeze(1) @ w1.unsqueeze(0)).to(dtype).expand(3, 1, 11, 11).contiguous()
    return F.conv2d(x, win, padding=5, groups=3)


def tile_sum(m):
    """(..., H, W) -> (..., gy * gx): sums over the 16 x 16 tiles, row-major tile order."""
    H, W = m.shape[-2:]
    gy, gx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    p = F.pad(m, (0, gx * TILE - W, 0, gy * TILE - H))
    return p.reshape(*m.shape[:-2], gy, TILE, gx, TILE).sum(dim=(-3, -1)).reshape(*m.shape[:-2], gy * gx)


def loss_ref(render4, gt_rgb, gt_depth, keep, ab, lambda_rgb, lambda_depth, dtype=torch.float64, blur=blur2d, c2=SSIM_C2,
             mask_target=True):
    """render4 (4,H,W); gt_rgb (H,W,3); gt_depth (H,W) or None; keep (H,W), 0 = masked out, or None; ab = (a, b) or None.
    Inputs are rounded to float32 first, then promoted to ``dtype``.  L = lambda_rgb (mean err_px + 1 - mean S) +
    lambda_depth mean depth_px.  As in the kernels, the depth term exists only with lambda_depth != 0.
    ``blur``, ``c2``, ``mask_target`` are there for tests/test_loss_ref_host.py to state another implementation, and a wrong one.

    Returns a dict of detached tensors of ``dtype``:
      S (3,H,W), err_px (H,W), depth_px (H,W), da_px, db_px (H,W: each pixel's share of dL/da, dL/db),
      sums (5) = {sum err_px, sum S, sum depth_px, dL/da, dL/db}  (the layout of gfl_loss_fwd_bwd),
      p_ssim (3 T) indexed c * T + tile, p_grad (T,4) = per-tile {err_px, depth_px, dL/da, dL/db},
      d_render (4,H,W), d_ab (2), gt_stats (6,H,W) = [c][conv(y), conv(y^2)], loss."""
    r = render4.detach().float().to(dtype)
    H, W = r.shape[1:]
    x = r[:3].clone().requires_grad_(True)
    D = r[3].clone().requires_grad_(True)
    y = gt_rgb.detach().float().to(dtype).permute(2, 0, 1)
    k = None if keep is None else (keep != 0).to(dtype)
    xm = x if k is None else x * k
    ym = y if (k is None or not mask_target) else y * k
    err_px = ((xm - ym) ** 2).permute(1, 2, 0).mean(dim=2)
    bl = lambda t: blur(t.unsqueeze(0), dtype)[0]
    mu1, mu2 = bl(xm), bl(ym)
    e22 = bl(ym * ym)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = bl(xm * xm) - mu1_sq
    s2 = e22 - mu2_sq
    s12 = bl(xm * ym) - mu12
    S = ((2 * mu12 + SSIM_C1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + SSIM_C1) * (s1 + s2 + c2))
    with_depth = gt_depth is not None and ab is not None and lambda_depth != 0
    zero = torch.zeros(H, W, dtype=dtype)
    if with_depth:
        gd = gt_depth.detach().float().to(dtype).reshape(H, W)
        a32, b32 = (torch.tensor(float(v), dtype=torch.float32).to(dtype) for v in ab)
        a_px = a32.expand(H, W).clone().requires_grad_(True)
        b_px = b32.expand(H, W).clone().requires_grad_(True)
        d = a_px * D + b_px
        depth_px = (d - gd) ** 2 / (d + gd)
        if k is not None:
            depth_px = depth_px * k
    else:
        a_px = b_px = None
        depth_px = zero
    loss = lambda_rgb * (err_px.mean() + (1 - S.mean())) + lambda_depth * depth_px.mean()
    loss.backward()
    g = lambda t: zero.clone() if t is None or t.grad is None else t.grad
    d_render = torch.cat([x.grad if x.grad is not None else torch.zeros_like(x), g(D).unsqueeze(0)])
    da_px, db_px = g(a_px), g(b_px)
    S, err_px, depth_px = S.detach(), err_px.detach(), depth_px.detach()
    terms = torch.stack([err_px, depth_px, da_px, db_px])
    sums = torch.stack([err_px.sum(), S.sum(), depth_px.sum(), da_px.sum(), db_px.sum()])
    gt_stats = torch.stack([mu2.detach(), e22.detach()], dim=1).reshape(6, H, W)
    return dict(S=S, err_px=err_px, depth_px=depth_px, da_px=da_px, db_px=db_px, sums=sums, p_ssim=tile_sum(S).reshape(-1),
                p_grad=tile_sum(terms).T.contiguous(), d_render=d_render, d_ab=torch.stack([da_px.sum(), db_px.sum()]),
                gt_stats=gt_stats, loss=loss.detach())


# ------------------------------------------------------------------ images and masks (seeded)
REGIMES = ("noisy", "smooth1e-2", "smooth1e-3", "same_noisy", "same_smooth", "flat")
MASKS = ("none", "disc", "all_kept", "all_masked", "one_kept", "one_masked_15", "one_masked_16", "cols_ge16", "checker")
DEFAULT_AB = (1.1, -0.05)
FLAT_A, FLAT_B = 0.7, 0.6


def _sinusoid(H, W, g):
    """sin * sin with a period of 40 to 90 pixels per axis and random phases: in [-1, 1], smooth at every image size."""
    f = 1.0 / (40.0 + 50.0 * torch.rand(2, generator=g, dtype=torch.float64))
    ph = 2 * math.pi * torch.rand(2, generator=g, dtype=torch.float64)
    yy = torch.arange(H, dtype=torch.float64).unsqueeze(1)
    xx = torch.arange(W, dtype=torch.float64).unsqueeze(0)
    return torch.sin(2 * math.pi * f[0] * xx + ph[0]) * torch.sin(2 * math.pi * f[1] * yy + ph[1])


def _smooth_depth(H, W, g, ab):
    a, b = ab if ab is not None else (1.0, 0.0)
    gtd = 2.5 + 1.5 * _sinusoid(H, W, g)                                               # [1, 4]
    dm = (gtd - b) / a * (1.0 + 0.01 * (2.0 * torch.rand(H, W, generator=g, dtype=torch.float64) - 1.0))
    return gtd.float(), dm.float()


def noisy(H, W, seed):
    """The recipe of tests/test_gpu_loss_optim.py: local variance ~1/12, a hundred times C2."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, 3, generator=g)
    rgb = (gt.permute(2, 0, 1) + 0.08 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gtd = 1.0 + 3.0 * torch.rand(H, W, 1, generator=g)
    dm = (gtd.permute(2, 0, 1) * (1 + 0.1 * torch.randn(1, H, W, generator=g))).clamp(min=0.1)
    return dict(render4=torch.cat([rgb, dm]).contiguous(), gt_rgb=gt.contiguous(), gt_depth=gtd[..., 0].contiguous())


def smooth(H, W, seed, amp, ab=DEFAULT_AB):
    """Where a fit lives: the target a product of low-frequency sinusoids per channel in [0.15, 0.85], the render within
    ``amp`` of it (local variance below C2); gt_depth smooth in [1, 4], the render's depth within 1 % of (gt - b) / a."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.stack([0.5 + 0.35 * _sinusoid(H, W, g) for _ in range(3)], dim=2).float()
    rgb = gt.permute(2, 0, 1) if amp == 0 else (gt.permute(2, 0, 1) + amp * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gtd, dm = _smooth_depth(H, W, g, ab)
    return dict(render4=torch.cat([rgb, dm.unsqueeze(0)]).contiguous(), gt_rgb=gt.contiguous(), gt_depth=gtd.contiguous())


def flat(H, W, seed, a=FLAT_A, b=FLAT_B, ab=DEFAULT_AB):
    """Constant images: render a, target b (the depth planes are the smooth ones)."""
    g = torch.Generator().manual_seed(seed)
    gtd, dm = _smooth_depth(H, W, g, ab)
    return dict(render4=torch.cat([torch.full((3, H, W), a), dm.unsqueeze(0)]).contiguous(), gt_rgb=torch.full((H, W, 3), b),
                gt_depth=gtd.contiguous())


def make_inputs(regime, H, W, seed, ab=DEFAULT_AB):
    if regime == "noisy":
        return noisy(H, W, seed)
    if regime == "same_noisy":                                   # render == target, bit for bit
        d = noisy(H, W, seed)
        d["render4"][:3] = d["gt_rgb"].permute(2, 0, 1)
        return d
    if regime == "same_smooth":
        return smooth(H, W, seed, 0.0, ab)
    if regime == "flat":
        return flat(H, W, seed, ab=ab)
    return smooth(H, W, seed, {"smooth1e-2": 1e-2, "smooth1e-3": 1e-3}[regime], ab)


def make_keep(name, H, W):
    """uint8 (H,W), 0 = masked out; None for "none"; None as well where the image has no such pixel."""
    if name == "none":
        return None
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    keep = torch.ones(H, W, dtype=torch.bool)
    if name == "disc":
        keep = ~(((yy - H * 0.4) ** 2 + (xx - W * 0.6) ** 2) < (0.2 * H) ** 2)
    elif name == "all_masked":
        keep[:] = False
    elif name == "one_kept":
        keep[:] = False
        keep[0, 0] = True
    elif name in ("one_masked_15", "one_masked_16"):
        p = int(name[-2:])
        assert p < H and p < W, f"{name}: no pixel ({p},{p}) in a {H} x {W} image"
        keep[p, p] = False
    elif name == "cols_ge16":
        keep = xx < 16
    elif name == "checker":
        keep = ((yy + xx) % 2) == 0
    else:
        assert name == "all_kept", name
    return keep.to(torch.uint8).contiguous()


# ------------------------------------------------------------------ cells
class Cell(collections.namedtuple("Cell", "regime H W mask lam_rgb lam_depth ab")):
    """(regime, shape, mask, lambdas and depth affine); ab None = gt_depth and depth_ab are null."""
    __slots__ = ()

    @property
    def id(self):
        ab = "nodepth" if self.ab is None else f"ab{self.ab[0]:g},{self.ab[1]:g}"
        return f"{self.regime}-{self.H}x{self.W}-{self.mask}-lam{self.lam_rgb:g},{self.lam_depth:g}-{ab}"

    @property
    def seeds(self):
        n = 8 if self.H * self.W < 256 else 4          # a maximum over a handful of pixels is a lottery
        return tuple(range(100, 100 + n))


def cell(regime, H, W, mask="none", lam=(1.0, 0.1), ab=DEFAULT_AB):
    return Cell(regime, H, W, mask, float(lam[0]), float(lam[1]), ab)


# tile 16, halo 5, window 11, 8-way block remap: below a tile, below the window, below the halo, one pixel wide, fewer than
# eight workgroups, a width ending on a tile edge, one pixel past it, several tiles with a ragged edge
SHAPES = ((1, 1), (1, 40), (40, 1), (3, 5), (5, 5), (6, 6), (11, 11), (15, 15), (16, 16), (17, 17), (16, 32),
          (21, 27), (26, 47), (33, 17), (48, 70))
ALL_REGIME_SHAPES = ((5, 5), (16, 16), (21, 27), (48, 70))
MASK_SHAPES = ((16, 16), (21, 27), (48, 70))
LAMBDA_CASES = (((1.0, 0.1), (0.9, 0.2)), ((1.0, 0.0), None), ((0.0, 0.1), DEFAULT_AB), ((0.3, 1.0), DEFAULT_AB))


def _cells():
    shape_cells, mask_cells, lambda_cells, known = [], [], [], []
    for H, W in SHAPES:
        for regime in ("noisy", "smooth1e-2", "smooth1e-3"):
            if regime == "smooth1e-2" and (H, W) not in ALL_REGIME_SHAPES:
                continue
            shape_cells.append(cell(regime, H, W))
    for H, W in MASK_SHAPES:
        for mask in MASKS[1:]:
            if mask == "one_masked_16" and not (H > 16 and W > 16):
                continue
            for regime in ("noisy", "smooth1e-3"):
                mask_cells.append(cell(regime, H, W, mask))
    for lam, ab in LAMBDA_CASES:
        for regime in ("noisy", "smooth1e-3"):
            for mask in ("none", "disc"):
                lambda_cells.append(cell(regime, 21, 27, mask, lam, ab))
    for regime in ("same_noisy", "same_smooth"):
        for H, W in ((5, 5), (21, 27), (40, 40)):
            known.append(cell(regime, H, W))
    known.append(cell("flat", 48, 48))
    return tuple(shape_cells), tuple(mask_cells), tuple(lambda_cells), tuple(known)


SHAPE_CELLS, MASK_CELLS, LAMBDA_CELLS, KNOWN_CELLS = _cells()
CELLS = SHAPE_CELLS + MASK_CELLS + LAMBDA_CELLS + KNOWN_CELLS


def cell_inputs(c, seed):
    d = make_inputs(c.regime, c.H, c.W, seed, c.ab if c.ab is not None else DEFAULT_AB)
    d["keep"] = make_keep(c.mask, c.H, c.W)
    if c.ab is None:
        d["gt_depth"] = None
    return d


def run_ref(c, inp, dtype, **variant):
    return loss_ref(inp["render4"], inp["gt_rgb"], inp["gt_depth"], inp["keep"], c.ab, c.lam_rgb, c.lam_depth, dtype=dtype,
                    **variant)


# ------------------------------------------------------------------ the rule
QUANTITIES = ("d_render", "gt_stats", "p_ssim", "p_grad", "sums")


def _l1_maps(r):
    """The per-pixel terms behind every scalar: S (3,H,W) and (err_px, depth_px, da_px, db_px) (4,H,W)."""
    return r["S"], torch.stack([r["err_px"], r["depth_px"], r["da_px"], r["db_px"]])


class Rule:
    """E32 of one cell, from the float32 and float64 runs of ``loss_ref`` on all of its seeds, and the comparison.

    per-pixel arrays (d_render per plane, gt_stats per map): E32 = max |x32 - x64|, largest over the seeds;
    scalars and per-tile sums: E32 = sum over the pixels entering the sum of |x32 - x64| (an L1 bound: the signed errors
    of a sum cancel by luck), largest over the seeds;
    floor: 2^-22 of the quantity's own float64 scale (max abs of the array / sum of abs terms);
    a result must be within FACTOR * E32 of float64 on EVERY seed, no entry excluded."""

    def __init__(self, c):
        self.cell = c
        self.inputs = [cell_inputs(c, s) for s in c.seeds]
        self.r64 = [run_ref(c, i, torch.float64) for i in self.inputs]
        r32 = [{k: v.double() for k, v in run_ref(c, i, torch.float32).items()} for i in self.inputs]
        E = {}
        for a, b in zip(r32, self.r64):
            e = {}
            for q in ("d_render", "gt_stats"):
                e[q] = torch.maximum((a[q] - b[q]).abs().amax(dim=(1, 2)), FLOOR * b[q].abs().amax(dim=(1, 2)))
            (sa, ta), (sb, tb) = _l1_maps(a), _l1_maps(b)
            ds = torch.maximum(tile_sum((sa - sb).abs()), FLOOR * tile_sum(sb.abs()))            # (3, T)
            dt = torch.maximum(tile_sum((ta - tb).abs()), FLOOR * tile_sum(tb.abs()))            # (4, T)
            e["p_ssim"] = ds.reshape(-1)
            e["p_grad"] = dt.T.contiguous()
            tot_s = torch.maximum((sa - sb).abs().sum(), FLOOR * sb.abs().sum())
            tot_t = torch.maximum((ta - tb).abs().sum(dim=(1, 2)), FLOOR * tb.abs().sum(dim=(1, 2)))
            e["sums"] = torch.stack([tot_t[0], tot_s, tot_t[1], tot_t[2], tot_t[3]])
            for q, v in e.items():
                E[q] = v if q not in E else torch.maximum(E[q], v)
        self.E32 = E

    def bound(self, q, shape):
        e = self.E32[q]
        return e.reshape(-1, 1, 1).expand(shape) if q in ("d_render", "gt_stats") else e

    def compare(self, k, got):
        """``got``: name -> tensor for any of QUANTITIES (and ``err_px``), of seed number ``k``.  Returns (ratios, failures):
        the worst |got - x64| / E32 per quantity (0 / 0 counts as 0) and one line per quantity that breaks the rule."""
        ref, inp = self.r64[k], self.inputs[k]
        ratios, failures = {}, []
        for q in QUANTITIES:
            if q not in got:
                continue
            x = got[q].detach().double().cpu().reshape(ref[q].shape)
            err = (x - ref[q]).abs()
            err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
            B = self.bound(q, err.shape)
            ratio = torch.where(err == 0, torch.zeros_like(err), err / B)
            ratios[q] = float(ratio.max())
            if bool((err > FACTOR * B).any()):
                i = int(torch.argmax(ratio.reshape(-1)))
                failures.append(f"{q}[flat index {i} of {tuple(err.shape)}]: got "
                                f"{x.reshape(-1)[i]:.9e} float64 {ref[q].reshape(-1)[i]:.9e} err {err.reshape(-1)[i]:.3e} "
                                f"E32 {B.reshape(-1)[i]:.3e} ratio {ratios[q]:.2f}")
        if "err_px" in got:
            # three subtractions, three FMAs, one multiply: held to float64 directly; exactly 0 where masked out
            x = got["err_px"].detach().double().cpu().reshape(ref["err_px"].shape)
            bad = ~((x - ref["err_px"]).abs() <= 1e-6 * ref["err_px"].abs() + 1e-12)
            if inp["keep"] is not None:
                bad |= (inp["keep"] == 0) & (x != 0)
            if bool(bad.any()):
                i = int(torch.nonzero(bad.reshape(-1))[0])
                failures.append(f"err_px[{i // x.shape[1]},{i % x.shape[1]}]: got {x.reshape(-1)[i]:.9e} float64 "
                                f"{ref['err_px'].reshape(-1)[i]:.9e}")
        return ratios, failures


@functools.lru_cache(maxsize=None)
def rule(c):
    """The references of a cell, computed once per process and shared by every test that needs them (do not modify)."""
    return Rule(c)


def hold(c, results, label=""):
    """``results``: one dict per seed of the cell (see ``Rule.compare``).  Prints the worst ratios, then asserts the rule."""
    ru = rule(c)
    assert len(results) == len(c.seeds)
    worst, failures = {}, []
    for k, got in enumerate(results):
        ratios, f = ru.compare(k, got)
        for q, v in ratios.items():
            worst[q] = max(worst.get(q, 0.0), v)
        failures += [f"seed {c.seeds[k]}: {line}" for line in f]
    print(f"RATIO {label} {c.id} " + " ".join(f"{q}={v:.3f}" for q, v in worst.items()))
    assert not failures, f"{label} {c.id}: outside {FACTOR:g} x E32 of float64\n" + "\n".join(failures)
    return worst
