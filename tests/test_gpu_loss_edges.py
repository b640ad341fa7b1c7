"""The loss kernels of gfl_ssim.hip against float64 where they are most likely to be wrong (``-m gpu``): smooth images whose
local variance is below C2 (the SSIM term and its three derivative maps are differences of nearly equal float32 numbers),
images smaller than a tile, than the window, than the halo, one pixel wide, launches of fewer than eight workgroups, mask
edges on tile corners and tile boundaries, and every lambda a scale of its own.

All three entry points, through the C ABI: ``gfl_loss_fwd_bwd`` (sums through loss_fold_kernel), ``gfl_loss_fwd_bwd_partials``
and ``gfl_loss_prepare_gt`` + ``gfl_loss_fwd_bwd_partials_cached`` (the one the fused iteration calls).  Every plane of d_render,
err_px, every per-tile partial, the five sums and the six gt_stats planes are compared; the outputs are pre-filled with NaN,
so a pixel or a partial nobody wrote fails too.

ONE tolerance rule (tests/loss_ref.py: ``Rule``): within 4 x E32 of float64 on every seed of a cell, E32 being the error of
the float32 run of the reference's own arithmetic; tests/test_loss_ref_host.py shows that the rule passes an honest
separable float32 implementation and rejects five defective ones.  Nothing here is tuned on what the kernels give.

Every test prints, per cell and entry point, the worst |HIP - float64| / E32 of each quantity as a ``RATIO`` line; the
bound is 4.  Measured on an MI355X, worst over the cells of a regime (all shapes, masks and lambdas; the two partials entry
points give the same figures, the cached one to the digit shown, so mode 1's cached conv(y), conv(y^2) cost nothing):

    regime               d_render   p_ssim   p_grad   sums[0..4]   gt_stats
    noisy                    1.33     1.03     1.11      1.11         1.32
    smooth(1e-2)             1.88     0.47     0.50      0.59         0.99
    smooth(1e-3)             2.36     0.90     1.00      1.00         1.46
    render == target, noisy  1.95     0        0.44      0.44         1.01
    render == target, smooth 1.86     0        0.34      0.34         0.99
    flat 0.7 / 0.6           0.55     0.93     0.17      0.76         1.02
    flat, centre tile against the closed form: 0.90

Worst cells: d_render 2.36 at smooth(1e-3) 1x1 (one pixel, eight seeds; 48x70 has 0.79), gt_stats 1.46 at smooth(1e-3) 40x1,
p_ssim 1.03 at noisy 33x17, p_grad and sums 1.11 at noisy 21x27 with one kept pixel.  Nothing is above 2.4: the kernels sit
where the separable float32 restatement of tests/test_loss_ref_host.py sits (at most 2.1), not where a slip would put them.
"""
import ctypes

import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENTRIES = ("sums", "partials", "cached")
NAN = float("nan")
GFL_ERR_INVALID, GFL_ERR_WORKSPACE = -1, -2


def _device_inputs(c, inp):
    dev = lambda t: None if t is None else t.contiguous().to(DEV)
    ab = None if c.ab is None else torch.tensor(c.ab, dtype=torch.float32, device=DEV)
    return dev(inp["render4"]), dev(inp["gt_rgb"]), dev(inp["gt_depth"]), dev(inp["keep"]), ab


def _args(L, c, d, out, err):
    render, gt, gd, keep, ab = d
    return (L.ptr(render), L.ptr(gt), L.ptr(gd), L.ptr(keep), L.ptr(ab), c.lam_rgb, c.lam_depth, c.W, c.H, L.ptr(out), L.ptr(err))


def call(entry, c, d):
    """One call of an entry point on device inputs ``d``; every output as a CPU tensor.  Outputs and workspace start as NaN."""
    from gflow_amd import _lib as L
    lib = L.load()
    H, W = c.H, c.W
    T = ((H + 15) // 16) * ((W + 15) // 16)
    out = torch.full((4, H, W), NAN, device=DEV)
    err = torch.full((H, W), NAN, device=DEV)
    nbytes = lib.gfl_loss_workspace_bytes(W, H)
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=DEV)                   # 0xffffffff: a NaN
    common = _args(L, c, d, out, err)
    res = {}
    if entry == "sums":
        sums = torch.full((8,), NAN, device=DEV)
        L.check(lib.gfl_loss_fwd_bwd(*common, L.ptr(sums), L.ptr(ws), nbytes, L.stream()), "gfl_loss_fwd_bwd")
        torch.cuda.synchronize()
        assert torch.all(sums[5:] == 0)
        res["sums"] = sums[:5].cpu()
    else:
        ps, pg, ns, ng = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        tail = (ctypes.byref(ps), ctypes.byref(ns), ctypes.byref(pg), ctypes.byref(ng), L.stream())
        if entry == "cached":
            stats = torch.full((6, H, W), NAN, device=DEV)
            L.check(lib.gfl_loss_prepare_gt(common[1], common[3], W, H, L.ptr(stats), L.stream()), "gfl_loss_prepare_gt")
            L.check(lib.gfl_loss_fwd_bwd_partials_cached(*common, L.ptr(ws), nbytes, L.ptr(stats), *tail), "cached")
        else:
            L.check(lib.gfl_loss_fwd_bwd_partials(*common, L.ptr(ws), nbytes, *tail), "partials")
        torch.cuda.synchronize()
        assert ns.value == 3 * T and ng.value == T
        o_s, o_g = ps.value - ws.data_ptr(), pg.value - ws.data_ptr()
        assert 0 <= o_s and o_s + 12 * T <= o_g and o_g + 16 * T <= nbytes
        res["p_ssim"] = ws[o_s:o_s + 12 * T].view(torch.float32).clone().cpu()
        res["p_grad"] = ws[o_g:o_g + 16 * T].view(torch.float32).clone().cpu().reshape(T, 4)
        if entry == "cached":
            res["gt_stats"] = stats.cpu()
    res["d_render"], res["err_px"] = out.cpu(), err.cpu()
    return res


def run_cell(entry, c):
    """The entry point on every seed of the cell; prints the worst ratios, asserts the rule, returns the raw results."""
    ru = R.rule(c)
    results = [call(entry, c, _device_inputs(c, inp)) for inp in ru.inputs]
    R.hold(c, results, entry)
    return results


def _ids(v):
    return v.id if isinstance(v, R.Cell) else str(v)


# ------------------------------------------------------------------ shapes x regimes
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("c", R.SHAPE_CELLS, ids=_ids)
def test_shapes_and_regimes(c, entry):
    run_cell(entry, c)


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("c", R.MASK_CELLS, ids=_ids)
def test_masks(c, entry):
    results = run_cell(entry, c)
    if c.mask == "all_masked":
        n = c.H * c.W
        for got in results:
            assert torch.all(got["d_render"] == 0) and torch.all(got["err_px"] == 0)
            if "sums" in got:
                assert torch.all(got["sums"][[0, 2, 3, 4]] == 0)
                assert abs(got["sums"][1].item() - 3 * n) <= 3 * n * 2.0 ** -21              # S = C1 C2 / (C1 C2) everywhere
            else:
                assert torch.all(got["p_grad"] == 0)
                assert abs(got["p_ssim"].double().sum().item() - 3 * n) <= 3 * n * 2.0 ** -21
    if c.mask == "all_kept":
        # the KEEP = true instantiations on the numbers of the no-mask call: two compilations of one arithmetic, so every
        # output, reductions included, within 2e-6 of its own scale (p_grad and sums: column by column)
        for got, inp in zip(results, R.rule(c).inputs):
            d = _device_inputs(c, inp)
            plain = call(entry, c, d[:3] + (None,) + d[4:])
            assert set(plain) == set(got)
            assert torch.equal(got["err_px"], plain["err_px"])
            for q in ("d_render", "p_ssim"):
                if q in got:
                    assert (got[q] - plain[q]).abs().max().item() <= 2e-6 * plain[q].abs().max().item(), q
            for q in ("p_grad", "sums"):
                if q in got:
                    scale = plain[q].abs().reshape(-1, plain[q].shape[-1]).amax(dim=0)
                    assert bool(((got[q] - plain[q]).abs().reshape(-1, plain[q].shape[-1]) <= 2e-6 * scale).all()), q


# ------------------------------------------------------------------ lambdas, depth affine, null depth
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("c", R.LAMBDA_CELLS, ids=_ids)
def test_lambdas_and_depth(c, entry):
    for got in run_cell(entry, c):
        if c.lam_rgb == 0:
            assert torch.all(got["d_render"][:3] == 0)
        if c.lam_depth == 0:
            assert torch.all(got["d_render"][3] == 0)
            if "sums" in got:
                assert torch.all(got["sums"][2:] == 0)
            else:
                assert torch.all(got["p_grad"][:, 1:] == 0)


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("c", [c for c in R.KNOWN_CELLS if c.regime.startswith("same")], ids=_ids)
def test_render_equal_to_target(c, entry):
    """err_px and its sum exactly 0; loss and rgb gradient are the float32 residue of a value that is 1e-13 and 1e-16 in
    float64, so the rule's bound IS the float32 oracle's own residue."""
    for got in run_cell(entry, c):
        assert torch.all(got["err_px"] == 0)
        if "sums" in got:
            assert got["sums"][0].item() == 0
        else:
            assert torch.all(got["p_grad"][:, 0] == 0)


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_flat_images_centre_tile_closed_form(entry):
    """48 x 48, render 0.7, target 0.6: the centre tile is 16 pixels from every border and its three p_ssim entries are
    256 (2ab + C1) / (a^2 + b^2 + C1) -- worked out in python floats, independent of any oracle, held under the rule."""
    c = R.KNOWN_CELLS[-1]
    assert c.regime == "flat" and (c.H, c.W) == (48, 48)
    a, b = (float(torch.tensor(v, dtype=torch.float32)) for v in (R.FLAT_A, R.FLAT_B))
    want = 256 * (2 * a * b + R.SSIM_C1) / (a * a + b * b + R.SSIM_C1)
    E = R.rule(c).E32["p_ssim"]
    worst = 0.0
    for got in run_cell(entry, c):
        for ch in range(3):
            i = ch * 9 + 4
            worst = max(worst, abs(got["p_ssim"][i].item() - want) / E[i].item())
    print(f"RATIO {entry} flat-centre-tile-closed-form p_ssim={worst:.3f}")
    assert worst <= R.FACTOR


def test_flat_images_through_the_fold():
    run_cell("sums", R.KNOWN_CELLS[-1])


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_calls_are_bit_identical(entry):
    """The "ordered fold (reproducible)" of the file header: sums, partials and gradients, bit for bit."""
    c = R.cell("noisy", 21, 27, "disc")
    d = _device_inputs(c, R.rule(c).inputs[0])
    a, b = call(entry, c, d), call(entry, c, d)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ------------------------------------------------------------------ argument checks that return before any launch
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("what", ["zero_width", "null_gt_depth", "workspace_one_byte_short"])
def test_argument_checks(what, entry):
    from gflow_amd import _lib as L
    lib = L.load()
    c = R.cell("noisy", 21, 27)
    render, gt, gd, keep, ab = _device_inputs(c, R.rule(c).inputs[0])
    H, W = c.H, c.W
    out = torch.full((4, H, W), NAN, device=DEV)
    err = torch.full((H, W), NAN, device=DEV)
    nbytes = lib.gfl_loss_workspace_bytes(W, H)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    sums = torch.full((8,), NAN, device=DEV)
    stats = torch.zeros(6, H, W, device=DEV)
    want = GFL_ERR_INVALID
    if what == "zero_width":
        assert lib.gfl_loss_workspace_bytes(0, H) == 0
        W = 0
    elif what == "null_gt_depth":
        gd = None
    else:
        nbytes, want = nbytes - 1, GFL_ERR_WORKSPACE                   # the buffer itself keeps its full size
    common = (L.ptr(render), L.ptr(gt), L.ptr(gd), L.ptr(keep), L.ptr(ab), 1.0, 0.1, W, H, L.ptr(out), L.ptr(err))
    ps, pg, ns, ng = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
    tail = (ctypes.byref(ps), ctypes.byref(ns), ctypes.byref(pg), ctypes.byref(ng), L.stream())
    if entry == "sums":
        rc = lib.gfl_loss_fwd_bwd(*common, L.ptr(sums), L.ptr(ws), nbytes, L.stream())
    elif entry == "partials":
        rc = lib.gfl_loss_fwd_bwd_partials(*common, L.ptr(ws), nbytes, *tail)
    else:
        if what == "zero_width":
            assert lib.gfl_loss_prepare_gt(L.ptr(gt), None, W, H, L.ptr(stats), L.stream()) == GFL_ERR_INVALID
        rc = lib.gfl_loss_fwd_bwd_partials_cached(*common, L.ptr(ws), nbytes, L.ptr(stats), *tail)
    torch.cuda.synchronize()
    assert rc == want
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(err).all()) and bool(torch.isnan(sums).all())   # nothing ran
