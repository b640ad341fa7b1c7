"""The reconstruction score on the device (``-m gpu``; gfl_recon_frame, gflow_amd/quality.py): the kernel's two sums through
the C ABI against the float64 numpy restatement (tests/quality_ref.py) run on the bytes torch itself forms from the same
floats, on every shape at which the tiling takes another path; the row it writes and the rows it leaves; bit-identical
repeats; argument errors; and a fit's ``out["recon"]`` against the restatement run on the renders the fit recorded."""
import json

import numpy as np
import pytest
import torch

from tests import quality_ref as R
from tests import score_fit as SF

pytestmark = pytest.mark.gpu
DEV = "cuda"
GARBAGE = -1234.5678e100
TILE_H, TILE_W = 16 + 10, 32 + 10        # the image that is exactly one tile of window positions (gfl_recon.hip)


def _recon(render, gt, frame=0, T=1, sums=None):
    """gfl_recon_frame through the C ABI on device tensors; the sums are pre-filled with garbage.
    Returns (status, sums (T, 2) float64 array)."""
    from gflow_amd import _lib as L
    lib = L.load()
    _, h, w = render.shape
    assert render.is_contiguous() and gt.is_contiguous() and tuple(gt.shape) == (h, w, 3)
    ws = L.scratch(lib.gfl_recon_workspace_bytes(w, h), DEV)
    if sums is None:
        sums = torch.full((max(T, 1), 2), GARBAGE, dtype=torch.float64, device=DEV)
    rc = lib.gfl_recon_frame(L.ptr(render), L.ptr(gt), w, h, frame, T, L.ptr(sums), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return rc, sums.cpu().numpy()


def _seeded(h, w, seed=None):
    """a four-plane render that reaches below 0 and above 1, and a target that does too"""
    rng = np.random.default_rng(h * 1000 + w if seed is None else seed)
    render = torch.from_numpy(rng.uniform(-0.3, 1.3, size=(4, h, w)).astype(np.float32)).to(DEV)
    # (close to the render where it is inside [0, 1]: an SSIM away from 0, as a fit's is)
    gt = render[:3].permute(1, 2, 0).cpu().numpy() + rng.normal(scale=0.08, size=(h, w, 3)).astype(np.float32)
    assert render.min() < 0 and render.max() > 1 and gt.min() < 0 and gt.max() > 1
    return render, torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float32)).to(DEV)


def _exact(h=20, w=40):
    """every k / 255 in float32, 1.0, -0.0 and nextafter(1, 2), cycling through the image"""
    vals = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255.0),
                           np.array([1.0, -0.0, np.nextafter(np.float32(1), np.float32(2))], dtype=np.float32)])
    n = 3 * h * w
    flat = np.resize(vals, n)
    assert n >= 2 * len(vals)
    render = torch.from_numpy(flat.reshape(3, h, w).copy()).to(DEV)
    gt = torch.from_numpy(np.resize(vals[::-1], n).reshape(h, w, 3).copy()).to(DEV)
    return render, gt


def _want(render, gt):
    return R.sums(R.bytes_of(render), gt.cpu().numpy())


# a single window; one more column / row; one row of windows over three column tiles; exactly one tile; one tile plus one
# pixel in each direction (a second tile with one window position, in x, in y and in both); tiles cut in both directions
SHAPES = [(11, 11), (11, 12), (12, 11), (11, 75), (TILE_H, TILE_W), (TILE_H, TILE_W + 1), (TILE_H + 1, TILE_W),
          (TILE_H + 1, TILE_W + 1), (43, 27), (58, 91)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_sums_equal_the_restatement(h, w):
    render, gt = _seeded(h, w)
    rc, got = _recon(render, gt)
    assert rc == 0
    SF.assert_sums(got[0, 0], got[0, 1], *_want(render, gt), h, w, "seeded")


def test_sums_at_480p():
    h, w = 480, 854
    render, gt = _seeded(h, w)
    rc, got = _recon(render, gt)
    assert rc == 0
    SF.assert_sums(got[0, 0], got[0, 1], *_want(render, gt), h, w, "seeded")


def test_sums_on_exact_byte_values():
    render, gt = _exact()
    k = R.bytes_of(render)
    assert k.min() == 0 and k.max() == 255           # (whether (k / 255) * 255 truncates back to k is torch's to say)
    rc, got = _recon(render, gt)
    assert rc == 0
    _, h, w = render.shape
    SF.assert_sums(got[0, 0], got[0, 1], *_want(render, gt), h, w, "exact")
    # against itself read back: no error at all, SSIM 1
    same = torch.from_numpy(np.ascontiguousarray(R.read_back(k), dtype=np.float32)).to(DEV)
    rc, got = _recon(render, same)
    assert rc == 0
    SF.assert_sums(got[0, 0], got[0, 1], 0.0, 3.0 * (h - 10) * (w - 10), h, w, "identical")


def test_one_row_is_written_and_the_others_stay():
    render, gt = _seeded(43, 27)
    rc, got = _recon(render, gt, frame=1, T=3)
    assert rc == 0
    garbage = np.float64(GARBAGE)
    assert (got[0] == garbage).all() and (got[2] == garbage).all()
    SF.assert_sums(got[1, 0], got[1, 1], *_want(render, gt), 43, 27, "row 1")
    # (written, not accumulated: the row held garbage before the call)
    rc, first = _recon(render, gt, frame=0, T=1)
    assert rc == 0 and first[0].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("h,w", [(58, 91), (480, 854)])
def test_two_calls_are_bit_identical(h, w):
    render, gt = _seeded(h, w, seed=7)
    for det in (False, True):
        prev = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(det)
        try:
            a = _recon(render, gt)
            b = _recon(render, gt)
        finally:
            torch.use_deterministic_algorithms(prev)
        assert a[0] == 0 and b[0] == 0
        assert a[1].tobytes() == b[1].tobytes()


def test_argument_errors():
    from gflow_amd import _lib as L
    garbage = np.float64(GARBAGE)
    render, gt = _seeded(12, 13)
    for frame, T in ((-1, 2), (2, 2), (0, 0), (5, 1)):
        rc, got = _recon(render, gt, frame=frame, T=T)
        assert rc == -1 and L.load().gfl_status_string(rc) == L.load().gfl_status_string(-1)
        assert (got == garbage).all()                           # nothing written
    for h, w in ((10, 40), (40, 10), (10, 10)):
        render = torch.zeros((3, h, w), dtype=torch.float32, device=DEV)
        gt = torch.zeros((h, w, 3), dtype=torch.float32, device=DEV)
        rc, got = _recon(render, gt)
        assert rc == -1 and (got == garbage).all()
        assert L.load().gfl_recon_workspace_bytes(w, h) == 0
    assert L.load().gfl_recon_workspace_bytes(11, 11) == 3 * 2 * 8


def test_recorder_gives_the_scores():
    from gflow_amd import quality as QL
    h, w = 43, 27
    rec = QL.ReconRecorder(2, h, w, DEV)
    pairs = [_seeded(h, w, seed=1), _seeded(h, w, seed=2)]
    for i in (1, 0):                                            # (any order: a frame writes its own row)
        rec.frame(i, *pairs[i])
    out = rec.result()
    for i, (render, gt) in enumerate(pairs):
        sse, ssim_sum = _want(render, gt)
        SF.assert_sums(out["sse"][i], out["ssim_sum"][i], sse, ssim_sum, h, w, f"recorder {i}")
        assert out["PSNR"][i] == R.psnr(out["sse"][i], h, w) and out["SSIM"][i] == R.ssim(out["ssim_sum"][i], h, w)
    with pytest.raises(RuntimeError):
        rec.frame(2, *pairs[0])
    with pytest.raises(ValueError):
        rec.frame(0, pairs[0][0][:, :-1], pairs[0][1])


def test_fit_scores_equal_the_restatement_on_the_recorded_renders():
    frames, q, out, keep = SF.scored_fit()
    ev = SF.check_recon_contract(frames, out, keep)
    print("reconstruction quality", json.dumps(ev))
