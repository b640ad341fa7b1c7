"""The move mask from the flow on the device (``-m gpu``; gfl_epi_fundamental, gfl_epi_mask, gflow_amd/move_seg.py) through
the C ABI, every output pre-filled with garbage, against the float64 restatement (tests/move_seg_ref.py) on the scenes of
tests/test_move_seg_host.py: 40 x 56, 37 x 53 (no multiple of a workgroup's share) and 64 x 65 (two shares) with K = 64, a third with unknown
pixels and broken samples, a fourth of 8 x 8 where disk(5) covers most of the image; and 2 x 4 and 3 x 4 with eight known
pixels, where the median's rank rests on the count that the selection's first pass finds.

Bounds.  F_CONST: ||F_device - F_restatement|| <= F_CONST * eps64 * lambda_max / lambda_1 -- the form eigenvector perturbation
theory gives for a null vector taken from A^T A; the theory does not give the constant, so it is measured: the largest ratio
on these scenes was 0.454 (0.413 at 40 x 56, 0.454 at 37 x 53, 0.337 at 8 x 8; one hypothesis of 192 left out), and F_CONST
is ten times that.  (64 x 65, added later for its two workgroups of EPI_PER_BLOCK = 4096 pixels -- the second has 64 --, gave
0.574 with one hypothesis of 64 left out: F_CONST stays what the first three scenes made it.)  MEDIAN_REL: the largest relative difference measured between the device's medians and the restatement's
medians of the device's own F was 0 -- all 192, and the 60 of the scene with unknown pixels, equal bit for bit -- so ten
times that is 0 and the test asks for equality.  It is not near 1e-12, the level cancellation in z would give two
differently ordered sums, because both sides evaluate the one expression include/gflow_hip.h writes down, in its order,
with IEEE operations and no contraction, and an exact selection has no error of its own.  ERR_NORM_REL: one float32 ulp,
2^-23 = 1.19e-7 -- the output's rounding to float32 is at most half of it, the other half is left to last-bit differences of
the float64 quotient (measured: 5.78e-8 at most, all of it the rounding)."""
import numpy as np
import pytest
import torch

from tests import move_seg_ref as R
from tests.test_move_seg_host import iou, make_scene, scene_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = float(np.finfo(np.float64).eps)
F_CONST = 10 * 0.454
MEDIAN_REL = 10 * 0.0
ERR_NORM_REL = 2.0 ** -23
RATIO_MIN, LEFT_OUT_MAX = 1e-9, 0.05
K = 64
SCENES = [(40, 56, 0), (37, 53, 1), (8, 8, 0), (64, 65, 2)]      # 64 x 65: two workgroups of EPI_PER_BLOCK = 4096 pixels, the second with 64
GARBAGE_F64, GARBAGE_U8, GARBAGE_I32 = -1234.5678e100, 0xA5, -77


def _fundamental(flow, samples, want_all=True, ws_bytes=None):
    """gfl_epi_fundamental through the C ABI.  Returns (status, dict of numpy arrays)."""
    from gflow_amd import _lib as L
    lib = L.load()
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    h, w, _ = flow.shape
    samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 8)
    k = samples.shape[0]
    f = torch.tensor(flow, device=DEV)
    s = torch.tensor(samples, device=DEV)
    ws = L.scratch(lib.gfl_epi_workspace_bytes(w, h, max(k, 1)) if ws_bytes is None else ws_bytes, DEV)
    ws.fill_(GARBAGE_U8)
    F_all = torch.full((max(k, 1), 9), GARBAGE_F64, dtype=torch.float64, device=DEV) if want_all else None
    med = torch.full((max(k, 1),), GARBAGE_F64, dtype=torch.float64, device=DEV) if want_all else None
    F = torch.full((9,), GARBAGE_F64, dtype=torch.float64, device=DEV)
    best = torch.full((1,), GARBAGE_I32, dtype=torch.int32, device=DEV)
    rc = lib.gfl_epi_fundamental(L.ptr(f), w, h, L.ptr(s), k, L.ptr(F_all), L.ptr(med), L.ptr(F), L.ptr(best), L.ptr(ws),
                                 ws.numel(), L.stream())
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return rc, dict(F_all=host(F_all), medians=host(med), F=host(F), best=int(best.item()))


def _mask(flow, F, threshold=0.01, outputs=("err_norm", "mask", "open", "erode", "dilate"), ws_bytes=None, k_for_ws=1):
    """gfl_epi_mask through the C ABI; outputs not asked for are passed as NULL.  Returns (status, dict of numpy arrays)."""
    from gflow_amd import _lib as L
    lib = L.load()
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    h, w, _ = flow.shape
    f = torch.tensor(flow, device=DEV)
    Fd = torch.from_numpy(np.ascontiguousarray(F, dtype=np.float64).reshape(9)).to(DEV)
    ws = L.scratch(lib.gfl_epi_workspace_bytes(w, h, k_for_ws) if ws_bytes is None else ws_bytes, DEV)
    ws.fill_(GARBAGE_U8)
    out = {}
    for name in outputs:
        out[name] = (torch.full((h, w), -7.5e30, dtype=torch.float32, device=DEV) if name == "err_norm"
                     else torch.full((h, w), GARBAGE_U8, dtype=torch.uint8, device=DEV))
    p = lambda name: L.ptr(out.get(name))
    rc = lib.gfl_epi_mask(L.ptr(f), w, h, L.ptr(Fd), float(threshold), p("err_norm"), p("mask"), p("open"), p("erode"),
                          p("dilate"), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return rc, {n: t.cpu().numpy() for n, t in out.items()}


def _rel(got, want):
    return abs(got - want) / want if want != 0 else (0.0 if got == 0 else np.inf)


# ------------------------------------------------------------------------------------------------------------ 1, 2: F, medians
@pytest.mark.parametrize("H,W,seed", SCENES)
def test_F_all_equals_the_restatement(H, W, seed):
    flow, disc, samples, ref = scene_case(H, W, seed, K)
    rc, got = _fundamental(flow, samples)
    assert rc == 0
    keep = ref["ratio"] >= RATIO_MIN
    assert np.isfinite(ref["ratio"]).all() and (~keep).mean() <= LEFT_OUT_MAX
    dF = np.linalg.norm(got["F_all"] - ref["F_all"].reshape(K, 9), axis=1)
    const = dF * ref["ratio"] / EPS
    print(f"F {H}x{W}: left out {(~keep).sum()} of {K}, largest ||dF|| {dF[keep].max():.3e}, largest constant {const[keep].max():.4f}"
          f" (all hypotheses: {const.max():.4f})")
    # the common scale and sign rule holds on the device's side as well
    norms = np.linalg.norm(got["F_all"], axis=1)
    assert np.abs(norms - 1.0).max() <= 8 * EPS
    big = got["F_all"][np.arange(K), np.abs(got["F_all"]).argmax(axis=1)]
    assert (big > 0).all()
    assert (const[keep] <= F_CONST).all()


@pytest.mark.parametrize("H,W,seed", SCENES)
def test_medians_equal_the_restatement_on_the_devices_F(H, W, seed):
    flow, disc, samples, ref = scene_case(H, W, seed, K)
    rc, got = _fundamental(flow, samples)
    assert rc == 0
    want = np.array([R.median_of(flow, got["F_all"][k]) for k in range(K)])
    rel = np.array([_rel(got["medians"][k], want[k]) for k in range(K)])
    print(f"medians {H}x{W}: largest relative difference {rel.max():.3e}, bit-equal {int((got['medians'] == want).sum())} of {K}")
    assert (rel <= MEDIAN_REL).all()
    b = got["best"]
    assert 0 <= b < K and want[b] <= want.min() * (1 + MEDIAN_REL)
    assert b == int(np.argmin(got["medians"]))                   # (np.argmin: the lowest index among equal medians)
    np.testing.assert_array_equal(got["F"], got["F_all"][b])
    # without the optional outputs: the same choice
    rc, lean = _fundamental(flow, samples, want_all=False)
    assert rc == 0 and lean["best"] == b and lean["F"].tobytes() == got["F"].tobytes()


# ------------------------------------------------------------------------------------------------------------ 3: unknown pixels
def _holes_case():
    from gflow_amd import move_seg as MS
    flow, disc = make_scene(40, 56, 2)
    flow = flow.copy()
    flow[5:11, 20:31, 0] = np.nan
    flow[30, 3, 1] = np.inf
    flow[31, 4] = -np.inf
    known = MS.known_pixels(flow)
    samples = MS.draw_samples(known, K, 2).copy()
    hole = 7 * 56 + 25
    assert not known[hole] and (~known).sum() == 68
    samples[5, 3] = samples[5, 0]                                # repeated
    samples[9, 2] = hole                                         # unknown
    samples[12, 0] = -1                                          # out of range, both sides
    samples[20, 7] = 40 * 56
    return flow, known, samples, [5, 9, 12, 20]


def test_unknown_pixels_and_broken_samples():
    flow, known, samples, broken = _holes_case()
    rc, got = _fundamental(flow, samples)
    assert rc == 0
    ok = np.ones(K, bool)
    ok[broken] = False
    assert np.isposinf(got["medians"][broken]).all() and not got["F_all"][broken].any()
    assert np.isfinite(got["medians"][ok]).all() and got["best"] not in broken
    # the median's n is the number of known pixels: the restatement's median over them, not over the image
    x1, x2, _ = R.correspondences(flow)
    over_known = np.array([R.median_of(flow, got["F_all"][k]) for k in np.flatnonzero(ok)])
    with np.errstate(invalid="ignore"):
        over_all = np.array([R.lower_median(np.where(known, R.sampson(got["F_all"][k], x1, x2), 0.0)) for k in np.flatnonzero(ok)])
    rel = np.array([_rel(g, w) for g, w in zip(got["medians"][ok], over_known)])
    print(f"holes: largest relative difference {rel.max():.3e}")
    assert (rel <= MEDIAN_REL).all() and (over_all != over_known).any()
    rc, m = _mask(flow, got["F"])
    assert rc == 0
    unknown = ~known.reshape(40, 56)
    for name in ("err_norm", "mask"):
        assert not m[name][unknown].any(), name
    assert m["err_norm"].max() == 1.0
    # a threshold below zero sets every known pixel and still no unknown one
    rc, low = _mask(flow, got["F"], threshold=-1.0, outputs=("mask",))
    assert rc == 0 and not low["mask"][unknown].any() and (low["mask"][~unknown] == 255).all()


# ------------------------------------------------------------------------------------------------------------------ 4: the mask
@pytest.mark.parametrize("H,W,seed", SCENES)
def test_mask_equals_the_restatement(H, W, seed):
    flow, disc, samples, ref = scene_case(H, W, seed, K)
    rc, got = _mask(flow, ref["F"])
    assert rc == 0
    want = ref["err_norm"]
    nz = want != 0
    rel = np.abs(got["err_norm"].astype(np.float64) - want)[nz] / want[nz]
    print(f"mask {H}x{W}: err_norm largest relative difference {rel.max():.3e} (2^-24 = {2.0 ** -24:.3e})")
    assert (rel <= ERR_NORM_REL).all() and not got["err_norm"][~nz].any()
    assert got["err_norm"].max() == 1.0 and got["err_norm"].min() >= 0.0
    near = np.abs(want - 0.01) <= ERR_NORM_REL * 0.01
    assert near.mean() <= 0.005
    np.testing.assert_array_equal(got["mask"][~near], ref["mask"][~near])
    assert set(np.unique(got["mask"])) <= {0, 255}
    o, e, d = R.morphology(got["mask"])
    np.testing.assert_array_equal(got["open"], o)
    np.testing.assert_array_equal(got["erode"], e)
    np.testing.assert_array_equal(got["dilate"], d)
    # each output alone (the mask then lives in the workspace): the same bytes
    for name in ("open", "erode", "dilate", "err_norm"):
        rc, one = _mask(flow, ref["F"], outputs=(name,), k_for_ws=K)
        assert rc == 0 and one[name].tobytes() == got[name].tobytes(), name


def test_morphology_on_masks_that_touch_every_border():
    """a threshold low enough to set most of the 8 x 8 and the 37 x 53 image: the eroded mask then depends on what counts
    as outside"""
    for (H, W, seed) in ((8, 8, 0), (37, 53, 1)):
        flow, disc, samples, ref = scene_case(H, W, seed, K)
        thr = float(np.quantile(ref["err_norm"], 0.2))
        rc, got = _mask(flow, ref["F"], threshold=thr)
        assert rc == 0
        assert 0.6 <= (got["mask"] != 0).mean() <= 0.9
        o, e, d = R.morphology(got["mask"])
        for name, want in (("open", o), ("erode", e), ("dilate", d)):
            np.testing.assert_array_equal(got[name], want, err_msg=f"{name} {H}x{W}")
        assert got["open"].any() and (H > 8 or got["dilate"].all())


# --------------------------------------------------------------------------------------------------------- 5: zeros, degenerate
def test_zero_flow_and_all_degenerate():
    H, W = 37, 53
    zero = np.zeros((H, W, 2), np.float32)
    skew = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) / np.sqrt(2.0)
    for F in (skew, np.zeros((3, 3))):                          # (a zero F is what best = -1 leaves in F_best)
        rc, got = _mask(zero, F)
        assert rc == 0
        for name, a in got.items():
            assert not a.any(), name
    # the fit of a zero flow runs (its F is some skew matrix, to rounding) ...
    _, _, samples, _ = scene_case(H, W, 1, K)
    rc, fit = _fundamental(zero, samples)
    assert rc == 0 and 0 <= fit["best"] < K and np.isfinite(fit["medians"]).all() and (fit["medians"] >= 0).all()
    assert np.abs(fit["F"].reshape(3, 3) + fit["F"].reshape(3, 3).T).max() < 1e-6
    # ... every hypothesis degenerate: nothing known, or every sample broken
    nothing = np.full((H, W, 2), np.nan, np.float32)
    repeated = samples.copy()
    repeated[:, 1] = repeated[:, 0]
    for flow, smp in ((nothing, samples), (zero, repeated), (zero, np.full((K, 8), H * W, np.int32))):
        rc, fit = _fundamental(flow, smp)
        assert rc == 0 and fit["best"] == -1 and not fit["F"].any() and not fit["F_all"].any()
        assert np.isposinf(fit["medians"]).all()
    rc, got = _mask(nothing, skew)
    assert rc == 0 and not any(a.any() for a in got.values())


# ------------------------------------------------------------------------------------------- 5b: the smallest images, the rank
def _tiny_case(H, W, seed, unknown=()):
    flow = np.random.default_rng(seed).uniform(-1.5, 1.5, (H, W, 2)).astype(np.float32)
    flow.reshape(-1, 2)[list(unknown), 0] = np.inf
    return flow, np.setdiff1d(np.arange(H * W), unknown).astype(np.int32)


def _check_tiny(flow, samples, got):
    """the median's rank comes from the count the selection's first pass finds: (8 - 1) // 2 of the eight known pixels"""
    assert got["best"] == 0 and np.isfinite(got["F_all"][0]).all() and got["F_all"][0].any()
    want = R.median_of(flow, got["F_all"][0])
    print(f"tiny {flow.shape[0]}x{flow.shape[1]}: median {got['medians'][0]:.3e}, the restatement's {want:.3e}")
    assert got["medians"][0] == want
    np.testing.assert_array_equal(got["F"], got["F_all"][0])
    rc, again = _fundamental(flow, samples)
    assert rc == 0 and again["best"] == 0
    for name in ("F_all", "medians", "F"):
        assert again[name].tobytes() == got[name].tobytes(), name


def test_eight_pixels_one_hypothesis():
    for seed in (0, 1, 2):
        flow, known = _tiny_case(2, 4, seed)
        assert known.tolist() == list(range(8))
        rc, got = _fundamental(flow, known[None])
        assert rc == 0
        _check_tiny(flow, known[None], got)


def test_eight_known_of_twelve_and_a_degenerate_hypothesis():
    for seed in (0, 1, 2):
        flow, known = _tiny_case(3, 4, seed, unknown=(1, 5, 6, 10))
        assert known.size == 8
        samples = np.stack([known, known])
        samples[1, 0] = 1                                        # an unknown pixel: degenerate
        rc, got = _fundamental(flow, samples)
        assert rc == 0
        assert np.isposinf(got["medians"][1]) and not got["F_all"][1].any()
        _check_tiny(flow, samples, got)


# ----------------------------------------------------------------------------------------------------------- 6: repeatability
def test_two_calls_are_bit_identical():
    flow, known, samples, broken = _holes_case()
    for det in (False, True):
        prev = torch.are_deterministic_algorithms_enabled()
        torch.use_deterministic_algorithms(det)
        try:
            a, b = _fundamental(flow, samples), _fundamental(flow, samples)
            ma, mb = _mask(flow, a[1]["F"]), _mask(flow, b[1]["F"])
        finally:
            torch.use_deterministic_algorithms(prev)
        assert a[0] == 0 and b[0] == 0 and ma[0] == 0 and mb[0] == 0 and a[1]["best"] == b[1]["best"]
        for name in ("F_all", "medians", "F"):
            assert a[1][name].tobytes() == b[1][name].tobytes(), name
        for name in ma[1]:
            assert ma[1][name].tobytes() == mb[1][name].tobytes(), name


def test_argument_errors():
    flow, disc, samples, ref = scene_case(40, 56, 0, K)
    for bad in (np.zeros((1, 40, 2), np.float32), np.zeros((40, 1, 2), np.float32), np.zeros((2, 3, 2), np.float32)):
        rc, got = _fundamental(bad, samples, ws_bytes=1 << 20)
        assert rc == -1 and got["best"] == GARBAGE_I32 and (got["F"] == GARBAGE_F64).all()
        rc, m = _mask(bad, ref["F"], ws_bytes=1 << 20)
        assert rc == -1 and all((a == (GARBAGE_U8 if a.dtype == np.uint8 else np.float32(-7.5e30))).all() for a in m.values())
    rc, got = _fundamental(flow, np.zeros((0, 8), np.int32), ws_bytes=1 << 20)
    assert rc == -1 and got["best"] == GARBAGE_I32
    for thr in (np.nan, np.inf, -np.inf):
        rc, m = _mask(flow, ref["F"], threshold=thr)
        assert rc == -1 and (m["mask"] == GARBAGE_U8).all()
    from gflow_amd import _lib as L
    need = L.load().gfl_epi_workspace_bytes(56, 40, K)
    rc, got = _fundamental(flow, samples, ws_bytes=need - 256)
    assert rc == -2 and got["best"] == GARBAGE_I32
    rc, m = _mask(flow, ref["F"], ws_bytes=L.load().gfl_epi_workspace_bytes(56, 40, 1) - 256)
    assert rc == -2 and (m["mask"] == GARBAGE_U8).all()


# ------------------------------------------------------------------------------------------------------------ 7, 8: end to end
def test_epipolar_move_mask_covers_the_disc():
    from gflow_amd import move_seg as MS
    flow, disc, samples, ref = scene_case(40, 56, 0, 512)
    out = MS.epipolar_move_mask(torch.tensor(flow))
    assert all(t.is_cuda for t in out.values())
    assert out["F"].shape == (3, 3) and out["F"].dtype == torch.float64 and out["err_norm"].dtype == torch.float32
    for k in ("mask", "open", "erode", "dilate"):
        assert out[k].shape == (40, 56) and out[k].dtype == torch.uint8
    opened = out["open"].cpu().numpy()
    print(f"end to end: IoU {iou(opened, disc):.4f} (the restatement's: {iou(ref['open'], disc):.4f}), best {int(out['best'])}")
    assert iou(opened, disc) >= 0.9
    # the default sampler is draw_samples(known, 512, 0): the same call with the samples given, and the median is best's
    again = MS.epipolar_move_mask(torch.tensor(flow, device=DEV), samples=samples)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    assert _rel(float(out["median"]), R.median_of(flow, out["F"].cpu().numpy())) <= MEDIAN_REL
    other = MS.epipolar_move_mask(torch.tensor(flow), hypotheses=64, seed=3, threshold=0.02)
    assert int(other["best"]) >= 0 and not torch.equal(other["F"], out["F"])


def test_clip_fit_with_computed_masks():
    from gflow_amd import move_seg as MS
    from gflow_amd.fit_video import fit_clip
    from tests.score_fit import FIT, H, W, clip
    frames = clip(n_frames=3)
    given = [torch.as_tensor(fr["move_mask"]).clone() for fr in frames]
    MS.clip_move_masks(frames, hypotheses=K)
    for fr, g in zip(frames, given):
        mm = fr["move_mask"]
        assert mm.dtype == torch.bool and tuple(mm.shape) == (H, W) and mm.device == torch.as_tensor(fr["image"]).device
        assert tuple(g.shape) == (H, W)
    assert not frames[-1]["move_mask"].any()                     # no forward flow: zeros, as load_sequence leaves it
    out = fit_clip(frames, DEV, FIT, seed=0, deterministic=True, segment=True)
    seg = out["segmentation"]
    assert seg["masks"].shape == (3, H, W)
    for k in ("J", "F", "JF"):
        assert seg[k].shape == (3,) and np.isfinite(seg[k]).all(), k
    assert np.isfinite(out["psnr_sum"])


def test_sequence_masks_from_the_loader_and_the_cli(tmp_path):
    import os
    from PIL import Image
    from gflow_amd import io as gio
    from gflow_amd import move_seg as MS
    from gflow_amd import synthetic as S
    sp = gio.write_sequence(S.make_clip(4, 24, 32, seed=0), str(tmp_path / "seq"))
    from_files = gio.load_sequence(sp)
    frames = gio.load_sequence(sp, move_masks="epipolar")
    assert len(frames) == len(from_files) == 3
    # (the reference's file lists drop the last image: each of the three loaded frames has a flow file)
    for fr in frames:
        assert fr["move_mask"].dtype == torch.bool and not fr["move_mask"].is_cuda
        assert torch.equal(fr["move_mask"], MS.epipolar_move_mask(fr["flow"])["open"].cpu() != 0)
    assert not MS.clip_move_masks(gio.load_sequence(sp))[-1]["move_mask"].any()    # a clip's last frame: zeros
    for a, b in zip(frames, from_files):                         # nothing else differs
        assert torch.equal(a["flow"], b["flow"]) and torch.equal(a["image"], b["image"])
    # the CLI overwrites the folder's _open.png and adds the other three, for every forward flow of the sequence
    assert MS.main(["--img_dir", sp + "/"]) == 0
    names = [os.path.splitext(os.path.basename(p))[0] for p in gio.sequence_paths(sp)["img"]]
    flows = gio.sequence_paths(sp)["flow"]
    assert len(names) == len(flows) == 3
    for name, fp in zip(names, flows):
        want = MS.result_images(MS.epipolar_move_mask(gio.read_flow(fp)))
        for k in MS.SUFFIXES:
            png = np.asarray(Image.open(os.path.join(sp + "_epipolar", f"{name}_{k}.png")))
            np.testing.assert_array_equal(png, want[k], err_msg=f"{name}_{k}")
    assert sorted(os.listdir(sp + "_epipolar")) == sorted([f"{n}_{k}.png" for n in names for k in MS.SUFFIXES] + ["00003_open.png"])
