"""GPU: depth and camera from the flows (csrc/gfl_sfm.hip, gflow_amd/sfm.py) against the float64 restatement
(tests/sfm_ref.py) on the analytic scenes of tests/test_sfm_host.py.

What is compared, and how the bounds were obtained:
  inlier bytes, counts, votes, flags   exactly.  Every input is first checked: the restatement's Sampson error lies at no pixel
                       within a relative 1e-9 of its inlier threshold (the float64 differences below are far smaller).
  F, R, t, parallax, the poses' rotations   float64 on both sides, but cyclic Jacobi and fixed-order partial sums here,
                       LAPACK and numpy's sums there.  Measured on an MI355X on exactly these inputs (the largest over all
                       cases, printed by every test): F 6.71e-12, R 4.09e-13, t 1.54e-11, parallax 8.50e-12 px, the
                       rotations of the chained poses 6.44e-14.  The bounds are 16 x those figures.
  rho, weight          evaluated in float64 and stored as float32: 2 x 2^-24 x max |v| (the rounding of the store, and as much
                       again for the float64 difference behind it, amplified by 1 / sin of the parallax angle <= 1e3 here).
  depth                float32 fusion, pull-push and sweeps; each value is a convex combination of earlier ones, so n
                       operations cost n x 2^-24 x max |rho| in rho = 1 / depth; n is counted from the kernels (below).
  medians              the device's float32 quotients are IEEE: equal to numpy's float32, bit for bit.

The motions, cameras and sizes of sfm_ref.CASES (every winner of the cheirality vote, fx != fy with the principal point off
the centre, 0.3 px of flow noise so that the threshold is K2 x median and a scattered subset is left out, a motion too
small for any parallax, the epipole inside the image; 8 x 8, 33 x 47, 64 x 65 = two workgroups of 4096 pixels a pair, the
second with 64, and 91 x 91 = three).  What a case is there for is asserted on the restatement before the device is compared
(sfm_ref.check_case; tests/test_sfm_host.py does the same without a device).  Their float64 bounds are NOT fitted to the
device: each is the constant above or 16 x what the restatement's own sensitivity probe gives for the case (sfm_ref.sensitivity:
the entries of the normalised A^T A perturbed by a relative 2^-50, 8 repeats), whichever is larger.  The largest figures, the
probe's from the device's starting matrices, the device's measured on an MI355X (both printed by every test):

                               probe                                      device
                       F         R         t         parallax     F         R         t         parallax
  8 x 8, exact flows   5.72e-09  2.55e-10  1.19e-08  1.56e-10     1.27e-09  5.76e-11  2.68e-09  5.31e-11
  small (F, R kept)    1.29e-09  1.74e-12  -         6.12e-11     1.31e-10  1.71e-13  -         8.68e-12
  noisy                2.93e-12  1.66e-13  4.66e-12  8.81e-12     2.06e-12  8.80e-14  3.56e-12  4.72e-12
  every other case     2.78e-11  8.68e-13  2.52e-11  4.84e-11     4.46e-11  5.72e-13  2.39e-11  3.40e-11
  chained rotations, 64 x 65 clip        2.63e-13 (the two pairs' sum)              1.07e-13

(8 x 8 has 64 correspondences and a parallax of 0.2 px: A^T A's smallest eigenvalues lie 1e3 x closer together than at
33 x 47, and the probe says so.)  The device's figure exceeds the probe's own in six cases, all at 33 x 47, by 1.9 x at the
most (F of fwd-33x47-centred, 1.63e-11 against 8.68e-12): a random perturbation is no worst-case ordering, which the factor 16
is for; no case comes nearer than a factor of 8 to its bound.

Near the epipole (forward and backward motion) sin^2 of the parallax angle falls below 1e-6 and the 1 / sin <= 1e3 behind the
rho bound no longer holds: those pixels -- their number is capped on the restatement, max(1, 0.005 H W) -- are left out of the
rho comparison and have to be finite with a weight under 2e-6.  Where the epipole is a pixel's centre (forward motion, centred
camera) that one pixel's bearings are parallel up to the error of R (sin^2 1e-17 .. 1e-21): the sign of its depths is the
rounding's on either side, so its vote and its weight are not compared; every other vote is (sfm_ref.UNDECIDED_W).
Pure rotation with a flow that is not zero stays uncompared: its F is not unique.
"""
import os
import shutil

import numpy as np
import pytest
import torch

from gflow_amd import sfm
from tests import sfm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = 2.0 ** -24
F_BOUND, R_BOUND, T_BOUND, PAR_BOUND = 16 * 6.71e-12, 16 * 4.09e-13, 16 * 1.54e-11, 16 * 8.50e-12
CHAIN_BOUND = 16 * 6.44e-14


def scene(H, W, kind="plain"):
    """(flow, intr, exclude) of the analytic scene scaled to H x W"""
    sc = R.make_scene(H, W, f=40.0 * max(H, W) / 48.0)
    flow, exclude = sc["flow"], None
    if kind in ("block", "excluded"):
        flow, block = R.add_block(flow, H // 4, W // 4, min(H, W) // 3)
        if kind == "excluded":                                     # the block and a stripe of good pixels
            exclude = block.astype(np.uint8) * 7
            exclude[:, -3:] = 1
    if kind == "inf":
        flow = flow.copy()
        flow[1::5, 2::7, 0] = np.inf
        flow[3::6, 1::4, 1] = -np.inf
        flow[0, 0] = np.nan
    if kind == "zero":
        flow = np.zeros_like(flow)
    return flow, sc["intr"], exclude


def device_two_view(flows, intr, exclude=None, F_init=None, **kw):
    flows = torch.from_numpy(np.asarray(flows)).to(DEV)
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude)).to(DEV)
    if F_init is None:
        F_init = sfm.initial_F(flows.reshape((-1,) + tuple(flows.shape[-3:])), None if ex is None else ex.reshape(-1, *ex.shape[-2:]))
    out = sfm.two_view(flows, intr, ex, F_init=F_init, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, F_init.cpu().numpy()


def probe_bounds(probe):
    """the float64 bounds (F, R, t, parallax) of a new case: the constant measured on the first inputs, or 16 x what the
    restatement's own sensitivity probe gives for the case, whichever is larger"""
    print("   probe: " + " ".join(f"{k} {v:.2e}" for k, v in probe.items()))
    return tuple(max(c, 16 * probe[k]) for c, k in ((F_BOUND, "F"), (R_BOUND, "R"), (T_BOUND, "t"), (PAR_BOUND, "parallax")))


def compare_pair(tag, dev, ref, bounds=None, left_out=None, undecided=None, votes_decided=None, by_parallax=False):
    """one pair's device result against the restatement's.  ``bounds``: (F, R, t, parallax), the constants by default.
    ``left_out`` (H, W) bool: pixels so near the epipole that rho is not compared (finite, and next to no weight, is asked
    there).  ``undecided``: the pixel whose depths have no pinned sign (sfm_ref.UNDECIDED_W); ``votes_decided``: the
    restatement's votes without it.  ``by_parallax``: the pair is degenerate by its parallax alone: F, R, the votes and the
    parallax are compared all the same."""
    bF, bR, bt, bp = (F_BOUND, R_BOUND, T_BOUND, PAR_BOUND) if bounds is None else bounds
    no = np.zeros(ref["inlier"].shape, dtype=bool)
    left_out, undecided = (no if left_out is None else left_out), (no if undecided is None else undecided)
    assert R.threshold_margin(ref) > 1e-9, (tag, R.threshold_margin(ref))
    assert np.array_equal(dev["inlier"], ref["inlier"]), tag
    assert tuple(dev["counts"]) == tuple(ref["counts"]), tag
    assert bool(dev["degenerate"]) == bool(ref["degenerate"]), tag
    for k in ("F", "R", "t", "rho", "weight", "parallax"):
        assert np.isfinite(dev[k]).all(), (tag, k)
    if not ref["degenerate"] or by_parallax:
        if undecided.any():
            extra = dev["votes"] - votes_decided
            print(f"{tag}: votes {dev['votes']}, the restatement's {ref['votes']}, without the undecided pixel {votes_decided}")
            assert (extra >= 0).all() and (extra <= undecided.sum()).all() and np.argmax(dev["votes"]) == np.argmax(ref["votes"]), tag
        else:
            assert np.array_equal(dev["votes"], ref["votes"]), tag
        dF = np.abs(R.normalise_F(dev["F"]) - R.normalise_F(ref["F"])).max()
        dR, dt = np.abs(dev["R"] - ref["R"]).max(), np.abs(dev["t"] - ref["t"]).max()
        dp = abs(dev["parallax"] - ref["parallax"])
        print(f"{tag}: F {dF:.2e} R {dR:.2e} t {dt:.2e} parallax {dp:.2e}")
        assert dF <= bF and dR <= bR and dt <= bt and dp <= bp, tag
        assert abs(np.linalg.norm(dev["F"]) - 1.0) < 1e-12 and dev["F"].reshape(-1)[np.argmax(np.abs(dev["F"]))] > 0
    if ref["degenerate"]:
        assert not dev["t"].any() and not dev["rho"].any() and not dev["weight"].any(), tag
    assert np.array_equal((dev["weight"] > 0)[~undecided], (ref["weight"] > 0)[~undecided]), tag
    keep = ~left_out
    for k in ("rho", "weight"):
        err, bound = np.abs(dev[k] - ref[k])[keep].max(), 2 * EPS32 * np.abs(ref[k][keep]).max()
        print(f"{tag}: {k} err {err:.2e} bound {bound:.2e}" + (f" ({left_out.sum()} pixels left out)" if left_out.any() else ""))
        assert err <= bound, (tag, k)
    assert (dev["weight"][left_out] < 2e-6).all(), tag              # (finite: asserted above)


def kind_against_the_restatement(H, W, kind, probe=False):
    flow, intr, exclude = scene(H, W, kind)
    dev, F0 = device_two_view(flow, intr, exclude)
    ref = R.two_view(flow, intr, F0[0], exclude)
    compare_pair(f"{H}x{W} {kind}", dev, ref, probe_bounds(R.sensitivity(flow, intr, F0[0], exclude)) if probe else None)
    assert not ref["degenerate"] and ref["counts"][1] >= 0.5 * H * W
    if kind == "inf":
        known = np.isfinite(flow).all(-1)
        assert ref["counts"][0] == known.sum() < H * W and not dev["inlier"][~known].any()
    if kind == "excluded":
        assert not dev["inlier"][exclude != 0].any() and ref["counts"][0] == (exclude == 0).sum()
    if kind == "block":
        assert ref["counts"][1] < H * W


@pytest.mark.parametrize("H,W", [(16, 24), (33, 47)])
@pytest.mark.parametrize("kind", ["plain", "block", "excluded", "inf"])
def test_two_view_against_the_restatement(H, W, kind):
    kind_against_the_restatement(H, W, kind)


@pytest.mark.parametrize("kind", ["excluded", "inf"])
def test_excluded_and_unknown_pixels_over_two_workgroups(kind):
    """64 x 65 = 4096 + 64 pixels: the excluded block and stripe, and the unknown pixels, fall into both workgroups' shares"""
    kind_against_the_restatement(64, 65, kind, probe=True)


def case_against_the_restatement(case, dev, F0, **kw):
    """the device's result of one case of sfm_ref.CASES against the restatement from the same starting matrix, after the
    restatement itself was held to reach what the case is there for (sfm_ref.check_case)"""
    sc, tag = R.case_scene(case), R.case_id(case)
    kw = dict(R.case_kw(case), **kw)
    with np.errstate(all="ignore"):
        ref = R.two_view(sc["flow"], sc["intr"], F0, **kw)
        probe = R.sensitivity(sc["flow"], sc["intr"], F0, **kw)
    info = R.check_case(case, sc["flow"], sc["intr"], ref)
    votes_decided = None
    if info["undecided"].any():
        with np.errstate(all="ignore"):
            votes_decided = R.pose(sc["flow"], ref["F"], ref["inlier"] * ~info["undecided"], ref["counts"], sc["intr"])["votes"]
    print(f"{tag}: chunks {-(-case[1] * case[2] // R.PER_WORKGROUP)} votes {ref['votes']} thr {ref['thr']:.4f} counts {ref['counts']} "
          f"parallax {ref['parallax']:.3f} degenerate {ref['degenerate']}")
    compare_pair(tag, dev, ref, probe_bounds(probe), info["left_out"], info["undecided"], votes_decided, by_parallax=case[0] == "small")
    return ref, info


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] != "fwd"], ids=R.case_id)
def test_two_view_over_motions_cameras_and_sizes(case):
    """every winner of the cheirality vote, fx != fy with the principal point off the centre, a threshold above its floor
    with a scattered subset of inliers, a pair that is degenerate by its parallax alone; one, two and three workgroups a pair"""
    sc = R.case_scene(case)
    dev, F0 = device_two_view(sc["flow"], sc["intr"], **R.case_kw(case))
    case_against_the_restatement(case, dev, F0[0])


@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] == "fwd"], ids=R.case_id)
def test_the_epipole_inside_the_image(case):
    """forward motion: |a x b|^2 -> 0 at the principal point, where sfm_depths divides by it.  rho is compared wherever
    sin^2 >= 1e-6; nearer the epipole it has to be finite and carry next to no weight, and those pixels are few (asserted
    on the restatement before anything is compared).  With the centred camera the epipole is a pixel's centre."""
    sc = R.case_scene(case)
    dev, F0 = device_two_view(sc["flow"], sc["intr"])
    ref, info = case_against_the_restatement(case, dev, F0[0])
    H, W = case[1:3]
    assert 1 <= info["left_out"].sum() <= R.epipole_cap(H, W)
    if case[3] == "centred":
        cx, cy = int(sc["intr"][2]), int(sc["intr"][3])
        assert info["left_out"][cy, cx] and not sc["flow"][cy, cx].any() and ref["inlier"][cy, cx]
        assert info["undecided"].sum() == 1 and info["undecided"][cy, cx]


def test_a_batch_with_every_winner():
    """64 x 65 under the general camera, P = 6: four motions with the four winners, the small motion (degenerate under
    min_parallax = 0.2 px) and the noisy flow in one call -- cand + 21 p, votes + 4 p and the pairs' rows of partial, sums and
    prefix, two workgroups a pair"""
    H, W = 64, 65
    motions = ("base", "neg-x", "roll", "roll-neg", "small", "noisy")
    cases = [(m, H, W, "general") for m in motions]
    scenes = [R.case_scene(c) for c in cases]
    flows, intr = np.stack([s["flow"] for s in scenes]), scenes[0]["intr"]
    assert all(s["intr"] == intr for s in scenes) and intr[0] != intr[1]
    dev, F0 = device_two_view(flows, intr, min_parallax=0.2)
    assert [int(np.argmax(v)) for v in dev["votes"]] == [0, 1, 2, 3, 0, 0]
    assert list(dev["degenerate"]) == [False, False, False, False, True, False]
    for p, case in enumerate(cases):
        single, _ = device_two_view(flows[p], intr, F_init=torch.from_numpy(F0[p:p + 1]).to(DEV), min_parallax=0.2)
        for k in dev:
            assert np.array_equal(dev[k][p], single[k], equal_nan=True), (motions[p], k)
        ref, _ = case_against_the_restatement(case, {k: v[p] for k, v in dev.items()}, F0[p], min_parallax=0.2)
        assert int(np.argmax(ref["votes"])) == [0, 1, 2, 3, 0, 0][p] and ref["degenerate"] == (motions[p] == "small")


def test_a_batch_equals_its_single_calls():
    """36 x 48, P = 4: the scene, the moving block, a zero flow (degenerate) and unknown pixels in one call"""
    H, W = 36, 48
    cases = [scene(H, W, k) for k in ("plain", "block", "zero", "inf")]
    flows, intr = np.stack([c[0] for c in cases]), cases[0][1]
    dev, F0 = device_two_view(flows, intr)
    again, _ = device_two_view(flows, intr, F_init=torch.from_numpy(F0).to(DEV))
    for k in dev:
        assert np.array_equal(dev[k], again[k], equal_nan=True), k   # two calls: the same bits
    assert list(dev["degenerate"]) == [False, False, True, False]
    for p, kind in enumerate(("plain", "block", "zero", "inf")):
        single, _ = device_two_view(flows[p], intr, F_init=torch.from_numpy(F0[p:p + 1]).to(DEV))
        for k in dev:
            assert np.array_equal(dev[k][p], single[k], equal_nan=True), (kind, k)
        with np.errstate(all="ignore"):
            ref = R.two_view(flows[p], intr, F0[p])
        compare_pair(f"batch {kind}", {k: v[p] for k, v in dev.items()}, ref)


def fill_ops(H, W, sweeps):
    """the float32 operations behind one output of stage e: fusion 8, per pyramid level a pull (11) and a push (12), 9 per
    sweep, 2 for lambda and 2 for the rounding of the inputs"""
    levels = int(np.ceil(np.log2(max(H, W)))) + 1
    return 8 + 23 * levels + 9 * sweeps + 4


def device_fill(rho0, w, lam, sweeps, rho_min=1e-6, fused=True):
    from gflow_amd import _lib as L
    lib = L.load()
    T, H, W = rho0.shape
    r, ww = torch.from_numpy(rho0).to(DEV), torch.from_numpy(w).to(DEV)
    lm = torch.tensor(lam, dtype=torch.float64, device=DEV)
    depth = torch.empty_like(r)
    ws = L.scratch(lib.gfl_sfm_workspace_bytes(T, H, W), DEV)
    before = os.environ.get("GFL_SFM_FUSED")
    os.environ["GFL_SFM_FUSED"] = "1" if fused else "0"
    try:
        L.check(lib.gfl_sfm_fill(L.ptr(r), L.ptr(ww), L.ptr(lm), T, H, W, sweeps, rho_min, L.ptr(depth), L.ptr(ws), ws.numel(),
                                 L.stream()), "sfm fill")
        torch.cuda.synchronize()
    finally:
        if before is None:
            del os.environ["GFL_SFM_FUSED"]
        else:
            os.environ["GFL_SFM_FUSED"] = before
    return depth.cpu().numpy()


@pytest.mark.parametrize("H,W", [(16, 24), (33, 47), (57, 70), (64, 65)])
def test_fill_against_the_restatement(H, W):
    """pull-push and sweeps on random inverse depths with holes: one tile, odd sizes with partial tiles and odd pyramid
    levels, several tiles; sweep counts around the four of a fused launch.  64 x 65: more than the 4096 pixels of a
    workgroup's share (gfl_sfm_fill itself walks pixels, not shares: test_fusion_over_several_workgroups holds the kernel
    that chunks)"""
    rng = np.random.default_rng(H * W)
    T = 3
    rho0 = rng.uniform(0.2, 1.0, (T, H, W)).astype(np.float32)
    w = rng.uniform(0.01, 1.0, (T, H, W)).astype(np.float32)
    w[0, 2:9, 3:11] = 0                                            # a hole
    w[1, :, W // 2:] = 0                                           # half the frame, up to two edges
    w[1, H // 2:, :] = 0
    w[2] = 0                                                       # nothing at all ...
    w[2, H - 1, W - 1] = 0.5                                       # ... but one corner pixel
    lam = [0.05, 0.3, 0.02]
    for sweeps in (0, 1, 3, 4, 5, 20):
        got = device_fill(rho0, w, lam, sweeps)
        assert np.array_equal(got, device_fill(rho0, w, lam, sweeps, fused=False)), sweeps    # the bits of plain sweeps
        n = fill_ops(H, W, sweeps)
        for t in range(T):
            ref = R.fill(rho0[t].astype(np.float64), w[t].astype(np.float64), lam[t], sweeps)[1]
            err, bound = np.abs(1.0 / got[t].astype(np.float64) - ref).max(), n * EPS32 * np.abs(ref).max()
            assert err <= bound, (sweeps, t, err, bound)
            assert np.abs(got[t] - 1.0 / ref).max() <= n * EPS32 * (ref.max() / ref.min()) * (1.0 / ref).max()
    one = 1.0 / rho0[2, H - 1, W - 1]                                                      # one pixel fills its frame
    assert np.abs(device_fill(rho0, w, lam, 7)[2] - one).max() <= fill_ops(H, W, 7) * EPS32 * one
    full = rng.uniform(0.01, 1.0, (T, H, W)).astype(np.float32)
    assert np.array_equal(device_fill(rho0, full, [0.0] * T, 5), 1.0 / rho0)               # weighted, lambda = 0: the identity
    assert np.all(device_fill(rho0, np.zeros_like(w), lam, 3) == np.float32(1) / np.float32(1e-6))                  # no weight: rho = 0, clamped by rho_min


@pytest.mark.parametrize("H,W", [(33, 47), (64, 65), (91, 91)])
def test_fusion_over_several_workgroups(H, W):
    """sfm_fuse_kernel, a workgroup per 4096 pixels and frame: float32 with every product and sum rounded on its own, so
    numpy's float32 gives the same bits; the count of pixels with weight comes from the medians' first histogram"""
    rng = np.random.default_rng(H)
    T = 3
    rf, rb = (rng.uniform(0.2, 1.0, (T, H, W)).astype(np.float32) for _ in range(2))
    wf, wb = (rng.uniform(0.0, 1.0, (T, H, W)).astype(np.float32) for _ in range(2))
    wf[0].reshape(-1)[-64:] = 0                                    # the last 64 pixels: the backward side alone ...
    wb[1].reshape(-1)[:-64] = 0
    wf[1].reshape(-1)[:-64] = 0                                    # ... or the only ones with any weight
    wb[2] = 0
    wf[2, ::2] = 0
    sf, sb = np.array([1.0, 0.7, 1.3]), np.array([0.9, 1.0, 1.1])
    up = lambda x: torch.from_numpy(x).to(DEV)
    res = sfm.fuse_fill(up(rf), up(wf), up(rb), up(wb), up(sf), up(sb), sweeps=0)
    s0, s1 = sf.astype(np.float32)[:, None, None], sb.astype(np.float32)[:, None, None]
    w = wf + wb
    with np.errstate(all="ignore"):
        rho = np.where(w > 0, (wf * (rf * s0) + wb * (rb * s1)) / w, np.float32(0))
    assert rho.dtype == np.float32 and (w[1] > 0).sum() == 64 and (w[2] > 0).sum() < H * W
    assert np.array_equal(res["weight"].cpu().numpy(), w) and np.array_equal(res["rho0"].cpu().numpy(), rho)
    assert np.array_equal(res["pixels"].cpu().numpy(), (w > 0).sum((1, 2)))
    ref = R.fuse(*(x.astype(np.float64) for x in (rf, wf, rb, wb)), s0.astype(np.float64), s1.astype(np.float64))[0]
    assert np.abs(rho - ref).max() <= 8 * EPS32 * np.abs(ref).max()      # (fill_ops: the fusion's 8 operations)


def medians_are_exact(M, H, W):
    """rows 0 - 4: the five kinds; a sixth row (M = 6) has all its finite values in the image's last 64 pixels -- at 64 x 65
    the share of the second, partial workgroup, which then decides the selection alone"""
    rng = np.random.default_rng(5)
    a = rng.normal(size=(M, H, W)).astype(np.float32)
    b = rng.uniform(0.5, 2.0, (M, H, W)).astype(np.float32)
    wa, wb = (rng.uniform(0, 1, (M, H, W)).astype(np.float32) for _ in range(2))
    a[0] = np.round(a[0] * 2) / 2                                  # many ties
    b[0] = 1.0
    a[1, ::3] = np.nan                                             # quotients that are not finite are left out
    b[1, 1::3] = 0.0
    wa[2] = 0.0                                                    # a row without values
    a[3] = np.abs(a[3]) * 1e-30                                    # tiny and huge magnitudes, both signs
    a[4] *= 1e30
    if M > 5:
        a[5].reshape(-1)[:-64] = np.nan
        wa[5].reshape(-1)[-64:], wb[5].reshape(-1)[-64:] = 1.0, 1.0
    up = lambda x: None if x is None else torch.from_numpy(x).to(DEV)
    for (bb, waa, wbb, w_min) in ((b, wa, wb, 0.3), (None, wa, None, 0.0), (b, None, None, 0.0), (None, None, wb, 0.9)):
        med, cnt = sfm.masked_median(up(a), up(bb), up(waa), up(wbb), w_min)
        med, cnt = med.cpu().numpy(), cnt.cpu().numpy()
        for m in range(M):
            with np.errstate(all="ignore"):
                q = a[m] if bb is None else a[m] / bb[m]           # float32, as the device divides
            ok = np.isfinite(q)
            for w in (waa, wbb):
                if w is not None:
                    ok &= w[m] > np.float32(w_min)
            want, n = R.lower_median(np.where(ok, q, np.nan))
            assert cnt[m] == n and (np.isnan(med[m]) if n == 0 else med[m] == want), (H, W, m, w_min)
            assert m != 5 or n == 64, (H, W, w_min)


def test_medians_are_exact():
    medians_are_exact(5, 33, 47)
    for (H, W) in ((64, 65), (91, 91)):                            # two and three workgroups a row
        assert -(-H * W // R.PER_WORKGROUP) == {64: 2, 91: 3}[H]
        medians_are_exact(6, H, W)


def device_clip(fwd, bwd, **kw):
    up = lambda x: None if x is None else torch.from_numpy(np.stack(x)).to(DEV)
    if bwd is None:                                                # the last frame has no pair at all
        with pytest.warns(UserWarning, match="frame"):
            res = sfm.clip_depth_camera(up(fwd), None, **kw)
    else:
        res = sfm.clip_depth_camera(up(fwd), up(bwd), **kw)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("H,W,both", [(36, 48, True), (33, 47, True), (33, 47, False), (64, 65, True)])
def test_clip_against_the_restatement(H, W, both):
    """three frames with baselines 0.08 and 0.12: ratios, baselines, chained poses and depth; with the forward flows alone
    every baseline comes from the medians (the path of a missing ratio).  64 x 65: two workgroups a pair and a frame, the
    principal point (W / 2 - 3.25, H / 2 + 2.5) given as pp= (one focal length: fx != fy stays with the two-view tests)"""
    wide = (H, W) == (64, 65)
    s3 = R.make_scene3(H, W, f=40.0 * max(H, W) / 48.0, pp=(W / 2 - 3.25, H / 2 + 2.5) if wide else None)
    fwd, bwd = s3["fwd"], (s3["bwd"] if both else None)
    flows = torch.from_numpy(np.stack(fwd + (bwd or []))).to(DEV)
    F0 = sfm.initial_F(flows)
    intr = s3["intr"]
    res = device_clip(fwd, bwd, focal=intr[0], pp=intr[2:], median_depth=2.0, F_init=F0)
    again = device_clip(fwd, bwd, focal=intr[0], pp=intr[2:], median_depth=2.0, F_init=F0)
    assert torch.equal(res["depth"], again["depth"]) and torch.equal(res["extr"], again["extr"])
    F0 = F0.cpu().numpy()
    ref = R.clip_depth_camera(fwd, bwd, intr, F_fwd=F0[:2], F_bwd=F0[2:] if both else None, median_depth=2.0)
    assert all(R.threshold_margin(p) > 1e-9 for p in ref["pairs_fwd"] + ref["pairs_bwd"])
    assert np.array_equal(res["degenerate"], ref["degenerate"]) and np.array_equal(res["unreliable"], ref["unreliable"])
    assert res["focal"] == intr[0] and list(res["pp"]) == list(intr[2:])
    count, ratio = res["count"].cpu().numpy(), res["ratio"].cpu().numpy()
    assert np.array_equal(count, ref["count"])
    if both:
        assert count[1] == H * W
        # the ratio is a float32 quotient of float32 inverse depths: three roundings
        assert abs(ratio[1] - ref["ratio"][1]) <= 3 * EPS32 * 1.5 and abs(ratio[1] - 1.5) < 1e-6
    base, extr = res["baseline"].cpu().numpy(), res["extr"].cpu().numpy()
    depth = res["depth"].cpu().numpy()
    assert np.array_equal(extr[0], np.eye(4)[:3]) and depth.dtype == np.float32 and np.isfinite(depth).all() and (depth > 0).all()
    # the ratio's and the scales' roundings on top; without ratios a baseline carries two medians of filled depth
    n = (fill_ops(H, W, 20) + 6) * (1 if both else 2)
    chain_bound = CHAIN_BOUND
    if wide:                                                       # a new input: the probe's figures of the chained pairs, added
        probes = [R.sensitivity(fwd[i], intr, F0[i])["R"] for i in range(2)]
        print(f"{H}x{W}: probe R {probes[0]:.2e} {probes[1]:.2e}")
        chain_bound = max(CHAIN_BOUND, 16 * sum(probes))
    r0 = 1.0 / ref["depth"][0]
    kappa = r0.max() / r0.min()                                    # rho's error seen in a depth: relative, times max / min
    # the baselines carry the float32 medians of depth; the poses' rotations are float64
    assert np.abs(base / ref["baseline"] - 1.0).max() <= n * EPS32 * kappa
    for i in range(3):
        dR = np.abs(extr[i][:, :3] - ref["extr"][i][:, :3]).max()
        print(f"{H}x{W} frame {i}: chained rotation {dR:.2e}")
        assert dR <= chain_bound
        assert np.abs(extr[i][:, 3] - ref["extr"][i][:, 3]).max() <= 2 * n * EPS32 * kappa * np.abs(ref["extr"][i][:, 3]).max() + 1e-15
        rr = 1.0 / ref["depth"][i]
        err = np.abs(1.0 / depth[i].astype(np.float64) - rr).max()
        print(f"{H}x{W} frame {i}: rho err {err:.2e} bound {2 * n * EPS32 * kappa * rr.max():.2e}")
        assert err <= 2 * n * EPS32 * kappa * rr.max()                 # (the frame's own operations and the global scale's)
    if both:
        s = base[0] / s3["baselines"][0]
        assert abs(base[1] / s - s3["baselines"][1]) < 1e-6 and np.abs(depth[1] / s - s3["depth"][1]).max() < 0.03
    else:
        assert res["unreliable"][2] and np.all(depth[2] == 2.0)


def test_invalid_arguments_are_refused_before_any_launch():
    from gflow_amd import _lib as L
    lib = L.load()
    H, W, P = 16, 24, 2
    flow = torch.zeros(P, H, W, 2, device=DEV)
    F = torch.zeros(P, 9, dtype=torch.float64, device=DEV)
    counts = torch.zeros(P, 2, dtype=torch.int32, device=DEV)
    med = torch.zeros(P, dtype=torch.float64, device=DEV)
    inl = torch.zeros(P, H, W, dtype=torch.uint8, device=DEV)
    Rm = torch.zeros(P, 9, dtype=torch.float64, device=DEV)
    t = torch.zeros(P, 3, dtype=torch.float64, device=DEV)
    votes = torch.zeros(P, 4, dtype=torch.int32, device=DEV)
    deg = torch.zeros(P, dtype=torch.int32, device=DEV)
    rho, wt, depth = (torch.zeros(P, H, W, device=DEV) for _ in range(3))
    ws = L.scratch(lib.gfl_sfm_workspace_bytes(P, H, W), DEV)
    p, n, s = L.ptr, ws.numel(), L.stream()
    INVALID, WORKSPACE = -1, lib.gfl_sfm_refit(p(flow), p(F), None, P, H, W, 2, 0.0625, p(F), p(counts), p(med), p(inl), p(ws), 16, s)
    assert WORKSPACE not in (0, INVALID)                           # a short workspace

    def refit(P_=P, H_=H, W_=W, flow_=flow, F_=F, rounds=2, floor=0.0625, ws_=ws):
        return lib.gfl_sfm_refit(p(flow_), p(F_), None, P_, H_, W_, rounds, floor, p(F_), p(counts), p(med), p(inl), p(ws_), n, s)

    def pose(P_=P, H_=H, W_=W, fx=20.0, cx=12.0, flow_=flow, par=0.1):
        return lib.gfl_sfm_pose(p(flow_), p(F), p(inl), p(counts), P_, H_, W_, fx, 20.0, cx, 8.0, par, 0.2, p(Rm), p(t), p(votes),
                                p(med), p(deg), p(ws), n, s)

    def tri(P_=P, H_=H, fx=20.0, rho_=rho):
        return lib.gfl_sfm_triangulate(p(flow), p(inl), p(Rm), p(t), p(deg), P_, H_, W, fx, 20.0, 12.0, 8.0, p(rho_), p(wt), s)

    assert refit() == 0 and pose() == 0 and tri() == 0
    assert lib.gfl_status_string(INVALID).decode().lower().count("invalid") == 1
    for rc in (refit(P_=0), refit(H_=7), refit(W_=7), refit(flow_=None), refit(F_=None), refit(ws_=None), refit(rounds=-1),
               refit(floor=float("nan")), pose(P_=0), pose(H_=7), pose(W_=7), pose(fx=float("inf")), pose(fx=float("nan")),
               pose(fx=0.0), pose(cx=float("nan")), pose(flow_=None), pose(par=float("nan")), tri(P_=0), tri(H_=7),
               tri(fx=float("inf")), tri(rho_=None)):
        assert rc == INVALID
    lam = torch.zeros(P, dtype=torch.float64, device=DEV)
    fill = lambda T_=P, W_=W, sweeps=3, rmin=1e-6, lam_=lam, nb=n: lib.gfl_sfm_fill(p(rho), p(wt), p(lam_), T_, H, W_, sweeps, rmin,
                                                                                p(depth), p(ws), nb, s)
    median = lambda M_=P, a_=rho, wmin=0.0, nb=n: lib.gfl_sfm_median(p(a_), None, None, None, wmin, M_, H, W, p(med), p(deg), p(ws),
                                                                     nb, s)
    wsum = torch.zeros_like(rho)
    fuse = lambda T_=P, a_=rho: lib.gfl_sfm_fuse(p(a_), p(wt), p(rho), p(wt), p(lam), p(lam), T_, H, W, p(depth), p(wsum), s)
    assert fill() == 0 and median() == 0 and fuse() == 0
    for rc in (fill(T_=0), fill(W_=7), fill(sweeps=-1), fill(rmin=0.0), fill(rmin=float("nan")), fill(lam_=None), median(M_=0),
               median(a_=None), median(wmin=-1.0), fuse(T_=0), fuse(a_=None)):
        assert rc == INVALID
    assert fill(nb=16) == WORKSPACE and median(nb=16) == WORKSPACE
    torch.cuda.synchronize()


def _same_frames(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert fa.keys() == fb.keys()
        for k in fa:
            if torch.is_tensor(fa[k]):
                assert fa[k].device == fb[k].device and torch.equal(fa[k], fb[k]), k
            else:
                assert fa[k] == fb[k], k


def test_a_sequence_without_depth_and_camera_files(tmp_path, capsys):
    """load_sequence(depth_camera="estimate") on a written clip whose depth and camera folders are gone, and a fit of it
    through fit_video --make-depth-camera: completion and finiteness only -- the quality of a fit from estimated depth is
    unmeasured (DESIGN.md records the figures of one run)"""
    from gflow_amd import fit_video
    from gflow_amd import io as gio
    from gflow_amd import synthetic as SY
    sp = gio.write_sequence(SY.make_clip(3, H=48, W=64), str(tmp_path / "seq"))
    for device in (None, DEV):                                     # the regression: "files" is what it was
        _same_frames(gio.load_sequence(sp, device=device), gio.load_sequence(sp, device=device, depth_camera="files"))
    with_files = {device: gio.load_sequence(sp, device=device) for device in (None, DEV)}
    args = ["--sequence", sp, "--num_points", "1000", "--iterations_first", "30", "--iterations_after", "30",
            "--iterations_camera", "30"]
    psnr_files = fit_video.main(args)["psnr_mean_db"]
    shutil.rmtree(sp + "_depth_mast3r_s2")
    shutil.rmtree(sp + "_camera_mast3r_s2")
    for device in (None, DEV):
        for resize in (None, 32):
            frames = gio.load_sequence(sp, resize=resize, device=device, depth_camera="estimate", depth_offset=0.25)
            assert len(frames) == len(with_files[device]) == 2
            for fr, ff in zip(frames, gio.load_sequence(sp, resize=resize, device=device, flows="files", depth_camera="estimate",
                                                       depth_offset=0.25)):
                assert torch.equal(fr["depth"], ff["depth"])       # the same bits on every call
            for fr, ff in zip(frames, with_files[device]):
                assert fr.keys() == ff.keys() and fr["depth"].dtype == torch.float32 and fr["extr"].dtype == torch.float32
                assert fr["depth"].shape == fr["image"].shape[:2] + (1,) and fr["extr"].shape == (3, 4)
                assert fr["depth"].is_cuda == (device is not None) and not fr["extr"].is_cuda
                assert torch.isfinite(fr["depth"]).all() and (fr["depth"] > 0.25).all() and torch.isfinite(fr["extr"]).all()
                assert fr["focal"] == 64.0 and fr["pp"] == [32, 24]
            assert torch.equal(frames[0]["extr"], torch.eye(4)[:3])
    assert gio.load_sequence(sp, depth_camera="estimate", focal=50.0)[0]["focal"] == 50.0
    with pytest.raises(ValueError, match="skip_interval"):
        gio.load_sequence(sp, depth_camera="estimate", skip_interval=2)
    out = fit_video.main(args + ["--make-depth-camera"])
    capsys.readouterr()
    with capsys.disabled():
        print(f"psnr with the true files {psnr_files:.2f} dB, with the estimate {out['psnr_mean_db']:.2f} dB")
    assert out["frames"] == 2 and np.isfinite(out["psnr_mean_db"])
    assert sorted(os.listdir(tmp_path)) == ["seq", "seq_epipolar", "seq_flow_unimatch"]          # nothing was written


def test_command_line_writes_what_the_loader_reads(tmp_path):
    from gflow_amd import io as gio
    from gflow_amd import optflow
    from gflow_amd import synthetic as SY
    sp = gio.write_sequence(SY.make_clip(3, H=48, W=64), str(tmp_path / "seq"))
    shutil.rmtree(sp + "_depth_mast3r_s2")
    shutil.rmtree(sp + "_camera_mast3r_s2")
    with pytest.raises(SystemExit, match="backward"):
        sfm.main(["--img_dir", sp])                                # the written clip has no backward flows
    assert optflow.main(["--img_dir", sp, "--overwrite"]) == 0
    assert sfm.main(["--img_dir", sp, "--focal", "70"]) == 0
    names = [f"{i:05d}" for i in range(3)]
    assert sorted(os.listdir(sp + "_depth_mast3r_s2")) == [n + ".npy" for n in names]
    assert sorted(os.listdir(sp + "_camera_mast3r_s2")) == [n + ".json" for n in names]
    with pytest.raises(SystemExit, match="overwrite"):
        sfm.main(["--img_dir", sp])
    frames = gio.load_sequence(sp, frame_range=3)
    assert len(frames) == 3 and all(fr["focal"] == 70.0 and fr["pp"] == [32, 24] for fr in frames)
    assert torch.equal(frames[0]["extr"], torch.eye(4)[:3]) and all(torch.isfinite(fr["depth"]).all() for fr in frames)
