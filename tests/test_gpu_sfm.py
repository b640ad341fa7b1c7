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


def device_two_view(flows, intr, exclude=None, F_init=None):
    flows = torch.from_numpy(np.asarray(flows)).to(DEV)
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude)).to(DEV)
    if F_init is None:
        F_init = sfm.initial_F(flows.reshape((-1,) + tuple(flows.shape[-3:])), None if ex is None else ex.reshape(-1, *ex.shape[-2:]))
    out = sfm.two_view(flows, intr, ex, F_init=F_init)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, F_init.cpu().numpy()


def compare_pair(tag, dev, ref):
    """one pair's device result against the restatement's"""
    assert R.threshold_margin(ref) > 1e-9, (tag, R.threshold_margin(ref))
    assert np.array_equal(dev["inlier"], ref["inlier"]), tag
    assert tuple(dev["counts"]) == tuple(ref["counts"]), tag
    assert bool(dev["degenerate"]) == bool(ref["degenerate"]), tag
    for k in ("F", "R", "t", "rho", "weight", "parallax"):
        assert np.isfinite(dev[k]).all(), (tag, k)
    if not ref["degenerate"]:
        assert np.array_equal(dev["votes"], ref["votes"]), tag
        dF = np.abs(R.normalise_F(dev["F"]) - R.normalise_F(ref["F"])).max()
        dR, dt = np.abs(dev["R"] - ref["R"]).max(), np.abs(dev["t"] - ref["t"]).max()
        dp = abs(dev["parallax"] - ref["parallax"])
        print(f"{tag}: F {dF:.2e} R {dR:.2e} t {dt:.2e} parallax {dp:.2e}")
        assert dF <= F_BOUND and dR <= R_BOUND and dt <= T_BOUND and dp <= PAR_BOUND, tag
        assert abs(np.linalg.norm(dev["F"]) - 1.0) < 1e-12 and dev["F"].reshape(-1)[np.argmax(np.abs(dev["F"]))] > 0
    else:
        assert not dev["t"].any() and not dev["rho"].any() and not dev["weight"].any(), tag
    assert np.array_equal(dev["weight"] > 0, ref["weight"] > 0), tag
    for k in ("rho", "weight"):
        err, bound = np.abs(dev[k] - ref[k]).max(), 2 * EPS32 * np.abs(ref[k]).max()
        print(f"{tag}: {k} err {err:.2e} bound {bound:.2e}")
        assert err <= bound, (tag, k)


@pytest.mark.parametrize("H,W", [(16, 24), (33, 47)])
@pytest.mark.parametrize("kind", ["plain", "block", "excluded", "inf"])
def test_two_view_against_the_restatement(H, W, kind):
    flow, intr, exclude = scene(H, W, kind)
    dev, F0 = device_two_view(flow, intr, exclude)
    ref = R.two_view(flow, intr, F0[0], exclude)
    compare_pair(f"{H}x{W} {kind}", dev, ref)
    assert not ref["degenerate"] and ref["counts"][1] >= 0.5 * H * W
    if kind == "inf":
        known = np.isfinite(flow).all(-1)
        assert ref["counts"][0] == known.sum() < H * W and not dev["inlier"][~known].any()
    if kind == "excluded":
        assert not dev["inlier"][exclude != 0].any() and ref["counts"][0] == (exclude == 0).sum()
    if kind == "block":
        assert ref["counts"][1] < H * W


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


@pytest.mark.parametrize("H,W", [(16, 24), (33, 47), (57, 70)])
def test_fill_against_the_restatement(H, W):
    """pull-push and sweeps on random inverse depths with holes: one tile, odd sizes with partial tiles and odd pyramid
    levels, several tiles; sweep counts around the four of a fused launch"""
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


def test_medians_are_exact():
    rng = np.random.default_rng(5)
    M, H, W = 5, 33, 47
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
            assert cnt[m] == n and (np.isnan(med[m]) if n == 0 else med[m] == want), (m, w_min)


def device_clip(fwd, bwd, **kw):
    up = lambda x: None if x is None else torch.from_numpy(np.stack(x)).to(DEV)
    if bwd is None:                                                # the last frame has no pair at all
        with pytest.warns(UserWarning, match="frame"):
            res = sfm.clip_depth_camera(up(fwd), None, **kw)
    else:
        res = sfm.clip_depth_camera(up(fwd), up(bwd), **kw)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("H,W,both", [(36, 48, True), (33, 47, True), (33, 47, False)])
def test_clip_against_the_restatement(H, W, both):
    """three frames with baselines 0.08 and 0.12: ratios, baselines, chained poses and depth; with the forward flows alone
    every baseline comes from the medians (the path of a missing ratio)"""
    s3 = R.make_scene3(H, W, f=40.0 * max(H, W) / 48.0)
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
    r0 = 1.0 / ref["depth"][0]
    kappa = r0.max() / r0.min()                                    # rho's error seen in a depth: relative, times max / min
    # the baselines carry the float32 medians of depth; the poses' rotations are float64
    assert np.abs(base / ref["baseline"] - 1.0).max() <= n * EPS32 * kappa
    for i in range(3):
        dR = np.abs(extr[i][:, :3] - ref["extr"][i][:, :3]).max()
        print(f"{H}x{W} frame {i}: chained rotation {dR:.2e}")
        assert dR <= CHAIN_BOUND
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
