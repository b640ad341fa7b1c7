"""GPU: optical flow from the images (csrc/gfl_optflow.hip, gflow_amd/optflow.py) against the float64 restatement
(tests/optflow_ref.py).

No bound is fixed in advance.  For every case the restatement runs on the CPU in float32 and in float64 on the case's own
inputs; the largest absolute difference between the two is the case's gap, and the device must stay within 4 x that gap of the
float64 result (the factor allows for rounding differences between torch's CPU float32 and the device).  The kernels round
every product and sum on their own, in the restatement's order, with IEEE division and a correctly rounded square root: where
these figures were taken the device's result was the float32 restatement's, bit for bit, in every case below, so
err = max |device - float64| equalled the gap.

Measured on an MI355X (gap = max |float32 - float64| of the restatement; tile 52 x 52 of a 64 x 64 region, S = 6):
  one level, warps = outer = 1, sweeps in {1, 5, 6, 7, 15}, the seven shapes: zero start 2.2e-10 .. 5.4e-9 px; smooth and
  outside starts 3.1e-7 .. 3.2e-5 px; flat images 2.8e-7 .. 1.5e-6 px; warps = outer = 2 with 7 sweeps: 1.3e-4 px;
  pyramid and upsample (min_side 8, warps = outer = sweeps = 1): 33 x 47 1.9e-6 px, 65 x 31 5.2e-4 px;
  whole estimate, defaults, P = 2: 96 x 128 seed 0 / 2: max 1.5e-4 / 2.4e-4 px (mean 1.5e-6 / 2.0e-6); 120 x 214 seed 0 / 2:
  max 2.4e-4 / 1.2e-1 px (mean 1.9e-6 / 2.5e-5: seed 2 has a few pixels at the disc's rim where the robust weights amplify the
  last bit); mean EPE of the device 0.0538 / 0.0528, 0.1059 / 0.0846, 0.0461 / 0.0462, 0.0895 / 0.0853 px forward / backward,
  equal to the float64 restatement's to 3e-5 px.
"""
import os

import numpy as np
import pytest
import torch

from tests import optflow_ref as R
from tests.test_optflow_host import epe, kernel_constants, level_images, scene_pair, scene_reference, start_flow

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, RY, RX = kernel_constants()
TY, TX = RY - 2 * S, RX - 2 * S                    # what a launch of the tiled path writes per workgroup
SWEEPS = sorted({1, S - 1, S, S + 1, 2 * S + 3} - {0})
STARTS = ("zero", "smooth", "outside")
# 8 x 8; odd; one pixel under and over the tile in each axis; the largest level that is one workgroup, and one row / one column
# more than that
LEVEL_SHAPES = [(8, 8), (17, 23), (TY - 1, TX - 1), (TY + 1, TX + 1), (RY, RX), (RY + 1, RX), (RY, RX + 1)]


def device_level(Ia, Ib, flow, alpha=5.0, warps=1, outer=1, sweeps=1):
    """gfl_optflow_level on float32 host tensors; returns the new flow on the host"""
    from gflow_amd import _lib as L
    lib = L.load()
    P, H, W = Ia.shape
    a, b = Ia.to(DEV).contiguous(), Ib.to(DEV).contiguous()
    fl = flow.to(DEV).contiguous().clone()
    assert a.dtype == b.dtype == fl.dtype == torch.float32
    ws = L.scratch(lib.gfl_optflow_workspace_bytes(P, H, W, 16), DEV)
    L.check(lib.gfl_optflow_level(L.ptr(a), L.ptr(b), L.ptr(fl), P, H, W, alpha, warps, outer, sweeps, L.ptr(ws), ws.numel(),
                                  L.stream()), "optflow level")
    torch.cuda.synchronize()
    return fl.cpu()


def hold_to_the_gap(tag, got, ref32, ref64):
    """print the figures, then assert max |got - float64| <= 4 max |float32 - float64|"""
    gap = (ref32.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    print(f"{tag}: gap {gap:.3e} err {err:.3e} bitwise-float32 {torch.equal(got, ref32)}")
    assert torch.isfinite(got).all()
    assert err <= 4.0 * gap, (tag, err, gap)
    return gap, err


def level_case(Ia, Ib, flow, **kw):
    """(float32 restatement, float64 restatement) of one level on the float32-rounded inputs"""
    return R.flow_level(Ia, Ib, flow, **kw), R.flow_level(Ia.double(), Ib.double(), flow.double(), **kw)


@pytest.mark.parametrize("H,W", LEVEL_SHAPES)
def test_one_level_against_the_restatement(H, W):
    P = 3
    Ia, Ib = (t.float() for t in level_images(P, H, W))
    for kind in STARTS:
        flow = start_flow(kind, P, H, W).float()
        if kind == "outside":
            xs, ys = torch.arange(W) + flow[..., 0], torch.arange(H)[:, None] + flow[..., 1]
            assert xs.min() <= -3.9 and xs.max() >= W + 2.9 and ys.min() <= -3.9 and ys.max() >= H + 2.9
        for sweeps in SWEEPS:
            ref32, ref64 = level_case(Ia, Ib, flow, warps=1, outer=1, sweeps=sweeps)
            got = device_level(Ia, Ib, flow, sweeps=sweeps)
            hold_to_the_gap(f"{H}x{W} {kind} sweeps {sweeps}", got, ref32, ref64)
            if kind != "zero":
                assert not torch.equal(got, flow)


def test_one_level_with_several_warps_and_reweightings():
    """the loops around the sweeps: warps = 2, outer = 2 on a tiled shape and on a one-workgroup shape"""
    for (H, W) in ((TY + 5, TX + 9), (RY - 3, RX - 5)):
        Ia, Ib = (t.float() for t in level_images(3, H, W))
        flow = start_flow("smooth", 3, H, W).float()
        kw = dict(warps=2, outer=2, sweeps=S + 1)
        ref32, ref64 = level_case(Ia, Ib, flow, **kw)
        hold_to_the_gap(f"{H}x{W} warps 2 outer 2", device_level(Ia, Ib, flow, **kw), ref32, ref64)


@pytest.mark.parametrize("H,W", [(17, 23), (TY + 1, TX + 1)])
def test_flat_images(H, W):
    P = 3
    flat = torch.full((P, H, W), 100.0)
    # b == a and a zero start: the flow stays exactly zero (textured and flat)
    Ia = level_images(P, H, W)[0].float()
    zero = torch.zeros(P, H, W, 2)
    assert not device_level(Ia, Ia, zero, warps=2, outer=2, sweeps=S + 1).any()
    assert not device_level(flat, flat, zero, warps=2, outer=2, sweeps=S + 1).any()
    # a constant image: Ix = Iy = It = 0, only the smoothness term acts.  A constant flow stays (each sweep forms
    # (sum_n w_n c - ws c) / ws: a few ulp of c, 1e-5 px is far above n sweeps of that) ...
    const = torch.zeros(P, H, W, 2)
    const[..., 0], const[..., 1] = 1.25, -0.75
    got = device_level(flat, flat, const, sweeps=2 * S + 3)
    assert torch.isfinite(got).all() and (got - const).abs().max() <= 1e-5
    # ... and a smooth flow is diffused: every new value is a weighted mean of neighbours, so nothing leaves the range
    for kind in ("smooth", "outside"):
        flow = start_flow(kind, P, H, W).float()
        for sweeps in (1, 2 * S + 3):
            ref32, ref64 = level_case(flat, flat, flow, warps=1, outer=1, sweeps=sweeps)
            got = device_level(flat, flat, flow, sweeps=sweeps)
            hold_to_the_gap(f"flat {H}x{W} {kind} sweeps {sweeps}", got, ref32, ref64)
            assert not torch.equal(got, flow)
            for c in range(2):
                assert got[..., c].min() >= flow[..., c].min() - 1e-5 and got[..., c].max() <= flow[..., c].max() + 1e-5


@pytest.mark.parametrize("H,W,sizes", [(33, 47, [(33, 47), (17, 24), (9, 12)]), (65, 31, [(65, 31), (33, 16), (17, 8)])])
def test_pyramid_and_upsample(H, W, sizes):
    """odd sizes through gfl_optflow with one warp, one re-weighting, one sweep per level: grey, the 5-tap pyramid and the
    flow's upsampling carry the result.  min_side = 8, so that both shapes get two more levels (at the default 16 the
    second has none: 31 / 2 < 16)."""
    from gflow_amd import optflow as OF
    from gflow_amd import synthetic as SY
    assert R.level_sizes(H, W, 8) == sizes
    sc = SY._Scene(H, W, 1)
    i2, i3 = sc.frame(2)["image"].float(), sc.frame(3)["image"].float()
    a, b = torch.stack([i2, i3, i2]), torch.stack([i3, i2, i2.flip(1)])
    kw = dict(warps=1, outer=1, sweeps=1, min_side=8)
    ref32, ref64 = R.estimate_flow(a, b, dtype=torch.float32, **kw), R.estimate_flow(a, b, **kw)
    got = OF.estimate_flow(a, b, **kw)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, H, W, 2)
    hold_to_the_gap(f"pyramid {H}x{W}", got.cpu(), ref32, ref64)
    assert ref64.abs().max() > 0.01                # (no trivial case: one sweep per level moves the flow by hundredths of a pixel)


@pytest.mark.parametrize("H,W,seed", [(96, 128, 0), (96, 128, 2), (120, 214, 0), (120, 214, 2)])
def test_whole_estimate(H, W, seed):
    from gflow_amd import optflow as OF
    a, b, truth = scene_pair(H, W, seed)
    ref64 = scene_reference(H, W, seed)
    ref32 = R.estimate_flow(a, b, dtype=torch.float32)
    got = OF.estimate_flow(a, b).cpu()
    gap, _ = hold_to_the_gap(f"whole {H}x{W} seed {seed}", got, ref32, ref64)
    off = ((got.double() - ref64).abs() > 4.0 * gap).double().mean().item()
    mean_gap = (ref32.double() - ref64).abs().mean().item()
    e_dev, e_ref = epe(got, truth), epe(ref64, truth)
    print(f"mean gap {mean_gap:.3e} share off {off} EPE device {e_dev.tolist()} float64 {e_ref.tolist()}")
    assert off == 0.0
    assert (e_dev <= 1.25 * e_ref).all()


def test_determinism_batching_and_uint8():
    from gflow_amd import optflow as OF
    from gflow_amd import synthetic as SY
    H, W = 40, 72                                   # two levels; the finer one is tiled, the coarser one workgroup
    sc = SY._Scene(H, W, 3)
    u8 = torch.stack([(sc.frame(k)["image"].float().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8) for k in range(4)])
    a, b = u8[:3].to(DEV), u8[1:].to(DEV)
    first = OF.estimate_flow(a, b)
    assert torch.equal(first, OF.estimate_flow(a, b))
    for p in range(3):
        alone = OF.estimate_flow(a[p], b[p])
        assert tuple(alone.shape) == (H, W, 2) and torch.equal(alone, first[p])
    as_float = torch.from_numpy(u8.numpy().astype(np.float32) / np.float32(255))       # (a true division, as the kernel's)
    assert torch.equal(first, OF.estimate_flow(as_float[:3], as_float[1:]))
    assert torch.equal(first, OF.estimate_flow(u8[:3].numpy(), u8[1:].numpy()))             # (arrays, from the host)
    fwd, bwd = OF.clip_flows(u8)
    assert torch.equal(fwd, first) and torch.equal(bwd, OF.estimate_flow(b, a))
    assert first.abs().mean() > 0.5


def test_fused_sweeps_have_the_bits_of_plain_sweeps(monkeypatch):
    """GFL_OPTFLOW_FUSED=0 (read at every call) launches every sweep on its own, one lane per pixel"""
    for (H, W) in ((TY + TY // 2, 2 * TX + 3), (RY, RX), (RY - 5, RX - 7)):
        Ia, Ib = (t.float() for t in level_images(3, H, W))
        flow = start_flow("outside", 3, H, W).float()
        for sweeps in (S - 1, 2 * S + 3):
            kw = dict(warps=2, outer=2, sweeps=sweeps)
            monkeypatch.delenv("GFL_OPTFLOW_FUSED", raising=False)
            fused = device_level(Ia, Ib, flow, **kw)
            monkeypatch.setenv("GFL_OPTFLOW_FUSED", "0")
            plain = device_level(Ia, Ib, flow, **kw)
            monkeypatch.delenv("GFL_OPTFLOW_FUSED")
            assert torch.equal(fused, plain), (H, W, sweeps)


def test_refusals_on_the_device():
    from gflow_amd import _lib as L
    from gflow_amd import optflow as OF
    lib = L.load()
    z = torch.zeros(1, 8, 8, device=DEV)
    fl = torch.zeros(1, 8, 8, 2, device=DEV)
    ws = L.scratch(lib.gfl_optflow_workspace_bytes(1, 8, 8, 16), DEV)
    args = lambda nbytes: (L.ptr(z), L.ptr(z), L.ptr(fl), 1, 8, 8, 5.0, 1, 1, 1, L.ptr(ws), nbytes, L.stream())
    assert lib.gfl_optflow_level(*args(68 * 64 - 1)) == -2 and lib.gfl_optflow_level(*args(ws.numel())) == 0      # (68 B a pixel)
    img = torch.zeros(1, 8, 8, 3, device=DEV)
    flow_args = lambda nbytes: (L.ptr(img), L.ptr(img), 0, 1, 8, 8, 5.0, 1, 1, 1, 16, L.ptr(fl), L.ptr(ws), nbytes, L.stream())
    assert lib.gfl_optflow(*flow_args(ws.numel() - 1)) == -2 and lib.gfl_optflow(*flow_args(ws.numel())) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        OF.estimate_flow(torch.zeros(8, 8, 3, device=DEV), torch.zeros(8, 8, 3, device=DEV), sweeps=0)


def _same_frames(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert sorted(fa) == sorted(fb)
        for k in fa:
            if torch.is_tensor(fa[k]):
                assert fa[k].device == fb[k].device and torch.equal(fa[k], fb[k]), k
            else:
                assert fa[k] == fb[k], k


def test_flows_of_a_sequence_from_its_images(tmp_path):
    """the command line writes the .flo files under the names the loader and gflow_amd.occlusion pick up, and
    load_sequence(flows="estimate") gives the frames that loading those files gives, bit for bit"""
    import shutil
    from gflow_amd import io as gio
    from gflow_amd import occlusion as OC
    from gflow_amd import optflow as OF
    from gflow_amd import synthetic as SY
    sp = gio.write_sequence(SY.make_clip(4, 96, 128, seed=0), str(tmp_path / "seq"))
    flows = sp + "_flow_unimatch"
    shutil.rmtree(flows)
    est = {}
    for resize in (None, 64):
        for device in (None, DEV):
            est[resize, device] = gio.load_sequence(sp, resize=resize, device=device, flows="estimate", occ_masks="flow",
                                                    move_masks="epipolar")
    assert not os.path.exists(flows)
    assert OF.main(["--img_dir", sp]) == 0
    names = [f"{i:05d}_{k}.flo" for i in range(3) for k in ("pred", "pred_bwd")]
    assert sorted(os.listdir(flows)) == sorted(names)
    p = gio.sequence_paths(sp)
    assert [f.name for f in p["flow"]] == [f"{i:05d}_pred.flo" for i in range(3)]
    assert [f.name for f in p["flow_bwd"]] == [f"{i:05d}_pred_bwd.flo" for i in range(3)]
    with pytest.raises(SystemExit, match="overwrite"):
        OF.main(["--img_dir", sp])
    assert OC.main(["--img_dir", sp]) == 0
    assert sorted(os.listdir(flows)) == sorted(names + [f"{i:05d}_{k}.png" for i in range(3) for k in ("occ", "occ_bwd")])
    for (resize, device), frames in est.items():
        files = gio.load_sequence(sp, resize=resize, device=device, flows="files", occ_masks="flow", move_masks="epipolar")
        _same_frames(frames, files)
        assert len(frames) == 3 and all("occ_mask" in fr for fr in frames[1:]) and "occ_mask" not in frames[0]
        for fr in frames:
            assert fr["flow"].dtype == torch.float32 and fr["flow"].shape[:2] == fr["image"].shape[:2]
            assert fr["flow"].is_cuda == (device is not None) and fr["flow"].abs().mean() > 0.5
    # the estimate is the scene's flow: the written forward flow of frame 1 against the clip's own
    truth = SY.make_clip(4, 96, 128, seed=0)[1]["flow"]
    got = gio.read_flow(os.path.join(flows, "00001_pred.flo"))
    assert (got - torch.as_tensor(truth).float()).norm(dim=-1).mean() < 0.25
    # every image of the folder: the last frame has no following image and gets zeros
    every = gio.load_sequence(sp, frame_range=4, flows="estimate")
    assert len(every) == 4 and not every[3]["flow"].any() and torch.equal(every[2]["flow"], est[None, None][2]["flow"])


def test_fit_video_fits_a_sequence_that_has_only_images_depth_and_cameras(tmp_path, capsys):
    import shutil
    from gflow_amd import fit_video
    from gflow_amd import io as gio
    from gflow_amd import synthetic as SY
    sp = gio.write_sequence(SY.make_clip(4, 96, 128, seed=0), str(tmp_path / "seq"))
    shutil.rmtree(sp + "_flow_unimatch")
    shutil.rmtree(sp + "_epipolar")
    assert sorted(os.listdir(tmp_path)) == ["seq", "seq_camera_mast3r_s2", "seq_depth_mast3r_s2"]
    out = fit_video.main(["--sequence", sp, "--make-flows", "--make-occ-masks", "--make-move-masks", "--num_points", "1000",
                          "--iterations_first", "30", "--iterations_after", "10", "--iterations_camera", "5"])
    assert out["frames"] == 3 and np.isfinite(out["psnr_mean_db"])
    assert sorted(os.listdir(tmp_path)) == ["seq", "seq_camera_mast3r_s2", "seq_depth_mast3r_s2"]      # nothing was written
    capsys.readouterr()
