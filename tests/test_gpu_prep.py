"""Frame preparation on the device (``-m gpu``; gfl_prep_frames, gflow_amd/prep.py, io.load_sequence(device=...)) against
the float64 restatement tests/prep_ref.py and against torch's CPU kernels.

Every comparison with the restatement uses the tolerance float32 arithmetic gives (prep_ref.tolerance, computed from the
shape; nothing is tuned); against torch the bound is that tolerance plus torch's own distance from the restatement on the
same input -- the triangle inequality.  Masks are compared exactly."""
import numpy as np
import pytest
import torch

from tests import prep_ref as R
from tests.test_prep_host import DYADIC, SHAPES, source, torch_mask, torch_resize

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = (("u8", 255.0, 1.0), ("f32", 1.0, 1e3))          # (source, div, max|v| after the conversion)


def run(src, resize=None, **kw):
    from gflow_amd import prep as P
    out = P.prep_frames(torch.from_numpy(np.array(src)).to(DEV), resize, **kw)
    return out.cpu().numpy()


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_resize_against_the_restatement_and_torch(shape, C):
    H, W, r = shape
    for kind, div, vmax in KINDS:
        src = source(kind, 3, H, W, C)
        got, ref = run(src, r, div=div), R.prep_frames(src, r, div=div)
        assert got.dtype == np.float32 and got.shape == ref.shape == (3,) + R.out_shape(H, W, r) + (C,)
        tol = R.tolerance(H, W, r, vmax)
        err = np.abs(got - ref).max()
        want = torch_resize(src, r, div)
        own = np.abs(want - ref).max()
        print(shape, C, kind, "device vs restatement", err, "tolerance", tol, "torch vs restatement", own)
        assert err <= tol
        assert np.abs(got - want).max() <= tol + own
        for t in range(3):                                  # a frame of a batch is its own single-frame call, bit for bit
            assert np.array_equal(run(src[t:t + 1], r, div=div)[0], got[t]), (kind, t)
        assert not np.array_equal(got[0], got[1])
        if R.out_shape(H, W, r) == (H, W):                  # identity: the conversion alone, bit for bit
            assert np.array_equal(got, (torch.from_numpy(np.array(src)).float() / div).numpy())


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_masks_equal_the_restatement_exactly(shape, C):
    H, W, r = shape
    src = source("mask", 3, H, W, C)
    got = run(src, r, as_mask=True)
    assert got.dtype == np.bool_ and got.shape == (3,) + R.out_shape(H, W, r)
    assert np.array_equal(got, R.prep_frames(src, r, as_mask=True))
    assert np.array_equal(run(np.array(src).astype(np.float32), r, as_mask=True), got)      # a float32 mask file
    if shape in DYADIC:
        assert np.array_equal(got, torch_mask(src, r))
    for t in range(3):
        assert np.array_equal(run(src[t:t + 1], r, as_mask=True)[0], got[t])


@pytest.mark.parametrize("k,sigma", [(7, 5.0), (3, 1.0)])
@pytest.mark.parametrize("H,W,r", [(4, 9, None), (16, 16, None), (20, 30, 8)])
def test_blur_against_the_restatement_and_the_host_formula(H, W, r, k, sigma):
    from gflow_amd import io as gio
    for kind, div, vmax in KINDS:
        src = source(kind, 2, H, W, 3 if kind == "u8" else 2)
        kw = dict(div=div, blur=True, blur_kernel_size=k, blur_sigma=sigma)
        got = run(src, r, **kw)
        ref = R.prep_frames(src, r, div=div, blur_k=k, blur_sigma=sigma)
        tol = R.tolerance(H, W, r, vmax, blur_k=k)
        err = np.abs(got - ref).max()
        host = torch.from_numpy(torch_resize(src, r, div))
        host = torch.stack([gio._blur_chw(f.permute(2, 0, 1), True, k, sigma).permute(1, 2, 0) for f in host]).numpy()
        own = np.abs(host - ref).max()
        print((H, W, r), k, kind, "device vs restatement", err, "tolerance", tol, "host vs restatement", own)
        assert got.shape == ref.shape and err <= tol
        assert np.abs(got - host).max() <= tol + own
        assert np.array_equal(run(src[1:2], r, **kw)[0], got[1])


def test_depth_scale_and_offset_are_a_multiply_and_an_add():
    src = source("f32", 2, 9, 13, 1)
    t = torch.from_numpy(np.array(src))
    assert np.array_equal(run(src, None, mul=0.5, add=2.0), (t * 0.5 + 2.0).numpy())
    assert np.array_equal(run(src, None, mul=1.7, add=-0.3), (t * 1.7 + (-0.3)).numpy())
    # after a resize: the restatement's value within the tolerance, scaled
    got, ref = run(src, 4, mul=0.5, add=2.0), R.prep_frames(src, 4, mul=0.5, add=2.0)
    assert np.abs(got - ref).max() <= 0.5 * R.tolerance(9, 13, 4, 1e3) + 2.0 * R.U * (0.5 * 1e3 + 2.0)


def test_two_calls_give_identical_bits():
    for kw in (dict(div=255.0), dict(div=255.0, blur=True), dict(as_mask=True)):
        src = source("u8", 3, 31, 47, 3)
        a, b = run(src, 7, **kw), run(src, 7, **kw)
        assert np.array_equal(a, b), kw


def test_ranks_long_batches_and_the_cached_workspace():
    from gflow_amd import prep as P
    src = source("u8", 19, 13, 29, 3)                        # more than one call of 16 frames
    got = run(src, 5, div=255.0)
    assert got.shape == (19, 5, 11, 3)
    assert np.array_equal(got[17], run(src[17:18], 5, div=255.0)[0]) and np.array_equal(got[3], run(src[3:4], 5, div=255.0)[0])
    assert np.abs(got - R.prep_frames(src, 5, div=255.0)).max() <= R.tolerance(13, 29, 5, 1.0)
    ws = P._workspaces[torch.device(DEV, torch.cuda.current_device()).index]
    run(src[:2], 5, div=255.0)
    assert P._workspaces[torch.cuda.current_device()] is ws          # a smaller call reuses it
    # (H, W, C) and (H, W): the missing axes are added and removed again
    one = run(src[0], 5, div=255.0)
    assert one.shape == (5, 11, 3) and np.array_equal(one, got[0])
    plane = np.ascontiguousarray(src[0, ..., 0])
    assert np.array_equal(run(plane, 5, div=255.0), run(plane[None, ..., None], 5, div=255.0)[0, ..., 0])
    assert run(plane, 5, as_mask=True).shape == (5, 11) and run(src[0], 5, as_mask=True).shape == (5, 11)
    four = source("f32", 2, 13, 29, 4)                       # four channels: the wide loads and stores
    assert np.abs(run(four, 5) - R.prep_frames(four, 5)).max() <= R.tolerance(13, 29, 5, 1e3)
    assert np.array_equal(run(four, None), four)


# ------------------------------------------------------------------------------------------------------------ end to end
H0, W0 = 48, 64


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """a synthetic clip on disk (it loads as 3 frames: the reference's file lists drop the last image)"""
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    return gio.write_sequence(S.make_clip(4, H0, W0, seed=0), str(tmp_path_factory.mktemp("prep") / "seq"))


TENSORS = ("image", "depth", "flow", "move_mask", "occ_mask")


def _raw(sp, i, key):
    """the decoded file behind frame i's tensor, as (1, H, W, C), and its prep_ref keywords"""
    from gflow_amd import io as gio
    p = gio.sequence_paths(sp)
    if key == "image":
        a, div = gio._decode_image(p["img"][i])
        return a[None], dict(div=div)
    if key == "occ_mask":
        a, div = gio._decode_image(p["occ"][i - 1])
        return a[None], dict(div=div)
    if key == "flow":
        return gio._read_flo(p["flow"][i])[None], {}
    return np.load(p["depth"][i]).astype(np.float32)[None, ..., None], {}


def test_device_loaded_frames_equal_host_loaded_frames_without_resize(sequence):
    from gflow_amd import io as gio
    from gflow_amd.fit_video import upload_clip
    host, dev = gio.load_sequence(sequence), gio.load_sequence(sequence, device=DEV)
    assert len(host) == len(dev) == 3
    up = upload_clip(host, DEV)
    for fh, fd, fu in zip(host, dev, up):
        assert sorted(set(fd) - {"occ_count"}) == sorted(fh)
        for k in fh:
            if k in TENSORS:
                assert fd[k].is_cuda and fd[k].dtype == fh[k].dtype and fd[k].shape == fh[k].shape, k
                assert torch.equal(fd[k].cpu(), fh[k]), k
            elif k == "extr":
                assert not fd[k].is_cuda and torch.equal(fd[k], fh[k])
            else:
                assert fd[k] == fh[k], k
        assert fd.get("occ_count") == fu.get("occ_count") and ("occ_count" in fd) == ("occ_mask" in fh)
    again = upload_clip(dev, DEV)                            # device tensors pass through: the same storage
    for fd, fa in zip(dev, again):
        assert all(fa[k].data_ptr() == fd[k].data_ptr() for k in TENSORS if k in fd)
        assert fa.get("occ_count") == fd.get("occ_count")


@pytest.mark.parametrize("blur", [False, True])
def test_device_loaded_frames_with_resize_and_blur(sequence, blur):
    from gflow_amd import io as gio
    r = 24                                                   # scale 2.0
    host, dev = gio.load_sequence(sequence, resize=r, blur=blur), gio.load_sequence(sequence, resize=r, blur=blur, device=DEV)
    from gflow_amd.fit_video import upload_clip
    up = upload_clip(host, DEV)
    for i, (fh, fd) in enumerate(zip(host, dev)):
        assert torch.equal(fd["move_mask"].cpu(), fh["move_mask"]) and fd["move_mask"].shape == (24, 32)
        for k in ("image", "depth", "flow", "occ_mask"):
            if k not in fh:
                assert k not in fd
                continue
            assert fd[k].shape == fh[k].shape and fd[k].dtype == fh[k].dtype, k
            raw, kw = _raw(sequence, i, k)
            k_blur = 7 if blur and k != "depth" else 0
            ref = R.prep_frames(raw, r, blur_k=k_blur, **kw)[0]
            vmax = float(np.abs(R.convert(raw, kw.get("div", 1.0))).max())
            tol = R.tolerance(H0, W0, r, vmax, blur_k=k_blur)
            got, want = fd[k].cpu().numpy(), fh[k].numpy()
            err, own = np.abs(got - ref).max(), np.abs(want - ref).max()
            print(i, k, "device vs restatement", err, "tolerance", tol, "host vs restatement", own)
            assert err <= tol and np.abs(got - want).max() <= tol + own, k
        if not blur:
            assert fd.get("occ_count") == up[i].get("occ_count")


def test_masks_made_from_the_flows_load_on_the_device(sequence, tmp_path):
    """move_masks="epipolar" and occ_masks="flow" with device=: the same masks as the host path gives (the occlusion check
    runs at native size, its mask is then resized on the device; scale 2.0: exact)"""
    import os
    import shutil
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    sp = str(tmp_path / "seq")
    for suffix in ("", "_depth_mast3r_s2", "_flow_unimatch", "_epipolar", "_camera_mast3r_s2"):
        shutil.copytree(sequence + suffix, sp + suffix)
    sc = S._Scene(H0, W0, 0)
    for k in range(1, 4):
        gio.write_flow(os.path.join(sp + "_flow_unimatch", f"{k - 1:05d}_pred_bwd.flo"), sc.backward_flow(k).numpy())
    for r, blur in ((None, False), (24, False), (24, True)):
        kw = dict(resize=r, blur=blur, move_masks="epipolar", occ_masks="flow")
        host, dev = gio.load_sequence(sp, **kw), gio.load_sequence(sp, device=DEV, **kw)
        tol = R.tolerance(H0, W0, r, 1.0, blur_k=7 if blur else 0)
        for i, (fh, fd) in enumerate(zip(host, dev)):
            assert ("occ_mask" in fd) == ("occ_mask" in fh) == (i >= 1)
            assert fd["move_mask"].is_cuda and fd["move_mask"].dtype == torch.bool
            if r is None:
                assert torch.equal(fd["move_mask"].cpu(), fh["move_mask"].cpu())
            if i >= 1:
                assert fd["occ_mask"].shape == fh["occ_mask"].shape and fd["occ_mask"].dtype == torch.float32
                if not blur:
                    assert torch.equal(fd["occ_mask"].cpu() > 0, fh["occ_mask"].cpu() > 0)
                # the device is within tol of the restatement, the host within tol + 2 (H + W) 2^-24 (the bound that
                # test_prep_host.test_restatement_agrees_with_torch_resize holds torch to)
                assert (fd["occ_mask"].cpu() - fh["occ_mask"].cpu()).abs().max() <= 2 * tol + 2 * (H0 + W0) * R.U


def test_a_fit_of_device_loaded_frames_has_the_same_psnr_bits(sequence):
    from gflow_amd import io as gio
    from gflow_amd.fit_video import fit_clip
    cfg = dict(num_points=1500, iterations_first=40, iterations_after=20, iterations_camera=10, densify_interval=20,
               densify_times=1, densify_interval_after=10, densify_times_after=1, lambda_depth=1e-2)
    ka, kb = {}, {}
    a = fit_clip(gio.load_sequence(sequence, frame_range=2), DEV, cfg, seed=0, keep=ka, deterministic=True)
    b = fit_clip(gio.load_sequence(sequence, frame_range=2, device=DEV), DEV, cfg, seed=0, keep=kb, deterministic=True)
    assert a["frames"] == b["frames"] == 2
    pa, pb = torch.stack([p.float() for p in ka["psnr"]]), torch.stack([p.float() for p in kb["psnr"]])
    assert torch.equal(pa, pb) and a["psnr_sum"] == b["psnr_sum"]


def test_fit_video_runs_with_prep_device_and_blur(sequence, capsys):
    from gflow_amd import fit_video
    out = fit_video.main(["--sequence", sequence, "--prep", "device", "--blur", "--resize", "24", "--num_points", "1000",
                          "--iterations_first", "30", "--iterations_after", "10", "--iterations_camera", "5"])
    assert out["frames"] == 3 and np.isfinite(out["psnr_mean_db"])
    capsys.readouterr()
