"""CPU: frame preparation -- the float64 restatement (tests/prep_ref.py) against torch's CPU kernels, the host side of
gflow_amd/prep.py, the blur option of the readers, the fit_video flags and the ABI entries.  Also holds the shapes and the
sources the GPU tests (tests/test_gpu_prep.py) share."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import prep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Hs, Ws, resize): dyadic scales (2.0, 2.5, 2.5; landscape and portrait), non-dyadic scales, an upscale, a single output
# pixel, rows wider than a workgroup whose width is no multiple of 64, the identity
SHAPES = [(8, 12, 4), (20, 30, 8), (25, 10, 4), (31, 47, 7), (13, 29, 5), (12, 12, 18), (7, 7, 1), (5, 600, 4), (9, 9, 9)]
DYADIC = SHAPES[:3]


@functools.lru_cache(maxsize=None)
def source(kind, T, H, W, C, seed=0):
    """(T, H, W, C) frames that differ: "u8" uint8 with 0 and 255 in every frame, "f32" float32 with negative values and
    magnitudes up to 1e3, "mask" uint8 with 3 % of the pixels set (any channel).  Computed once, left unchanged."""
    rng = np.random.default_rng([seed, T, H, W, C, len(kind)])
    if kind == "u8":
        a = rng.integers(0, 256, size=(T, H, W, C), dtype=np.uint8)
        a[:, 0, 0, :] = 0
        a[:, -1, -1, :] = 255
    elif kind == "f32":
        a = (rng.standard_normal((T, H, W, C)) * 200.0).clip(-1e3, 1e3).astype(np.float32)
        a[:, 0, 0, 0] = -1e3
        a[:, -1, -1, -1] = 1e3
    else:
        a = ((rng.random((T, H, W, C)) < 0.03) * 255).astype(np.uint8)
    a.setflags(write=False)
    return a


def torch_resize(src, resize, div=1.0):
    """torch's CPU result for (T, H, W, C): io._resize_chw per frame, as the host path runs it"""
    from gflow_amd import io as gio
    t = torch.from_numpy(np.array(src)).float() / div
    return torch.stack([gio._resize_chw(f.permute(2, 0, 1), resize).permute(1, 2, 0) for f in t]).numpy()


def torch_mask(src, resize):
    """read_mask's arithmetic on (T, H, W, C) arrays"""
    return torch.from_numpy(torch_resize(src, resize)).sum(dim=-1).numpy() > 0


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_entries_within_312():
    from gflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    assert re.search(r"^#define GFL_VERSION 312$", hdr, flags=re.M) and _lib.MIN_VERSION == 312
    assert _lib.load().gfl_version() == 312
    assert "frame preparation (additive within 312" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n in (("gfl_prep_workspace_bytes", 7), ("gfl_prep_frames", 18)):
        args = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1).split(",")
        assert len(args) == n == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["gfl_prep_workspace_bytes"][0] is ctypes.c_size_t
    assert "gfl_prep.hip" in open(os.path.join(ROOT, "gflow_amd", "csrc", "Makefile")).read()


def test_refused_arguments_return_invalid_before_any_launch():
    from gflow_amd import _lib
    lib = _lib.load()
    ws_bytes = lib.gfl_prep_workspace_bytes
    good = dict(T=2, C=3, Hs=20, Ws=30, Hd=8, Wd=12, blur_k=0)
    need = ws_bytes(*good.values())
    assert need >= 4 * 2 * 3 * 20 * 12 and ws_bytes(*dict(good, blur_k=7).values()) > need
    assert ws_bytes(*dict(good, Hd=20, Wd=30).values()) > 0                      # (identity: the conversion table alone)
    bad_shapes = [dict(T=0), dict(T=-1), dict(C=0), dict(C=5), dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=0), dict(Hs=-4),
                  dict(Hs=16385, Hd=16385), dict(Ws=16385), dict(Wd=16385), dict(Hd=16385),
                  dict(Hs=65, Hd=1), dict(Ws=129, Wd=2),                                   # more than 64 to 1
                  dict(T=1 << 20, Hs=64, Ws=64, Hd=1, Wd=1),                               # 2^32 elements in src
                  dict(T=1 << 10, C=1, Hs=16384, Ws=256, Hd=256, Wd=16384),                # ... in the intermediate
                  dict(T=1 << 16, C=4, Hs=8, Ws=8, Hd=128, Wd=128),                        # ... in dst
                  dict(blur_k=1), dict(blur_k=4), dict(blur_k=33), dict(blur_k=-7), dict(blur_k=17),       # 17 / 2 >= Hd
                  dict(Hs=4, Ws=9, Hd=4, Wd=9, blur_k=9)]
    # host memory stands in for every buffer: a call that got past the checks would hand it to the device runtime
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)

    def call(u8=0, div=1.0, mul=1.0, add=0.0, sigma=5.0, mask=0, src=p, dst=p, ws=p, ws_size=None, **shape):
        s = dict(good, **shape)
        size = ws_bytes(*s.values()) if ws_size is None else ws_size
        return lib.gfl_prep_frames(src, u8, s["T"], s["C"], s["Hs"], s["Ws"], s["Hd"], s["Wd"], div, mul, add, s["blur_k"],
                                   sigma, mask, dst, ws, max(size, 1), null)

    for bad in bad_shapes:
        assert ws_bytes(*dict(good, **bad).values()) == 0, bad
        assert call(**bad, ws_size=1 << 40) == -1, bad
    assert ws_bytes(*dict(good, Hs=4, Ws=9, Hd=4, Wd=9, blur_k=7).values()) > 0            # 7 / 2 < 4: the smallest extent
    nan, inf = float("nan"), float("inf")
    for kw in (dict(div=0.0), dict(div=-1.0), dict(div=nan), dict(div=inf), dict(mul=nan), dict(mul=inf), dict(add=nan),
               dict(add=-inf), dict(blur_k=7, sigma=0.0), dict(blur_k=7, sigma=-1.0), dict(blur_k=7, sigma=nan),
               dict(blur_k=7, sigma=inf), dict(mask=1, blur_k=7), dict(mask=1, mul=2.0), dict(mask=1, add=1.0),
               dict(mask=2), dict(u8=2), dict(src=null), dict(dst=null), dict(ws=null),
               dict(src=ctypes.c_void_p(p.value + 2)), dict(dst=ctypes.c_void_p(p.value + 1)),
               dict(ws=ctypes.c_void_p(p.value + 4)), dict(ws_size=need - 1), dict(ws_size=0)):
        assert call(**kw) == -1, kw
    assert not any(buf)


# ------------------------------------------------------------------------------------------------------ the restatement
def test_out_shape_is_the_shorter_side_rule():
    from gflow_amd import io as gio
    from gflow_amd import prep as P
    cases = [(10, 25, 4), (25, 10, 4), (480, 854, 480), (1080, 1920, 480), (1920, 1080, 480), (7, 7, 1), (9, 9, 9),
             (5, 600, 4), (12, 12, 18), (31, 47, 7)]
    for h, w, r in cases:
        want = tuple(gio._resize_chw(torch.zeros(3, h, w), r).shape[1:])
        assert P.out_shape(h, w, r) == want == R.out_shape(h, w, r), (h, w, r)
    assert P.out_shape(10, 25, 4) == (4, 10) and P.out_shape(25, 10, 4) == (10, 4) and P.out_shape(480, 854, 480) == (480, 854)
    assert P.out_shape(33, 17, None) == (33, 17)


def test_weights_are_normalised_and_cover_their_support():
    for n_in, n_out in ((12, 6), (30, 12), (47, 10), (29, 11), (12, 18), (7, 1), (600, 480), (64, 1)):
        m, taps = R.axis_matrix(n_in, n_out)
        assert taps <= 2 * int(np.ceil(max(n_in / n_out, 1.0))) + 2
        assert (m >= 0).all() and np.abs(m.sum(axis=1) - 1.0).max() <= taps * R.U
    assert np.array_equal(R.axis_matrix(9, 9)[0][:, :9].diagonal(), np.ones(9))              # scale 1: weight 1 on itself


@pytest.mark.parametrize("shape", SHAPES + [(135, 240, 54)])
def test_restatement_agrees_with_torch_resize(shape):
    """torch forms the same filter's weights in float32 from float32 coordinates: a weight is off by a few roundings of a
    coordinate of magnitude <= n_in, scaled by 1 / support -- at most about 2 n_in 2^-24 summed over an output's taps --
    and its float32 sums add what tolerance() allows.  d = (2 (Hs + Ws) 2^-24) max|v| + tolerance."""
    H, W, r = shape
    src = source("u8", 2, H, W, 3)
    got, want = R.prep_frames(src, r, div=255.0), torch_resize(src, r, 255.0)
    assert got.shape == want.shape
    d = 2.0 * (H + W) * R.U + R.tolerance(H, W, r, 1.0)
    err = np.abs(got - want).max()
    print(shape, "restatement vs torch", err, "bound", d)
    assert err <= d
    if R.out_shape(H, W, r) == (H, W):
        assert np.array_equal(got, R.convert(src, 255.0).astype(np.float64))


@pytest.mark.parametrize("shape", DYADIC + [(16, 24, 8), (9, 18, 4)])
@pytest.mark.parametrize("C", [1, 3])
def test_restatement_masks_equal_torch_at_dyadic_scales(shape, C):
    H, W, r = shape
    for seed in range(4):
        src = source("mask", 2, H, W, C, seed)
        assert np.array_equal(R.prep_frames(src, r, as_mask=True), torch_mask(src, r))


@pytest.mark.parametrize("k,sigma,H,W", [(7, 5.0, 4, 9), (7, 5.0, 16, 16), (3, 1.0, 16, 16), (3, 1.0, 2, 5)])
def test_restatement_blur_is_pad_and_conv2d(k, sigma, H, W):
    """against io._blur_chw (reflect pad + grouped conv2d with the outer product of float32 taps): the taps agree to a
    float32 rounding each, the k^2 products are summed in float32 -- (k^2 + 2 k + 2) 2^-24 max|v|"""
    from gflow_amd import io as gio
    src = source("f32", 1, H, W, 2)
    got = R.prep_frames(src, None, blur_k=k, blur_sigma=sigma)[0]
    want = gio._blur_chw(torch.from_numpy(np.array(src[0])).permute(2, 0, 1), True, k, sigma).permute(1, 2, 0).numpy()
    bound = (k * k + 2 * k + 2) * R.U * np.abs(src).max()
    err = np.abs(got - want).max()
    print(k, sigma, H, W, err, bound)
    assert err <= bound
    m = R.blur_matrix(5, 7, 5.0)                                     # index -i reads i; the edge is not repeated
    t = R.blur_taps(7, 5.0).astype(np.float64)
    assert np.allclose(m[0], [t[3], t[2] + t[4], t[1] + t[5], t[0] + t[6], 0.0], rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------------------------------- the readers, host
def _sequence(tmp_path, n=4, H=24, W=32):
    """a clip of n frames on disk; it loads as n - 1 frames (the reference's file lists drop the last image)"""
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    return gio.write_sequence(S.make_clip(n, H, W, seed=0), str(tmp_path / "seq"))


def _same(a, b):
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_load_sequence_defaults_give_the_same_bytes(tmp_path):
    from gflow_amd import io as gio
    sp = _sequence(tmp_path)
    for resize in (None, 12):
        a = gio.load_sequence(sp, resize=resize)
        b = gio.load_sequence(sp, resize=resize, blur=False, device=None)
        assert len(a) == len(b) == 3
        for i, (fa, fb) in enumerate(zip(a, b)):
            assert sorted(fa) == sorted(fb) and all(_same(fa[k], fb[k]) for k in fa)
            # and they are what the readers give one file at a time
            p = gio.sequence_paths(sp)
            assert torch.equal(fa["image"], gio.image_path_to_tensor(p["img"][i], resize))
            assert torch.equal(fa["depth"], gio.read_depth(p["depth"][i], resize).unsqueeze(-1))
            assert torch.equal(fa["move_mask"], gio.read_mask(p["move"][i], resize))
            if i < len(p["flow"]):
                assert torch.equal(fa["flow"], gio.read_flow(p["flow"][i], resize))
            assert all(not v.is_cuda for v in fa.values() if torch.is_tensor(v))


@pytest.mark.parametrize("resize", [None, 12])
def test_load_sequence_blur_is_the_formula_on_image_occlusion_mask_and_flow(tmp_path, resize):
    from gflow_amd import io as gio
    sp = _sequence(tmp_path)
    plain, blurred = gio.load_sequence(sp, resize=resize), gio.load_sequence(sp, resize=resize, blur=True)
    formula = lambda t: gio._blur_chw(t.permute(2, 0, 1), True).permute(1, 2, 0)
    n_flows = len(gio.sequence_paths(sp)["flow"])
    for i, (fa, fb) in enumerate(zip(plain, blurred)):
        assert sorted(fa) == sorted(fb)
        assert torch.equal(fb["image"], formula(fa["image"])) and not torch.equal(fb["image"], fa["image"])
        assert torch.equal(fb["flow"], formula(fa["flow"]) if i < n_flows else fa["flow"])
        if i >= 1:
            assert torch.equal(fb["occ_mask"], formula(fa["occ_mask"]))
        assert torch.equal(fb["depth"], fa["depth"]) and torch.equal(fb["move_mask"], fa["move_mask"])
        assert fb["image"].shape == fa["image"].shape and fb["flow"].shape == fa["flow"].shape


def test_blur_of_the_readers_is_gaussian_blur_7_5():
    from gflow_amd import io as gio
    t = torch.zeros(1, 9, 9)
    t[0, 4, 4] = 1.0
    out = gio._blur_chw(t, True)[0]
    x = torch.linspace(-3, 3, 7)
    k = torch.exp(-0.5 * (x / 5.0) ** 2)
    k = k / k.sum()
    assert torch.allclose(out[1:8, 1:8], torch.outer(k, k), rtol=0, atol=1e-7) and abs(float(out.sum()) - 1.0) < 1e-5
    assert gio._blur_chw(t, False) is t


def test_fit_video_knows_blur_and_prep(capsys):
    from gflow_amd import fit_video
    args = fit_video._parser().parse_args([])
    assert args.blur is False and args.prep == "host"
    args = fit_video._parser().parse_args(["--blur", "--prep", "device"])
    assert args.blur is True and args.prep == "device"
    with pytest.raises(SystemExit):
        fit_video._parser().parse_args(["--prep", "cuda"])
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------- the Python layer, host
def test_prep_frames_argument_checks_and_no_cpu_fallback():
    from gflow_amd import prep as P
    z = torch.zeros(2, 8, 12, 3)
    for bad, kw in ((torch.zeros(8), {}), (torch.zeros(1, 2, 8, 12, 3), {}), (z.double(), {}), (z.to(torch.int32), {}),
                    (torch.zeros(2, 8, 12, 5), {}), (torch.zeros(0, 8, 12, 3), {}), (torch.zeros(2, 0, 12, 3), {}),
                    (z.permute(0, 2, 1, 3), {}), (z, dict(resize=0)), (z, dict(resize=2.5)), (z, dict(resize=20000)),
                    (torch.zeros(1, 130, 130, 1), dict(resize=2)),                                     # 65 to 1
                    (z, dict(div=0.0)), (z, dict(div=float("nan"))), (z, dict(mul=float("inf"))), (z, dict(add=float("nan"))),
                    (z, dict(blur=True, blur_kernel_size=4)), (z, dict(blur=True, blur_kernel_size=33)),
                    (z, dict(blur=True, blur_sigma=0.0)), (z, dict(blur=True, blur_kernel_size=17)),   # 17 / 2 >= 8
                    (z, dict(as_mask=True, blur=True)), (z, dict(as_mask=True, mul=2.0)), (z, dict(as_mask=True, add=1.0))):
        with pytest.raises(ValueError):
            P.prep_frames(bad, **kw)
    for ok in (z, z[0], z[0, ..., 0].contiguous(), z.to(torch.uint8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P.prep_frames(ok, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.prep_frames(z, 4, as_mask=True)


def test_load_sequence_device_path_has_no_cpu_fallback(tmp_path):
    from gflow_amd import io as gio
    sp = _sequence(tmp_path, n=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gio.load_sequence(sp, device="cpu")
