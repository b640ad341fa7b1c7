"""The flow and label kernels walk a tile's list as the operator blend does, bit for bit (``-m gpu``;
operator_tile_walk, csrc/gfl_splat_alpha.hpp).

What the tracker, the flow score and the object maps assume -- a pixel is made of the same splats with the same weights as
in the render -- is pinned here as an identity between launches: given the splat's motion, or the one-hot of its label,
as the blend's FEATURE, ``msplat.alpha_blending`` leaves the very sums the other two kernels form, so their outputs follow
from its planes by one float32 division and a comparison on the host.  Every pixel is compared, none is left out:

- flow: the blend adds ``fmaf(f, w, acc)`` with f = (dx, dy, 1), the flow kernel ``fmaf(w, dx, nx)``, ``fmaf(w, dy, ny)`` and
  ``den += w`` -- the same roundings (a product by 1 is exact); the background term ``fmaf(T, 0, acc)`` is ``acc``;
- labels: f is 0 or 1, so the blend's plane k is the label kernel's ``acc[k] += w`` over the rows of class k;
- both divide once, correctly rounded (the library is built without fast-math), as numpy does.

The scenes: tests/label_ref.py's (tile 0's list crosses the 256-record staging batch, pixels of tile 1 reach the T_MIN
stop, rows outside the image and behind the camera) and a 9 x 5 image, one tile in which every wave has lanes outside.
The records come from ``flow.operator_state``: the floats the blend reads from its separate arrays."""
import functools

import numpy as np
import pytest
import torch

from tests import label_ref as LR
from tests import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_WEIGHT = 0.5
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _state(name):
    """a scene through the five operators on the device, computed once and never written to: dict(rec, n, ids, tr, W, H)
    and the blend's own views of the records (uv, conic, opacity)"""
    from gflow_amd import flow as FL
    s = LR.label_scene() if name == "label" else scenes.random_scene(60, 9, 5, seed=2)
    W, H = s["W"], s["H"]
    d = lambda k: s[k].to(DEV)
    with torch.no_grad():
        rec, n, ids, tr = FL.operator_state([d("xyz"), d("scale"), d("rotate"), d("opacity"), d("rgb"), d("intr"), d("extr"),
                                             0.0, W, H])
    torch.cuda.synchronize()
    return dict(rec=rec, n=n, ids=ids.contiguous(), tr=tr.contiguous(), W=W, H=H, uv=rec[:, 0:2].contiguous(),
                conic=rec[:, 2:5].contiguous(), opacity=rec[:, 5:6].contiguous())


def _blend(st, feature):
    """(C, H, W) float32 on the host: the operator blend of ``feature`` (n, C) over a zero background"""
    import gflow_amd.msplat as ms
    with torch.no_grad():
        out = ms.alpha_blending(st["uv"], st["conic"], st["opacity"], torch.from_numpy(np.ascontiguousarray(feature, f32)).to(DEV),
                                st["ids"], st["tr"], 0.0, st["W"], st["H"])
    return out.cpu().numpy()


def _check_scene(name, st):
    lens = (st["tr"][:, 1] - st["tr"][:, 0]).cpu().numpy()
    if name == "label":
        assert st["n"] == LR.N_FAINT + LR.N_OPAQUE + LR.N_REST and lens[0] >= 300      # across the staging batch
        assert int((st["rec"][:, 9] == 0).sum()) >= 5                                  # rows that are in no list
    else:
        assert len(lens) == 1 and 0 < lens[0] <= 256                                   # one tile, 45 of its 256 lanes inside


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


@pytest.mark.parametrize("name", ["label", "9x5"])
def test_flow_is_the_blend_of_the_motion(name):
    from gflow_amd import _lib as L
    lib = L.load()
    st = _state(name)
    _check_scene(name, st)
    n, W, H = st["n"], st["W"], st["H"]
    uv_a = st["uv"].cpu().numpy()
    rng = np.random.default_rng(7)
    uv_b = (uv_a + rng.uniform(-3.0, 3.0, (n, 2)).astype(f32)).astype(f32)
    d = uv_b - uv_a                                                                    # float32: the kernel's own subtraction
    planes = _blend(st, np.concatenate([d, np.ones((n, 1), f32)], axis=1))
    uv_b_d, depth_b = torch.from_numpy(uv_b).to(DEV), torch.ones(n, dtype=torch.float32, device=DEV)
    gt = torch.zeros(H, W, 2, dtype=torch.float32, device=DEV)
    sums = torch.zeros(1, 3, 6, dtype=torch.float64, device=DEV)
    flow = torch.full((H, W, 2), -7.0, dtype=torch.float32, device=DEV)
    valid = torch.full((H, W), 7, dtype=torch.uint8, device=DEV)
    ws = L.scratch(lib.gfl_flow_workspace_bytes(W, H), DEV)
    L.check(lib.gfl_flow_pair(L.ptr(st["rec"]), n, L.ptr(st["ids"]), L.ptr(st["tr"]), L.ptr(uv_b_d), 2, L.ptr(depth_b), 1, n,
                              L.ptr(gt), None, W, H, MIN_WEIGHT, 0, 1, L.ptr(sums), L.ptr(flow), L.ptr(valid), L.ptr(ws),
                              ws.numel(), L.stream()), "flow pair")
    flow, valid = flow.cpu().numpy(), valid.cpu().numpy()
    want_valid = planes[2] >= f32(MIN_WEIGHT)
    print(f"flow = blend, {name}: valid {float(want_valid.mean()):.3f}, den {planes[2].min():.3g} .. {planes[2].max():.3g}")
    np.testing.assert_array_equal(valid, want_valid.astype(np.uint8))
    assert want_valid.any()
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(want_valid[..., None], np.stack([planes[0] / planes[2], planes[1] / planes[2]], axis=-1), f32(0))
    np.testing.assert_array_equal(_bits(flow), _bits(want))


def _labels(name, n, K):
    if name == "label":
        return LR.scene_labels(n, K)
    rng = np.random.default_rng(3 + K)
    lab = rng.integers(0, K, n - 5).astype(np.uint8)
    lab[rng.random(n - 5) < 0.1] = LR.NONE
    return lab, n - 5


@pytest.mark.parametrize("K", [2, 5, 16])
def test_labels_are_the_blend_of_the_one_hot_classes(K):
    from gflow_amd import _lib as L
    lib = L.load()
    for name in ("label", "9x5"):
        st = _state(name)
        _check_scene(name, st)
        n, W, H = st["n"], st["W"], st["H"]
        lab, n_labels = _labels(name, n, K)
        hot = np.zeros((n, K), f32)                                                    # an unlabelled row: all zeros
        rows = np.nonzero(lab < K)[0]
        hot[rows, lab[rows]] = 1
        planes = _blend(st, hot)
        out = torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
        conf = torch.full((H, W), -1.0, dtype=torch.float32, device=DEV)
        lab_d = torch.from_numpy(lab).to(DEV)
        L.check(lib.gfl_label_frame(L.ptr(st["rec"]), n, L.ptr(st["ids"]), L.ptr(st["tr"]), L.ptr(lab_d), n_labels, K, W, H, MIN_WEIGHT, LR.NONE, L.ptr(out), L.ptr(conf), L.stream()), "label frame")
        out, conf = out.cpu().numpy(), conf.cpu().numpy()
        den, best, arg = planes[0].copy(), planes[0].copy(), np.zeros((H, W), np.int64)
        for k in range(1, K):                                                          # ascending, in float32
            den = den + planes[k]
            more = planes[k] > best                                                    # strict: the smallest k among equals
            best, arg = np.where(more, planes[k], best), np.where(more, k, arg)
        assert den.dtype == f32 and best.dtype == f32
        known = den >= f32(MIN_WEIGHT)
        print(f"label = blend, {name}, K = {K}: known {float(known.mean()):.3f}, classes seen {np.unique(arg[known]).tolist()}")
        np.testing.assert_array_equal(out, np.where(known, arg, LR.NONE).astype(np.uint8))
        if name == "label":
            assert known.any() and not known.all()
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(known, best / den, f32(0))
        np.testing.assert_array_equal(_bits(conf), _bits(want))
