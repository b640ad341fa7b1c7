"""The flow score's host side (gflow_amd/flow.py, fit_video.reduce_flow, tests/flow_ref.py) without a device: the pooled
numbers and their NaN rules, the reduction over a 2-rank gloo group, the .flo round trip with Middlebury's unknown-flow
mark, and the restatement's own known answers in float64."""
import math
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

from gflow_amd import flow as FL
from gflow_amd import fit_video as FV
from gflow_amd import io as gio
from tests import flow_ref as R


def _result(sums):
    s = np.asarray(sums, np.float64).reshape(-1, 3, 6)
    return dict(sums=s, **FL.scores_from_sums(s))


#            n_pixels n_valid epe_sum n<1 n<3 n<5
PAIR_A = [[100, 80, 40.0, 60, 70, 80], [70, 60, 12.0, 55, 60, 60], [30, 20, 28.0, 5, 10, 20]]
PAIR_B = [[100, 20, 60.0, 0, 10, 15], [100, 20, 60.0, 0, 10, 15], [0, 0, 0.0, 0, 0, 0]]


def test_scores_per_pair_and_pooled_evaluate():
    r = _result([PAIR_A, PAIR_B])
    assert r["EPE"].shape == (2, 3) and r["EPE"].dtype == np.float64
    np.testing.assert_array_equal(r["EPE"][0], [0.5, 0.2, 1.4])
    np.testing.assert_array_equal(r["coverage"][0], [0.8, 60 / 70, 20 / 30])
    np.testing.assert_array_equal(r["acc_3px"][1][:2], [0.5, 0.5])
    assert np.isnan(r["EPE"][1, 2]) and np.isnan(r["coverage"][1, 2]) and np.isnan(r["acc_1px"][1, 2])    # nothing to count
    ev = FL.evaluate(r)
    # sums over sums: every valid pixel once, NOT the mean of the pairs' ratios
    assert ev == {"EPE": 100.0 / 100, "EPE_still": 72.0 / 80, "EPE_moving": 28.0 / 20, "acc_1px": 60 / 100, "acc_3px": 80 / 100,
                  "acc_5px": 95 / 100, "coverage": 100 / 200, "pairs": 2}
    assert ev["EPE"] != np.mean(r["EPE"][:, 0])


def test_evaluate_of_nothing_is_nan():
    ev = FL.evaluate(_result(np.zeros((0, 3, 6))))
    assert ev["pairs"] == 0 and all(math.isnan(ev[k]) for k in FL.EVAL_KEYS)
    ev = FL.evaluate(_result([PAIR_B]))                  # no moving pixel; a NULL mask leaves classes 1 and 2 zero
    assert math.isnan(ev["EPE_moving"]) and ev["EPE_still"] == 3.0 and ev["coverage"] == 0.2
    nomask = np.array(PAIR_A, np.float64)
    nomask[1:] = 0
    ev = FL.evaluate(_result([nomask]))
    assert ev["EPE"] == 0.5 and math.isnan(ev["EPE_still"]) and math.isnan(ev["EPE_moving"])


def test_recorder_refuses_bad_arguments_before_touching_a_device():
    for kw in (dict(min_weight=0.0), dict(min_weight=1.5), dict(min_weight=float("nan"))):
        with pytest.raises(ValueError):
            FL.FlowRecorder(3, 32, 32, "cpu", **kw)
    with pytest.raises(ValueError):
        FL.FlowRecorder(0, 32, 32, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FL.FlowRecorder(3, 32, 32, "cpu")
    from gflow_amd import _lib
    lib = _lib.load()
    assert lib.gfl_flow_workspace_bytes(70, 45) == 5 * 3 * 18 * 8
    assert lib.gfl_flow_workspace_bytes(0, 45) == 0 and lib.gfl_flow_workspace_bytes(16 * 16385, 16) == 0
    assert lib.gfl_flow_pair(None, 0, None, None, None, 2, None, 1, 0, None, None, 8, 8, 0.5, 0, 1, None, None, None, None, 0,
                             None) == -1               # refused before any launch


def test_reduce_flow_averages_over_clips():
    flows = {0: _result([PAIR_A, PAIR_B]), 4: _result([PAIR_B]), 5: _result(np.zeros((0, 3, 6)))}
    out = FV.reduce_flow(flows)
    a, b = FL.evaluate(flows[0]), FL.evaluate(flows[4])
    assert out["pairs"] == 3 and out["clips"] == 2
    for k in ("EPE", "EPE_still", "acc_1px", "acc_3px", "acc_5px", "coverage"):
        assert out[k] == (a[k] + b[k]) / 2, k
    assert out["EPE_moving"] == a["EPE_moving"]        # the one clip that has a moving valid pixel
    none = FV.reduce_flow({5: flows[5]})
    assert none["clips"] == 0 and none["pairs"] == 0 and all(none[k] is None for k in FV.FLOW_KEYS)
    assert "flow" not in FV.csv_metrics({"flow": out}) and FV.csv_metrics({"flow": out}) == {}    # metrics.csv has no flow key


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    flows = {0: _result([PAIR_A, PAIR_B])} if rank == 0 else {1: _result([PAIR_B]), 2: _result(np.zeros((0, 3, 6)))}
    out = FV.reduce_flow(flows, dist, torch.device("cpu"))
    dist.destroy_process_group()
    q.put((rank, out))


def test_reduce_flow_over_two_rank_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = FV.reduce_flow({0: _result([PAIR_A, PAIR_B]), 1: _result([PAIR_B]), 2: _result(np.zeros((0, 3, 6)))})
    assert outs[0] == outs[1] == want
    assert want["clips"] == 2 and want["pairs"] == 3


def test_flo_round_trip_with_the_unknown_flow_mark(tmp_path):
    rng = np.random.default_rng(0)
    maps = rng.normal(0, 3, (2, 9, 5, 2)).astype(np.float32)
    valid = rng.random((2, 9, 5)) < 0.7
    maps[~valid] = 0                                     # (as the kernel leaves them)
    paths = FL.write_flo_maps(str(tmp_path / "clip_0"), dict(maps=maps, valid=valid))
    assert [os.path.basename(p) for p in paths] == ["flow_00000.flo", "flow_00001.flo"]
    for t, p in enumerate(paths):
        back = gio.read_flow(p).numpy()
        assert back.shape == (9, 5, 2) and back.dtype == np.float32
        np.testing.assert_array_equal(back[valid[t]], maps[t][valid[t]])
        assert (back[~valid[t]] == np.float32(1e10)).all()
        assert (np.abs(back[valid[t]]) < 1e9).all()        # (Middlebury: a component above 1e9 means unknown)
    with pytest.raises(ValueError):
        FL.write_flo_maps(str(tmp_path / "x"), dict(sums=np.zeros((1, 3, 6))))


def test_pack_records_layout():
    uv, conic = torch.tensor([[1.0, 2.0]]), torch.tensor([[3.0, 4.0, 5.0]])
    rec = FL.pack_records(uv, conic, torch.tensor([[0.5]]), torch.tensor([[7.0]]))
    assert rec.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0, 0.5, 0, 0, 0, 7.0, 0, 0]]


# ------------------------------------------------------------------------------------ the restatement's known answers
def _ref(case, **kw):
    return R.flow_pair(case["rec_a"], case["ids"], case["tile_range"], case["uv_b"], case["depth_b"], case["gt_flow"], None,
                       case["W"], case["H"], **kw)


def test_restatement_one_splat():
    c = R.known_case("one")
    r = _ref(c)
    ys, xs = np.nonzero(r["valid"])
    assert sorted(zip(xs.tolist(), ys.tolist())) == [(7, 8), (8, 7), (8, 8), (8, 9), (9, 8)]
    np.testing.assert_allclose(r["flow"][r["valid"]], np.tile(c["d"][0], (5, 1)), rtol=0, atol=1e-14)
    assert r["den"][8, 8] == pytest.approx(0.99, abs=1e-7) and r["den"][8, 9] == pytest.approx(math.exp(-0.5), abs=1e-12)
    assert r["den"][9, 9] == pytest.approx(math.exp(-1.0), abs=1e-12) and not r["valid"][9, 9]
    assert (r["flow"][~r["valid"]] == 0).all()
    s = r["sums"]
    assert s[0, 0] == 18 * 18 and s[0, 1] == 5 and s[0, 2] == pytest.approx(5 * math.sqrt(5.0), rel=1e-14)
    assert s[0, 3] == 0 and s[0, 4] == 5 and s[0, 5] == 5 and (s[1:] == 0).all()


def test_restatement_two_splats_and_a_culled_one():
    c = R.known_case("two")
    o = float(np.float32(0.8))
    r = _ref(c)
    w1, w2 = o, o * (1 - o)
    want = (w1 * c["d"][0] + w2 * c["d"][1]) / (w1 + w2)
    np.testing.assert_allclose(r["flow"][8, 8], want, rtol=1e-14)
    assert r["den"][8, 8] == pytest.approx(w1 + w2, rel=1e-14)
    c = R.known_case("two_culled")
    r = _ref(c)
    np.testing.assert_allclose(r["flow"][8, 8], c["d"][0], rtol=1e-14)
    assert r["den"][8, 8] == pytest.approx(w1, rel=1e-14)
    # a row without a future still occludes: behind a culled NEAR splat the far one weighs o (1 - o), below min_weight
    c["depth_b"] = np.array([0.0, 2.0], np.float32)
    c["uv_b"] = c["rec_a"][:, 0:2] + np.array([[0, 0], [0, 4]], np.float32)
    r = _ref(c)
    assert r["den"][8, 8] == pytest.approx(w2, rel=1e-14) and not r["valid"][8, 8]
    r = _ref(c, min_weight=0.1)
    np.testing.assert_allclose(r["flow"][8, 8], [0.0, 4.0], rtol=1e-14)


def test_restatement_on_scattered_lists_and_no_rows():
    p = R.random_pair(200, 40, 30, seed=1)
    gt = np.zeros((30, 40, 2), np.float32)
    a = R.flow_pair(p["rec_a"], p["ids"], p["tile_range"], p["uv_b"], p["depth_b"], gt, None, 40, 30)
    ids2, tr2 = R.shuffled_lists(p["ids"], p["tile_range"], seed=3)
    assert ids2.shape[0] > p["ids"].shape[0] and (tr2 != p["tile_range"]).any()
    b = R.flow_pair(p["rec_a"], ids2, tr2, p["uv_b"], p["depth_b"], gt, None, 40, 30)
    np.testing.assert_array_equal(a["flow"], b["flow"])
    np.testing.assert_array_equal(a["valid"], b["valid"])
    assert 0.3 < a["valid"].mean() < 1.0
    e = R.flow_pair(np.zeros((0, 12), np.float32), ids2, tr2, p["uv_b"], p["depth_b"], gt, None, 40, 30)
    assert not e["valid"].any() and e["sums"][0, 0] == 1200 and (e["sums"].reshape(-1)[1:] == 0).all()


def test_sums_from_maps_classes_and_nan_targets():
    H, W = 12, 20
    ref = np.zeros((H, W, 2))
    gt, mask = R.test_targets(ref, W, H)
    valid = np.isfinite(gt).all(-1)
    valid[0, :] = False
    s = R.sums_from_maps(ref, valid, gt, mask)
    assert s[0, 0] == H * W and s[1, 0] + s[2, 0] == H * W and s[2, 0] == mask.sum() > 0
    np.testing.assert_array_equal(s[0, [1, 3, 4, 5]], (s[1] + s[2])[[1, 3, 4, 5]])
    assert s[0, 2] == pytest.approx(s[1, 2] + s[2, 2], rel=1e-13)
    assert 0 < s[0, 3] < s[0, 4] < s[0, 5] == s[0, 1] and np.isfinite(s).all()
    s0 = R.sums_from_maps(ref, valid, gt, None)
    np.testing.assert_array_equal(s0[0], s[0])
    assert (s0[1:] == 0).all()
