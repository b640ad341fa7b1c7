"""CPU: the numpy restatement of the DAVIS counts and scores (tests/seg_ref.py) and segmentation.scores_from_counts against
J and F captured from the reference (tests/golden/davis_seg.npz, make_seg_golden.py); bound_pix; the recorder's carry-over
and invalid-frame rules on hand-made inputs, with the device scoring replaced by the restatement; fit_video.reduce_davis
on hand-written clip scores, alone and over a 2-rank gloo group."""
import math
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

from gflow_amd import fit_video as FV
from gflow_amd import segmentation as SG
from tests import seg_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "davis_seg.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def cases(gold):
    for i in range(int(gold["n_cases"])):
        p = f"c{i}_"
        pred, gt = gold[p + "pred"], gold[p + "gt"]
        yield (str(gold["names"][i]), pred, gt, SG.bound_pix(*pred.shape, float(gold[p + "bound_th"])), float(gold[p + "J"]),
               float(gold[p + "F"]))


def test_restatement_equals_the_reference(gold):
    names = []
    for name, pred, gt, radius, J, F in cases(gold):
        j, f = R.scores(R.counts(pred, gt, radius))
        assert j == J and f == F, (name, j, J, f, F)
        names.append(name)
    assert len(names) == 12
    for shape in ("37x53", "70x130", "64x65", "65x64", "1x200", "2x2"):
        assert any(n.startswith(shape) for n in names)


def test_scores_from_counts_equal_the_reference(gold):
    rows, want = [], []
    for name, pred, gt, radius, J, F in cases(gold):
        rows.append(R.counts(pred, gt, radius))
        want.append((J, F))
    J, F, JF = SG.scores_from_counts(np.stack(rows))
    assert J.dtype == F.dtype == JF.dtype == np.float64
    want = np.array(want)
    assert (J == want[:, 0]).all() and (F == want[:, 1]).all()
    assert (JF == (want[:, 0] + want[:, 1]) / 2).all()


def test_score_branches():
    # inter, uni, n_fg, n_gt, fg_match, gt_match
    c = np.array([[0, 0, 0, 0, 0, 0],         # both empty: J = 1, p = r = 1
                  [0, 9, 0, 7, 0, 0],         # empty prediction: p = 1, r = 0
                  [0, 9, 7, 0, 0, 0],         # empty ground truth: p = 0, r = 1
                  [0, 9, 5, 5, 0, 0],         # disjoint: p + r = 0 -> F = 0
                  [1, 3, 4, 8, 2, 2]])
    J, F, JF = SG.scores_from_counts(c)
    assert J.tolist() == [1.0, 0.0, 0.0, 0.0, float(np.int64(1) / np.float32(3))]
    assert F.tolist() == [1.0, 0.0, 0.0, 0.0, 2 * 0.5 * 0.25 / 0.75]
    # the float32 divisor: np.int64 / np.float32 is a float64 quotient (a Python int over np.float32 would be float32)
    assert J[4] == 1 / 3 and J[4] != float(1 / np.float32(3))
    big = np.array([[12345677, 16777217 + 2, 0, 0, 0, 0]])       # a union float32 cannot hold: it rounds, as in the reference
    assert SG.scores_from_counts(big)[0][0] == 12345677 / float(np.float32(16777219))


def test_bound_pix():
    assert SG.bound_pix(480, 854) == 8
    assert SG.bound_pix(37, 53) == 1 and SG.bound_pix(37, 53, 3) == 3 and SG.bound_pix(1, 200) == 2
    assert isinstance(SG.bound_pix(480, 854), int)
    with pytest.raises(ValueError):
        SG.bound_pix(480, 854, 2.5)


def _ring(cx, cy, r, n=40):
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1).astype(np.float32)


def _stub_scoring(monkeypatch):
    calls = []

    def seg_counts(pred, gt, radius, valid=None):
        calls.append(radius)
        return R.counts_stack(pred.numpy(), gt.numpy(), radius, None if valid is None else valid.numpy())

    monkeypatch.setattr(SG, "seg_counts", seg_counts)
    return calls


def test_recorder_carries_a_mask_over_a_frame_with_few_points(monkeypatch):
    from gflow_amd.hull import FastConcaveHull2D
    calls = _stub_scoring(monkeypatch)
    H, W, T = 48, 64, 4
    rec = SG.MoveSegRecorder(T, H, W, "cpu")
    pts = [_ring(20, 20, 10), _ring(30, 22, 9), _ring(40, 24, 8), _ring(44, 24, 8)]
    still = np.array([[5.0, 5.0], [60.0, 40.0]], np.float32)              # rows that are not selected
    for t in range(T):
        uv = np.concatenate([still, pts[t]])
        sel = np.concatenate([[False, False], np.ones(len(pts[t]), bool)])
        if t == 1:
            sel[7:] = False                                               # five selected points: no hull, the mask stays
            assert sel.sum() == 5
        if t == 2:
            continue                                                      # a frame without a joint stage: the mask stays
        rec.frame = t
        rec.record(torch.from_numpy(uv), torch.from_numpy(sel))
    yy, xx = np.mgrid[0:H, 0:W]
    gts = [torch.from_numpy((xx - 20 - 8 * t) ** 2 + (yy - 20) ** 2 <= 100) for t in range(T)]
    out = rec.result(gts)
    m0 = (FastConcaveHull2D(pts[0]).mask(W, H) * 255).astype(np.uint8)
    m3 = (FastConcaveHull2D(pts[3]).mask(W, H) * 255).astype(np.uint8)
    assert out["masks"].dtype == np.uint8 and out["masks"].shape == (T, H, W)
    assert out["valid"].tolist() == [True] * 4
    for t, want in enumerate((m0, m0, m0, m3)):
        np.testing.assert_array_equal(out["masks"][t], want)
    assert not np.array_equal(m0, m3) and m0.max() == 255
    assert calls == [SG.bound_pix(H, W)]                                  # one scoring call for the clip
    want = R.counts_stack(out["masks"], np.stack([g.numpy() for g in gts]), calls[0])
    np.testing.assert_array_equal(out["counts"], want)
    assert out["counts"].dtype == np.int64
    for t in range(T):
        j, f = R.scores(want[t])
        assert out["J"][t] == j and out["F"][t] == f and out["JF"][t] == (j + f) / 2
    ev = SG.evaluate(out)
    assert ev["frames_scored"] == 4 and ev["J"] == float(np.mean(out["J"])) and ev["J&F"] == float(np.mean(out["JF"]))
    assert out["J"][0] > 0.8 and out["J"][2] < out["J"][0]               # (the carried mask falls behind the moving disc)


def test_recorder_marks_leading_frames_without_a_mask_invalid(monkeypatch):
    _stub_scoring(monkeypatch)
    H, W, T = 32, 40, 3
    rec = SG.MoveSegRecorder(T, H, W, "cpu")
    few = _ring(10, 10, 5, n=5)
    for t, p in enumerate((few, few, _ring(20, 16, 8))):
        rec.frame = t
        rec.record(torch.from_numpy(p), torch.ones(len(p), dtype=torch.bool))
    gts = [torch.zeros(H, W, dtype=torch.bool)] * T
    out = rec.result(gts)
    assert out["valid"].tolist() == [False, False, True]
    assert not out["masks"][:2].any() and out["masks"][2].any()
    assert not out["counts"][:2].any() and out["counts"][2].any()
    assert out["J"][:2].tolist() == [0.0, 0.0] and out["F"][:2].tolist() == [0.0, 0.0]
    ev = SG.evaluate(out)
    assert ev["frames_scored"] == 1 and ev["J"] == out["J"][2] and ev["F"] == out["F"][2]
    # nothing recorded at all: nothing scored
    empty = SG.MoveSegRecorder(T, H, W, "cpu").result(gts)
    assert not empty["valid"].any() and SG.evaluate(empty)["frames_scored"] == 0 and np.isnan(SG.evaluate(empty)["J"])
    with pytest.raises(ValueError):
        rec.result(gts[:2])


def _seg(J, F, valid=None):
    J, F = np.asarray(J, np.float64), np.asarray(F, np.float64)
    return dict(J=J, F=F, JF=(J + F) / 2, valid=np.ones(len(J), bool) if valid is None else np.asarray(valid, bool))


# clip 0: J 0.625, F 0.375, J&F 0.5 over 2 frames; clip 2: no scored frame; clip 5: J 0.1875, F 0.5625, J&F 0.375 over 2
SEGS = {0: _seg([0.5, 0.75], [0.25, 0.5]), 2: _seg([0.0, 0.0], [0.0, 0.0], valid=[False, False]),
        5: _seg([0.875, 0.25, 0.125], [0.875, 0.75, 0.375], valid=[False, True, True])}
DAVIS = {"J": (0.625 + 0.1875) / 2, "F": (0.375 + 0.5625) / 2, "J&F": (0.5 + 0.375) / 2, "frames_scored": 4, "clips": 2}


def test_reduce_davis_averages_over_the_clips_with_a_scored_frame():
    out = FV.reduce_davis(SEGS)
    assert out == DAVIS and list(out) == ["J", "F", "J&F", "frames_scored", "clips"]
    assert type(out["frames_scored"]) is int and type(out["clips"]) is int and type(out["J"]) is float
    assert FV.reduce_davis({0: SEGS[0]}) == {"J": 0.625, "F": 0.375, "J&F": 0.5, "frames_scored": 2, "clips": 1}
    for none in (FV.reduce_davis({}), FV.reduce_davis({2: SEGS[2]})):          # nothing to average: NaN, zero totals
        assert none["frames_scored"] == 0 and none["clips"] == 0
        assert all(type(none[k]) is float and math.isnan(none[k]) for k in ("J", "F", "J&F"))


def _davis_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    segs = {0: SEGS[0], 5: SEGS[5]} if rank == 0 else {2: SEGS[2]}             # rank 1 holds no scored clip
    out = FV.reduce_davis(segs, dist, torch.device("cpu"))
    dist.destroy_process_group()
    q.put((rank, out))


def test_reduce_davis_over_two_rank_gloo():
    """the mean over the clips of all ranks (rank 1's own mean does not exist), the same dict on every rank"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_davis_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert outs[0] == outs[1] == DAVIS == FV.reduce_davis(SEGS)
