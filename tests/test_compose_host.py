"""The row composer's host side (no GPU): the float64 restatement the device test compares against (tests/compose_ref.py), the
viewer's pure pieces around it -- load_labels, camera_at, slowmo, parse_edit, Edit -- and the argument checks of
gfl_compose_rows, which answer before anything touches a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from gflow_amd import _lib as L
from gflow_amd import viewer as V
from tests import compose_ref as CR
from tests.test_viewer_host import D, _rot, _training_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(n, seed):
    g = np.random.default_rng(seed)
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([g.normal(size=(n, 3)), g.uniform(0.01, 0.2, (n, 3)), q, g.uniform(0.05, 0.95, (n, 1)),
                           g.uniform(0, 1, (n, 3)), np.zeros((n, 2))], axis=1).astype(np.float32)


# ------------------------------------------------------------------ the restatement
def test_restatement_ends_are_the_source_rows():
    P = _rows(40, 1)
    for s, first in ((0.0, 0), (1.0, 20)):
        r = CR.compose_job(P, None, (0, 20, 20, 20), np.float32(s), None, 32)
        assert r["flag"] == 0 and r["kept"].tolist() == list(range(20))
        assert np.array_equal(r["rows"], P[first:first + 20].astype(np.float64))
    mid = CR.compose_job(P, None, (0, 20, 20, 20), np.float32(0.5), None, 32)["rows"]
    want = 0.5 * (P[:20].astype(np.float64) + P[20:40])
    assert np.allclose(mid[:, [0, 1, 2, 3, 4, 5, 10, 11, 12, 13]], want[:, [0, 1, 2, 3, 4, 5, 10, 11, 12, 13]], atol=1e-15)
    assert np.allclose(np.linalg.norm(mid[:, 6:10], axis=1), 1.0, atol=1e-14)


def test_restatement_identity_edit_and_hidden_groups():
    P = _rows(30, 2)
    labels = (np.arange(30) % 3).astype(np.uint8)
    plain = CR.compose_job(P, labels, (0, 30, 0, 30), np.float32(0.0), None, 30)
    ident = CR.compose_job(P, labels, (0, 30, 0, 30), np.float32(0.0), np.stack([CR.IDENTITY] * 3), 30)
    assert np.array_equal(plain["rows"], ident["rows"]) and np.array_equal(plain["rows"], P.astype(np.float64))
    # q = (-1, 0, 0, 0) is the same rotation: still no transform
    flipped = np.stack([CR.edit_row(q=(-1.0, 0.0, 0.0, 0.0))] * 3)
    assert np.array_equal(CR.compose_job(P, labels, (0, 30, 0, 30), np.float32(0.0), flipped, 30)["rows"], plain["rows"])
    # gain 0 on group 1 drops exactly its rows; a group beyond the table is left alone
    hide = np.stack([CR.IDENTITY, CR.edit_row(gain=0.0)])
    r = CR.compose_job(P, labels, (0, 30, 0, 30), np.float32(0.0), hide, 30)
    assert r["kept"].tolist() == [i for i in range(30) if i % 3 != 1]
    assert np.array_equal(r["rows"], P[r["kept"]].astype(np.float64))
    # gain is capped at 1, the tint is a lerp of the colour
    e = np.stack([CR.edit_row(gain=50.0, tint=(1.0, 0.0, 0.5), mix=0.25)])
    r = CR.compose_job(P, None, (0, 30, 0, 30), np.float32(0.0), e, 30)["rows"]
    assert np.array_equal(r[:, 10], np.minimum(P[:, 10].astype(np.float64) * 50.0, 1.0))
    assert np.allclose(r[:, 11:14], 0.75 * P[:, 11:14] + 0.25 * np.array([1.0, 0.0, 0.5]), atol=1e-15)
    assert np.array_equal(r[:, 0:10], P[:, 0:10].astype(np.float64))


def test_restatement_transform_about_a_pivot():
    P = _rows(10, 3)
    h = math.sqrt(0.5)
    e = np.stack([CR.edit_row(size=2.0, q=(h, 0.0, h, 0.0), pivot=(1.0, 2.0, 3.0), shift=(0.5, 0.0, 0.0))])
    r = CR.compose_job(P, None, (0, 10, 0, 10), np.float32(0.0), e, 10)["rows"]
    d = P[:, 0:3].astype(np.float64) - np.array([1.0, 2.0, 3.0])
    # a quarter turn about y: (x, y, z) -> (z, y, -x)
    want = np.array([1.0, 2.0, 3.0]) + 2.0 * np.stack([d[:, 2], d[:, 1], -d[:, 0]], axis=1) + np.array([0.5, 0.0, 0.0])
    assert np.allclose(r[:, 0:3], want, atol=1e-6)
    assert np.allclose(r[:, 3:6], 2.0 * P[:, 3:6], atol=0)
    assert np.allclose(np.linalg.norm(r[:, 6:10], axis=1), 1.0, atol=1e-14)
    Rq = CR.quat_matrix(np.array([h, 0.0, h, 0.0]))
    for k in range(10):
        assert np.allclose(CR.quat_matrix(r[k, 6:10]), Rq @ CR.quat_matrix(P[k, 6:10].astype(np.float64)), atol=1e-6)


def test_restatement_rows_of_one_frame_fade_and_the_quaternion_sign():
    P = _rows(50, 4)
    # 20 rows at frame a, 30 at frame b: the last ten fade in with s, and are gone at s = 0
    for s in (0.0, 0.25, 1.0):
        r = CR.compose_job(P, None, (0, 20, 20, 30), np.float32(s), None, 30)
        assert r["kept"].tolist() == list(range(30 if s > 0 else 20))
        if s > 0:
            assert np.array_equal(r["rows"][20:, 10], P[40:50, 10].astype(np.float64) * s)
            assert np.array_equal(np.delete(r["rows"][20:], 10, axis=1), np.delete(P[40:50].astype(np.float64), 10, axis=1))
    # the other way round the last ten fade out with 1 - s
    for s in (0.0, 0.25, 1.0):
        r = CR.compose_job(P, None, (20, 30, 0, 20), np.float32(s), None, 30)
        assert r["kept"].tolist() == list(range(30 if s < 1 else 20))
        if s < 1:
            assert np.array_equal(r["rows"][20:, 10], P[40:50, 10].astype(np.float64) * (1.0 - s))
    # b = -a: the same rotation, so every blend of the two is a (not a zero quaternion)
    Q = np.concatenate([P[:20], P[:20]])
    Q[20:, 6:10] *= -1
    r = CR.compose_job(Q, None, (0, 20, 20, 20), np.float32(0.5), None, 20)["rows"]
    assert np.allclose(r[:, 6:10], P[:20, 6:10], atol=1e-7)
    # a refused job keeps nothing
    for src in ((0, 20, 45, 10), (-1, 5, 0, 5), (0, 31, 0, 5)):
        r = CR.compose_job(P, None, src, np.float32(0.5), None, 30)
        assert r["flag"] == 2 and r["kept"].size == 0


# ------------------------------------------------------------------ labels
def test_load_labels():
    assert V.load_labels({"still_mask": None}, 5).tolist() == [0] * 5
    assert V.load_labels({}, 3).tolist() == [0] * 3
    mask = torch.tensor([True, False, False, True, True, False])
    lab = V.load_labels({"still_mask": mask}, 6)
    assert lab.dtype == torch.uint8 and lab.shape == (6,) and lab.tolist() == [0, 1, 1, 0, 0, 1]
    assert V.load_labels({"still_mask": mask}, 9).tolist() == [0, 1, 1, 0, 0, 1, 0, 0, 0]       # rows after the mask: still
    assert V.load_labels({"still_mask": mask}, 4).tolist() == [0, 1, 1, 0]
    assert V.load_labels({"still_mask": mask}, 0).shape == (0,)


# ------------------------------------------------------------------ time
def test_camera_at_ends_and_midpoint():
    E = _training_cameras()
    I = torch.stack([torch.tensor([100.0 + k, 90.0 - k, 48.0 + 0.5 * k, 32.0], dtype=D) for k in range(E.shape[0])])
    for t in range(E.shape[0]):
        e, i = V.camera_at(E, I, float(t))
        assert torch.equal(e, E[t]) and torch.equal(i, I[t])
        e, i = V.camera_at(E, I, t)
        assert torch.equal(e, E[t]) and torch.equal(i, I[t])
    # two cameras that differ by a rotation theta about one axis (camera -> world): the midpoint is theta / 2 about it
    theta, axis = 1.1, [0.3, -0.5, 0.8]
    A = V.quat_pos_to_extr(torch.tensor([0, 0, 0, 1], dtype=D), torch.tensor([0.0, 0.0, 0.0], dtype=D))
    c2w = _rot(axis, theta)
    B = torch.cat([c2w.T, -(c2w.T @ torch.tensor([[2.0], [0.0], [-1.0]], dtype=D))], dim=1)
    mid, intr = V.camera_at(torch.stack([A, B]), I[:2], 0.5)
    assert torch.allclose(mid[:, :3].T, _rot(axis, theta / 2), atol=1e-9)
    assert torch.allclose(V.extr_to_quat_pos(mid)[1], torch.tensor([1.0, 0.0, -0.5], dtype=D), atol=1e-9)
    assert torch.allclose(intr, 0.5 * (I[0] + I[1]), atol=1e-12)
    assert float((mid - V.lerp(A, B, 3)[1]).abs().max()) < 1e-12
    quarter = V.camera_at(torch.stack([A, B]), I[:2], 0.25)[0]
    assert torch.allclose(quarter[:, :3].T, _rot(axis, theta / 4), atol=1e-9)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            V.camera_at(torch.stack([A, B]), I[:2], bad)
    assert V.split_time(3.25, 6) == (3, 4, 0.25) and V.split_time(5, 6) == (5, 5, 0.0) and V.split_time(2.0, 6) == (2, 2, 0.0)


def test_slowmo_counts_and_exact_integral_times():
    for T, k in ((1, 3), (2, 1), (3, 3), (5, 4), (4, 7), (60, 4)):
        ts = V.slowmo(T, k)
        assert len(ts) == (T - 1) * k + 1 and ts[0] == 0.0 and ts[-1] == float(T - 1)
        assert all(b > a for a, b in zip(ts, ts[1:]))
        for f in range(T):
            assert ts[f * k] == float(f) and V.split_time(ts[f * k], T)[2] == 0.0
        assert all(abs(t - i / k) < 1e-12 for i, t in enumerate(ts))
    assert V.slowmo(3, 4) == [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
    for bad in ((0, 2), (3, 0)):
        with pytest.raises(ValueError):
            V.slowmo(*bad)


# ------------------------------------------------------------------ edits
def test_parse_edit_good_and_bad_texts():
    g, e = V.parse_edit("moving:shift=0.1,0,0;size=1.2;turn=y,30;tint=1,0,0,0.5;gain=0.5")
    assert g == 1 and e.shift == (0.1, 0.0, 0.0) and e.size == 1.2 and e.turn == ((0.0, 1.0, 0.0), 30.0)
    assert e.tint == (1.0, 0.0, 0.0) and e.mix == 0.5 and e.gain == 0.5 and e.pivot is None
    row = e.row()
    assert len(row) == 16 and row[0] == 0.5 and row[1] == 1.2 and row[9:12] == [0.1, 0.0, 0.0] and row[12:16] == [1.0, 0.0, 0.0, 0.5]
    assert np.allclose(row[2:6], [math.cos(math.radians(15)), 0.0, math.sin(math.radians(15)), 0.0], atol=1e-15)
    assert V.parse_edit("still:gain=0")[0] == 0 and V.parse_edit("still:gain=0")[1].gain == 0.0
    for k in range(8):
        assert V.parse_edit(f"{k}:size=2")[0] == k
    g, e = V.parse_edit("3:turn=1,1,0,90;pivot=1,2,3")
    assert g == 3 and e.pivot == (1.0, 2.0, 3.0)
    h = math.sqrt(0.5)
    assert np.allclose(e.quat(), [h, 0.5, 0.5, 0.0], atol=1e-15)
    # no edit at all is the identity of the library, exactly
    assert V.Edit().row() == CR.IDENTITY.tolist() and not V.Edit().moves()
    assert V.Edit(gain=0.3).hidden().gain == 0.0 and V.Edit(size=2.0).hidden().size == 2.0
    for bad in ("", "moving", "moving:", "spin:gain=1", "8:gain=1", "-1:gain=1", "moving:gain", "moving:gain=a", "moving:gain=1,2",
                "moving:shift=1,2", "moving:turn=w,30", "moving:turn=y", "moving:tint=1,0,0", "moving:colour=1", "moving:gain=1;gain=2",
                "moving:turn=0,0,0,30", "moving:size=nan", "01:gain=1", "moving:gain=1;"):
        with pytest.raises(ValueError) as err:
            V.parse_edit(bad)
        assert repr(bad) in str(err.value)


def test_a_layer_hides_the_other_group():
    assert V._with_layer("all", None) is None
    still = V._with_layer("still", None)
    assert sorted(still) == [0, 1] and still[1].gain == 0.0 and still[0].row() == CR.IDENTITY.tolist()
    moving = V._with_layer("moving", [("moving", V.Edit(shift=(0.1, 0.0, 0.0))), (0, V.Edit(size=3.0))])
    assert moving[0].gain == 0.0 and moving[0].size == 3.0 and moving[1].shift == (0.1, 0.0, 0.0) and moving[1].gain == 1.0
    with pytest.raises(ValueError):
        V._with_layer("both", None)
    with pytest.raises(ValueError):
        V._with_layer("all", [(1, V.Edit()), ("moving", V.Edit())])


# ------------------------------------------------------------------ gfl_compose_rows: signature and arguments
def test_ctypes_signatures_have_the_headers_arity():
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, restype in (("gfl_compose_rows_workspace_bytes", ctypes.c_size_t), ("gfl_compose_rows", ctypes.c_int)):
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        params = [p.strip() for p in m.group(2).split(",")]
        res, args = L.SIGNATURES[name]
        assert res is restype and len(args) == len(params), name
        for p, a in zip(params, args):
            want = ctypes.c_void_p if ("*" in p or p.startswith("gfl_stream_t")) else ctypes.c_size_t if p.startswith("size_t") else ctypes.c_int
            assert a is want, (name, p)


def test_compose_rows_workspace_grows_with_both_arguments():
    size = L.load().gfl_compose_rows_workspace_bytes
    b = size(4, 1000)
    assert b > 0
    assert size(8, 1000) > b and size(4, 2000) > b
    # at least: a keep bit per source row, a count and an offset per chunk of 256 rows
    assert b >= 4 * (1000 // 8 + 4 * 2 * 4)
    assert size(0, 1000) == 0 or size(0, 1000) < b
    for bad in ((-1, 1000), (4, -1), (1 << 20, 1 << 20)):
        assert size(*bad) == 0


def test_compose_rows_rejects_bad_arguments_before_touching_a_device():
    lib = L.load()
    INVALID = -1
    mem = (ctypes.c_char * 4096)()                           # host bytes: a rejected call reads none of its pointers
    p = ctypes.c_void_p(ctypes.addressof(mem))
    J, rows_max = 2, 100
    ws = lib.gfl_compose_rows_workspace_bytes(J, rows_max)
    good = dict(params=p, labels=p, R=100, job_src=p, job_s=p, job_edit=p, G=2, J=J, rows_max=rows_max, out_rows=p, out_job_rows=p,
                flags=p, workspace=p, workspace_bytes=ws, stream=None)
    bads = [dict(J=-1), dict(R=-1), dict(rows_max=-1), dict(G=0), dict(G=9), dict(G=-3), dict(params=None), dict(job_src=None),
            dict(job_s=None), dict(out_rows=None), dict(out_job_rows=None), dict(flags=None), dict(workspace=None),
            dict(workspace_bytes=ws - 1), dict(workspace_bytes=0), dict(J=1 << 20, rows_max=1 << 20)]
    for bad in bads:
        assert lib.gfl_compose_rows(*{**good, **bad}.values()) == INVALID, bad
    # no jobs: success, nothing written, nothing needed
    none = {**good, **dict(J=0, params=None, labels=None, job_src=None, job_s=None, job_edit=None, out_rows=None,
                           out_job_rows=None, flags=None, workspace=None, workspace_bytes=0)}
    assert lib.gfl_compose_rows(*none.values()) == 0
    assert lib.gfl_compose_rows(*{**none, "job_edit": p, "G": 0}.values()) == INVALID
    assert lib.gfl_compose_rows(*{**none, "R": -1}.values()) == INVALID
    assert bytes(mem) == bytes(4096)
