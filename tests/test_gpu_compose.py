"""The row composer gfl_compose_rows (include/gflow_hip.h), render.render_composed on top of it and the viewer's in-between
frames, layers and edits (``-m gpu``).  The reference is the float64 restatement tests/compose_ref.py; the frame is 96 x 64 and
the row counts are where a compaction by chunks of 256 rows and waves of 64 can break: 0, 1, 63, 64, 65, 1023, 1024, 1025, 2500."""
import math
import os

import numpy as np
import pytest
import torch

from tests import compose_ref as CR
from tests.scenes import random_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = 96, 64
COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2500)
NA, NC = 2500, 1100                      # rows of frames a and b; rows of the frame whose quaternions are a's negated
R_ALL = 2 * NA + NC
U = 2.0 ** -24
SENTINEL = -12345.678


def _block(s):
    n = s["xyz"].shape[0]
    return torch.cat([s[k].float().reshape(n, -1) for k in ("xyz", "scale", "rotate", "opacity", "rgb")] + [torch.zeros(n, 2)], dim=1)


@pytest.fixture(scope="module")
def clip():
    """Three 'frames' in one block: a (rows 0 .. 2499), b = a slightly moved (2500 .. 4999: positions, sizes, opacities and
    colours perturbed, quaternions perturbed by 0.05 so that |dot| > 0.1) and c = a's first 1100 rows with the quaternions
    negated (5000 .. 6099).  Opacities stay >= 1e-3.  Labels 0 .. 3 by row index; group 1 -- the group the tables hide --
    holds the rows on both sides of the boundaries 64, 256 and 1024."""
    sc = random_scene(NA, W, H, seed=21, sigma_px=2.5, behind=0.0)
    a = _block(sc)
    g = torch.Generator().manual_seed(22)
    b = a.clone()
    b[:, 0:3] += 0.02 * torch.randn(NA, 3, generator=g)
    b[:, 3:6] *= 1.0 + 0.1 * (torch.rand(NA, 3, generator=g) - 0.5)
    b[:, 6:10] = torch.nn.functional.normalize(a[:, 6:10] + 0.05 * torch.randn(NA, 4, generator=g), dim=1)
    b[:, 10] = (a[:, 10] + 0.1 * (torch.rand(NA, generator=g) - 0.5)).clamp(1e-3, 0.999)
    b[:, 11:14] = (a[:, 11:14] + 0.1 * (torch.rand(NA, 3, generator=g) - 0.5)).clamp(0.0, 1.0)
    c = a[:NC].clone()
    c[:, 6:10] = -c[:, 6:10]
    block = torch.cat([a, b, c]).contiguous()
    assert float(block[:, 10].min()) >= 1e-3 and float((a[:, 6:10] * b[:, 6:10]).sum(1).abs().min()) > 0.1
    idx = torch.arange(NA)
    lab = (idx % 4).to(torch.uint8)
    lab[(idx % 7) == 3] = 1
    for edge in (64, 256, 1024):
        lab[edge - 2:edge + 2] = 1
    lab[60] = 1; lab[61] = 0; lab[66] = 2; lab[1021] = 3
    labels = torch.cat([lab, lab, lab[:NC]]).contiguous()
    return dict(block=block, labels=labels, intr=sc["intr"], extr=sc["extr"])


def _quat(axis, degrees):
    n = math.sqrt(sum(x * x for x in axis))
    h = math.radians(degrees) / 2
    return (math.cos(h),) + tuple(math.sin(h) * x / n for x in axis)


HIDE = CR.edit_row(gain=0.0)
TINT = CR.edit_row(gain=0.5, tint=(1.0, 0.2, 0.0), mix=0.3)
MOVE = CR.edit_row(gain=1.5, size=1.3, q=_quat((0.2, 1.0, -0.3), 30.0), pivot=(0.1, -0.2, 2.5), shift=(0.1, 0.0, -0.05))
TABLES = (np.stack([TINT, HIDE, MOVE]), np.stack([MOVE, HIDE, TINT]))          # G = 3: rows of group 3 are left alone


def run_compose(block, labels, src, s, table, rows_max, guard=1 << 12):
    """gfl_compose_rows through ctypes on device copies; out_rows is filled with SENTINEL before the call.
    dict(rc, rows (J * rows_max, 16), job_rows (J, 2), flags (J,), guard_ok)"""
    from gflow_amd import _lib as L
    lib = L.load()
    J = len(src)
    blk = block.float().contiguous().to(DEV)
    lab = None if labels is None else labels.contiguous().to(DEV)
    d_src = torch.tensor(src, dtype=torch.int32).reshape(J, 4).to(DEV)
    d_s = torch.tensor(s, dtype=torch.float32).reshape(J).to(DEV)
    d_tab = None if table is None else torch.from_numpy(np.ascontiguousarray(table)).float().to(DEV)
    G = 1 if table is None else table.shape[1]
    out = torch.full((J * rows_max + 4, 16), SENTINEL, device=DEV)          # (four rows of guard behind the last job)
    jr = torch.full((max(J, 1), 2), -7, dtype=torch.int32, device=DEV)
    fl = torch.full((max(J, 1),), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.gfl_compose_rows_workspace_bytes(J, rows_max)
    ws = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = lib.gfl_compose_rows(L.ptr(blk), L.ptr(lab), blk.shape[0], L.ptr(d_src), L.ptr(d_s), L.ptr(d_tab), G, J, rows_max,
                              L.ptr(out), L.ptr(jr), L.ptr(fl), L.ptr(ws), nbytes, L.stream())
    torch.cuda.synchronize()
    return dict(rc=rc, rows=out.cpu(), job_rows=jr.cpu()[:J], flags=fl.cpu()[:J], guard_ok=bool((ws[nbytes:] == 0xA5).all()))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _slot(res, j, rows_max):
    """job j's kept rows"""
    first, kept = res["job_rows"][j].tolist()
    assert first == j * rows_max and 0 <= kept <= rows_max
    return res["rows"][first:first + kept]


def _assert_contained(res, rows_max):
    """every float outside the jobs' [j rows_max, j rows_max + kept) still holds the sentinel"""
    touched = torch.zeros(res["rows"].shape[0], dtype=torch.bool)
    for j in range(res["job_rows"].shape[0]):
        first, kept = res["job_rows"][j].tolist()
        touched[first:first + kept] = True
    sentinel = _bits(torch.tensor([SENTINEL]))[0]
    assert bool((_bits(res["rows"])[~touched] == sentinel).all()), "rows outside a job's kept range were written"
    assert not bool((_bits(res["rows"])[touched] == sentinel).all(dim=1).any()), "a kept row was not written"
    assert res["guard_ok"], "bytes behind the workspace were written"


# ------------------------------------------------------------------ 1. identity
def test_identity_copies_the_source_rows_and_renders_like_render_block(clip):
    import gflow_amd.render as R
    block = clip["block"]
    for n in COUNTS:
        res = run_compose(block, None, [(0, n, 0, n)], [0.0], None, NA)
        assert res["rc"] == 0 and res["flags"].tolist() == [0] and res["job_rows"].tolist() == [[0, n]], n
        assert torch.equal(_bits(res["rows"][:n]), _bits(block[:n])), n
        _assert_contained(res, NA)
        # a range that starts inside the block, with labels and an identity table: still a bit copy
        res = run_compose(block, clip["labels"], [(37, n, 37, n)], [0.0], np.stack([np.stack([CR.IDENTITY] * 2)]), NA)
        assert res["job_rows"].tolist() == [[0, n]] and torch.equal(_bits(res["rows"][:n]), _bits(block[37:37 + n])), n
    blk = block.to(DEV)
    J = len(COUNTS)
    intr, extr = clip["intr"].to(DEV), clip["extr"].to(DEV).reshape(1, 3, 4).expand(J, 3, 4).contiguous()
    src = [(0, n, 0, n) for n in COUNTS]
    for u8 in (False, True):
        want = R.render_block(blk, [(0, n) for n in COUNTS], intr, extr, 0.33, W, H, uint8=u8)
        got = R.render_composed(blk, None, src, [0.0] * J, None, intr, extr, 0.33, W, H, NA, uint8=u8, rows=True)
        assert got["out_job_rows"].tolist() == [[j * NA, n] for j, n in enumerate(COUNTS)]
        if u8:
            assert torch.equal(got["img"], want["img"]) and len(set(got["img"][-1].reshape(-1).tolist())) > 30
        else:
            assert torch.equal(_bits(got["rgb"]), _bits(want["rgb"])) and torch.equal(_bits(got["depth_map"]), _bits(want["depth_map"]))
    R.check_overflow()


# ------------------------------------------------------------------ 2. parity with the restatement
PARITY_ROWS_MAX = NA
PARITY_JOBS = [            # (first_a, count_a, first_b, count_b), s, table
    ((0, 1023, NA, 1025), 0.25, 0),            # count_a < count_b: two rows fade in
    ((0, 2500, NA, 1024), 0.25, 1),            # count_b < count_a: 1476 rows fade out
    ((0, 0, NA, 65), 0.25, 0),                 # nothing at frame a
    ((100, 64, NA + 130, 63), 0.25, 1),        # ranges inside those of the jobs above
    ((0, 1025, NA, 1025), 0.0, 0),
    ((0, 1025, NA, 1025), 1.0, 1),
    ((0, NC, 2 * NA, NC), 0.25, 0),            # b = -a
    ((0, 0, NA, 300), 0.0, 0),                 # every row drops: rows of frame b alone, at s = 0
    ((0, 0, 0, 0), 0.25, 1),
    ((5, 1, NA + 5, 1), 0.25, 1),
    ((7, 63, NA + 7, 63), 0.25, 0),
    ((0, 1024, NA, 1023), 1.0, 0),             # the last row of a fades out completely
    ((0, 2500, NA, 2500), 0.25, 1),
]


@pytest.fixture(scope="module")
def parity(clip):
    src = [j[0] for j in PARITY_JOBS]
    s = [j[1] for j in PARITY_JOBS]
    table = np.stack([TABLES[j[2]] for j in PARITY_JOBS])
    got = run_compose(clip["block"], clip["labels"], src, s, table, PARITY_ROWS_MAX)
    ref = CR.compose(clip["block"].numpy(), clip["labels"].numpy(), src, np.array(s, dtype=np.float32), table, PARITY_ROWS_MAX)
    return dict(src=src, s=s, table=table, got=got, ref=ref)


def test_parity_with_the_float64_restatement(clip, parity):
    """Bounds from the arithmetic, u = 2^-24 (the issue's): xyz 32 u M with M = size |xyz - pivot|_1 + |pivot|_inf + |shift|_inf
    (the blended xyz of the restatement; an untouched transform is size 1, pivot 0, shift 0); scale, opacity, rgb
    8 u max(1, |a|, |b|) size; rotate 32 u and unit norm to 1e-6.  The kernel's order -- fmaf(s, b - a, a); d = xyz - pivot,
    three fmaf per row of R(q), fmaf(size, ., pivot) + shift -- stays inside them: no wider bound is needed."""
    got, ref = parity["got"], parity["ref"]
    assert got["rc"] == 0 and got["flags"].tolist() == [0] * len(PARITY_JOBS)
    _assert_contained(got, PARITY_ROWS_MAX)
    labels = clip["labels"].numpy()
    dropped_near_edges = set()
    for j, (src, s, t) in enumerate(PARITY_JOBS):
        r = ref[j]
        rows = _slot(got, j, PARITY_ROWS_MAX).double().numpy()
        # which rows stay: the restatement's drop set is exact (opacities >= 1e-3, gains 0 or >= 0.5)
        n = max(src[1], src[3])
        have_group = labels[[(src[0] + i) if i < src[1] else (src[2] + i) for i in range(n)]] if n else np.zeros(0, dtype=np.uint8)
        assert rows.shape[0] == r["kept"].size, f"job {j}: {rows.shape[0]} rows kept, the restatement keeps {r['kept'].size}"
        dropped = sorted(set(range(n)) - set(r["kept"].tolist()))
        dropped_near_edges |= {i for i in dropped if i in (62, 63, 64, 65, 1022, 1023, 1024, 1025)}
        if s not in (0.0, 1.0) or src[1] == src[3]:
            assert dropped == [i for i in range(n) if have_group[i] == 1], f"job {j}: the hidden group is what drops"
        if not rows.shape[0]:
            continue
        e = parity["table"][j][np.minimum(r["group"], 2)].astype(np.float64)
        e[r["group"] > 2] = CR.IDENTITY
        still = np.array([CR.is_still_transform(x.astype(np.float32)) for x in e])
        size = np.where(still, 1.0, e[:, 1])
        pivot = np.where(still[:, None], 0.0, e[:, 6:9])
        shift = np.where(still[:, None], 0.0, e[:, 9:12])
        M = size * np.abs(r["blended"][:, 0:3] - pivot).sum(1) + np.abs(pivot).max(1) + np.abs(shift).max(1)
        err = np.abs(rows - r["rows"])
        what = f"job {j} (s = {s}): "
        worst = (err[:, 0:3].max(1) / (32 * U * M)).max()
        print(what + f"xyz error / bound {worst:.3f}")
        assert worst <= 1.0, what + "xyz"
        big = np.maximum(1.0, r["big"]) * size[:, None]
        for name, cols in (("scale", slice(3, 6)), ("opacity", slice(10, 11)), ("rgb", slice(11, 14))):
            worst = (err[:, cols] / (8 * U * big[:, cols])).max()
            print(what + f"{name} error / bound {worst:.3f}")
            assert worst <= 1.0, what + name
        worst = err[:, 6:10].max() / (32 * U)
        print(what + f"rotate error / bound {worst:.3f}")
        assert worst <= 1.0, what + "rotate"
        assert np.abs(np.linalg.norm(rows[:, 6:10], axis=1) - 1.0).max() <= 1e-6, what + "unit quaternions"
        assert not rows[:, 14:16].any(), what + "pad columns"
        if s == 0.0:                      # a's bits where nothing edits them
            a = clip["block"][src[0]:src[0] + src[1]][torch.from_numpy(r["kept"])]
            same = torch.from_numpy(r["group"] > 2)
            assert torch.equal(_bits(_slot(got, j, PARITY_ROWS_MAX)[same]), _bits(a[same])), what + "rows of group 3 are a's"
    assert dropped_near_edges == {62, 63, 64, 65, 1022, 1023, 1024, 1025}
    assert ref[7]["kept"].size == 0 and got["job_rows"][7].tolist() == [7 * PARITY_ROWS_MAX, 0]
    assert ref[6]["kept"].size > 500 and ref[0]["kept"].size > 500


# ------------------------------------------------------------------ 3. determinism
def test_a_job_is_a_function_of_its_own_tables(clip, parity):
    got = parity["got"]
    pick = [0, 1, 6, 12]

    def call(order):
        return run_compose(clip["block"], clip["labels"], [parity["src"][j] for j in order], [parity["s"][j] for j in order],
                           np.stack([parity["table"][j] for j in order]), PARITY_ROWS_MAX)
    for j in pick:
        solo = call([j])
        assert torch.equal(_bits(_slot(solo, 0, PARITY_ROWS_MAX)), _bits(_slot(got, j, PARITY_ROWS_MAX))), f"job {j} alone"
    for order in ([6, 0, 12, 1], [1, 12, 0, 6], [12, 6, 1, 0]):
        res = call(order)
        for pos, j in enumerate(order):
            assert torch.equal(_bits(_slot(res, pos, PARITY_ROWS_MAX)), _bits(_slot(got, j, PARITY_ROWS_MAX))), f"job {j} at {pos} of {order}"
    again = call(list(range(len(PARITY_JOBS))))
    assert torch.equal(_bits(again["rows"]), _bits(got["rows"])) and torch.equal(again["job_rows"], got["job_rows"])


# ------------------------------------------------------------------ 4. containment and refused jobs
def test_refused_jobs_keep_nothing_and_disturb_nobody(clip):
    rows_max = NC
    good = [((0, 1025, NA, 1023), 0.25, 0), ((0, NC, 2 * NA, NC), 0.25, 1), ((200, 65, NA + 200, 64), 0.25, 0)]
    bad = [((R_ALL - 100, 200, 0, 100), 0.25, 0),        # leaves [0, R)
           ((0, 100, R_ALL - 50, 51), 0.25, 0),          # b leaves [0, R) by one row
           ((0, NC + 1, NA, 10), 0.25, 0),               # longer than rows_max
           ((-1, 10, 0, 10), 0.25, 0), ((0, 10, 0, -1), 0.25, 0)]
    order = [bad[0], good[0], bad[1], bad[2], good[1], bad[3], good[2], bad[4]]

    def call(jobs):
        return run_compose(clip["block"], clip["labels"], [j[0] for j in jobs], [j[1] for j in jobs],
                           np.stack([TABLES[j[2]] for j in jobs]), rows_max)
    mixed, clean = call(order), call(good)
    assert mixed["rc"] == 0 and clean["rc"] == 0 and clean["flags"].tolist() == [0, 0, 0]
    assert mixed["flags"].tolist() == [2, 0, 2, 2, 0, 2, 0, 2]
    _assert_contained(mixed, rows_max)
    _assert_contained(clean, rows_max)
    for pos, job in enumerate(order):
        if job in bad:
            assert mixed["job_rows"][pos].tolist() == [pos * rows_max, 0]
        else:
            k = good.index(job)
            assert _slot(clean, k, rows_max).shape[0] >= 20
            assert torch.equal(_bits(_slot(mixed, pos, rows_max)), _bits(_slot(clean, k, rows_max))), f"job at {pos}"
    # a job that fills its room to the last row, in front of another one
    full = run_compose(clip["block"], None, [(0, NC, 0, NC), (NA, 64, NA, 64)], [0.0, 0.0], None, rows_max)
    assert full["job_rows"].tolist() == [[0, NC], [NC, 64]]
    _assert_contained(full, rows_max)
    assert torch.equal(_bits(full["rows"][:NC]), _bits(clip["block"][:NC]))
    assert torch.equal(_bits(full["rows"][NC:NC + 64]), _bits(clip["block"][NA:NA + 64]))


# ------------------------------------------------------------------ 5. viewer, end to end
def _logit(p):
    return torch.log(p / (1.0 - p))


@pytest.fixture(scope="module")
def log_folder(tmp_path_factory):
    """three checkpoints of 300, 300 and 340 rows with still_mask, as SimpleGaussian.save_checkpoint writes them (raw
    attributes: the loader applies the activations); the last mask is 300 long, so the 40 appended rows count as still"""
    folder = tmp_path_factory.mktemp("clip")
    os.makedirs(folder / "ckpt")
    sc = random_scene(340, W, H, seed=31, sigma_px=2.5, behind=0.0)
    g = torch.Generator().manual_seed(32)
    still = (torch.arange(340) % 3) != 1
    for k, n in enumerate((300, 300, 340)):
        move = 0.03 * k * (~still[:n]).float().unsqueeze(1) * torch.tensor([[1.0, 0.2, 0.0]])
        attrs = {"xyz": sc["xyz"][:n] + move + 0.002 * k * torch.randn(n, 3, generator=g),
                 "scale": sc["scale"][:n] * (1.0 + 0.02 * k) * torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).unsqueeze(1),
                 "rotate": 1.7 * torch.nn.functional.normalize(sc["rotate"][:n] + 0.03 * k * torch.randn(n, 4, generator=g), dim=1),
                 "opacity": _logit(sc["opacity"][:n].clamp(0.02, 0.98)) / 10.0,
                 "rgb": _logit((sc["rgb"][:n] + 0.02 * k).clamp(0.02, 0.98))}
        extr = sc["extr"].clone()
        extr[:, 3] += torch.tensor([0.02 * k, -0.01 * k, 0.0])
        torch.save({"attributes": attrs, "intr": sc["intr"] + torch.tensor([0.5 * k, 0.5 * k, 0.0, 0.0]), "extr": extr,
                    "still_mask": still[:min(n, 300)].clone(), "move_seg": None, "last_uv": None, "width": W, "height": H},
                   folder / "ckpt" / f"frame_{k:04d}.tar")
    return folder


def test_viewer_in_between_frames_layers_and_the_command_line(log_folder, tmp_path):
    import gflow_amd.render as R
    from gflow_amd import viewer as V
    session = V.ViewerSession(str(log_folder), DEV)
    assert len(session) == 3 and session.ranges == [(0, 300), (300, 300), (600, 340)] and session.rows_max == 340
    lab = session.labels
    assert lab.dtype == torch.uint8 and lab.shape == (940,) and lab.is_cuda
    want = ((torch.arange(340) % 3) == 1).to(torch.uint8)
    assert lab[:300].cpu().tolist() == want[:300].tolist() and lab[600:900].cpu().tolist() == want[:300].tolist()
    assert int(lab[900:].sum()) == 0
    # an integral time is the frame
    assert torch.equal(session.frame_at(1.0), session.frame(1)) and torch.equal(session.frame_at(2), session.frame(2))
    # a layer is a bit copy of its rows, in their order
    counts = {}
    for layer, group in (("still", 0), ("moving", 1)):
        res = session.frame_at(0.0, layer=layer, rows=True)
        rows = session.block[0:300][lab[0:300] == group].contiguous()
        counts[layer] = int(res["out_job_rows"][0, 1])
        assert counts[layer] == rows.shape[0] and torch.equal(_bits(res["out_rows"][:rows.shape[0]]), _bits(rows))
        ref = R.render_block(rows, [(0, rows.shape[0])], session.intrs[0], session.extrs[0:1], session.bg, W, H, uint8=True)["img"][0]
        assert torch.equal(res["img"][0], ref) and torch.equal(session.frame_at(0.0, layer=layer), ref)
    assert counts["still"] + counts["moving"] == 300 and counts["moving"] == 100
    assert not torch.equal(session.frame_at(0.0, layer="still"), session.frame_at(0.0, layer="moving"))
    # between two frames: the image is the rasteriser's on the composed rows (their values: the parity test)
    res = session.frame_at(1.5, rows=True)
    kept = int(res["out_job_rows"][0, 1])
    assert kept == 340 and res["out_rows"].shape == (340, 16)
    extr, intr = V.camera_at(session.extrs.cpu(), session.intrs.cpu(), 1.5)
    ref = R.render_block(res["out_rows"][:kept].contiguous(), [(0, kept)], intr.to(DEV), extr.reshape(1, 3, 4).to(DEV), session.bg, W, H,
                         uint8=True)["img"][0]
    mid = session.frame_at(1.5)
    assert torch.equal(res["img"][0], ref) and torch.equal(mid, ref)
    assert not torch.equal(mid, session.frame(1)) and not torch.equal(mid, session.frame(2))
    # play_at: the frames one by one
    taus = V.slowmo(3, 2)
    imgs = session.play_at(taus)
    assert imgs.shape == (5, H, W, 3) and imgs.dtype == torch.uint8
    for k, tau in enumerate(taus):
        assert torch.equal(imgs[k], session.frame_at(tau)), tau
    # an edit: the moving group shifted; its centroid pivot is taken on the device
    e = {"moving": V.Edit(shift=(0.1, 0.0, 0.0), turn=("y", 20.0), size=1.1)}
    edited = session.frame_at(1.0, edits=e, rows=True)
    assert int(edited["out_job_rows"][0, 1]) == 300
    moved = lab[300:600] == 1
    assert torch.equal(_bits(edited["out_rows"][:300][~moved]), _bits(session.block[300:600][~moved]))
    d = (edited["out_rows"][:300, 0:3] - session.block[300:600, 0:3])[moved]
    assert float(d.abs().max()) > 0.05 and abs(float(d.mean(0)[0]) - 0.1) < 1e-4      # about the centroid: the mean moves by the shift
    R.check_overflow()
    out = tmp_path / "slow"
    assert V.main(["--folder", str(log_folder), "--out", str(out), "--slowmo", "3", "--layer", "moving", "--edit",
                   "moving:shift=0.1,0,0"]) == 0
    assert sorted(os.listdir(out)) == [f"{k:06d}.png" for k in range((3 - 1) * 3 + 1)]


# ------------------------------------------------------------------ 6. graph capture
def test_a_captured_frame_at_replays_the_eager_image(log_folder):
    import gflow_amd.render as R
    from gflow_amd import viewer as V
    session = V.ViewerSession(str(log_folder), DEV)
    extr = V.camera_at(session.extrs.cpu(), session.intrs.cpu(), 1.25)[0].to(DEV)
    e = {"moving": V.Edit(shift=(0.05, 0.0, 0.0), tint=(1.0, 0.0, 0.0), mix=0.5)}
    eager = session.frame_at(1.25, extr=extr, edits=e).clone()              # (eager: workspace and edit table exist from here on)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = session.frame_at(1.25, extr=extr, edits=e)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert not torch.equal(eager, session.frame_at(1.25, extr=extr))
    R.check_overflow()
