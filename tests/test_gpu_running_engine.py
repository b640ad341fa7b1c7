"""Gradient parity on a RUNNING engine (``-m gpu``): the gradient of iteration k of a fit whose splats have moved since
iteration k - 1.  The fused backward keeps a pair's gradient row at (splat, index of the tile in the splat's tile rectangle)
-- 32 rows of its own per splat, a run out of a pool for a splat of more than 32 tiles -- never clears a row and tells this
forward's rows from older ones by a stamp.  After the first iteration nearly every row holds a plausible gradient of some
earlier forward; every other gradient test of the suite reads a fresh engine (workspace all zero) or keeps lr = 0.

Scenes, row sets and the reference's own error: tests/test_running_engine_host.py (on the CPU).  The gradient is read as in
tests/test_gpu_fused.py (g = m / 0.1) after zeroing Adam's first moments in place behind the engine's back; the reference is
the float32 oracle on the rows read back from the device just before the iteration, the float64 oracle says which rows get
nothing at all.

What each test is there to catch: a gather that accepts a stamp other than this forward's (every test on the transition
scene, and the pile toggle, whose 22 rows then keep last iteration's gradient); a wide row's gather or store that ignores the
stamp or uses another run (the transition scene: rows enter and leave the pool every step); the two launches working out a
row's index from different rectangles (the row sets by transition, "same layout, moved", "clipped"); a pool counter that is
not back at zero, or runs that overlap (check_pool); a run that does not fit (the pool test).  The figures a run leaves
(the observed-parity log) are 1e-6 .. 4e-4 relative on every row set; the largest of them, d_rgb of the class rows on
the frozen-camera paths, have the absolute size of ONE pixel's alpha T dL/dC at the 1 / 255 visibility threshold of a wide,
faint row, where the last bits of exp() decide: not a pair row."""
import numpy as np
import pytest
import torch

from oracle import msplat_oracle as MO
from tests.scenes import (ATTRS, N_CULLED, REGIME_LAMBDAS, apply_transition, capped_pile_scene, layout_class, oracle_front_end,
                          pile_phase, pile_toggle_rows, reference_fit)
from tests.test_gpu_fused import POSE, _engine, _reserved_on
from tests.test_gpu_parity import close_frac, observe, rel_l2, subset_check
from tests.test_running_engine_host import PILE_SEED, TRANSITIONS, nonzero_rows, targets, transition_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL, RTOL, ATOL_SCALE, BAD = 2e-3, 5e-3, 5e-4, 1e-2        # tests/test_gpu_fused.py:_check_fused_gradients
PATHS = ("exact", "reserved", "graph")


def gradient_of_next_iteration(eng, scene, img, dep, **how):
    """Runs ONE iteration (``how``: the arguments of FitEngine.iteration) and returns its gradients next to the oracle's on the
    rows, pose and depth affine read back just before it.  Adam's first moments are zeroed in place first (the engine is
    not told; second moments and the step counter stay): m = 0.1 g exactly afterwards.  A void iteration (pairs dropped, a
    reserved region outgrown) steps nothing and would pass every comparison below vacuously: refused here."""
    from gflow_amd.fused import COLS
    n = eng.N
    rows = eng.params[:n, :14].clone()
    raw = {k: rows[:, a:b].cpu().contiguous() for k, (a, b) in COLS.items()}
    pose, ab = eng.pose.cpu().clone(), eng.depth_ab.cpu().clone()
    eng.adam_m.zero_(); eng.pose_m.zero_(); eng.ab_m.zero_()
    step = int(eng.step.item())
    eng.iteration(**how)
    torch.cuda.synchronize()
    assert eng.overflow.tolist() == [0, 0, 0, 0], f"a void iteration: overflow words {eng.overflow.tolist()}"
    assert int(eng.step.item()) == step + 1
    g = (eng.adam_m[:n] / (1.0 - 0.9)).cpu()
    sc = dict(scene, raw=raw)
    l_rgb, l_depth = eng.loss_terms()
    return dict(grads={k: g[:, a:b] for k, (a, b) in COLS.items()}, d_pose=(eng.pose_m / 0.1).cpu(), d_ab=(eng.ab_m / 0.1).cpu(),
                l_rgb=l_rgb.item(), l_depth=l_depth.item(), before=rows.cpu(), after=eng.params[:n, :14].cpu(), scene=sc, pose=pose,
                r32=reference_fit(sc, pose, img, dep, torch.float32, ab=ab), r64=reference_fit(sc, pose, img, dep, torch.float64, ab=ab))


def check_gradients(res, sets, tag, camera):
    """The bounds of tests/test_gpu_fused.py:_check_fused_gradients over all rows, then over each row set of ``sets`` (name ->
    boolean (N,)) in the form of tests/test_gpu_regimes.py:_regime_check (the rows' own norm, atol from the rows' own largest
    entry); rows the float64 oracle gives nothing in any attribute get exactly nothing and do not move."""
    ref = res["r32"]
    assert abs(res["l_rgb"] - ref["l_rgb"]) <= 1e-4 * abs(ref["l_rgb"]), (tag, res["l_rgb"], ref["l_rgb"])
    assert abs(res["l_depth"] - ref["l_depth"]) <= 1e-4 * abs(ref["l_depth"]), (tag, res["l_depth"], ref["l_depth"])
    for k in ATTRS:
        got, want = res["grads"][k], ref["grads"][k]
        rel = rel_l2(got, want)
        observe(f"{tag}d_{k}: relative L2 {rel:.2e} (bound {REL:g})")
        assert rel < REL, f"{tag}d_{k}: relative L2 error {rel:.2e}"
        close_frac(got, want, RTOL, ATOL_SCALE * want.abs().max().item(), bad_frac=BAD, what=f"{tag}d_{k}")
        for name, rows in sets.items():
            if float(want[rows].abs().max()) == 0.0:
                assert float(got[rows].abs().max()) == 0.0, f"{tag}d_{k}, {name} rows: the reference is zero, the device is not"
                observe(f"{tag}d_{k}, {name} rows: zero in both")
                continue
            subset_check(got, want, rows, f"{tag}d_{k}, {name} rows", rel_bound=REL,
                         frac=(RTOL, ATOL_SCALE * want[rows].abs().max().item(), BAD))
    if camera:
        rel = rel_l2(res["d_pose"], ref["d_pose"])
        observe(f"{tag}d_pose: relative L2 {rel:.2e} (bound {REL:g})")
        assert rel < REL, f"{tag}d_pose: relative L2 error {rel:.2e}  {res['d_pose']} vs {ref['d_pose']}"
    else:
        assert float(res["d_pose"].abs().max()) == 0.0
    # (the depth affine is stepped on every path: by the camera launch, or with a frozen camera by the loss tail, which fills ab_m)
    np.testing.assert_allclose(res["d_ab"].numpy(), ref["d_ab"].numpy(), rtol=2e-3, err_msg=tag + "depth affine")
    none = ~nonzero_rows(res["r64"]["grads"])
    g_all = torch.cat([res["grads"][k] for k in ATTRS], dim=1)
    observe(f"{tag}{int(none.sum())} rows without a float64 reference gradient")
    assert float(g_all[none].abs().max()) == 0.0, f"{tag}a row without a reference gradient got one"
    assert torch.equal(res["after"][none], res["before"][none]), f"{tag}a row without a gradient moved"
    return none


def device_rects(eng):
    """Per row, from the records of the engine's last forward: the tile count and the tile rectangle (x0, x1, y0, y1) the
    backward blend and the per-splat launch both work out (rec columns 0, 1: uv, column 11: the radius as an int)."""
    rec = eng.rec[:eng.N].cpu()
    rad = rec[:, 11].contiguous().view(torch.int32)
    x0, x1, y0, y1 = MO.tile_rect(rec[:, 0:2], rad, eng.W, eng.H)
    tiles = torch.where(rad > 0, (x1 - x0) * (y1 - y0), torch.zeros_like(x0))
    gx, gy = MO.tile_grid(eng.W, eng.H)
    r = rad.float()
    clipped = (rad > 0) & ((rec[:, 0] - r < 0) | (rec[:, 1] - r < 0) | (torch.trunc((rec[:, 0] + r + 15) / 16) > gx)
                           | (torch.trunc((rec[:, 1] + r + 15) / 16) > gy))
    return dict(tiles=tiles, rect=torch.stack([x0, x1, y0, y1], dim=1), clipped=clipped)


def pool_state(eng):
    """White box, through the workspace's layout table (gfl_fit_workspace_layout): the pool counter and the stamp (words 0
    and 56 of the ``counters`` region, gfl_fit.hip: FitCounters) and the rows' run offsets (``wide_off``: written for wide rows
    only)."""
    import ctypes
    room = 64
    names, offsets, sizes = (ctypes.c_char_p * room)(), (ctypes.c_size_t * room)(), (ctypes.c_size_t * room)()
    k = eng.lib.gfl_fit_workspace_layout(eng.cap, eng.K_cap, eng.W, eng.H, names, offsets, sizes, room)
    assert 0 < k <= room
    at = {names[i].decode(): int(offsets[i]) for i in range(k)}
    torch.cuda.synchronize()
    counters = eng.workspace[at["counters"]:at["counters"] + 256].view(torch.int32).cpu()
    wide_off = eng.workspace[at["wide_off"]:at["wide_off"] + 4 * eng.N].view(torch.int32).cpu()
    return dict(counter=int(counters[0]), stamp=int(counters[56]), wide_off=wide_off.long())


def check_pool(eng, rects, tag, dropped=0):
    """After an iteration: the pool counter is back at zero for the next preprocess, and the runs of this iteration's wide
    rows (more than 32 tiles) lie side by side from row 0 of the pool -- no two share a row, none starts where an earlier
    iteration's counter stood.  ``dropped``: so many of them have no run at all (offset -1: the pool was full)."""
    ps = pool_state(eng)
    assert ps["counter"] == 0, f"{tag}the pool counter stands at {ps['counter']} after the iteration"
    wide = rects["tiles"] > 32
    off, nt = ps["wide_off"][wide], rects["tiles"][wide]
    assert int((off < 0).sum()) == dropped, f"{tag}{int((off < 0).sum())} wide rows without a run"
    if dropped == 0:
        order = torch.argsort(off)
        start = torch.cumsum(nt[order], 0) - nt[order]
        assert torch.equal(off[order], start), f"{tag}the runs of the wide rows are not side by side from 0"
    observe(f"{tag}{int(wide.sum())} wide rows, {int(nt.sum())} pool rows, stamp {ps['stamp']}")
    return ps


def transition_sets(prev, now, class_rows, n):
    """Row sets of an iteration from the device's own rectangles in the forward before it (``prev``) and in its own
    (``now``): the class rows on each layout transition, those that kept their layout under another rectangle, those that
    came back from behind the camera, and every row whose rectangle the image border cuts."""
    cls = torch.zeros(n, dtype=torch.bool)
    cls[class_rows] = True
    c0, c1 = layout_class(prev["tiles"]), layout_class(now["tiles"])
    sets = {f"{a} -> {b}": cls & (c0 == a) & (c1 == b) for a, b in TRANSITIONS}
    sets["same layout, moved"] = cls & (c0 == c1) & (c1 >= 0) & (prev["rect"] != now["rect"]).any(dim=1)
    sets["back in view"] = cls & (c0 < 0) & (c1 >= 0)
    sets["clipped"] = now["clipped"]
    sets["class"] = cls & (c1 >= 0)
    return {k: v for k, v in sets.items() if k != "back in view" or bool(v.any())}


def _how(path):
    return dict(reserved=False) if path == "exact" else dict(use_graph=True) if path == "graph" else {}


def _transition_engine(path, deterministic):
    case = transition_case(0)
    sc = case["sc"]
    camera = path == "exact"
    eng = _engine(sc["raw"], sc, case["img"], case["dep"], pose=POSE, lr=2e-3, lr_camera=1e-3 if camera else 0.0, total_iters=100,
                  **REGIME_LAMBDAS)
    eng.deterministic = deterministic
    if path != "exact" and not _reserved_on(eng):
        pytest.skip("reserved tile regions are switched off (GFL_RESERVED=0)")
    return eng, sc, case["img"], case["dep"], camera


# ------------------------------------------------------------------------------------------------ a moving fit
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("path", PATHS)
def test_gradients_of_a_moving_fit_whose_rows_change_their_layout_every_step(path, deterministic):
    """Six iterations at lr = 2e-3 on the transition scene; before each of iterations 2 .. 6 the class rows are edited in place
    (apply_transition: rectangles grow / shrink across 16 and 32 tiles, all move 9 pixels, six rows go behind the camera and
    come back).  The gradients of iterations 2, 3 and 6 against the oracle on the rows as they were: iteration 2 is the first
    with stale rows under another layout, iteration 3 the first where a narrow row's own 32 rows are two forwards old after a
    detour through the pool, iteration 6 has gone through every pool offset five times.  ``exact``: every iteration bins
    exactly, the camera moves (camera launch: d_pose); ``reserved``: iterations 2 .. 6 bin into the regions the one before
    reserved, the camera is frozen (loss tail); ``graph``: the same as replays of a one-iteration graph (captured at iteration
    2: that iteration is the capture's first replay, iterations 3 and 6 replay a graph captured before the rows were edited).  ``deterministic``: its own staging batch and row sums."""
    eng, sc, img, dep, camera = _transition_engine(path, deterministic)
    n, rows = eng.N, sc["rows"]
    eng.iteration()
    eng.check_overflow()
    for it in range(2, 7):
        prev = device_rects(eng)
        apply_transition(eng.views(), rows, it - 1, f=float(sc["intr"][0]))
        if it not in (2, 3, 6):
            eng.iteration(**_how(path))
            continue
        if path != "exact":
            assert eng._reserved_flag() == eng.GFL_ITER_RESERVED
        res = gradient_of_next_iteration(eng, sc, img, dep, **_how(path))
        if path == "graph":
            assert (1, eng.GFL_ITER_RESERVED) in eng.graphs.live
        now = device_rects(eng)
        sets = transition_sets(prev, now, rows, n)
        tag = f"[moving fit, {path}{', deterministic' if deterministic else ''}, iteration {it}] "
        check_pool(eng, now, tag)
        # The unfitted scene has 12 .. 14 rows on every transition (at least 8 asserted on the CPU).  Here the rows have taken up
        # to five Adam steps of at most lr = 2e-3 per raw value (1 % of a scale), so a row within that of a layout boundary may
        # be counted on another side: 8 .. 15 were seen.  6 is asked for: a few rows of drift below the CPU's floor, and
        # still several rows per transition, each with ten or more pair rows at stake.
        counts = {f"{a} -> {b}": int(sets[f"{a} -> {b}"].sum()) for a, b in TRANSITIONS}
        observe(f"{tag}rows per transition {counts}, same layout and moved {int(sets['same layout, moved'].sum())}, "
                f"clipped {int(sets['clipped'].sum())}")
        assert min(counts.values()) >= 6, (tag, counts)
        assert int(sets["same layout, moved"].sum()) >= 50 and int(sets["clipped"].sum()) >= 20
        none = check_gradients(res, sets, tag, camera)
        culled = rows[-N_CULLED:]
        if it % 2 == 0:                                        # an odd edit: the last class rows are behind the camera
            assert bool(none[culled].all()) and bool((now["tiles"][culled] == 0).all()) and bool((prev["tiles"][culled] > 0).all())
        else:
            assert "back in view" in sets and bool(sets["back in view"][culled].all())
    assert int(eng.step.item()) == 6
    eng.check_overflow()


# ------------------------------------------------------------------------------------------------ stamps without rows
@pytest.mark.parametrize("path", ["exact", "reserved"])
def test_gradients_after_forwards_that_leave_no_rows(path):
    """The stamp a row is valid under advances with every forward blend, the rows are written by backward blends only.  After
    the edit: a plain forward(), an iteration(snapshot=True) (the forward that also draws the snapshot images) and a
    snapshot() (which draws from the last forward and leaves the stamp alone) before the iteration under test; then the
    inverse edit and two plain forwards directly before the next one."""
    eng, sc, img, dep, camera = _transition_engine(path, False)
    n, rows = eng.N, sc["rows"]
    f = float(sc["intr"][0])
    eng.iteration(); eng.iteration(**_how(path))
    eng.check_overflow()
    prev = device_rects(eng)
    apply_transition(eng.views(), rows, 1, f=f)
    stamps = [pool_state(eng)["stamp"]]
    eng.forward()
    stamps.append(pool_state(eng)["stamp"])
    eng.iteration(snapshot=True)
    stamps.append(pool_state(eng)["stamp"])
    eng.snapshot()
    stamps.append(pool_state(eng)["stamp"])
    res = gradient_of_next_iteration(eng, sc, img, dep, **_how(path))
    now = device_rects(eng)
    stamps.append(check_pool(eng, now, f"[forward, snapshot iteration, snapshot; {path}] ")["stamp"])
    # every forward blend advances the stamp by one, drawing the snapshot from the last forward leaves it
    assert [b - a for a, b in zip(stamps, stamps[1:])] == [1, 1, 0, 1], stamps
    check_gradients(res, transition_sets(prev, now, rows, n), f"[forward, snapshot iteration, snapshot; {path}] ", camera)
    apply_transition(eng.views(), rows, 2, f=f)
    eng.forward(); eng.forward()
    res = gradient_of_next_iteration(eng, sc, img, dep, **_how(path))
    last = device_rects(eng)
    assert check_pool(eng, last, f"[two forwards; {path}] ")["stamp"] == stamps[-1] + 3
    sets = transition_sets(now, last, rows, n)
    assert "back in view" in sets
    check_gradients(res, sets, f"[two forwards; {path}] ", camera)
    assert int(eng.step.item()) == 5


# ------------------------------------------------------------------------------------------------ occlusion toggle
@pytest.mark.parametrize("path", ["exact", "reserved"])
def test_gradients_after_rows_in_front_of_a_pile_appear(path):
    """The capped pile with its 40 nearest rows invisible (raw opacity -1) for two iterations, then their committed opacities
    written in place: they now end every pixel of the pile's tile within a few layers, and the rows that had a gradient
    behind them (22 on the CPU, tests/test_running_engine_host.py) are walked by no pixel any more -- EVERY pair row they own
    is the last iteration's.  They must get exactly nothing and stay where they are (lambda_var = 0)."""
    base = capped_pile_scene(seed=PILE_SEED)
    toggled = pile_toggle_rows(base)
    sc = pile_phase(base, "A", toggled)
    img, dep = targets(sc["H"], sc["W"], 6)
    eng = _engine(sc["raw"], sc, img, dep, lr=2e-4, lr_camera=0.0, total_iters=100, **REGIME_LAMBDAS)
    if path != "exact" and not _reserved_on(eng):
        pytest.skip("reserved tile regions are switched off (GFL_RESERVED=0)")
    n = eng.N
    eng.iteration()
    eng.adam_m.zero_()
    eng.iteration(**_how(path))
    eng.check_overflow()
    had = (eng.adam_m[:n, :14] != 0).any(dim=1).cpu()                      # rows with a gradient in the last phase-A iteration
    tr = eng.tile_range[sc["pile_tile"]].tolist()
    before = eng.ids[tr[0]:tr[1]].cpu().long()
    assert not bool(torch.isin(toggled, before).any()) and not bool(had[toggled].any())
    eng.views()["opacity"][toggled.to(DEV)] = base["raw"]["opacity"][toggled].to(DEV)
    res = gradient_of_next_iteration(eng, sc, img, dep, **_how(path))
    tr = eng.tile_range[sc["pile_tile"]].tolist()
    after = eng.ids[tr[0]:tr[1]].cpu().long()
    assert bool(torch.isin(toggled, after).all())
    observe(f"[pile toggle, {path}] the pile's list: {before.numel()} -> {after.numel()} entries")
    assert after.numel() - before.numel() == toggled.numel()
    none = check_gradients(res, {"toggled": torch.zeros(n, dtype=torch.bool).index_fill_(0, toggled, True)},
                           f"[pile toggle, {path}] ", camera=False)
    stale = had & none
    observe(f"[pile toggle, {path}] {int(had.sum())} rows had a gradient before the toggle, {int((~none).sum())} have one after, "
            f"{int(stale.sum())} had one and have none now")
    assert int(stale.sum()) >= 20


# ------------------------------------------------------------------------------------------------ the pool runs out first
def test_the_pool_of_wide_runs_runs_out_before_the_lists_do():
    """Only wide rows (more than 32 tiles) at opacity 0.05 .. 0.10: the exact-disc test drops a good part of every rectangle
    from the lists, the pool hands out a run of the WHOLE rectangle per row.  With K_cap between the pair count and the sum
    of the rectangles the lists fit and the pool does not: the row gets no run (offset -1), the sticky flag is raised, the
    iteration steps nothing; settle_overflow grows the lists, the iteration is owed, and after making it up the engine is where
    one with room is (to the 1e-5 the reserved-region tests of tests/test_gpu_fused.py use)."""
    from gflow_amd.fused import FitEngine
    case = transition_case(0)
    full = case["sc"]
    wide = full["rows"][case["facts"]["tiles"][full["rows"]] > 32]
    sc = dict(full, raw={k: v[wide].clone().contiguous() for k, v in full["raw"].items()})
    g = torch.Generator().manual_seed(5)
    sc["raw"]["opacity"] = (torch.logit(0.05 + 0.05 * torch.rand(wide.numel(), 1, generator=g, dtype=torch.float64)) / 10.0).float()
    img, dep = case["img"], case["dep"]
    hyper = dict(lr=2e-3, lr_camera=0.0, total_iters=100, **REGIME_LAMBDAS)
    big = _engine(sc["raw"], sc, img, dep, pose=POSE, **hyper)
    big.iteration()
    big.check_overflow()
    K = big.K
    tiles = oracle_front_end(sc, POSE, torch.float32)["tiles"].reshape(-1).long()
    assert bool((tiles > 32).all())
    total = int(tiles.sum())
    observe(f"[pool] {wide.numel()} wide rows: {K} pairs in the lists, {total} tiles in their rectangles")
    assert K + 1 < total, "no K_cap holds the lists and not the pool"
    small = FitEngine(sc["W"], sc["H"], capacity=big.cap, device=DEV, K_cap=(K + total) // 2)
    small.set_splats({k: v.to(DEV) for k, v in sc["raw"].items()})
    small.intr.copy_(sc["intr"].to(DEV))
    small.pose.copy_(POSE.to(DEV))
    small.set_targets(img, dep)
    for k, v in hyper.items():
        setattr(small.hp, k, v)
    small.reset_optimizer()
    rows0 = small.params[:small.N].clone()
    small.iteration()
    torch.cuda.synchronize()
    assert small.overflow[:2].tolist() == [1, 1]
    off = pool_state(small)["wide_off"]
    observe(f"[pool] K_cap {small.K_cap}: {int((off < 0).sum())} of {small.N} rows got no run")
    assert int((off < 0).sum()) >= 1 and int(tiles[off >= 0].sum()) <= small.K_cap
    assert small.K == K                                                       # the lists themselves held
    assert torch.equal(small.params[:small.N], rows0) and int(small.step.item()) == 0
    assert float(small.adam_m.abs().max()) == 0.0 and float(small.adam_v.abs().max()) == 0.0
    assert torch.equal(small.depth_ab.cpu(), torch.tensor([1.0, 0.0]))
    assert small.settle_overflow() == 1 and small.pairs_grown == 1 and small.K_cap == 2 * ((K + total) // 2)
    small.iteration()
    torch.cuda.synchronize()
    assert small.overflow.tolist() == [0, 0, 0, 0] and int(small.step.item()) == int(big.step.item()) == 1
    check_pool(small, device_rects(small), "[pool, after growing] ")
    for name in ("params", "adam_m"):
        x, y = getattr(small, name)[:small.N], getattr(big, name)[:big.N]
        rel = ((x - y).norm() / y.norm()).item()
        observe(f"[pool] {name} after the owed iteration against an engine with room: relative {rel:.1e} (bound 1e-05)")
        assert rel < 1e-5, (name, rel)
    assert float(big.adam_m[:big.N, :14].abs().max()) > 0.0
