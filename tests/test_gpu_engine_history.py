"""Used-engine parity (``-m gpu``): given the same declared inputs, a FitEngine that has been through another fit produces what
a new one does.  A clip fit drives ONE engine through every frame and stage, gflow_amd.render.render() hands pooled engines to
callers with other row counts and cameras -- and the workspace (pair-gradient rows and their stamps, the wide-run pool, tile
queues, reserved regions, cached target statistics), the rows behind N, the capacity-sized side inputs, ids[K:] and the graph
cache all stay behind from the calls before.  Deterministic mode promises bit-identical results for identical inputs, so the
comparisons are torch.equal over everything tests/test_gpu_deterministic.py lists (OUT, the sorted lists): no tolerance of
this file's own.  Nothing is carried over by design: no output is left out of a comparison.

Problems, their sizes and why a stale index is a valid one: tests/test_engine_history_host.py (on the CPU)."""
import pytest
import torch

from oracle import fit_oracle as FO
from oracle import loss_oracle as LO
from tests.scenes import apply_transition
from tests.test_engine_history_host import (CAMERA_ONLY, CAP, H, JOINT, K_CAP, W, disc, history_problem, joint_inputs,
                                            poison_row, problem)
from tests.test_gpu_deterministic import OUT, _assert_same
from tests.test_gpu_fused import POSE, _lists
from tests.test_gpu_running_engine import ATOL_SCALE, BAD, REL, RTOL, check_gradients, gradient_of_next_iteration

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "scale", "rotate", "opacity", "rgb")


def new_engine(capacity=CAP):
    from gflow_amd.fused import FitEngine
    return FitEngine(W, H, capacity=capacity, device=DEV, K_cap=K_CAP)


def _set_hyper(eng, **hp):
    for k, v in hp.items():
        setattr(eng.hp, k, v)


def hand_over(eng, q):
    """What FusedStage.__init__ does to the engine it is given (gflow_amd/stage.py), in its order and through the same public
    calls; ``q``: a problem of tests/test_engine_history_host.py.  Nothing else: no buffer is cleared, no engine is made."""
    sc = q["sc"]
    eng.set_splats({k: v.to(DEV) for k, v in sc["raw"].items()})
    eng.drop_pending()
    eng.pose.copy_(q["pose"].to(DEV))
    eng.invalidate_regions()
    eng.depth_ab.zero_()
    eng.depth_ab[0:1].fill_(1.0)
    eng.intr.copy_(sc["intr"].to(DEV))
    eng.reset_optimizer()
    _set_hyper(eng, **q["hp"])
    eng.set_regularisers(**q["reg"])
    eng.set_targets(q["img"], q["dep"] if q["hp"]["lambda_depth"] > 0 else None, q["keep"])
    if q["foot"] is not None:
        eng.set_footprint_mask(*q["foot"])
    return eng


def dirty(eng):
    """``eng`` (capacity CAP, K_CAP pairs) through ten iterations of a fit of the history scene H, in default mode: three
    first-frame iterations with a depth term and a frozen camera (the loss tail's short cut); the odd transition edit and two
    iterations, one replayed from a graph; the even edit, a snapshot iteration and a snapshot; a camera-only stretch with a
    keep mask and a footprint mask; a joint stretch with all five regulariser inputs and the flow, still and scale terms, one
    iteration of it from a graph.  No pair was dropped and the lists never grew."""
    h = history_problem(0)
    sc, rows, f = h["sc"], h["sc"]["rows"], float(h["sc"]["intr"][0])
    n = h["n"]
    eng.deterministic = False
    hand_over(eng, h)
    assert eng.hp.lambda_depth > 0 and eng.hp.lr_camera == 0
    for _ in range(3):
        eng.iteration()
    apply_transition(eng.views(), rows, 1, f=f)
    eng.invalidate_regions()
    eng.iteration()
    eng.iteration(use_graph=True)
    apply_transition(eng.views(), rows, 2, f=f)
    eng.invalidate_regions()
    eng.iteration(snapshot=True)
    eng.snapshot()
    # camera only
    _set_hyper(eng, **dict(CAMERA_ONLY, total_iters=eng.hp.total_iters))
    eng.set_targets(h["img"], h["dep"], disc(70.0, 60.0, 55.0))
    moving = torch.zeros(n, dtype=torch.bool)
    moving[rows[0::2]] = True
    eng.set_footprint_mask(~disc(70.0, 60.0, 55.0), moving)
    eng.iteration()
    eng.iteration()
    # joint
    reg, _, _ = joint_inputs(history_problem(2)["sc"]["raw"], sc["intr"], 21)
    _set_hyper(eng, **dict(JOINT, total_iters=eng.hp.total_iters))
    eng.set_regularisers(**reg)
    eng.set_targets(h["img"], h["dep"])
    eng.iteration()
    eng.iteration(use_graph=True)
    assert eng.graphs.live, "no graph was replayed"
    eng.check_overflow()
    assert eng.pairs_grown == 0 and eng.N == n and int(eng.step.item()) > 0
    return eng


def run_and_compare(fresh, used, what, k=4, moves="params"):
    """``k`` deterministic iterations on both engines, everything of OUT and every tile's sorted list bit-equal after each: the
    first on the exact binning path, the second and third on reserved regions, the fourth replayed from a graph.  Refuses to
    pass vacuously: no void iteration, the step counter advances, the rows move (``moves="pose"``: the camera does, the
    rows do not)."""
    n = fresh.N
    assert n == used.N and n > 0
    for e in (fresh, used):
        e.deterministic = True
    step0 = int(used.step.item())
    assert int(fresh.step.item()) == step0
    rows0, pose0 = used.params[:n].clone(), used.pose.clone()
    for it in range(k):
        if it == 0:
            assert fresh._reserved_N == used._reserved_N == -1                 # (set_splats / invalidate_regions: exact binning)
        else:
            assert fresh._reserved_flag() and used._reserved_flag()
        for e in (fresh, used):
            e.iteration(use_graph=it == 3)
        torch.cuda.synchronize()
        for e in (fresh, used):
            assert e.overflow.tolist() == [0, 0, 0, 0], f"{what}, iteration {it + 1}: overflow words {e.overflow.tolist()}"
        assert int(fresh.step.item()) == int(used.step.item()) == step0 + it + 1
        assert fresh.regions_outgrown == used.regions_outgrown
        _assert_same(fresh, used, f"{what}, iteration {it + 1}")
    if k > 3:
        for e in (fresh, used):
            assert (1, e.GFL_ITER_RESERVED) in e.graphs.live
    if moves == "pose":
        assert not torch.equal(used.pose, pose0) and torch.equal(used.params[:n], rows0)
    else:
        assert not torch.equal(used.params[:n], rows0)


# ------------------------------------------------------------------------------------------------ A: hand-over
@pytest.mark.parametrize("name", ["Q1", "Q2", "Q3"])
def test_an_engine_handed_over_from_another_fit_gives_what_a_new_engine_gives(name):
    """An engine that ran the history of ``dirty`` on H (1668 rows, wide rows in and out of the pool, graphs, snapshots, a keep
    and a footprint mask, all regularisers) is handed Q (600 rows under another camera; Q1 first frame, Q2 camera only under a
    keep mask, Q3 joint with flow, still and scale terms) the way a stage hands a problem to its engine; a new engine of the
    same sizes is handed the same.  Four deterministic iterations, bit for bit after each.  What would show here: a gather
    that takes a stale stamp after the row count shrank, a pool counter or queue word of H's last stage, target statistics,
    a footprint or keep mask that outlives set_targets, a regulariser that outlives set_regularisers, a graph replayed for
    another state."""
    q = problem(name)
    used = hand_over(dirty(new_engine()), q)
    fresh = hand_over(new_engine(), q)
    assert used.foot_flags is None and (used.flow_w is None) == (name != "Q3") and (used.keep is None) == (name != "Q2")
    run_and_compare(fresh, used, f"{name} after H", moves="pose" if name == "Q2" else "params")


# ------------------------------------------------------------------------------------------------ B: default mode
def test_a_handed_over_engine_in_default_mode():
    """Q1 in default mode on a used and on a new engine.  The forward has no float atomics (its bits repeat:
    tests/test_gpu_fused.py:_check_fused_forward), so render, final_T, n_contrib, the records and the sorted lists are
    bit-equal between the two.  Then the used engine's next iteration against the float32 oracle with the bounds of
    tests/test_gpu_running_engine.py (REL, RTOL, ATOL_SCALE, BAD through check_gradients, as
    test_gradients_of_a_moving_fit_whose_rows_change_their_layout_every_step holds its iterations); rows the float64 oracle gives
    nothing get exactly nothing."""
    assert (REL, RTOL, ATOL_SCALE, BAD) == (2e-3, 5e-3, 5e-4, 1e-2)
    q = problem("Q1")
    used = hand_over(dirty(new_engine()), q)
    fresh = hand_over(new_engine(), q)
    n = q["n"]
    for e in (fresh, used):
        assert not e.deterministic
        e.forward()
    torch.cuda.synchronize()
    for e in (fresh, used):
        assert e.overflow.tolist() == [0, 0, 0, 0]
    for k in ("render", "final_T", "n_contrib"):
        assert torch.equal(getattr(fresh, k), getattr(used, k)), f"forward after H: {k} differs"
    assert torch.equal(fresh.rec[:n], used.rec[:n]), "forward after H: the records differ"
    assert used.K == fresh.K > 0
    assert all(torch.equal(x, y) for x, y in zip(_lists(fresh), _lists(used))), "forward after H: a tile's sorted list differs"
    res = gradient_of_next_iteration(used, q["sc"], q["img"], q["dep"])
    check_gradients(res, {}, "[Q1 after H, default mode] ", camera=False)


# ------------------------------------------------------------------------------------------------ C: outside the inputs
@pytest.mark.parametrize("name", ["Q1", "Q3"])
def test_what_lies_outside_the_inputs_is_not_read_and_every_output_is_fully_written(name):
    """Two new engines on Q.  In one of them, before the first iteration: rows [N, cap) of ``params`` are the poison row (a
    12-pixel magenta splat in the middle of the view: 1510 pixels of the oracle's render change if row N is read), of
    ``adam_m`` / ``adam_v`` 1.0, of ``rec`` a visible 70-pixel record of H; [N, cap) of the regulariser inputs (Q3) 1.0 and of
    ``row_flags`` 0xFF; the float outputs render, final_T, d_render, err_px, sums and d_extr NaN.  Four deterministic iterations,
    bit for bit.

    Deliberately NOT poisoned: the workspace (its pool counter must start at zero, FitEngine._alloc_pairs) and every buffer
    that holds indices or loop bounds (ids, tile_range, tile_offsets, n_contrib): a kernel that did read those would be led out
    of bounds, and no test may be able to fault a device that others share.  For those buffers the stale but valid contents the
    hand-over tests leave there are the test."""
    q = problem(name)
    n = q["n"]
    h = history_problem(0)
    donor = hand_over(new_engine(), h)
    donor.forward()
    wide = int(torch.argmax(donor.rec[:h["n"], 11].contiguous().view(torch.int32)))
    record = donor.rec[wide].clone()
    assert int(record[11:12].view(torch.int32)) >= 60 and float(record[9]) > 0          # radius in pixels, depth
    fresh, other = hand_over(new_engine(), q), hand_over(new_engine(), q)
    other.params[n:, :14] = poison_row(q["sc"]).to(DEV)
    other.adam_m[n:] = 1.0
    other.adam_v[n:] = 1.0
    other.rec[n:] = record
    for k in ("flow_w", "still_w", "flow_target", "still_target"):
        assert (getattr(other, k) is not None) == (name == "Q3")
        if getattr(other, k) is not None:
            getattr(other, k)[n:] = 1.0
    if other.row_flags is not None:
        other.row_flags[n:] = 0xFF
    for k in ("render", "final_T", "d_render", "err_px", "sums", "d_extr"):
        getattr(other, k).fill_(float("nan"))
    run_and_compare(fresh, other, f"{name}, poisoned behind N")
    for k in ("d_render", "err_px"):                                          # (poisoned outputs that OUT does not list)
        assert k not in OUT and torch.equal(getattr(fresh, k), getattr(other, k)), k


# ------------------------------------------------------------------------------------------------ D: transplant
def transplant(a, b):
    """``b`` receives the declared state of ``a`` and nothing else: the live rows with their moments, camera and depth affine
    with theirs, the step counter, the intrinsics, every hyper-parameter, the targets, the regularisers."""
    n = a.N
    b.set_splats({k: v.clone() for k, v in a.views().items()})
    for k in ("adam_m", "adam_v"):
        getattr(b, k)[:n].copy_(getattr(a, k)[:n])
    for k in ("pose", "pose_m", "pose_v", "depth_ab", "ab_m", "ab_v", "step", "intr"):
        getattr(b, k).copy_(getattr(a, k))
    for k, _ in type(a.hp)._fields_:
        setattr(b.hp, k, getattr(a.hp, k))
    cut = lambda t: None if t is None else t[:n]
    b.set_regularisers(cut(a.flow_target), cut(a.flow_w), cut(a.still_target), cut(a.still_w), cut(a.row_flags))
    b.set_targets(a.gt_rgb, a.gt_depth, a.keep)
    assert a.foot_flags is None
    return b


def test_the_declared_state_of_a_running_fit_continues_alike_on_a_new_engine():
    """Engine ``a`` runs five iterations on H -- three in default mode, one from a graph, the odd transition edit in between.
    A new engine receives its declared state (``transplant``) and both go on for four deterministic iterations: whatever
    else ``a`` holds by then (stamped pair rows of five forwards, its pool and queues, its graphs) changes no bit."""
    h = history_problem(0)
    a = hand_over(new_engine(), h)
    a.iteration()
    a.iteration()
    apply_transition(a.views(), h["sc"]["rows"], 1, f=float(h["sc"]["intr"][0]))
    a.invalidate_regions()
    a.iteration()
    a.deterministic = True
    a.iteration(use_graph=True)
    a.iteration()
    a.check_overflow()
    assert int(a.step.item()) == 5 and a.graphs.live
    b = transplant(a, new_engine())
    a.invalidate_regions()
    run_and_compare(b, a, "H, transplanted after five iterations")


def test_the_declared_state_continues_alike_after_the_engine_has_grown():
    """``a`` starts with room for 1024 rows and the first 1000 of H, runs two iterations, grows (ensure_capacity(1500): new
    buffers of 2048 rows, a new workspace) and gets 500 rows appended the way a densification appends them
    (Trainer.densification_postfix: in place behind the live rows, set_count; then the flags of FusedStage.one_iteration:
    fresh splat moments, constant lr, the camera no longer stepped).  ``b``: a new engine of 2048 rows, same K_cap."""
    from gflow_amd.fused import COLS
    h = history_problem(0, rows=1000)
    full = history_problem(0)["sc"]["raw"]
    a = hand_over(new_engine(1024), h)
    a.iteration()
    a.iteration()
    n0, k = a.N, 500
    a.ensure_capacity(n0 + k)
    assert a.cap == 2048 and a.K_cap == K_CAP
    rows = a.params[n0:n0 + k]
    for name, (c0, c1) in COLS.items():
        rows[:, c0:c1] = full[name][n0:n0 + k].to(DEV)
    rows[:, 14:] = 0
    a.set_count(n0 + k)
    a.reset_optimizer(splats=True, camera=False)
    a.hp.total_iters = 0
    a.hp.step_camera = 0
    b = transplant(a, new_engine(2048))
    a.invalidate_regions()
    run_and_compare(b, a, "H, grown from 1000 to 1500 rows")
    a.check_overflow()
    assert a.pairs_grown == 0


# ------------------------------------------------------------------------------------------------ E: the pooled operator
def test_a_pooled_render_engine_gives_what_a_new_one_gives(monkeypatch):
    """gflow_amd.render.render() keeps its engines in a pool.  Under torch's deterministic switch: H's 1668 rows under H's
    camera over bg 0.2 with a backward, then Q1's 600 rows under the "general" camera over bg 0 with a backward through random
    weights on all four outputs -- on the engine the first call left.  The same Q1 call on an empty pool: the four outputs,
    the five attribute gradients and d_extr are bit-equal."""
    import gflow_amd.render as R
    h, q = history_problem(0), problem("Q1")
    s = q["activated"]
    g = torch.Generator().manual_seed(77)
    shapes = dict(rgb=(3, H, W), depth_map=(1, H, W), uv=(q["n"], 2), depth=(q["n"], 1))
    weights = {k: torch.randn(v, generator=g).to(DEV) for k, v in shapes.items()}

    def call(act, intr, extr, bg, weights=None):
        leaves = {k: v.to(DEV).clone().requires_grad_(True) for k, v in zip(NAMES, act)}
        extr = extr.to(DEV).clone().requires_grad_(True)
        out = R.render(leaves, dict(intr=intr.to(DEV), extr=extr, W=W, H=H), bg=bg)
        sum((out[k] * (1.0 if weights is None else weights[k])).sum() for k in shapes).backward()
        R.check_overflow()
        return [out[k].detach() for k in shapes] + [leaves[k].grad for k in NAMES] + [extr.grad]

    q1 = lambda: call([s[k] for k in NAMES], s["intr"], s["extr"], 0.0, weights)
    before, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        monkeypatch.setattr(R, "_POOL", {})
        call(FO.activate(h["sc"]["raw"]), h["sc"]["intr"], LO.pose_to_extr(POSE), 0.2)
        used = q1()
        assert sum(len(v) for v in R._POOL.values()) == 1                      # one engine served both calls
        monkeypatch.setattr(R, "_POOL", {})
        fresh = q1()
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn_only)
    names = tuple(shapes) + tuple("d_" + k for k in NAMES) + ("d_extr",)
    for name, x, y in zip(names, used, fresh):
        assert torch.equal(x, y), f"render() on a pooled engine: {name} differs from a new engine's"
        assert bool(torch.isfinite(x).all()), name
    assert float(used[4].abs().max()) > 0 and float(used[9].abs().max()) > 0
