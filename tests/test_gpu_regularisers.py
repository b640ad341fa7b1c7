"""The per-splat launch's regularisers (fused_preprocess_bwd_adam_kernel, gfl_fit_splat.hip: flow, still, scale, variance) and
its gradient masks ALONE against float64, term by term and stage by stage (``-m gpu``): rows, pose and d_extr.

Isolation: lambda_rgb = lambda_depth = 0 -- the loss launch writes a zero d_render, every pair row gathers to zero, and what
reaches Adam is the term alone (test_without_a_term_nothing_reaches_adam holds that).  Gradients are read from the first
moments after ONE iteration from a fresh optimiser: m = (1 - beta1) g.  The reference is tests/regulariser_ref.py (tied to
oracle/loss_oracle.py by tests/test_regularisers_host.py); the bounds are built from it on each case's own inputs:

  rows, per column group    err = max |device - float64| <= 4 gap + 32 * 2^-24 * max |float64 reference of the group|
  pose / d_extr, value k    err_k <= 4 gap_k + rows * 2^-24 * S_k,   S_k = sum_i |d t_i / d k|  (any order of a float32 sum)

with gap = max |float32 reference - float64 reference| of the quantity (regulariser_ref.row_bounds, pose_bounds).

Measured on an MI355X (the run's log has err / gap / bound of every case; ranges over the cases of a kind):
  quantity (cases)                                    err                gap                bound              err / bound
  rows, flow term, d_xyz (joint)                      1.0e-08            1.0e-08            5.1e-08            0.20
  rows, still term, d_xyz (joint)                     4.5e-09            4.1e-09            7.7e-08            0.06
  rows, scale term, d_xyz | d_scale (joint)           6.2e-11 | 1.9e-10  6.3e-11 | 2.0e-10  1.1e-09 | 3.2e-09  0.06
  rows, variance term, d_scale (joint)                1.7e-08            1.1e-08            6.1e-08            0.28
  pose | d_extr, flow term (camera-only, joint)       1.3e-07 .. 2.1e-07 | 6.7e-08 .. 9.5e-08   bounds 3.9e-05 .. 4.1e-05 | 1.7e-05   <= 0.01
  pose | d_extr, scale term (camera-only, joint)      1.3e-09 | 9.7e-10 .. 2.9e-09              bounds 2.3e-06 .. 2.8e-06             <= 0.01
  sizes 1 .. 1025, scale term: rows | pose, d_extr    4.3e-11 .. 2.7e-08 | 5.5e-10 .. 3.2e-09   bounds 7.3e-10 .. 5.5e-07 | 1.2e-08 .. 4.1e-06   <= 0.08 | <= 0.22
  sizes 1 .. 1025, flow term: rows | pose, d_extr     5.3e-09 .. 3.8e-07 | 1.1e-07 .. 1.1e-06   bounds 3.1e-08 .. 2.8e-06 | 2.5e-06 .. 6.0e-05   <= 0.17 | <= 0.22
  additivity, d_xyz | d_scale | pose | d_extr         2.9e-09 | 2.4e-09 | 1.3e-08 | 7.5e-09     bounds 1.3e-07 | 6.4e-08 | 4.3e-05 | 1.7e-05     <= 0.04 (spread 0)
  trainer, camera-only, pose (fused | operators)      1.8e-06 | 6.8e-07  4.0e-06 | 1.4e-05  1.9e-03            <= 0.01
  trainer, joint, d_xyz | d_scale (fused)             1.3e-07 | 4.1e-07  1.3e-07 | 3.6e-07  5.1e-07 | 1.5e-06  0.25 | 0.28
  trainer, joint, d_xyz | d_scale (operators)         4.9e-08 | 3.1e-07  1.4e-07 | 2.4e-07  5.4e-07 | 9.5e-07  0.09 | 0.32
  every quantity whose bound is 0 (a term's other columns, the still and variance terms' pose and d_extr, all rows of the
  camera-only stage, rotation / opacity / rgb in the additivity run): err exactly 0.
Before the variance term skipped rows of three equal scales (gfl_fit_splat.hip), six of the ten equal-scale rows had
d_scale off by 1.0e-02 (bound 6.1e-08): (s + s + s) / 3 is not s in float32.
"""
import pytest
import torch

from tests import regulariser_ref as RR
from tests.test_gpu_parity import observe

pytestmark = pytest.mark.gpu
DEV = "cuda"

_IMG = {}


def _image(W, H):
    if (W, H) not in _IMG:
        _IMG[(W, H)] = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(5))
    return _IMG[(W, H)]


def _engine(sc, stage, lam, render=False, deterministic=False, **hyper):
    """Like _engine of tests/test_gpu_fused.py, with K_cap = 65536 (the default workspace is hundreds of MB per engine) and the
    stage's side inputs as the library's interface takes them: pre-divided weights, targets, row flags.  ``lam``: {term: weight}
    of the terms that are on; ``render``: lambda_rgb = 1 instead of 0; ``deterministic``: FitEngine's mode."""
    from gflow_amd.fused import FitEngine
    N, M = sc["N"], sc["M"]
    eng = FitEngine(sc["W"], sc["H"], capacity=max(2 * N, 1024), device=DEV, K_cap=65536, deterministic=deterministic)
    eng.set_splats({k: v.to(DEV) for k, v in sc["raw"].items()})
    eng.intr.copy_(sc["intr"].to(DEV))
    eng.pose.copy_(sc["pose"].to(DEV))
    eng.set_targets(_image(sc["W"], sc["H"]), None)
    hp = eng.hp
    hp.lambda_rgb, hp.lambda_depth = (1.0 if render else 0.0), 0.0
    hp.lambda_flow, hp.lambda_still = lam.get("flow", 0.0), lam.get("still", 0.0)
    hp.lambda_scale, hp.lambda_var = lam.get("scale", 0.0), lam.get("var", 0.0)
    hp.lr, hp.freeze_rgb = 1e-3, 1
    if stage == "camera_only":
        hp.freeze_all_splats, hp.lr_camera, hp.step_camera = 1, 1e-3, 1
    else:
        hp.freeze_all_splats, hp.lr_camera, hp.step_camera = 0, 0.0, 2          # (2: the pose gradient is wanted, nothing moves)
    for k, v in hyper.items():
        setattr(hp, k, v)
    sel = RR.flow_rows(sc, stage)
    eng.set_regularisers(flow_target=RR.flow_target(sc), flow_w=sel.float() / (2.0 * sel.sum().clamp(min=1)),
                         still_target=sc["last_xyz"], still_w=sc["last_still"].float() / sc["last_still"].sum().clamp(min=1),
                         row_flags=sc["still"].to(torch.uint8) | 2)          # bit 0: still, bit 1: the row has a label
    eng.reset_optimizer()
    return eng


def _read(eng, n):
    """(rows (n, 14), pose (7,), d_extr (12,)) float64 on the CPU: the gradients the iteration used, m / (1 - beta1)"""
    c = 1.0 - float(eng.hp.beta1)
    return (eng.adam_m[:n, :14].double().cpu() / c, eng.pose_m.double().cpu() / c, eng.d_extr.double().cpu())


_RUNS = {}


def _run(term, stage):
    """One iteration of the term alone on the shared scene: (engine, rows, pose, d_extr, params before).  Run once per case."""
    if (term, stage) not in _RUNS:
        sc = RR.shared_scene()
        eng = _engine(sc, stage, {term: RR.LAMBDAS[term]})
        before = eng.params[:sc["N"]].clone()
        eng.iteration()
        eng.check_overflow()
        _RUNS[(term, stage)] = (eng, *_read(eng, sc["N"]), before)
    return _RUNS[(term, stage)]


def _hold_rows(tag, got, r64, rb, fails):
    for k, (a, b) in RR.GROUPS.items():
        err = (got[:, a:b] - r64["rows"][:, a:b]).abs().max().item()
        gap, bound = rb[k]
        observe(f"{tag} d_{k}: err {err:.2e}  gap {gap:.2e}  bound {bound:.2e}")
        if not err <= bound:
            fails.append(f"{tag} d_{k}: err {err:.2e} > bound {bound:.2e}")


def _hold_pose(tag, got_pose, got_extr, r64, pb, fails):
    for name, got in (("pose", got_pose), ("d_extr", got_extr)):
        if got is None:
            continue
        err = (got - r64[name]).abs()
        gap, bound = pb[name]
        j = int((err - bound).argmax())
        observe(f"{tag} {name}: err {err.max().item():.2e}  gap {gap.max().item():.2e}  bound {bound.max().item():.2e}"
                f"  (nearest its bound [{j}]: err {err[j].item():.2e}, gap {gap[j].item():.2e}, bound {bound[j].item():.2e})")
        if not bool((err <= bound).all()):
            fails.append(f"{tag} {name}: err {err.tolist()} > bound {bound.tolist()}")


def test_without_a_term_nothing_reaches_adam():
    """lambda_rgb = lambda_depth = 0 and all four regularisers at 0, their side inputs in place: one iteration leaves the
    moments, the rows and the pose's moment exactly as they were -- what the other tests read is the term alone."""
    sc = RR.shared_scene()
    for stage in RR.STAGES:
        eng = _engine(sc, stage, {}, lr_camera=1e-3)
        p0 = eng.params.clone()
        eng.iteration()
        eng.check_overflow()
        assert int(eng.step.item()) == 1
        assert float(eng.d_render.abs().max()) == 0.0
        assert torch.equal(eng.params, p0), stage
        assert float(eng.adam_m.abs().max()) == 0.0 and float(eng.adam_v.abs().max()) == 0.0, stage
        assert float(eng.pose_m.abs().max()) == 0.0 and float(eng.d_extr.abs().max()) == 0.0, stage
        assert torch.equal(eng.pose.cpu(), sc["pose"]), stage


@pytest.mark.parametrize("stage", RR.STAGES)
@pytest.mark.parametrize("term", RR.TERMS)
def test_rows_of_a_term_alone_match_float64(term, stage):
    """All 14 columns of all 700 rows under the per-row bound; exactly zero where the term cannot reach: other columns, rows
    the flow term selects but the camera culls, rows beyond last_num and beyond the labels, dead still rows, rows at zero
    distance, the rgb columns, and everything in the camera-only stage (rows and both moments bit-unchanged there)."""
    sc = RR.shared_scene()
    N, M = sc["N"], sc["M"]
    eng, rows, _, _, before = _run(term, stage)
    r32, r64, rb, pb = RR.shared_reference(sc, term, stage)
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(eng.params[:N]).all())
    fails = []
    _hold_rows(f"[{term}, {stage}]", rows, r64, rb, fails)
    must = RR.untouched(sc, term, stage)
    assert bool((r64["rows"][must] == 0).all()), "the reference disagrees with the scene's classes"
    assert bool((rows[must] == 0).all()), f"{int((rows[must] != 0).sum())} entries the {term} term cannot touch are not zero"
    assert bool((rows[r64["rows"] == 0] == 0).all())
    assert bool((rows[:, 11:14] == 0).all())                                      # freeze_rgb
    if term in ("flow", "still"):
        assert bool((rows[M:] == 0).all())                                          # beyond last_num / the labelled rows
    if term == "flow":
        sel = RR.flow_rows(sc, stage)
        assert bool((rows[:M][sel & sc["culled_now"][:M]] == 0).all())
    if term == "still":
        assert bool((rows[:M][sc["still_dead"]] == 0).all()) and bool((rows[:M][sc["zero_distance"]] == 0).all())
    if term == "var":
        assert bool((rows[sc["equal_scale"]][:, 3:6] == 0).all()), rows[sc["equal_scale"]][:, 3:6]
    if term in ("var", "scale"):
        assert bool((rows[:, 3:6][sc["zero_scale_comp"]] == 0).all())
        assert bool(torch.isfinite(rows[sc["equal_scale"] | sc["zero_scale"]]).all())
    if stage == "camera_only":
        assert torch.equal(eng.params[:N], before)
        assert float(eng.adam_m.abs().max()) == 0.0 and float(eng.adam_v.abs().max()) == 0.0
    else:
        touched = (rows != 0).any(dim=1)
        assert int(touched.sum()) >= 5 and not torch.equal(eng.params[:N], before)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("term", RR.TERMS)
def test_pose_gradient_of_a_term_alone_in_the_camera_only_stage(term):
    """freeze_all_splats = 1, lr_camera = 1e-3: the 7 pose values and the 12 of d_extr against float64; the still and the
    variance term give exactly zero (their bounds are zero)."""
    sc = RR.shared_scene()
    eng, _, pose, d_extr, _ = _run(term, "camera_only")
    r32, r64, rb, pb = RR.shared_reference(sc, term, "camera_only")
    fails = []
    _hold_pose(f"[{term}, camera_only]", pose, d_extr, r64, pb, fails)
    if term in ("still", "var"):
        assert float(pose.abs().max()) == 0.0 and float(d_extr.abs().max()) == 0.0
        assert torch.equal(eng.pose.cpu(), sc["pose"])
    else:
        assert float(pose.abs().max()) > 0.0 and not torch.equal(eng.pose.cpu(), sc["pose"])
    assert int(eng.step.item()) == 1
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("term", RR.TERMS)
def test_pose_gradient_of_a_term_alone_in_the_joint_stage(term):
    """step_camera = 2 (lr_camera = 0, gradient wanted): the same bounds; with step_camera = 1 no pose gradient is formed --
    d_extr exactly zero, pose_m unchanged -- and the rows get the same gradient."""
    sc = RR.shared_scene()
    eng, rows, pose, d_extr, _ = _run(term, "joint")
    r32, r64, rb, pb = RR.shared_reference(sc, term, "joint")
    fails = []
    _hold_pose(f"[{term}, joint]", pose, d_extr, r64, pb, fails)
    assert torch.equal(eng.pose.cpu(), sc["pose"]) and int(eng.step.item()) == 1
    if term in ("still", "var"):
        assert float(pose.abs().max()) == 0.0 and float(d_extr.abs().max()) == 0.0
    short = _engine(sc, "joint", {term: RR.LAMBDAS[term]}, step_camera=1)
    short.iteration()
    rows1, pose1, d_extr1 = _read(short, sc["N"])
    assert float(d_extr1.abs().max()) == 0.0 and float(short.pose_m.abs().max()) == 0.0 and int(short.step.item()) == 1
    assert torch.equal(rows1, rows)                      # (no render: nothing unordered is summed, the two orders give the same bits)
    assert torch.equal(short.params[:sc["N"]], eng.params[:sc["N"]])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 512, 513, 1025])
@pytest.mark.parametrize("term", ["scale", "flow"])
def test_sizes_at_the_workgroup_edges(term, n):
    """The first n rows of a 1025-row scene, min(n, 600) of them labelled, joint stage: the workgroup edges of the per-splat
    launch (256) and of the preprocess launch's scale-row partials (512 rows, two partials per block).  A count that is off
    by one moves the term by 1 / count of itself."""
    sc = RR.shared_scene(1025, 600, 5, first=n, lead=True)
    assert int(RR.scale_rows(sc, "joint").sum()) >= 1 and int(RR.flow_rows(sc, "joint").sum()) >= 1
    eng = _engine(sc, "joint", {term: RR.LAMBDAS[term]})
    eng.iteration()
    eng.check_overflow()
    rows, pose, d_extr = _read(eng, n)
    r32, r64, rb, pb = RR.shared_reference(sc, term, "joint")
    assert float(r64["rows"].abs().max()) > 0
    fails = []
    _hold_rows(f"[{term}, {n} rows]", rows, r64, rb, fails)
    _hold_pose(f"[{term}, {n} rows]", pose, d_extr, r64, pb, fails)
    assert bool((rows[r64["rows"] == 0] == 0).all())
    assert float(eng.adam_m[n:].abs().max()) == 0.0          # nothing beyond the live rows
    assert not fails, "\n".join(fails)


def test_the_terms_add_to_the_render_gradient():
    """Render on (lambda_rgb = 1), all four terms, joint stage: the gradient minus that of an engine without the terms is the
    sum of the four isolated gradients -- to the sum of their bounds plus the run-to-run spread of the render's gradient,
    measured from two engines without terms.  The engines run in the deterministic mode: in the default mode the backward
    blend's LDS adds are unordered, the difference of two runs is ONE draw of that spread, and on the columns no term
    touches (rotation, opacity: bound = spread alone) the error is another draw of the same quantity -- it exceeds the
    measured one every other time.  With a fixed order the measured spread is exactly 0 and those columns agree bit for bit."""
    sc = RR.shared_scene()
    N = sc["N"]
    got = []
    for lam in (RR.LAMBDAS, {}, {}):
        eng = _engine(sc, "joint", dict(lam), render=True, deterministic=True)
        eng.iteration()
        eng.check_overflow()
        got.append(_read(eng, N))
    (rows_t, pose_t, extr_t), (rows_0, pose_0, extr_0), (rows_1, pose_1, extr_1) = got
    assert float(rows_0[:, 6:11].abs().max()) > 0 and float(pose_0.abs().max()) > 0      # the render is really on
    assert bool((rows_t[:, 11:14] == 0).all()) and bool((rows_0[:, 11:14] == 0).all())   # freeze_rgb, with the render on
    refs = [RR.shared_reference(sc, t, "joint") for t in RR.TERMS]
    iso = [_run(t, "joint") for t in RR.TERMS]
    fails = []
    for k, (a, b) in RR.GROUPS.items():
        spread = (rows_0[:, a:b] - rows_1[:, a:b]).abs().max().item()
        bound = sum(r[2][k][1] for r in refs) + spread
        err = ((rows_t[:, a:b] - rows_0[:, a:b]) - sum(i[1][:, a:b] for i in iso)).abs().max().item()
        observe(f"[additivity] d_{k}: err {err:.2e}  spread {spread:.2e}  bound {bound:.2e}")
        if not err <= bound:
            fails.append(f"[additivity] d_{k}: err {err:.2e} > bound {bound:.2e}")
    for name, t, z, z1, j in (("pose", pose_t, pose_0, pose_1, 2), ("d_extr", extr_t, extr_0, extr_1, 3)):
        spread = (z - z1).abs()
        bound = sum(r[3][name][1] for r in refs) + spread
        err = ((t - z) - sum(i[j] for i in iso)).abs()
        observe(f"[additivity] {name}: err {err.max().item():.2e}  spread {spread.max().item():.2e}  bound {bound.max().item():.2e}")
        if not bool((err <= bound).all()):
            fails.append(f"[additivity] {name}: err {err.tolist()} > bound {bound.tolist()}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ the trainer's two paths to the same terms
def _second_frame_trainer(fused):
    """test_camera_only_phase_moves_the_pose_not_the_splats' set-up, shorter: a first frame fitted for six iterations at
    96 x 128 with 1 500 splats, the second frame's targets set."""
    from gflow_amd import synthetic as S
    from gflow_amd.trainer import SimpleGaussian
    f0, f1 = S.make_clip(2, 96, 128, seed=0)
    tr = SimpleGaussian(f0["image"], f0["depth"], num_points=1500, device=DEV, seed=0, fused=fused)
    tr.load_camera(focal=f0["focal"], pp=f0["pp"])
    tr.init_gaussians_from_image(f0["image"], f0["depth"], num_points=1500)
    tr.train(iterations=6, lr=4e-3, lambda_rgb=1.0, lambda_depth=1e-2, lambda_var=10.0, move_mask=f0["move_mask"],
             densify_interval=0, snapshot_interval=0)
    tr.set_gt_image(f1["image"]); tr.set_gt_depth(f1["depth"]); tr.set_gt_flow(f0["flow"])
    return tr, f1


def _held_by(tr):
    """What the trainer holds at the start of a stage, as a scene of tests/regulariser_ref.py (float32, on the CPU)."""
    n = tr.current_pts_num()
    cpu = lambda t: t.detach().clone().cpu()
    assert tr.last_num == tr.last_uv.shape[0] == tr.last_xyz.shape[0] == tr.last_still_mask.shape[0] <= tr.still_mask.shape[0] <= n
    return dict(raw={k: cpu(tr._attributes[k]).reshape(n, -1) for k in RR.ATTRS}, intr=cpu(tr.intr), pose=cpu(tr.pose),
                W=tr.W, H=tr.H, N=n, M=tr.last_num, still=cpu(tr.still_mask), last_still=cpu(tr.last_still_mask),
                last_xyz=cpu(tr.last_xyz), last_uv=cpu(tr.last_uv), gt_flow=cpu(tr.gt_flow))


def _trainer_rows(tr, fused):
    n = tr.current_pts_num()
    if fused:
        return tr.engine.adam_m[:n, :14].double().cpu() / (1.0 - float(tr.engine.hp.beta1))
    c = 1.0 - float(torch.tensor(0.9, dtype=torch.float32))
    state = tr.optimizer.state
    return torch.cat([state[id(tr._attributes[k])]["exp_avg"].reshape(n, -1) if id(tr._attributes[k]) in state else
                      torch.zeros_like(tr._attributes[k]).reshape(n, -1) for k in RR.ATTRS], dim=1).double().cpu() / c


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_hands_the_flow_term_to_the_camera_only_stage(fused):
    """make_stepper(camera_only=True, lambda_flow=0.01, lr_camera=1e-3) with the image terms off, one iteration: the pose
    gradient is the float64 restatement's on what the trainer holds (_flow_selection, FusedStage._set_regularisers /
    OperatorStage's expressions against trainer.py:511-528), and no row moves."""
    tr, f1 = _second_frame_trainer(fused)
    before = {k: v.detach().clone() for k, v in tr._attributes.items()}
    st = tr.make_stepper(iterations=20, camera_only=True, lambda_rgb=0.0, lambda_depth=0.0, lambda_flow=0.01, lr_camera=1e-3,
                         move_mask=f1["move_mask"], densify_interval=0, snapshot_interval=0)
    sc = _held_by(tr)
    sel = RR.flow_rows(sc, "camera_only")
    print(f"fused={fused}: {int(sel.sum())} of {sc['M']} rows in the flow term, {int(sc['still'].sum())} still")
    assert int(sel.sum()) >= 5 and int((~sc["still"]).sum()) >= 5
    st()
    c = 1.0 - float(torch.tensor(0.9, dtype=torch.float32))
    if fused:
        pose_g, d_extr = tr.engine.pose_m.double().cpu() / c, tr.engine.d_extr.double().cpu()
    else:
        pose_g, d_extr = tr.optimizer.state[id(tr.pose)]["exp_avg"].double().cpu() / c, None
    r64 = RR.reference(sc, "flow", "camera_only", torch.float64)
    r32 = RR.float32_references(sc, "flow", "camera_only")
    fails = []
    _hold_pose(f"[trainer, fused={fused}, camera_only]", pose_g, d_extr, r64, RR.pose_bounds(r32, r64, sc["N"]), fails)
    assert float(pose_g.abs().max()) > 0
    for k in before:
        assert torch.equal(before[k], tr._attributes[k].detach()), k
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_hands_the_terms_to_the_joint_stage(fused):
    """The joint stepper with lambda_still = 10, lambda_flow = 0.01, lambda_var = 10 and the image terms off, one iteration
    on a rebuilt trainer: the rows' gradient is the restatement's sum of the three terms on what the trainer holds after
    its warp of the moving splats.  Here the two still masks coincide, as in the reference (trainer.py:505 against :543-546):
    the still term contributes exactly nothing."""
    tr, f1 = _second_frame_trainer(fused)
    st = tr.make_stepper(iterations=20, lambda_rgb=0.0, lambda_depth=0.0, lambda_flow=0.01, lambda_still=10.0, lambda_var=10.0,
                         densify_interval=0, snapshot_interval=0)
    sc = _held_by(tr)
    assert torch.equal(sc["still"][:sc["M"]], sc["last_still"])
    sel = RR.flow_rows(sc, "joint")
    print(f"fused={fused}: {int(sel.sum())} of {sc['M']} rows in the flow term, {int(sc['last_still'].sum())} in the still term")
    assert int(sel.sum()) >= 5 and int(sc["last_still"].sum()) >= 5
    st()
    rows = _trainer_rows(tr, fused)
    terms = ("flow", "still", "var")
    r64 = RR.reference(sc, terms, "joint", torch.float64, jacobian=False)
    r32 = RR.float32_references(sc, terms, "joint")
    without = RR.reference(sc, ("flow", "var"), "joint", torch.float64, jacobian=False)
    assert torch.equal(without["rows"], r64["rows"])                         # the still term: exactly nothing, masked
    fails = []
    _hold_rows(f"[trainer, fused={fused}, joint]", rows, r64, RR.row_bounds(r32, r64), fails)
    assert bool((rows[:sc["M"], 0:3][sc["last_still"]] == 0).all())          # the rows the still term acts on: xyz frozen
    assert bool((rows[:sc["M"], 0:3][~sel] == 0).all())                      # ... and no other term reaches an xyz outside the flow rows
    assert bool((rows[:, 11:14] == 0).all()) and bool((rows[:, 6:11] == 0).all())
    assert float(rows[:, 0:3].abs().max()) > 0 and float(rows[:, 3:6].abs().max()) > 0
    assert not fails, "\n".join(fails)
