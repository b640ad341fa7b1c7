"""The problems of tests/test_gpu_engine_history.py on the CPU: a FitEngine that has been through another fit (the history
scene H: the transition scene of tests/test_running_engine_host.py, whose rows move between the three pair-row layouts) is
handed a smaller problem Q and must give what a new engine gives.  Here, with the oracle only: H leaves wide rows behind at
every step, every Q is smaller than H in rows and in pairs (so whatever stale index a kernel might read was valid for H, in
buffers sized for H), the Q problems are what they claim to be, and the poison row the GPU tests write behind the live rows
would be seen if it were ever read."""
import math

import torch

from oracle import fit_oracle as FO
from oracle import loss_oracle as LO
from oracle import msplat_oracle as MO
from tests.scenes import ATTRS, REGIME_LAMBDAS, assert_regime, camera_scene, layout_class, oracle_front_end
from tests.test_gpu_fused import POSE, _raw_from_scene
from tests import test_running_engine_host as RH
from tests.test_running_engine_host import targets, transition_case

W, H = 168, 120
CAP = 4096
K_CAP = 22880                 # twice the largest pair count of the oracle front end over H at steps 0 .. 2 and over the Q problems
Q_ROWS, Q_SEED, Q_TARGET_SEED = 600, 79, 12
# 600 rows are few for the "general" camera's regime (assert_regime: 100 live rows on each clamp branch): with camera_scene's
# defaults no seed of 0 .. 299 has more than 72 on the y branch (the clamp takes rows in the image's top 6 pixel rows and above).
# Wider splats over a wider field, none behind the camera: seed 79 has 129 / 105 / 26 on the x / y / both branches.
Q_SCENE = dict(sigma_px=4.0, spread=1.3, behind=0.0)
STEPS = (0, 1, 2)
NAMES = ("Q1", "Q2", "Q3")
LAM_FLOW, LAM_STILL, LAM_SCALE = 0.01, 10.0, 0.5          # tests/test_gpu_fused.py: the regulariser and scale-term tests
# every field of FitHyper a stage sets (gflow_amd/stage.py: FusedStage.__init__), as a first-frame stage sets them
FIRST_FRAME = dict(bg=0.0, **REGIME_LAMBDAS, lr=2e-3, lr_camera=0.0, lambda_scale=0.0, lr_end_factor=0.1, total_iters=100,
                   freeze_rgb=0, freeze_all_splats=0, step_camera=1, lambda_flow=0.0, lambda_still=0.0)
CAMERA_ONLY = dict(FIRST_FRAME, freeze_rgb=1, freeze_all_splats=1, lr_camera=1e-3)
JOINT = dict(FIRST_FRAME, freeze_rgb=1, lambda_flow=LAM_FLOW, lambda_still=LAM_STILL, lambda_scale=LAM_SCALE)

_CACHE = {}


def disc(cx, cy, r):
    """(H, W) bool: the pixels within ``r`` of (cx, cy)"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def joint_inputs(raw, intr, seed):
    """Flow and still targets, their weights and the row flags of a joint stage for the raw rows ``raw``, built as in
    tests/test_gpu_fused.py:test_fused_regularisers_and_masks (the last 100 rows carry no label, as rows appended later):
    the arguments of FitEngine.set_regularisers, and the two selections."""
    n = raw["xyz"].shape[0]
    g = torch.Generator().manual_seed(seed)
    uv0, _ = MO.project_point(FO.activate(raw)[0], intr, LO.pose_to_extr(POSE), W, H)
    last_uv = uv0 + torch.randn(n, 2, generator=g)
    gt_flow = torch.randn(H, W, 2, generator=g)
    still = torch.rand(n, generator=g) > 0.5
    last_xyz = raw["xyz"] + 0.01 * torch.randn(n, 3, generator=g)
    and_mask = (last_uv[:, 0] > 0) & (last_uv[:, 0] < W - 1) & (last_uv[:, 1] > 0) & (last_uv[:, 1] < H - 1) & ~still
    yx = last_uv.long()
    gt_f = gt_flow[yx[:, 1].clamp(0, H - 1), yx[:, 0].clamp(0, W - 1)]
    flags = still.to(torch.uint8)
    flags[:n - 100] |= 2
    reg = dict(flow_target=last_uv + gt_f, flow_w=and_mask.float() / (2.0 * and_mask.sum()), still_target=last_xyz,
               still_w=still.float() / still.sum(), row_flags=flags)
    return reg, and_mask, still


def _problem(name, sc, img, dep, hp, keep=None, foot=None, reg=None, **more):
    return dict(name=name, sc=sc, n=sc["raw"]["xyz"].shape[0], pose=POSE, img=img, dep=dep, hp=hp, keep=keep, foot=foot,
                reg=reg or {}, **more)


def history_problem(step=0, rows=None):
    """H: the transition scene after ``step`` edits with its targets, as a first-frame problem (``rows``: its first rows only)"""
    case = transition_case(step)
    sc = case["sc"]
    if rows is not None:
        sc = dict(sc, raw={k: v[:rows].contiguous() for k, v in sc["raw"].items()})
    return _problem(f"H{step}", sc, case["img"], case["dep"], FIRST_FRAME, fe=case["fe"] if rows is None else None)


def problem(name):
    """Q1: 600 rows under the "general" camera, a first-frame stage; Q2: the same rows in a camera-only stage with a keep mask
    (a disc); Q3: the same rows in a joint stage with flow, still and scale terms (once per process)."""
    if "scene" not in _CACHE:
        s = camera_scene(Q_ROWS, W, H, "general", extr=LO.pose_to_extr(POSE), seed=Q_SEED, **Q_SCENE)
        with torch.random.fork_rng():
            torch.manual_seed(Q_SEED)                      # (_raw_from_scene draws the signs of the raw scales)
            raw = {k: v.contiguous() for k, v in _raw_from_scene(s).items()}
        _CACHE["scene"] = (s, dict(raw=raw, intr=s["intr"], extr=s["extr"], W=W, H=H), *targets(H, W, Q_TARGET_SEED))
    s, sc, img, dep = _CACHE["scene"]
    if name not in _CACHE:
        if name == "Q1":
            _CACHE[name] = _problem(name, sc, img, dep, FIRST_FRAME, activated=s)
        elif name == "Q2":
            _CACHE[name] = _problem(name, sc, img, dep, CAMERA_ONLY, keep=disc(90.0, 55.0, 50.0))
        else:
            reg, and_mask, still = joint_inputs(sc["raw"], sc["intr"], 9)
            _CACHE[name] = _problem(name, sc, img, dep, JOINT, reg=reg, and_mask=and_mask, still=still)
    return _CACHE[name]


def poison_row(sc):
    """One raw splat that is conspicuous if ever read: at the centre of the view of ``sc``'s camera under POSE, depth 2,
    sigma 12 pixels, opacity 0.9, rgb (1, 0, 1) -- as a (1, 14) packed row (the columns of gflow_amd.fused.COLS)."""
    fx, fy, cx, cy = (float(a) for a in sc["intr"])
    z = 2.0
    cam = torch.tensor([(W / 2 - cx) / fx * z, (H / 2 - cy) / fy * z, z], dtype=torch.float64)
    extr = LO.pose_to_extr(POSE).double()
    xyz = (cam - extr[:, 3]) @ extr[:, :3]
    sig = 12.0 / math.sqrt(fx * fy) * z
    rgb = torch.logit(torch.tensor([0.98, 0.02, 0.98], dtype=torch.float64))
    return torch.cat([xyz, torch.full((3,), sig, dtype=torch.float64), torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64),
                      torch.tensor([math.log(9.0) / 10.0], dtype=torch.float64), rgb]).float().reshape(1, 14)


def _front_end(name):
    if ("fe", name) not in _CACHE:
        _CACHE[("fe", name)] = oracle_front_end(problem(name)["sc"], POSE, torch.float32)
    return _CACHE[("fe", name)]


def test_the_history_leaves_wide_rows_at_every_step():
    """H has rows of layout 2 (more than 32 tiles: runs out of the pool) at steps 0, 1 and 2, and rows change their layout
    between the steps (the test of tests/test_running_engine_host.py, run here as it stands)."""
    for step in STEPS:
        case = transition_case(step)
        cls = layout_class(case["facts"]["tiles"][case["sc"]["rows"]])
        print(f"step {step}: rows per layout {[int((cls == k).sum()) for k in (0, 1, 2)]}")
        assert int((cls == 2).sum()) >= 1
    RH.test_the_transition_edit_moves_rows_between_the_pair_row_layouts()


def test_every_handed_over_problem_is_smaller_than_the_history():
    """Fewer rows and fewer pairs in every Q than in H at every step, and K_CAP is twice the largest pair count of them all: no
    engine of these tests drops a pair or grows its lists, and an index left by H is inside every buffer a Q is run in."""
    pairs_h = [int(transition_case(step)["fe"]["ids"].numel()) for step in STEPS]
    rows_h = transition_case(0)["sc"]["raw"]["xyz"].shape[0]
    pairs_q = {name: int(_front_end(name)["ids"].numel()) for name in NAMES}
    print("H: rows", rows_h, "pairs", pairs_h, " Q: rows", Q_ROWS, "pairs", pairs_q)
    for name in NAMES:
        assert problem(name)["n"] == Q_ROWS < rows_h <= CAP
        assert 0 < pairs_q[name] < min(pairs_h)
    assert K_CAP == 2 * max(pairs_h + list(pairs_q.values()))


def test_the_first_problem_is_in_the_general_cameras_regime():
    sets = assert_regime("general", problem("Q1")["activated"])
    print("live", int(sets["live"].sum()), "clamped in x / y / both", *(int(sets[k].sum()) for k in ("x", "y", "both")))


def test_the_keep_mask_of_the_camera_only_problem_is_a_part_of_the_image():
    share = problem("Q2")["keep"].float().mean().item()
    print(f"kept pixels: {share:.1%}")
    assert 0.2 <= share <= 0.8
    assert problem("Q2")["foot"] is None and not problem("Q2")["reg"]


def test_the_selections_of_the_joint_problem_are_proper_subsets():
    q = problem("Q3")
    for k in ("and_mask", "still"):
        m = int(q[k].sum())
        print(k, m, "of", q["n"])
        assert 0 < m < q["n"]
    assert set(q["reg"]) == {"flow_target", "flow_w", "still_target", "still_w", "row_flags"}
    assert sorted(q["reg"]["row_flags"].unique().tolist()) == [0, 1, 2, 3]
    assert q["hp"]["lambda_flow"] > 0 and q["hp"]["lambda_still"] > 0 and q["hp"]["lambda_scale"] > 0


def test_the_poison_row_would_be_seen():
    """The oracle's render of Q1 with the poison row appended as row N against the render without it: more than 0.05 apart
    on at least 100 pixels.  A kernel that read one row past N would change the image."""
    sc = problem("Q1")["sc"]
    row = poison_row(sc)
    cols = dict(zip(ATTRS, ((0, 3), (3, 6), (6, 10), (10, 11), (11, 14))))          # gflow_amd.fused.COLS
    with_row = {k: torch.cat([sc["raw"][k], row[:, a:b]]) for k, (a, b) in cols.items()}
    extr = LO.pose_to_extr(POSE)
    img = [MO.render_multiple([*FO.activate(raw), sc["intr"], extr, 0.0, W, H], ["rgb"])["rgb"] for raw in (sc["raw"], with_row)]
    seen = ((img[0] - img[1]).abs().max(dim=0).values > 0.05).sum().item()
    print("pixels the poison row changes by more than 0.05:", seen)
    assert seen >= 100
