"""The four per-splat regularisers of the fit iteration (flow, still, scale, variance: trainer.py:490-528) and the gradient
masks behind them (:535-551), one term at a time, in plain torch on the CPU and in any dtype -- the reference
tests/test_gpu_regularisers.py holds fused_preprocess_bwd_adam_kernel (gfl_fit_splat.hip) against, and the trainer's two
paths through it.  tests/test_regularisers_host.py ties it to oracle/loss_oracle.py.

Every term is written as a sum over rows of ``t_i`` with multiplicative masks and no gathers: ``term_rows`` returns the
(N,) vector, so that a row-by-row Jacobian gives each row's share of the pose gradient (``reference``: S_k).
"""
import torch

from oracle import loss_oracle as LO
from oracle import msplat_oracle as MO

TERMS = ("flow", "still", "scale", "var")
STAGES = ("joint", "camera_only")
LAMBDAS = dict(flow=0.01, still=10.0, scale=0.5, var=10.0)        # clip_fit.py's flow / still / variance weights
GROUPS = {"xyz": (0, 3), "scale": (3, 6), "rotate": (6, 10), "opacity": (10, 11), "rgb": (11, 14)}   # = gflow_amd.fused.COLS
ATTRS = tuple(GROUPS)


def within(uv, W, H):
    """trainer.py:424 / :512"""
    return (uv[:, 0] > 0) & (uv[:, 0] < W - 1) & (uv[:, 1] > 0) & (uv[:, 1] < H - 1)


def stage_rows(inside, still, stage):
    """``inside`` (N,) narrowed over the labelled rows to the rows the stage fits (trainer.py:467-471, :513-517)"""
    out = inside.clone()
    m = still.shape[0]
    out[:m] = (still if stage == "camera_only" else ~still) & inside[:m]
    return out


def regulariser_scene(n_rows=700, n_labelled=600, seed=5, lead=False):
    """A 64 x 48 scene (4 x 3 tiles) of ``n_rows`` splats under POSE of tests/test_gpu_fused.py with every class of row the
    four terms tell apart; float32 tensors, the classes as named boolean masks (see the module's tests for their counts).
    ``lead``: row 0 changes places with the row that projects nearest the image centre and is labelled moving, so that the
    scene's first n rows have a row in the joint stage's flow and scale terms for every n >= 1 (random_scene puts the rows
    behind the camera first)."""
    from tests.scenes import random_scene
    from tests.test_gpu_fused import POSE, _raw_from_scene
    W, H = 64, 48
    N, M = int(n_rows), int(n_labelled)
    s = random_scene(N, W, H, seed, sigma_px=2.5, tilt=False)
    with torch.random.fork_rng():
        torch.manual_seed(seed)                              # (_raw_from_scene draws the signs of the raw scales)
        raw = _raw_from_scene(s)
    raw = {k: v.clone() for k, v in raw.items()}
    g = torch.Generator().manual_seed(1000 + seed)
    intr, pose = s["intr"], POSE.clone()
    uv, depth = MO.project_point(raw["xyz"], intr, LO.pose_to_extr(pose), W, H)
    if lead:
        centre = torch.tensor([W / 2.0, H / 2.0])
        j = int(torch.where(depth[:, 0] != 0, (uv - centre).norm(dim=1), torch.full((N,), 1e9)).argmin())
        for t in (*raw.values(), uv, depth):
            t[[0, j]] = t[[j, 0]]
    culled_now = depth[:, 0] == 0
    inside_now = within(uv, W, H)
    # ---- degenerate scales, on unlabelled rows inside the image (rows of the scale term in both stages)
    free = torch.nonzero(inside_now[M:]).flatten() + M
    assert free.numel() >= 15, "too few unlabelled rows inside the image"
    equal_scale, zero_scale = free[:10], free[10:15]
    sign = torch.where(torch.rand(10, 3, generator=g) > 0.5, 1.0, -1.0)
    raw["scale"][equal_scale] = raw["scale"][equal_scale, :1].abs() * sign
    raw["scale"][zero_scale, torch.arange(5) % 3] = 0.0
    # ---- two still masks over the labelled rows that differ on about a quarter of them
    still = torch.rand(M, generator=g) > 0.5
    last_still = torch.where(torch.rand(M, generator=g) < 0.25, ~still, still)
    last_xyz = raw["xyz"][:M] + 0.01 * torch.randn(M, 3, generator=g)
    zero_distance = torch.zeros(M, dtype=torch.bool)
    zero_distance[torch.randperm(M, generator=g)[:10]] = True
    if lead:
        zero_distance[0] = False
    zrows = torch.nonzero(zero_distance).flatten()
    last_still[zrows] = True
    still[zrows[:5]] = False                                 # live: the still term reaches Adam
    still[zrows[5:]] = True                                  # dead: masked by row_flags bit 0
    if lead:
        still[0] = False
    last_xyz[zero_distance] = raw["xyz"][:M][zero_distance]
    # ---- flow targets: last_uv = uv + N(0, 1); rows the current camera culls get a last_uv inside the image
    last_uv = uv[:M] + torch.randn(M, 2, generator=g)
    redraw = torch.stack([1.0 + (W - 3.0) * torch.rand(M, generator=g), 1.0 + (H - 3.0) * torch.rand(M, generator=g)], dim=1)
    last_uv = torch.where(culled_now[:M, None], redraw, last_uv)
    gt_flow = torch.randn(H, W, 2, generator=g)
    scale_id = torch.zeros(N, dtype=torch.bool)
    scale_id[equal_scale] = True
    zero_id = torch.zeros(N, dtype=torch.bool)
    zero_id[zero_scale] = True
    zero_comp = torch.zeros(N, 3, dtype=torch.bool)
    zero_comp[zero_scale, torch.arange(5) % 3] = True
    return dict(raw=raw, intr=intr, pose=pose, W=W, H=H, N=N, M=M, still=still, last_still=last_still,
                still_live=last_still & ~still, still_dead=last_still & still, zero_distance=zero_distance,
                last_xyz=last_xyz, last_uv=last_uv, gt_flow=gt_flow, culled_now=culled_now,
                equal_scale=scale_id, zero_scale=zero_id, zero_scale_comp=zero_comp)


def first_rows(sc, n):
    """The scene of the first ``n`` rows of ``sc``: min(n, M) of them labelled."""
    m = min(int(n), sc["M"])
    out = dict(sc, N=int(n), M=m, raw={k: v[:n].clone() for k, v in sc["raw"].items()})
    for k in ("still", "last_still", "still_live", "still_dead", "zero_distance", "last_xyz", "last_uv"):
        out[k] = sc[k][:m].clone()
    for k in ("culled_now", "equal_scale", "zero_scale", "zero_scale_comp"):
        out[k] = sc[k][:n].clone()
    return out


# ------------------------------------------------------------------ row selections (the same in every dtype: checked on the CPU)
def flow_rows(sc, stage):
    """(M,) rows of last_uv the flow term counts (trainer.py:512-518)"""
    return stage_rows(within(sc["last_uv"], sc["W"], sc["H"]), sc["still"], stage)


def flow_target(sc):
    """last_uv + the ground-truth flow at trunc(last_uv) (trainer.py:522-525), float32 as the trainer hands it to the library"""
    yx = sc["last_uv"].long()
    return sc["last_uv"] + sc["gt_flow"][yx[:, 1].clamp(0, sc["H"] - 1), yx[:, 0].clamp(0, sc["W"] - 1)]


def scale_rows(sc, stage, dtype=torch.float64):
    """(N,) rows of the scale term (trainer.py:424, :467-471: within_index aliases valid_uv_index)"""
    uv, _ = _project(sc, _cast_raw(sc, dtype)["xyz"], LO.pose_to_extr(sc["pose"].to(dtype)), dtype)
    return stage_rows(within(uv, sc["W"], sc["H"]), sc["still"], stage)


def _cast_raw(sc, dtype):
    return {k: v.detach().to(dtype) for k, v in sc["raw"].items()}


def _project(sc, xyz, extr, dtype):
    return MO.project_point(xyz, sc["intr"].to(dtype), extr, sc["W"], sc["H"])


# ------------------------------------------------------------------ the terms, row by row
# ``mut``: a named mistake of tests/test_regularisers_host.py applied to the term (None: the term as it is)
def flow_term_rows(sc, stage, lam, raw, extr, mut=None, target_first=False):
    """``target_first``: uv - (last_uv + gt), the order of the library's interface (flow_target is handed over as one float32
    tensor, FusedStage._set_regularisers), instead of trainer.py:520-528's (uv - last_uv) - gt: the same number, rounded
    differently in float32 -- once more at the magnitude of uv"""
    dtype = extr.dtype
    N, M = sc["N"], sc["M"]
    uv, _ = _project(sc, raw["xyz"], extr, dtype)
    sel = flow_rows(sc, stage)
    count = sel.sum() if mut != "flow_labelled_count" else torch.tensor(M)
    yx = sc["last_uv"].long()
    gt = sc["gt_flow"][yx[:, 1].clamp(0, sc["H"] - 1), yx[:, 0].clamp(0, sc["W"] - 1)].to(dtype)
    d = uv[:M] - (sc["last_uv"].to(dtype) + gt) if target_first else uv[:M] - sc["last_uv"].to(dtype) - gt
    t = lam * sel.to(dtype) * (d * d).sum(dim=1) / (2.0 * count)          # F.mse_loss over (count, 2) elements
    if mut in ("flow_factor_2", "flow_sign"):
        t = (0.5 if mut == "flow_factor_2" else -1.0) * t
    return torch.cat([t, torch.zeros(N - M, dtype=dtype)])


def still_term_rows(sc, stage, lam, raw, extr, mut=None):
    dtype = extr.dtype
    N, M = sc["N"], sc["M"]
    m = sc["last_still"] if mut != "still_from_still" else sc["still"]
    a = raw["xyz"][:M] - sc["last_xyz"].to(dtype)
    dist = torch.norm(a, dim=1) if mut != "still_no_norm" else 0.5 * (a * a).sum(dim=1)
    t = lam * m.to(dtype) * dist / m.sum()
    return torch.cat([t, torch.zeros(N - M, dtype=dtype)]) + 0.0 * extr.sum()


def _abs_scale(raw, mut):
    """|raw scale|; under the mistake "sign_ignored" with the backward of the identity (the gradient wrt |s| taken for the raw one)"""
    x = raw["scale"]
    return x.detach().abs() + (x - x.detach()) if mut == "sign_ignored" else torch.abs(x)


def scale_term_rows(sc, stage, lam, raw, extr, mut=None):
    dtype = extr.dtype
    uv, depth = _project(sc, raw["xyz"], extr, dtype)
    inside = within(uv.detach(), sc["W"], sc["H"])
    if mut == "scale_wrong_stage":
        stage = "joint" if stage == "camera_only" else "camera_only"
    valid = stage_rows(inside, sc["still"], stage)
    count = valid.sum() + (1 if mut == "scale_count_off_by_one" else 0)
    z = torch.where(valid, depth[:, 0], torch.ones_like(depth[:, 0]))     # (an unselected row may be culled: depth 0)
    return lam * valid.to(dtype) * torch.norm(_abs_scale(raw, mut), dim=1) / z / count


def var_term_rows(sc, stage, lam, raw, extr, mut=None):
    sd = torch.std(_abs_scale(raw, mut), dim=1, unbiased=(mut != "var_biased"))
    return lam * sd / sc["N"] + 0.0 * extr.sum()


TERM_ROWS = dict(flow=flow_term_rows, still=still_term_rows, scale=scale_term_rows, var=var_term_rows)
MISTAKES = dict(flow_factor_2=("flow",), flow_sign=("flow",), flow_labelled_count=("flow",), still_no_norm=("still",),
                still_from_still=("still",), scale_count_off_by_one=("scale",), scale_wrong_stage=("scale",),
                var_biased=("var",), sign_ignored=("scale", "var"))


def apply_masks(g, sc, stage, freeze_rgb=True):
    """trainer.py:535-551 on an (N, 14) gradient: colours of a later frame, xyz of the still rows, everything in the camera-only stage"""
    g = g.clone()
    if freeze_rgb:
        g[:, 11:14] = 0
    m = sc["still"].shape[0]
    g[:m, 0:3] = g[:m, 0:3] * (~sc["still"]).to(g.dtype).unsqueeze(1)
    if stage == "camera_only":
        g = 0 * g
    return g


def untouched(sc, term, stage):
    """(N, 14) bool: the entries the term cannot touch, by the classes of the scene (not by the reference's zeros)"""
    N, M = sc["N"], sc["M"]
    z = torch.ones(N, 14, dtype=torch.bool)
    if stage == "camera_only":
        return z                                                     # freeze_all_splats
    if term == "flow":
        live = flow_rows(sc, stage) & ~sc["culled_now"][:M] & ~sc["still"]
        z[:M, 0:3] = ~live[:, None]
    elif term == "still":
        live = sc["still_live"] & ~sc["zero_distance"]
        z[:M, 0:3] = ~live[:, None]
    elif term == "scale":
        rows = scale_rows(sc, stage)
        z[:, 3:6] = ~rows[:, None] | sc["zero_scale_comp"]
        z[:, 0:3] = ~rows[:, None]
        z[:M, 0:3] |= sc["still"][:, None]
    else:
        z[:, 3:6] = sc["equal_scale"][:, None] | sc["zero_scale_comp"]
    return z


def reference(sc, term, stage, dtype, lam=None, mut=None, jacobian=True, masks=True, target_first=False):
    """The term's gradient alone: dict(rows (N, 14) in the column order of gflow_amd.fused.COLS, masks applied; pose (7,);
    d_extr (12,); S_pose (7,), S_extr (12,): S_k = sum_i |d t_i / d k| from a row-by-row Jacobian (``jacobian``); loss).
    ``masks=False``: the gradient before trainer.py:535-551; ``target_first``: flow_term_rows'.  ``term``: one of TERMS, or a tuple of them (their sum, each with its LAMBDAS weight or ``lam[term]``)."""
    terms = (term,) if isinstance(term, str) else tuple(term)
    lam = dict(LAMBDAS, **(lam or {}))
    raw = {k: v.clone().requires_grad_(True) for k, v in _cast_raw(sc, dtype).items()}
    pose = sc["pose"].to(dtype).clone().requires_grad_(True)

    def rows_of(extr, r=raw):
        return sum(TERM_ROWS[t](sc, stage, lam[t], r, extr, mut if t in MISTAKES.get(mut, ()) else None,
                                **(dict(target_first=target_first) if t == "flow" else {})) for t in terms)

    extr = LO.pose_to_extr(pose)
    extr.retain_grad()
    loss = rows_of(extr).sum()
    assert loss.dtype == dtype
    loss.backward()
    N = sc["N"]
    rows = torch.cat([(raw[k].grad if raw[k].grad is not None else torch.zeros_like(raw[k])).reshape(N, -1) for k in ATTRS], dim=1)
    out = dict(rows=apply_masks(rows, sc, stage) if masks else rows, pose=pose.grad.clone(), d_extr=extr.grad.reshape(12).clone(),
               loss=loss.detach())
    if jacobian:
        det = {k: v.detach() for k, v in raw.items()}
        J_e = torch.autograd.functional.jacobian(lambda e: rows_of(e, det), extr.detach()).reshape(N, 12)
        J_p = torch.autograd.functional.jacobian(lambda p: rows_of(LO.pose_to_extr(p), det), pose.detach()).reshape(N, 7)
        out["S_extr"], out["S_pose"] = J_e.abs().sum(dim=0), J_p.abs().sum(dim=0)
        # (the rows' shares add up to the gradient: the Jacobian is of the same function)
        if dtype == torch.float64:
            assert torch.allclose(J_e.sum(dim=0), out["d_extr"], rtol=1e-9, atol=1e-15)
    return out


def oracle_loss(sc, term, stage, lam, raw, pose):
    """The same term through oracle/loss_oracle.py (gathers, means) on the same inputs, for autograd."""
    dtype = pose.dtype
    extr = LO.pose_to_extr(pose)
    uv, depth = _project(sc, raw["xyz"], extr, dtype)
    if term == "flow":
        return lam * LO.flow_loss(uv, sc["last_uv"].to(dtype), sc["gt_flow"].to(dtype), flow_rows(sc, stage))
    if term == "still":
        return lam * LO.still_loss(raw["xyz"], sc["last_xyz"].to(dtype), sc["last_still"])
    if term == "scale":
        return lam * LO.scale_loss(torch.abs(raw["scale"]), uv, depth, sc["W"], sc["H"], sc["still"],
                                   camera_only=(stage == "camera_only"))
    return lam * LO.var_loss(torch.abs(raw["scale"]))


# ------------------------------------------------------------------ the bounds (ISSUE: built from the reference on the case's own inputs)
EPS32 = 2.0 ** -24
ROW_OPS = 32            # rounded operations between rec / params and g[k] that the per-row bound allows for


def float32_references(sc, term, stage):
    """The float32 reference in the two orders the flow residual is formed in (flow_term_rows: the operator path's and the
    library interface's); one reference for a term without the flow term.  The gap of a quantity is the larger of theirs."""
    terms = (term,) if isinstance(term, str) else tuple(term)
    return [reference(sc, term, stage, torch.float32, jacobian=False, target_first=tf) for tf in ((False, True) if "flow" in terms else (False,))]


def row_bounds(ref32, ref64):
    """{group: (gap, bound)}: gap = max |float32 reference - float64 reference| over the group's columns of all rows (``ref32``:
    a list of float32 references, float32_references); bound = 4 gap + 32 * 2^-24 * max |float64 reference of the group|."""
    out = {}
    for k, (a, b) in GROUPS.items():
        gap = max((r["rows"][:, a:b].double() - ref64["rows"][:, a:b]).abs().max().item() for r in ref32)
        out[k] = (gap, 4.0 * gap + ROW_OPS * EPS32 * ref64["rows"][:, a:b].abs().max().item())
    return out


def pose_bounds(ref32, ref64, rows):
    """{"pose": (gap (7,), bound (7,)), "d_extr": (gap (12,), bound (12,))}: bound_k = 4 gap_k + rows * 2^-24 * S_k, the worst
    case of a float32 sum of ``rows`` addends in any order."""
    out = {}
    for name, S in (("pose", "S_pose"), ("d_extr", "S_extr")):
        gap = torch.stack([(r[name].double() - ref64[name]).abs() for r in ref32]).max(dim=0).values
        out[name] = (gap, 4.0 * gap + rows * EPS32 * ref64[S])
    return out


# ------------------------------------------------------------------ computed once, shared by the tests, left unchanged
_SCENES, _REFS = {}, {}


def shared_scene(n_rows=700, n_labelled=600, seed=5, first=None, lead=False):
    """regulariser_scene(...), or its first ``first`` rows (first_rows) -- one object per argument tuple"""
    key = (n_rows, n_labelled, seed, first, lead)
    if key not in _SCENES:
        sc = (regulariser_scene(n_rows, n_labelled, seed, lead) if first is None else
              first_rows(shared_scene(n_rows, n_labelled, seed, lead=lead), first))
        _SCENES[key] = dict(sc, key=key)
    return _SCENES[key]


def shared_reference(sc, term, stage):
    """(float32 references, float64 reference, row_bounds, pose_bounds) of a shared_scene"""
    key = (sc["key"], term, stage)
    if key not in _REFS:
        r64 = reference(sc, term, stage, torch.float64)
        r32 = float32_references(sc, term, stage)
        _REFS[key] = (r32, r64, row_bounds(r32, r64), pose_bounds(r32, r64, sc["N"]))
    return _REFS[key]
