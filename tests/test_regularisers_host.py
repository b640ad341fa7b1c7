"""tests/regulariser_ref.py on the CPU: the scene holds every class of row, the per-row form of the four terms is the
oracle's (oracle/loss_oracle.py) to 1e-12 in float64, and the bounds tests/test_gpu_regularisers.py holds the kernel to
reject every named mistake by more than a factor of ten."""
import pytest
import torch

from tests import regulariser_ref as RR

MIN_ROWS = 5


def _classes(sc, stage):
    M = sc["M"]
    flow = RR.flow_rows(sc, stage)
    scale = RR.scale_rows(sc, stage)
    return {
        "still_live": sc["still_live"], "still_dead": sc["still_dead"],
        "still != last_still": sc["still"] != sc["last_still"],
        "zero_distance, live": sc["zero_distance"] & sc["still_live"],
        "zero_distance, dead": sc["zero_distance"] & sc["still_dead"],
        "flow rows": flow, "flow rows culled now": flow & sc["culled_now"][:M], "flow rows seen now": flow & ~sc["culled_now"][:M],
        "labelled rows outside the flow term": ~flow,
        "scale rows": scale, "scale rows, labelled": scale[:M], "scale rows, unlabelled": scale[M:],
        "rows outside the scale term": ~scale, "appended rows": torch.ones(sc["N"] - M, dtype=torch.bool),
        "equal scales": sc["equal_scale"], "equal scales in the scale term": sc["equal_scale"] & scale,
        "a zero raw scale": sc["zero_scale"], "a zero raw scale in the scale term": sc["zero_scale"] & scale,
        "negative raw scales": (sc["raw"]["scale"] < 0).any(dim=1),
    }


@pytest.mark.parametrize("stage", RR.STAGES)
def test_the_scene_holds_every_row_class_in_each_stage(stage):
    sc = RR.shared_scene()
    assert sc["N"] == 700 and sc["M"] == 600 and (sc["W"], sc["H"]) == (64, 48)
    for name, rows in _classes(sc, stage).items():
        print(f"{stage}: {name}: {int(rows.sum())} rows")
        assert int(rows.sum()) >= MIN_ROWS, (stage, name)
    quarter = (sc["still"] != sc["last_still"]).float().mean().item()
    assert 0.15 < quarter < 0.35, quarter
    es = sc["raw"]["scale"][sc["equal_scale"]]
    assert int(sc["equal_scale"].sum()) == 10 and bool((es.abs() == es.abs()[:, :1]).all())
    assert bool((es < 0).any()) and bool((es > 0).any())                        # mixed signs of the raw values
    assert int(sc["zero_scale"].sum()) == 5 and bool(((sc["raw"]["scale"] == 0) == sc["zero_scale_comp"]).all())
    assert bool((sc["last_xyz"][sc["zero_distance"]] == sc["raw"]["xyz"][:sc["M"]][sc["zero_distance"]]).all())
    # the selections do not hang on the number format: the same rows in float32 and in float64
    assert torch.equal(RR.scale_rows(sc, stage, torch.float32), RR.scale_rows(sc, stage, torch.float64))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 512, 513, 1025])
def test_every_size_of_the_size_sweep_has_rows_in_the_scale_and_flow_terms(n):
    sc = RR.shared_scene(1025, 600, 5, first=n, lead=True)
    assert sc["N"] == n and sc["M"] == min(n, 600)
    print(f"{n} rows: {int(RR.scale_rows(sc, 'joint').sum())} in the scale term, {int(RR.flow_rows(sc, 'joint').sum())} in the flow term")
    assert int(RR.scale_rows(sc, "joint").sum()) >= 1 and int(RR.flow_rows(sc, "joint").sum()) >= 1, n
    assert torch.equal(RR.scale_rows(sc, "joint", torch.float32), RR.scale_rows(sc, "joint", torch.float64))


@pytest.mark.parametrize("stage", RR.STAGES)
@pytest.mark.parametrize("term", RR.TERMS)
def test_the_per_row_form_is_the_oracles_term(term, stage):
    """float64: gradient of the sum of the rows == autograd gradient of LO.flow_loss / still_loss / scale_loss / var_loss"""
    sc = RR.shared_scene()
    lam = RR.LAMBDAS[term]
    mine = RR.reference(sc, term, stage, torch.float64, jacobian=False, masks=False)
    raw = {k: v.to(torch.float64).clone().requires_grad_(True) for k, v in sc["raw"].items()}
    pose = sc["pose"].double().clone().requires_grad_(True)
    loss = RR.oracle_loss(sc, term, stage, lam, raw, pose)
    loss.backward()
    assert abs(loss.item() - mine["loss"].item()) <= 1e-12 * abs(loss.item())
    rows = torch.cat([(raw[k].grad if raw[k].grad is not None else torch.zeros_like(raw[k])).reshape(sc["N"], -1)
                      for k in RR.ATTRS], dim=1)
    assert rows.abs().max() > 0
    assert (rows - mine["rows"]).abs().max() <= 1e-12 * rows.abs().max()
    # the entries the GPU test asks to be exactly zero are exactly zero here, and the term reaches rows beside them
    masked = RR.apply_masks(mine["rows"], sc, stage)
    must = RR.untouched(sc, term, stage)
    assert bool((masked[must] == 0).all())
    assert stage == "camera_only" or int((masked[~must] != 0).sum()) >= 5
    gp = pose.grad if pose.grad is not None else torch.zeros(7, dtype=torch.float64)
    assert (gp - mine["pose"]).abs().max() <= 1e-12 * max(gp.abs().max().item(), 1e-300)
    assert bool((gp.abs().max() > 0)) == (term in ("flow", "scale"))


@pytest.mark.parametrize("mistake", sorted(RR.MISTAKES))
def test_the_bounds_reject_each_named_mistake(mistake):
    """Each mistake applied to the float64 reference is further than 10 x the bound from the unperturbed reference on at
    least one quantity the GPU tests check (a column group of the rows in the joint stage; a pose or d_extr component)."""
    sc = RR.shared_scene()
    worst = 0.0
    for term in RR.MISTAKES[mistake]:
        for stage in RR.STAGES:
            r32, r64, rb, pb = RR.shared_reference(sc, term, stage)
            bad = RR.reference(sc, term, stage, torch.float64, mut=mistake, jacobian=False)
            for k, (a, b) in RR.GROUPS.items():
                dist = (bad["rows"][:, a:b] - r64["rows"][:, a:b]).abs().max().item()
                if dist > 0:
                    worst = max(worst, dist / rb[k][1])
                    print(f"{mistake}: {term}, {stage}, d_{k}: off by {dist:.2e}, bound {rb[k][1]:.2e}")
            for name in ("pose", "d_extr"):
                dist = (bad[name] - r64[name]).abs()
                for j in torch.nonzero(dist > 0).flatten().tolist():
                    worst = max(worst, dist[j].item() / pb[name][1][j].item())
                if bool((dist > 0).any()):
                    print(f"{mistake}: {term}, {stage}, {name}: off by up to {dist.max().item():.2e}, "
                          f"bounds up to {pb[name][1].max().item():.2e}")
    print(f"{mistake}: {worst:.1f} x the bound")
    assert worst > 10.0, f"{mistake} stays within 10 x every bound ({worst:.2f} x)"


def test_the_sum_of_terms_is_the_sum_of_the_references():
    """reference() of a tuple of terms (what the trainer tests and the additivity test use) adds the single ones"""
    sc = RR.shared_scene()
    both = RR.reference(sc, ("flow", "var", "still", "scale"), "joint", torch.float64, jacobian=False)
    rows = sum(RR.shared_reference(sc, t, "joint")[1]["rows"] for t in RR.TERMS)
    pose = sum(RR.shared_reference(sc, t, "joint")[1]["pose"] for t in RR.TERMS)
    assert (both["rows"] - rows).abs().max() <= 1e-14 * rows.abs().max()
    assert (both["pose"] - pose).abs().max() <= 1e-14 * pose.abs().max()
