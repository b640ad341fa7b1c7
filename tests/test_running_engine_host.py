"""The scenes of tests/test_gpu_running_engine.py on the CPU: a fit whose splats change their pair-row layout between two
iterations (narrow <-> wide tile rectangles, rectangles that move, rows that leave the frustum) and a pile whose front rows
appear between two iterations.  The scenes do what those tests need, and the float32 oracle they are held against is itself
far inside their bounds (against the float64 oracle)."""
import pytest
import torch

from oracle import loss_oracle as LO
from tests.scenes import (ATTRS, N_CULLED, apply_transition, capped_pile_scene, layout_class, oracle_front_end, pile_phase,
                          pile_toggle_rows, rect_facts, reference_fit, regime_error, transition_scene)
from tests.test_opacity_regimes_host import PILE_SEED, POSE, targets

NOISE_BOUND = 1e-4            # float32 oracle against float64 oracle, relative L2: a twentieth of the device's 2e-3
TRANSITIONS = ((0, 1), (1, 0), (1, 2), (2, 1))
PILE_POSE = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])              # the pile is placed for, and seen from, the identity

_CACHE = {}


class _Case(dict):
    """A scene with its targets; the float32 / float64 references (``r32``, ``r64``) are worked out when first asked for --
    the GPU tests that only need the scene do not pay for them."""

    def __missing__(self, key):
        if key not in ("r32", "r64"):
            raise KeyError(key)
        self[key] = reference_fit(self["sc"], self["pose"], self["img"], self["dep"], torch.float32 if key == "r32" else torch.float64)
        return self[key]


def transition_case(step):
    """The transition scene after ``apply_transition`` steps 1 .. ``step`` (0: as committed), its targets, the float32
    front end and the rectangle facts (once per process); ``r32`` / ``r64``: see _Case."""
    key = ("transition", step)
    if key not in _CACHE:
        sc = transition_scene(extr=LO.pose_to_extr(POSE))
        for k in range(1, step + 1):
            apply_transition(sc["raw"], sc["rows"], k, f=sc["intr"][0])
        img, dep = targets(sc["H"], sc["W"], 8)
        fe = oracle_front_end(sc, POSE, torch.float32)
        _CACHE[key] = _Case(sc=sc, img=img, dep=dep, pose=POSE, fe=fe, facts=rect_facts(fe, sc["W"], sc["H"]))
    return _CACHE[key]


def pile_case(phase):
    """The capped pile (seed 3) with its 40 nearest rows invisible ("A") or as committed ("B")."""
    key = ("pile", phase)
    if key not in _CACHE:
        base = capped_pile_scene(seed=PILE_SEED)
        sc = pile_phase(base, phase)
        img, dep = targets(sc["H"], sc["W"], 6)
        _CACHE[key] = _Case(sc=sc, img=img, dep=dep, pose=PILE_POSE, toggled=pile_toggle_rows(base))
    return _CACHE[key]


def nonzero_rows(grads):
    """rows with a non-zero entry in any attribute's gradient"""
    return torch.cat([grads[k] for k in ATTRS], dim=1).abs().sum(dim=1) != 0


def test_the_transition_edit_moves_rows_between_the_pair_row_layouts():
    """transition_scene (168 x 120, class-row seed 14: 168 class rows in front of 1500 ordinary ones) under POSE, float32
    oracle front end; layouts 0: at most 16 tiles, 1: 17 .. 32, 2: more than 32 (the pool).

      as committed   rectangles of 1 .. 72 tiles; 83 / 51 / 34 class rows in layout 0 / 1 / 2; 19 at exactly 16 tiles, 11 at
                     30 .. 32; clipped at the left / right / top / bottom border: 26 / 27 / 38 / 32; K = 11 433, longest list 183
      odd edit       0 -> 1: 14 rows, 1 -> 0: 14, 1 -> 2: 12, 2 -> 1: 12; 110 keep their layout and move; the last six rows
                     have depth 0, radius 0 and are in no tile; K = 11 440, longest list 184; no tile's list grows by more
                     than 8 entries (a reserved region has count / 4 + 32 to spare: no void iteration from the edit)
      even edit      back to the committed rectangles, row for row (the transitions above, reversed)
    (Class-row seeds 1 .. 24 were looked at: 14 is the first with eight rows on every transition, eight at 16 and at 30 .. 32
    tiles and no class row pushed off the image by the 9 pixels -- such a row has no gradient to compare.)"""
    a, b = transition_case(0), transition_case(1)
    rows = a["sc"]["rows"]
    t0, t1 = a["facts"]["tiles"][rows], b["facts"]["tiles"][rows]
    c0, c1 = layout_class(t0), layout_class(t1)
    print("tiles", int(t0.min()), "..", int(t0.max()), "layouts", [int((c0 == k).sum()) for k in (0, 1, 2)],
          "K", int(a["fe"]["ids"].numel()), int(b["fe"]["ids"].numel()),
          "longest", *(int((x["fe"]["tile_range"][:, 1] - x["fe"]["tile_range"][:, 0]).max()) for x in (a, b)))
    assert int(t0.min()) >= 1 and int(t0.max()) > 64
    for src, dst in TRANSITIONS:
        n = int(((c0 == src) & (c1 == dst)).sum())          # odd edits go src -> dst, even edits dst -> src: both directions
        print(f"{src} -> {dst}: {n} rows")
        assert n >= 8, (src, dst, n)
    stay = (c0 == c1) & (c0 >= 0) & (t0 > 0)
    moved = stay & (a["fe"]["uv"][rows] != b["fe"]["uv"][rows]).any(dim=1)
    print("same layout, rectangle moved:", int(moved.sum()))
    assert int(moved.sum()) >= 80
    n16, n30 = int((t0 == 16).sum()), int(((t0 >= 30) & (t0 <= 32)).sum())
    print("exactly 16 tiles:", n16, " 30 .. 32 tiles:", n30)
    assert n16 >= 8 and n30 >= 8
    for side in ("left", "right", "top", "bottom"):
        n = int(a["facts"][side][rows].sum())
        print(f"clipped at the {side} border: {n}")
        assert n >= 4, side
    culled = rows[-N_CULLED:]
    assert bool((a["fe"]["depth"][culled] > 0).all()) and bool((t0[-N_CULLED:] > 0).all())
    assert bool((b["fe"]["depth"][culled] == 0).all()) and bool((t1[-N_CULLED:] == 0).all())
    assert bool((b["fe"]["radius"][culled] == 0).all())
    grow = (b["fe"]["tile_range"][:, 1] - b["fe"]["tile_range"][:, 0]) - (a["fe"]["tile_range"][:, 1] - a["fe"]["tile_range"][:, 0])
    print("largest growth of a list:", int(grow.max()))
    assert int(grow.max()) < 32
    back = transition_case(2)
    assert torch.equal(back["facts"]["tiles"], a["facts"]["tiles"])
    assert torch.allclose(back["sc"]["raw"]["xyz"], a["sc"]["raw"]["xyz"], atol=1e-6)


def test_the_pile_toggle_leaves_rows_whose_every_pair_row_is_stale():
    """capped_pile_scene(seed 3) under the identity pose: with the pile's 40 nearest rows invisible (phase A) 24 rows have a float64
    reference gradient, with them back (phase B) 10; 22 rows have one in A and none in B (8 of them rows of the pile) -- in the
    iteration after the toggle every pair row they own is an earlier forward's.  The same sets in float32."""
    a, b = pile_case("A"), pile_case("B")
    for dt in ("r64", "r32"):
        na, nb = nonzero_rows(a[dt]["grads"]), nonzero_rows(b[dt]["grads"])
        gone = na & ~nb
        print(dt, "A:", int(na.sum()), "B:", int(nb.sum()), "A and not B:", int(gone.sum()), "of the pile:",
              int(gone[:a["sc"]["n_pile"]].sum()))
        assert int(gone.sum()) >= 20
    assert torch.equal(nonzero_rows(a["r64"]["grads"]), nonzero_rows(a["r32"]["grads"]))
    assert torch.equal(nonzero_rows(b["r64"]["grads"]), nonzero_rows(b["r32"]["grads"]))
    assert not bool(nonzero_rows(a["r64"]["grads"])[a["toggled"]].any())          # invisible rows get nothing


@pytest.mark.parametrize("name", ["transition1", "transition2", "pileB"])
def test_the_float32_reference_is_far_inside_the_bounds_of_the_running_engine_tests(name):
    """float32 oracle against float64 oracle on the scenes a running engine's gradient is checked on: the transition scene
    after the odd edit and after the even one, and the pile after the toggle (phase B, the committed scene).  Asserted:
    relative L2 per attribute at most 1e-4, a twentieth of the 2e-3 the device is held to, over all rows and (transition
    scene) over the class rows alone; no entry off rtol 5e-3 / atol 5e-4 max|ref|.  ONE exception, the pile's d_opacity (see
    below).  Measured:

                    after the odd edit           after the even edit          pile, phase B
                    all rows     class rows      all rows     class rows      all rows
      d_xyz         3.4e-06      4.8e-06         3.5e-06      1.3e-05         3.2e-07
      d_scale       2.9e-06      3.5e-06         3.0e-06      3.7e-06         4.9e-07
      d_rotate      2.5e-06      1.4e-06         2.6e-06      1.5e-06         6.3e-07
      d_opacity     1.3e-06      9.7e-07         1.3e-06      1.0e-06         1.4e-04 (rows with 1 - o >= 1e-2: 1.1e-06)
      d_rgb         1.8e-06      1.4e-06         1.7e-06      1.1e-06         4.5e-07
      d_pose        3.4e-06                      4.5e-06                      4.8e-07
      depth affine  3.5e-08                      4.4e-08                      6.5e-08
      render        5.0e-06 (largest error)      5.0e-06                      1.5e-07

    The pile's d_opacity does NOT meet 1e-4 over all rows, and it is not the blend: eight of its ten rows with a gradient have
    raw opacities of 0.55 .. 2, o within 3.4e-3 of 1.  The chain rule's factor 10 o (1 - o) takes 1 - o from a float32 o
    whose spacing below 1 is 2^-24: rounding o (half a spacing) and the sigmoid's own last bits (another one and a half,
    allowed for here) leave 1 - o off by up to 2 x 2^-24, relative 2 x 2^-24 / (1 - o) -- 2.1e-4 for the row that carries
    the norm (raw 0.748, 1 - o = 5.7e-4, measured 1.35e-4), and 1 where o rounds to 1.0f (five rows: float32 gives exactly 0
    for a float64 gradient of 1e-12 .. 2e-10).  So: rows with 1 - o >= 1e-2 are held to 1e-4 like everything else, every
    other row on its own to (1e-4 + 2 x 2^-24 / (1 - o)) of its float64 gradient.  The device tests compare with the float32
    oracle, which shares that factor with the device.

    No class row has an all-zero float64 gradient in any attribute, the six culled rows after the odd edit aside (theirs
    are all zero in both formats).  (Phase A of the pile is NOT such a scene: without its 40 front rows two layers at the cap
    meet on some pixels, (1 - 0.99)^2 against T_MIN is decided by the format -- tests/scenes.py:capped_pile_scene -- and the two
    oracles' renders differ by 1e-2 there; the tests use phase A for what it leaves behind, never for its gradient.)"""
    case = transition_case(int(name[-1])) if name.startswith("transition") else pile_case(name[-1])
    sc, r32, r64 = case["sc"], case["r32"], case["r64"]
    n = sc["raw"]["xyz"].shape[0]
    err = (r32["render"].double() - r64["render"]).abs().max().item()
    print(f"{name} render: max err {err:.1e}")
    assert err < 1e-4
    sets = {"all rows": torch.ones(n, dtype=torch.bool)}
    if name.startswith("transition"):
        cls = torch.zeros(n, dtype=torch.bool)
        cls[sc["rows"]] = True
        sets["class rows"] = cls
    for k in ATTRS:
        for what, rows in sets.items():
            rel, bad = regime_error(r32["grads"][k], r64["grads"][k], rows)
            print(f"{name} d_{k} {what}: relative L2 {rel:.1e}, off-tolerance share {bad:.1e}")
            if (name, k) == ("pileB", "opacity"):
                continue                                  # the one exception: held to its own rule below
            assert rel <= NOISE_BOUND and bad == 0.0, (k, what, rel, bad)
    for k in ("d_pose", "d_ab"):
        rel = ((r32[k].double() - r64[k]).norm() / r64[k].norm()).item()
        print(f"{name} {k}: relative L2 {rel:.1e}")
        assert rel <= NOISE_BOUND
    if name == "pileB":
        g32, g64 = r32["grads"]["opacity"].double().reshape(-1), r64["grads"]["opacity"].reshape(-1)
        gap = 1.0 / (1.0 + torch.exp(10.0 * sc["raw"]["opacity"].double().reshape(-1)))              # 1 - o
        away = gap >= 1e-2
        assert int((away & (g64 != 0)).sum()) >= 2 and int((~away & (g64 != 0)).sum()) >= 2
        rel, bad = regime_error(g32.unsqueeze(1), g64.unsqueeze(1), away)
        print(f"pileB d_opacity, rows with 1 - o >= 1e-2: relative L2 {rel:.1e}, off-tolerance share {bad:.1e}")
        assert rel <= NOISE_BOUND and bad == 0.0
        allowed = (NOISE_BOUND + 2.0 * 2.0 ** -24 / gap) * g64.abs()
        worst = ((g32 - g64).abs() / allowed.clamp(min=1e-300))[~away & (g64 != 0)]
        print(f"pileB d_opacity, {worst.numel()} rows next to o = 1: largest error / allowed {float(worst.max()):.2f}")
        assert bool(((g32 - g64).abs() <= allowed)[~away].all())
    if name.startswith("transition"):
        live = torch.ones(sc["rows"].numel(), dtype=torch.bool)
        if name == "transition1":
            live[-N_CULLED:] = False
            for k in ATTRS:
                assert float(r64["grads"][k][sc["rows"][-N_CULLED:]].abs().max()) == 0.0
                assert float(r32["grads"][k][sc["rows"][-N_CULLED:]].abs().max()) == 0.0
        for k in ATTRS:
            zero = (r64["grads"][k][sc["rows"]] == 0).all(dim=1) & live
            assert not bool(zero.any()), f"d_{k}: class rows {sc['rows'][zero].tolist()} have no float64 gradient"
