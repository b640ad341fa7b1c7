"""Digests of what the library computes, for comparing two builds of it bit for bit (a refactor's "same bits").

    GFLOW_HIP_LIB=/path/to/one/libgflow_hip.so   python tools/lib_bits.py > one.txt
    GFLOW_HIP_LIB=/path/to/other/libgflow_hip.so python tools/lib_bits.py > other.txt
    diff one.txt other.txt

One process, one library (gflow_amd/_lib.py reads GFLOW_HIP_LIB; without it the tree's own build).  One ``name sha256`` line per
tensor, on two scenes: the capped pile (48 x 48, 700 + 300 splats: the forward's long-tile walk, the backward's segments) and the
480 x 854 / 60 000-splat bench scene.

Deterministic engine (GFL_FIT_DETERMINISTIC): the three kinds of stage of tests/test_gpu_deterministic.py::STAGES and one with
lr_camera > 0 on the first frame's ten sums, three exact-path and three reserved-region iterations each, the camera stage with a
footprint mask; a snapshot iteration and eng.snapshot(); an iteration whose K_cap is too small for the lists (the void rule).
After each: that test's OUT tensors, every tile's sorted list, keep, overflow, the uint8 images.
Default mode (the backward's LDS adds are unordered there): the forward's outputs only, and render() forward and backward under
torch's deterministic switch.  ``--scenes pile`` leaves the large scene out.

A void iteration's ``sums`` are left out unless ``--void-sums`` asks for them: they are the loss of a render of TRUNCATED lists, and
which pairs of the tile that straddles K_cap survive the scatter is arrival order -- two runs of one library differ there."""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.test_gpu_deterministic import NAMES, OUT, STAGES, _bench_scene   # noqa: E402
from tests.test_gpu_fused import _engine, _lists                            # noqa: E402

DEV = "cuda"
ROWS = ("rec", "params", "adam_m", "adam_v")
COUNT = [0]


def digest(name, t):
    t = t.detach().contiguous().cpu()
    print(f"{name} {hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()}")
    COUNT[0] += 1


def outputs(tag, eng, images=None):
    torch.cuda.synchronize()
    for k in OUT:
        t = getattr(eng, k)
        digest(f"{tag}.{k}", t[:eng.N] if k in ROWS else t)
    tr = eng.tile_range.cpu()
    digest(f"{tag}.list_lengths", (tr[:, 1] - tr[:, 0]).contiguous())
    digest(f"{tag}.lists", torch.cat(_lists(eng)))
    digest(f"{tag}.overflow", eng.overflow)
    if eng.keep is not None:
        digest(f"{tag}.keep", eng.keep)
    if images is not None:
        digest(f"{tag}.images", images)


def scenes(which):
    if "pile" in which:
        from tests.test_opacity_regimes_host import POSE, pile_setup
        sc, img, dep = pile_setup()
        yield "pile", sc["raw"], sc, img, dep, POSE, 512
    if "bench" in which:
        frame, raw = _bench_scene()
        cam = dict(W=frame["image"].shape[1], H=frame["image"].shape[0], intr=raw["intr"])
        pose = torch.tensor([0.002, -0.001, 0.0015, 1.0, 0.01, -0.02, 0.015])
        yield "bench", {k: raw[k] for k in NAMES}, cam, frame["image"], frame["depth"], pose, 100_000


def footprint_inputs(cam, n):
    move_mask = torch.zeros(cam["H"], cam["W"], dtype=torch.bool)
    move_mask[cam["H"] // 8:cam["H"] // 4, cam["W"] // 2:cam["W"] * 3 // 4] = True
    return move_mask, (torch.arange(n) % 8) == 0


def deterministic_cases(name, raw, cam, img, dep, pose, small_k, void_sums):
    hyper = dict(lambda_rgb=1.0, lambda_depth=0.1, lambda_var=10.0, lr=1e-3, total_iters=500)
    n = raw["xyz"].shape[0]
    eng = _engine(raw, cam, img, dep, pose=pose, **hyper)
    eng.deterministic = True
    stages = [STAGES[0], STAGES[2], ("first_cam", dict(freeze_rgb=0, freeze_all_splats=0, lr_camera=1e-3)), STAGES[1]]
    for stage, hp in stages:
        for k, v in hp.items():
            setattr(eng.hp, k, v)
        if stage == "camera":
            eng.set_footprint_mask(*footprint_inputs(cam, n))
        for _ in range(3):
            eng.iteration(reserved=False)
        outputs(f"det.{name}.{stage}.exact", eng)
        for _ in range(3):
            eng.iteration()
        outputs(f"det.{name}.{stage}.reserved", eng)
    images = eng.iteration(snapshot=True)
    outputs(f"det.{name}.snapshot_iteration", eng, images)
    digest(f"det.{name}.snapshot.images", eng.snapshot())
    # the void rule: the lists do not fit, nothing is stepped, overflow[1] counts the iteration
    from gflow_amd.fused import FitEngine
    void = FitEngine(cam["W"], cam["H"], capacity=max(2 * n, 1024), device=DEV, K_cap=small_k, deterministic=True)
    void.set_splats({k: v.to(DEV) for k, v in raw.items()})
    void.intr.copy_(cam["intr"].to(DEV))
    void.pose.copy_(pose.to(DEV))
    void.set_targets(img, dep)
    for k, v in dict(hyper, lr_camera=1e-3).items():
        setattr(void.hp, k, v)
    void.reset_optimizer()
    void.iteration()
    void.iteration()
    torch.cuda.synchronize()
    if void.overflow.tolist()[0] == 0 or void.overflow.tolist()[1] != 2:
        print(f"# {name}: K_cap={small_k} did not make the two iterations void: overflow {void.overflow.tolist()}", file=sys.stderr)
    for k in ("params", "adam_m", "adam_v", "pose", "pose_m", "pose_v", "depth_ab", "ab_m", "ab_v", "step") + (("sums",) if void_sums else ()):
        t = getattr(void, k)
        digest(f"det.{name}.void.{k}", t[:n] if k in ROWS else t)
    digest(f"det.{name}.void.overflow", void.overflow)


def default_cases(name, raw, cam, img, dep, pose):
    import gflow_amd.render as R
    n = raw["xyz"].shape[0]
    eng = _engine(raw, cam, img, dep, pose=pose, lambda_rgb=1.0, lambda_depth=0.1)
    eng.forward()
    torch.cuda.synchronize()
    for k in ("render", "final_T", "n_contrib", "rec"):
        t = getattr(eng, k)
        digest(f"default.{name}.forward.{k}", t[:n] if k in ROWS else t)
    digest(f"default.{name}.forward.lists", torch.cat(_lists(eng)))
    eng.hp.lr = 0.0
    eng.hp.lr_camera = 0.0
    eng.set_footprint_mask(*footprint_inputs(cam, n))
    images = eng.iteration(snapshot=True)
    torch.cuda.synchronize()
    for k in ("render", "final_T", "n_contrib", "keep"):
        digest(f"default.{name}.snapshot_iteration.{k}", getattr(eng, k))
    digest(f"default.{name}.snapshot_iteration.images", images)
    digest(f"default.{name}.snapshot.images", eng.snapshot())
    # render() forward and backward under torch's switch (tests/test_gpu_deterministic.py)
    from oracle import loss_oracle as LO
    act = {"xyz": raw["xyz"], "scale": raw["scale"].abs(), "rotate": torch.nn.functional.normalize(raw["rotate"]),
           "opacity": torch.sigmoid(10 * raw["opacity"]), "rgb": torch.sigmoid(raw["rgb"])}
    rcam = dict(intr=cam["intr"].to(DEV), extr=LO.pose_to_extr(pose).to(DEV), W=cam["W"], H=cam["H"])
    before, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        leaves = {k: v.to(DEV).clone().requires_grad_(True) for k, v in act.items()}
        out = R.render(leaves, rcam)
        (out["rgb"].square().sum() + out["depth_map"].sum() + out["uv"].sum()).backward()
        for k in ("rgb", "depth_map", "uv"):
            digest(f"default.{name}.render.{k}", out[k])
        for k in NAMES:
            digest(f"default.{name}.render.d_{k}", leaves[k].grad)
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn_only)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="pile,bench")
    ap.add_argument("--void-sums", action="store_true", help="also the loss sums of the void iterations (not reproducible)")
    args = ap.parse_args()
    from gflow_amd import _lib
    print(f"# library {os.path.basename(os.path.dirname(_lib.LIB_PATH))}/{os.path.basename(_lib.LIB_PATH)}", file=sys.stderr)
    for name, raw, cam, img, dep, pose, small_k in scenes(args.scenes.split(",")):
        deterministic_cases(name, raw, cam, img, dep, pose, small_k, args.void_sums)
        default_cases(name, raw, cam, img, dep, pose)
    print(f"# {COUNT[0]} digests", file=sys.stderr)


if __name__ == "__main__":
    main()
