"""The fused fit iteration at every number of tile queues a share of the device can give (``-m gpu``).

The blend launches pull their tiles from one queue per compute unit; ``gfl_fit_state.cu_count`` (FitEngine(cu_count=)) sets
the number of queues ``nq`` (blend_queues, gflow_amd/csrc/gfl_fit.hip), and with it the XCD bands and the snake deal of
schedule_tiles_xcd, the ``ranked`` path (nq / 8 == 32 only), the forward's four-CU walk (helper stride nq / 4), the
backward's checkpointed segments (first_slot, ckpt_at(queue_slot)), the blend grids, the ticket arithmetic of next_item, the
queues' capacity, and WHICH launch builds the next schedule (the per-splat launch up to REDUCE_BLOCK = 256 queues, the
scatter launch in line above that, where there are no reserved tile regions either).  Every other test file runs the whole
device, nq = 256.  COUNTS below names the values held here and why; a test sets nothing but ``cu_count`` (no CU-masked
stream: the count sizes grids and queues, it does not confine them).  Counts above 256 are more queues than the device has
CUs -- the only way to run the path a larger part would take; their grids hold more workgroups than are resident at once,
which is safe because no workgroup of a blend launch waits for another (gfl_fit_fwd.hip / gfl_fit_bwd.hip: a workgroup's
only shared state is the pull counter of its queue, taken with one atomic add; no spin, no sleep).

Every tolerance is one an existing test uses for the same quantity (_check_fused_forward / _check_fused_gradients,
test_fused_gradients_with_four_segment_heavy_tiles, test_four_iterations_in_one_call_track_four_single_iterations,
test_render_operator_values_and_gradients_match_oracle); every other assertion is exact.

Observed on the MI355X (the lines the tests print through ``observe``).  Every exact assertion held at
every count: nothing in the library had to change.

``setup`` scene against the oracle (bounds: render 1e-4 / 1e-5 for all but 3e-4 of the values, gradients relative L2 2e-3).
At every count the render's largest error is 2.50e-06 (against the oracle and against the operator path), nothing off
tolerance; relative L2 of the gradients:

    queues   d_xyz     d_scale   d_rotate  d_opacity d_rgb     d_pose
    8        2.98e-06  2.39e-06  5.69e-06  6.53e-06  8.89e-06  1.83e-06
    16       2.97e-06  2.39e-06  5.69e-06  6.53e-06  8.90e-06  1.40e-06
    40       2.97e-06  2.39e-06  5.66e-06  6.71e-06  8.90e-06  1.11e-06
    48       2.98e-06  2.39e-06  5.64e-06  6.71e-06  8.89e-06  1.13e-06
    80       2.99e-06  2.39e-06  5.66e-06  6.71e-06  8.87e-06  1.19e-06
    128      2.99e-06  2.39e-06  5.66e-06  6.71e-06  8.87e-06  1.15e-06
    264      2.99e-06  2.39e-06  5.66e-06  6.71e-06  8.88e-06  1.13e-06
    512      2.99e-06  2.39e-06  5.66e-06  6.71e-06  8.87e-06  1.16e-06

Dense scene (lists of about 1100) against the operator path (bounds: render 2e-5 / 2e-6 for all but 1e-4, gradients 2e-3);
"split off": GFL_FWD_SPLIT_MIN=100000 in a process of its own; last row: 272 tiles, every list longer than 128:

    queues          render max  d_xyz     d_scale   d_rotate  d_opacity d_rgb
    8               9.54e-07    7.83e-07  1.15e-06  9.54e-07  9.48e-07  9.09e-07
    40              2.38e-07    7.22e-07  1.06e-06  8.54e-07  8.77e-07  7.40e-07
    128             2.38e-07    7.22e-07  1.06e-06  8.52e-07  8.76e-07  7.41e-07
    512             2.38e-07    7.22e-07  1.06e-06  8.48e-07  8.78e-07  7.40e-07
    8, split off    4.77e-07    8.81e-07  1.01e-06  1.22e-06  1.11e-06  7.97e-07
    40, split off   4.77e-07    5.25e-07  7.39e-07  9.58e-07  6.47e-07  7.21e-07
    128, split off  4.77e-07    5.25e-07  7.40e-07  9.59e-07  6.48e-07  7.21e-07
    512, split off  4.77e-07    5.25e-07  7.42e-07  9.58e-07  6.48e-07  7.21e-07
    512, 272 tiles  1.07e-06    8.01e-07  7.89e-07  1.13e-06  9.51e-07  6.60e-07

render() on a pooled engine of 8 / 320 queues against the oracle: rgb 2.98e-07, depth_map 1.43e-06 at both, d_extr
1.03e-06 / 1.09e-06; at 320 queues d_xyz 4.48e-07, d_scale 5.10e-07, d_rotate 5.48e-07, d_opacity 5.13e-07, d_rgb 4.04e-07.

Three libraries with one line changed each, against these tests: q = x * 8 + j in schedule_tiles_xcd fails
test_tile_schedule_at_every_queue_count at every count tried (64 to 512); checkpoints at queue_slot % 256 fail
test_checkpoints_of_queues_beyond_256 alone (d_xyz off by a factor of ten); a helper stride of nq / 2 in the forward
blend fails nothing, and cannot (test_long_lists_at_queue_count says why).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":              # (run as a script by test_long_lists_without_the_four_cu_walk_in_a_fresh_process)
    sys.path.insert(0, ROOT)

from tests.scenes import random_scene
from tests.test_gpu_fused import (POSE, _check_four_iterations_in_one_call, _check_fused_forward, _check_fused_gradients,
                                  _check_reserved_tile_regions, _engine, _forward_oracle, _gradient_oracle, _lists,
                                  _raw_from_scene, _reserved_on, _targets)
from tests.test_gpu_fused import setup  # noqa: F401  (the module-scoped fixture: 2500 splats, 168 x 120, 88 tiles)
from tests.test_gpu_parity import close_frac, observe

pytestmark = pytest.mark.gpu
DEV = "cuda"

SCHED_MAX_QUEUES, SCHED_PLAN_TILES, REDUCE_BLOCK, FWD_SPLIT_MIN = 512, 4096, 256, 448      # gfl_sched.hpp, gfl_fit.hpp

# cu_count given, queues expected (None: those of the whole device, 256 on the MI355X), why.  In the order they are run: the
# shares a partition really hands out first, then the smallest counts, then more queues than the device has CUs.
COUNTS = (
    (32, 32, "cu_partition(8): four queues per band"),
    (40, 40, "cu_partition(6); nq / 8 = 5 is no power of two"),
    (48, 48, "cu_partition(5); nq / 8 = 6"),
    (64, 64, "cu_partition(4): a band's queues are exactly one wave of the scheduling workgroup"),
    (80, 80, "cu_partition(3); a band's ten lanes lie across two waves"),
    (128, 128, "cu_partition(2)"),
    (100, 96, "rounded down to a multiple of 8"),
    (256, 256, "the ranked path (nq / 8 == 32), given explicitly: the control for 0"),
    (0, None, "the whole device"),
    (-5, None, "non-positive: the whole device"),
    (16, 16, "two queues per band: the snake has something to reverse"),
    (8, 8, "the floor: one queue per band, helper stride 2"),
    (7, 8, "rounded down to 0, raised to the floor"),
    (264, 264, "first count above REDUCE_BLOCK: scheduling in line, no reserved regions; nq / 8 = 33"),
    (320, 320, "as 264; nq / 8 = 40"),
    (512, 512, "SCHED_MAX_QUEUES; nq / 8 = 64"),
    (100000, 512, "capped at SCHED_MAX_QUEUES"),
)


def _id(cu_count):
    return f"cus{cu_count:06d}"         # (fixed width: no id is part of another, so ``-k`` can name one count)


def _cases(*counts):
    return pytest.mark.parametrize("cu_count", counts, ids=[_id(c) for c in counts])


def _whole_device():
    """blend_queues(cu_count <= 0): one queue per CU, at least 64, at most SCHED_MAX_QUEUES"""
    cus = torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count
    return min(max(cus, 64), SCHED_MAX_QUEUES)


def _expected_queues(cu_count):
    nq = {c: n for c, n, _ in COUNTS}.get(cu_count, cu_count)
    return _whole_device() if nq is None else nq


# ------------------------------------------------------------------------------------------------ 1. the schedule itself
# H, W -> splats: 12 tiles (fewer than most counts: empty bands and queues), 36, 88, 272, 1620, and 4225 -- above
# SCHED_PLAN_TILES, dealt by the general schedule_tiles without bands
GRIDS = {(48, 64): 800, (96, 96): 1500, (120, 168): 2500, (256, 272): 6000, (480, 854): 20000, (1040, 1040): 300}
_GRID_SCENES = {}


def _grid_scene(H, W, n):
    if (H, W) not in _GRID_SCENES:
        s = random_scene(n, W, H, seed=H + W, sigma_px=2.5, tilt=False)
        _GRID_SCENES[(H, W)] = (s, _raw_from_scene(s), *_targets(H, W, 5))
    return _GRID_SCENES[(H, W)]


def _queues(eng, forward):
    """(the tile ids of every queue, the capacity of one queue) as gfl_fit_schedule_info reports them; no queue is longer"""
    from gflow_amd import _lib as L
    nq, cap = ctypes.c_int(), ctypes.c_int()
    lists, counts = ctypes.c_void_p(), ctypes.c_void_p()
    fn = eng.lib.gfl_fit_schedule_info_fwd if forward else eng.lib.gfl_fit_schedule_info
    L.check(fn(ctypes.byref(eng.state()), ctypes.byref(nq), ctypes.byref(cap), ctypes.byref(lists), ctypes.byref(counts)), "info")
    nq, cap = nq.value, cap.value
    off_l, off_c = lists.value - eng.workspace.data_ptr(), counts.value - eng.workspace.data_ptr()
    assert 0 < off_l and off_l + 4 * nq * cap <= eng.workspace.numel() and 0 < off_c
    torch.cuda.synchronize()
    cnt = eng.workspace[off_c:off_c + 4 * nq].view(torch.int32).cpu().numpy()
    assert cnt.min() >= 0 and cnt.max() <= cap, f"a queue of {cnt.max()} items, capacity {cap}"
    lst = eng.workspace[off_l:off_l + 4 * nq * cap].view(torch.int32).reshape(nq, cap).cpu().numpy()
    return [(lst[q, :cnt[q]] & 0xffff).astype(np.int64) for q in range(nq)], cap


def _check_partition_and_bands(queues, nq, T, what):
    assert len(queues) == nq, f"{what}: {len(queues)} queues, expected {nq}"
    tiles = np.concatenate(queues)
    assert tiles.size == T and np.array_equal(np.sort(tiles), np.arange(T)), f"{what}: the queues are no partition of the tiles"
    if T > SCHED_PLAN_TILES:
        return
    # the band rule, whatever the weights: the queues q % 8 == x hold one contiguous run of tile indices, ascending with x
    last = -1
    for x in range(8):
        band = np.sort(np.concatenate(queues[x::8]))
        if band.size:
            assert band[0] == last + 1 and band[-1] - band[0] + 1 == band.size, f"{what}: band {x} is no run behind tile {last}"
            last = int(band[-1])
    assert last == T - 1, what


def _quantised(w, bins):
    shift = 0
    while (int(w.max()) >> shift) >= bins:
        shift += 1
    return w >> shift


def _check_first_schedule(queues, nq, lens, deterministic, what):
    """The schedule a fresh workspace gets from the scatter launch: no feedback, so the weights are the list lengths --
    schedule_tiles_xcd and schedule_tiles restated in integers."""
    T = lens.size
    w = np.minimum(np.maximum(lens.astype(np.int64), 1), 65535)
    if T > SCHED_PLAN_TILES:
        # schedule_tiles: the first round hands the nq heaviest tiles (counting sort on w >> shift, 1024 bins) to the queues
        qw = _quantised(w, 1024)
        cutoff = np.sort(qw)[::-1][nq - 1]
        for q in range(nq):
            assert queues[q].size > 0 and qw[queues[q][0]] >= cutoff, f"{what}: queue {q} does not start with one of the {nq} heaviest"
        return
    prefix = np.cumsum(w) - w
    band = np.minimum(7, prefix * 8 // max(int(w.sum()), 1))
    qw = _quantised(w, 128)
    for x in range(8):
        mine = np.nonzero(band == x)[0]
        got = np.sort(np.concatenate(queues[x::8]))
        assert np.array_equal(got, mine), f"{what}: band {x} holds {got.tolist()}, the cut gives {mine.tolist()}"
        order = mine[np.lexsort((mine, -qw[mine]))]          # descending quantised weight, ascending tile index
        for j in range(nq // 8):
            q = j * 8 + x
            if j >= order.size:
                assert queues[q].size == 0, f"{what}: queue {q} of a band of {order.size} tiles is not empty"
            elif deterministic:
                assert queues[q].size and queues[q][0] == order[j], f"{what}: queue {q} starts with {queues[q][:1]}, not {order[j]}"
            else:
                assert queues[q].size and qw[queues[q][0]] == qw[order[j]], f"{what}: queue {q} starts with the wrong weight"


@pytest.mark.parametrize("deterministic", [True, False], ids=["deterministic", "default"])
@pytest.mark.parametrize("cu_count", [c for c, _, _ in COUNTS], ids=[_id(c) for c, _, _ in COUNTS])
def test_tile_schedule_at_every_queue_count(cu_count, deterministic):
    """Six tile grids, a forward and three iterations each.  After every one of them, for the forward's queues and the
    backward's: the number of queues, a partition of the tiles, no queue beyond its capacity, the band rule.  After the first
    forward of the fresh engine also the band cut and every queue's first item, from the list lengths (in the default mode
    ties of a quantised weight are in arrival order: the weight is held, not the tile).  The later schedules are built from the
    blend kernels' work counts -- by the per-splat launch up to 256 queues and 4096 tiles, by the scatter launch otherwise."""
    nq = _expected_queues(cu_count)
    for (H, W), n in GRIDS.items():
        s, raw, img, dep = _grid_scene(H, W, n)
        eng = _engine(raw, s, img, dep, cu_count=cu_count, deterministic=deterministic, lr=1e-3, lambda_rgb=1.0, lambda_depth=0.1)
        T = eng.T
        assert T == ((H + 15) // 16) * ((W + 15) // 16)
        eng.forward()
        eng.check_overflow()
        lens = (eng.tile_range[:, 1] - eng.tile_range[:, 0]).cpu().numpy()
        for fwd in (True, False):
            what = f"{H}x{W}, {nq} queues, first forward, {'forward' if fwd else 'backward'} queues"
            queues, _ = _queues(eng, fwd)
            _check_partition_and_bands(queues, nq, T, what)
            _check_first_schedule(queues, nq, lens, deterministic, what)
        for it in range(3):
            eng.iteration()
            for fwd in (True, False):
                queues, _ = _queues(eng, fwd)
                _check_partition_and_bands(queues, nq, T, f"{H}x{W}, {nq} queues, iteration {it}, {'forward' if fwd else 'backward'} queues")
        eng.check_overflow()
        assert bool(torch.isfinite(eng.params[:eng.N]).all()) and int(eng.step.item()) == 3


# ------------------------------------------------------------------------ 2. forward and gradients against the oracle
@pytest.fixture(scope="module")
def oracles(setup):
    s, raw, img, dep = setup
    return _forward_oracle(s, raw), _gradient_oracle(s, raw, img, dep)


@_cases(40, 48, 80, 128, 16, 8, 264, 512)
def test_fused_forward_and_gradients_match_the_oracle_at_queue_count(setup, oracles, cu_count):
    """The ``setup`` scene of tests/test_gpu_fused.py (88 tiles: far above the smallest counts, below the largest) through
    _check_fused_forward and _check_fused_gradients with their own bounds; the oracle's side is computed once."""
    nq = _expected_queues(cu_count)
    _check_fused_forward(*setup, tag=f"[{nq} queues] ", oracle=oracles[0], cu_count=cu_count)
    _check_fused_gradients(*setup, tag=f"[{nq} queues] fused: ", oracle=oracles[1], cu_count=cu_count)


# --------------------------------------------------------------------- 3. long lists: segments and the four-CU walk
def _operator_reference(s, raw, img, dep):
    """render and the gradients of the fourteen columns through the operator path (autograd over the five msplat operators and
    the loss kernels), identity pose, lambda_rgb 1, lambda_depth 0.1 -- what test_fused_gradients_with_four_segment_heavy_tiles
    compares with"""
    from gflow_amd import losses
    from gflow_amd.fused import COLS
    from oracle import fit_oracle as FO
    from oracle import loss_oracle as LO
    import gflow_amd.render as R
    n = raw["xyz"].shape[0]
    leaf = {k: raw[k].to(DEV).clone().requires_grad_(True) for k in ("xyz", "scale", "rotate", "opacity", "rgb")}
    act = FO.activate(leaf)
    extr = LO.pose_to_extr(torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])).to(DEV)
    og = R.render_multiple([*act, s["intr"].to(DEV), extr, 0.0, s["W"], s["H"]], ["rgb", "depth_map"])
    render4 = torch.cat([og["rgb"], og["depth_map"]])
    ab = torch.tensor([1.0, 0.0], device=DEV)
    loss, _, _, _ = losses.image_loss(render4, img.to(DEV), dep.to(DEV), ab, 1.0, 0.1, None)
    loss.backward()
    return render4.detach(), {k: leaf[k].grad.reshape(n, b - a) for k, (a, b) in COLS.items()}


def _check_against_operator_path(scene, ref, cu_count, tag):
    """one iteration of a fresh engine of that count against _operator_reference; returns the engine"""
    from gflow_amd.fused import COLS
    s, raw, img, dep = scene
    render4, grads = ref
    n = raw["xyz"].shape[0]
    eng = _engine(raw, s, img, dep, cu_count=cu_count, lr=0.0, lr_camera=0.0, lambda_rgb=1.0, lambda_depth=0.1, lambda_var=0.0)
    eng.iteration()
    eng.check_overflow()
    close_frac(eng.render, render4, 2e-5, 2e-6, bad_frac=1e-4, hard=2e-2, what=f"{tag}fused vs operator path")
    for k, (a, b) in COLS.items():
        got = eng.adam_m[:n, a:b] / 0.1
        rel = ((got - grads[k]).norm() / grads[k].norm()).item()
        observe(f"{tag}d_{k}: relative L2 {rel:.2e} (bound 0.002)")
        assert rel < 2e-3, f"{tag}d_{k}: relative L2 error {rel:.2e}"
    return eng


def _dense_scene():
    """test_fused_gradients_with_four_segment_heavy_tiles': 20 000 splats on 96 x 96, 36 tiles, lists of about 1100"""
    s = random_scene(20000, 96, 96, seed=5, sigma_px=2.0, tilt=False)
    return s, _raw_from_scene(s), *_targets(96, 96, 9)


@pytest.fixture(scope="module")
def dense():
    scene = _dense_scene()
    return scene, _operator_reference(*scene)


def _check_dense(scene, ref, cu_count, tag=""):
    nq = _expected_queues(cu_count)
    eng = _check_against_operator_path(scene, ref, cu_count, f"[dense scene, {nq} queues{tag}] ")
    lens = eng.tile_range[:, 1] - eng.tile_range[:, 0]
    assert int(lens.max()) > max(FWD_SPLIT_MIN, 960), f"scene too sparse: longest list {int(lens.max())}"
    assert len(_queues(eng, True)[0]) == nq


@_cases(40, 128, 8, 512)
def test_long_lists_at_queue_count(dense, cu_count):
    """Every tile's list is longer than FWD_SPLIT_MIN and than 960: a queue's first tile is walked on four CUs (forward) and in
    up to eight checkpointed segments (backward).  At 8 queues only eight of the 36 tiles are a queue's first: the rest are
    walked whole by workgroups that pull many tickets each; at 40 there is almost one tile per queue; at 128 and 512 most
    queues are empty and their items 1 to 3 only help other queues' first tiles (owner (q + part nq / 4) % nq).
    What this holds is that every block of every tile is walked exactly once, from the right checkpoints, whoever walks it.
    It cannot tell the stride nq / 4 from another one: item ``part`` of queue q helps queue (q + part * stride) % nq, which for
    ANY stride gives block ``part`` of every first tile exactly one walker (a library built with nq / 2 passes this test, the
    fresh-process one below and the dense-scene test of tests/test_gpu_fused.py) -- the stride decides on which CU a block is walked, and the scheduler's load
    estimate (gfl_sched.hpp) assumes the same one; it is a matter of speed, not of results."""
    _check_dense(*dense, cu_count)


def _split_off_probe():
    """(this file run as a script, GFL_FWD_SPLIT_MIN=100000 in its environment: the switch is read once per process)"""
    sys.path.insert(0, ROOT)
    assert os.environ.get("GFL_FWD_SPLIT_MIN") == "100000"
    scene = _dense_scene()
    ref = _operator_reference(*scene)
    for cu_count in (40, 128, 8, 512):
        _check_dense(scene, ref, cu_count, ", no four-CU walk")
    print("RESULT ok")


def test_long_lists_without_the_four_cu_walk_in_a_fresh_process():
    """The same scene and counts with the forward's four-CU walk switched off (every first tile is walked whole by its own
    queue; the backward's segments stay): a wrong helper mapping and a wrong segment walk fail apart."""
    env = {k: v for k, v in os.environ.items() if k not in ("GFL_EWA_MFMA", "GFL_RESERVED", "GFL_FWD_SPLIT_MIN")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(env, GFL_FWD_SPLIT_MIN="100000"), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_checkpoints_of_queues_beyond_256():
    """40 000 splats on 256 x 272: 272 tiles, 34 to a band, every list longer than 128 -- so at 512 queues the first tiles of
    the queues j * 8 + x with j >= 32 leave their checkpoints in slots 256 and above (the 36 tiles of the dense scene never
    reach beyond queue 39: checkpoints indexed by queue_slot % 256 pass test_long_lists_at_queue_count at 512 queues and fail
    here, with a relative error of 10 in d_xyz).  Same comparison, same bounds."""
    s = random_scene(40000, 272, 256, seed=7, sigma_px=2.0, tilt=False)
    scene = (s, _raw_from_scene(s), *_targets(256, 272, 9))
    eng = _check_against_operator_path(scene, _operator_reference(*scene), 512, "[272 tiles, 512 queues] ")
    lens = (eng.tile_range[:, 1] - eng.tile_range[:, 0]).cpu().numpy()
    # (above 256 queues nothing deals new queues behind the backward: these are the ones the iteration ran on)
    queues, _ = _queues(eng, False)
    high = [q for q in range(256, 512) if queues[q].size]
    assert high and all(lens[queues[q][0]] > 128 for q in high), "no segmented first tile in a queue beyond 255"
    assert int(lens.min()) > 128, int(lens.min())


# ------------------------------------------------------------------------------------------------- 4. deterministic mode
_FIT_HYPER = dict(lambda_rgb=1.0, lambda_depth=0.1, lambda_var=10.0, lr=1e-3, lr_camera=1e-3, total_iters=100)
_OUT = ("render", "final_T", "n_contrib", "params", "adam_m", "adam_v", "pose", "pose_m", "pose_v", "depth_ab", "ab_m", "ab_v",
        "sums", "step")


def _assert_same_bits(a, b, what, raw_lists=True):
    """render, final_T, n_contrib, the sorted lists, rows and both moments, pose, depth affine, loss sums.  ``raw_lists``:
    ids[:K] and tile_range as they lie (False: tile by tile -- an iteration on reserved regions leaves gaps between the lists,
    one on the exact path does not)."""
    assert a.N == b.N and a.K == b.K, what
    for k in _OUT:
        x, y = getattr(a, k), getattr(b, k)
        if k in ("params", "adam_m", "adam_v"):
            x, y = x[:a.N], y[:b.N]
        assert torch.equal(x, y), f"{what}: {k} differs ({(x != y).float().mean().item():.2e} of the values)"
    assert all(torch.equal(x, y) for x, y in zip(a.loss_terms(), b.loss_terms())), f"{what}: loss terms"
    if raw_lists:
        assert torch.equal(a.tile_range, b.tile_range) and torch.equal(a.ids[:a.K], b.ids[:b.K]), f"{what}: ids / tile_range"
    else:
        assert all(torch.equal(x, y) for x, y in zip(_lists(a), _lists(b))), f"{what}: a tile's sorted list differs"


def _three_iterations(scene, cu_count, watch=None):
    s, raw, img, dep = scene
    eng = _engine(raw, s, img, dep, pose=POSE, cu_count=cu_count, deterministic=True, **_FIT_HYPER)
    for _ in range(3):
        eng.iteration()
        if watch is not None:
            watch(eng)
    eng.check_overflow()
    return eng


@_cases(80, 128, 8, 320)
def test_two_deterministic_engines_of_one_count_are_bit_identical(setup, cu_count):
    a, b = _three_iterations(setup, cu_count), _three_iterations(setup, cu_count)
    assert len(_queues(a, False)[0]) == _expected_queues(cu_count)
    _assert_same_bits(a, b, f"{_expected_queues(cu_count)} queues, engine against engine")


def test_the_whole_device_given_explicitly_is_the_default(setup):
    nq = _whole_device()
    a, b = _three_iterations(setup, nq), _three_iterations(setup, 0)
    _assert_same_bits(a, b, f"cu_count = {nq} against cu_count = 0")


def test_without_split_tiles_the_queue_count_changes_no_bit():
    """include/gflow_hip.h and gfl_sched.hpp: the schedule enters a result only through the tiles that are walked in segments
    (backward: lists longer than 128) or on four CUs (forward: longer than FWD_SPLIT_MIN); everything else moves whole tiles
    between CUs.  A scene without such a tile (checked after every iteration), deterministic mode, seven queue counts: every
    output bit for bit.  A queue's first tile with ONE part is walked as any other tile -- forward: fwd_walk_block with
    parts = 1 stores no checkpoint; backward: item.part = 0 = parts - 1 makes it the last part, lo = 0, hi = depth_n -- so
    nothing rounds differently.  Up to 256 queues an iteration bins into reserved tile regions, above it on the exact path:
    the lists are compared tile by tile across that line, ids and tile_range as they lie on either side of it."""
    s = random_scene(1200, 168, 120, seed=41, sigma_px=2.0, tilt=False)
    scene = (s, _raw_from_scene(s), *_targets(120, 168, 5))

    def watch(eng):
        lens = eng.tile_range[:, 1] - eng.tile_range[:, 0]
        assert 0 < int(lens.max()) <= 128, f"a list of {int(lens.max())}: the scene has a tile that is walked in segments"

    counts = (256, 48, 80, 128, 8, 320, 512)
    engines = {c: _three_iterations(scene, c, watch) for c in counts}
    for c in counts:
        assert len(_queues(engines[c], False)[0]) == c
    for c in counts[1:]:
        same_side = c <= REDUCE_BLOCK or not _reserved_on(engines[256])
        _assert_same_bits(engines[256], engines[c], f"256 queues against {c}", raw_lists=same_side)
    _assert_same_bits(engines[320], engines[512], "320 queues against 512")


# ------------------------------------------------------------------------------------------- 5. paths that nq switches
@_cases(80, 8)
def test_reserved_tile_regions_at_queue_count(setup, cu_count):
    _check_reserved_tile_regions(setup, False, cu_count=cu_count)


@_cases(264, 512)
def test_no_reserved_tile_regions_above_256_queues(setup, cu_count):
    """Above REDUCE_BLOCK queues the per-splat launch carries no scheduling workgroups and reserves nothing:
    gfl_fit_reserved_supported says so, an iteration told to use reserved regions is refused before any launch, and
    iteration(count=4) gives what four single iterations give (test_four_iterations_in_one_call_track_four_single_iterations)."""
    from gflow_amd import _lib as L
    s, raw, img, dep = setup
    eng = _engine(raw, s, img, dep, pose=POSE, cu_count=cu_count, lambda_rgb=1.0, lr=1e-3, lr_camera=0.0)
    assert len(_queues(eng, False)[0]) == cu_count
    assert not _reserved_on(eng)
    eng.iteration()
    assert eng._reserved_flag() == 0
    rows = eng.params[:eng.N].clone()
    rc = eng.lib.gfl_fit_iterations(ctypes.byref(eng.state()), ctypes.byref(eng.hp), 1, eng.GFL_ITER_RESERVED, L.stream())
    torch.cuda.synchronize()
    assert rc != 0 and int(eng.step.item()) == 1 and torch.equal(eng.params[:eng.N], rows)
    eng.check_overflow()
    _check_four_iterations_in_one_call(setup, cu_count=cu_count)


@_cases(8, 320)
def test_snapshot_images_do_not_depend_on_the_queue_count(setup, cu_count):
    """gfl_fit_iteration_snapshot's forward and gfl_fit_snapshot's composite launch on the engine's queues.  No list of the
    scene reaches FWD_SPLIT_MIN, so every tile is walked a splat at a time whatever queue holds it: the three images of a
    snapshot iteration and of a snapshot behind it, byte for byte those of a 256-queue engine, over three iterations (rows
    at rest: lr = 0; the second and third run on queues dealt from counted work)."""
    s, raw, img, dep = setup
    hyper = dict(lr=0.0, lr_camera=0.0, lambda_rgb=1.0, lambda_depth=0.1)
    a = _engine(raw, s, img, dep, pose=POSE, cu_count=cu_count, deterministic=True, **hyper)
    b = _engine(raw, s, img, dep, pose=POSE, cu_count=256, deterministic=True, **hyper)
    assert len(_queues(a, True)[0]) == cu_count and len(_queues(b, True)[0]) == 256
    for it in range(3):
        got, want = a.iteration(snapshot=True).clone(), b.iteration(snapshot=True).clone()
        lens = a.tile_range[:, 1] - a.tile_range[:, 0]
        assert 0 < int(lens.max()) <= FWD_SPLIT_MIN
        for k, name in enumerate(("rgb", "depth_map_color", "center")):
            assert torch.equal(got[k], want[k]), f"{name}, iteration {it}: {(got[k] != want[k]).float().mean().item():.2e} of the bytes differ"
        assert torch.equal(a.snapshot(), b.snapshot()), f"gfl_fit_snapshot, iteration {it}"
        assert torch.equal(a.render, b.render) and torch.equal(a.final_T, b.final_T) and torch.equal(a.n_contrib, b.n_contrib)
    assert int(got.max()) > 0


@pytest.fixture(scope="module")
def render_case():
    from tests.test_gpu_render_op import _render_oracle
    s = random_scene(3000, 200, 136, seed=11, sigma_px=2.5)
    return s, _render_oracle(s, 0.33)


@_cases(8, 320)
def test_render_operator_at_queue_count(render_case, cu_count):
    """gfl_render_fwd / gfl_render_bwd reach a FitEngine through render()'s pool of engines: one of ``cu_count`` is put there
    for the call -- scene and bounds of test_render_operator_values_and_gradients_match_oracle."""
    import gflow_amd.render as R
    from gflow_amd.fused import FitEngine
    from tests.test_gpu_render_op import _check_render_operator
    s, oracle = render_case
    key = (s["W"], s["H"], str(torch.zeros(1, device=DEV).device))
    eng = FitEngine(s["W"], s["H"], 65536, torch.zeros(1, device=DEV).device, cu_count=cu_count)
    saved = R._POOL.get(key)
    R._POOL[key] = [R._Slot(eng)]
    try:
        _check_render_operator(s, 0.33, tag=f"[{cu_count} queues] render(): ", oracle=oracle)
        assert len(R._POOL[key]) == 1 and not R._POOL[key][0].busy, "render() did not use the pooled engine"
        eng.check_overflow()
    finally:
        if saved is None:
            del R._POOL[key]
        else:
            R._POOL[key] = saved
    queues, _ = _queues(eng, False)
    assert len(queues) == cu_count and sum(q.size for q in queues) == eng.T      # (... and a forward has dealt its tiles)


def test_whole_fit_at_80_queues_is_bit_identical_run_to_run():
    """The three-frame clip of test_whole_fit_is_bit_identical_run_to_run through fit_clip_steps(cu_count=80,
    deterministic=True) -- what fit_clips_concurrent(partition=True) runs for each of three clips -- twice: everything
    tests/score_fit.py's assert_same_fit compares."""
    from gflow_amd.clip_fit import fit_clip_steps
    from gflow_amd.trainer import run_to_end
    from tests import score_fit as SF
    from tests.test_gpu_deterministic import SMALL
    from tests.test_gpu_fitvideo import _clip
    frames = _clip()
    _, q = SF.queries(n_frames=len(frames))
    runs = []
    stream = torch.cuda.Stream()
    for _ in range(2):
        keep = {}
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out = run_to_end(fit_clip_steps(frames, DEV, {**SMALL, "traj_num": 40}, seed=0, keep=keep, cu_count=80,
                                            deterministic=True, track_queries=q))
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        runs.append((out, keep))
    eng = runs[0][1]["trainer"].engine
    assert eng.cu_count == 80 and len(_queues(eng, False)[0]) == 80
    assert runs[0][0]["splats_final"] > SMALL["num_points"]            # densification ran
    SF.assert_same_fit(*runs[0], *runs[1])


if __name__ == "__main__":
    _split_off_probe()
