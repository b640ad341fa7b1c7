"""CPU: the workspaces' size queries and the fit workspace's layout (gfl_fit_workspace_layout) are what they were before the
layouts were described once -- totals and every region's offset, recorded from that build's own carve -- and the layout holds
its invariants.  Shapes: the cap = 0 -> 1 clamp, K_cap = 0, one tile, a grid that is no multiple of 16, cap = 513 (one row past a
512-splat binning block and two 256-row reduce blocks), the bench shape, the 8 x capacity FitEngine allocates, 720p, a grid
above 4096 tiles."""
import ctypes

import pytest

# (cap, K_cap, W, H): gfl_fit_workspace_bytes, gfl_fit_snapshot_workspace_bytes(cap, W, H), gfl_loss_workspace_bytes(W, H),
# gfl_bin_workspace_bytes(cap, K_cap, W, H)
TOTALS = {
    (0, 0, 1, 1): (18410496, 5376, 768, 512),
    (1, 0, 16, 16): (18425344, 14592, 9728, 512),
    (1, 1, 17, 33): (18444288, 27392, 20736, 768),
    (513, 1000, 64, 48): (19463680, 127232, 111104, 8704),
    (60000, 1000000, 854, 480): (195461632, 16401152, 14802688, 8006912),
    (480000, 4000000, 854, 480): (1035846912, 16401152, 14802688, 32006912),
    (200000, 4000000, 1280, 720): (621876224, 36868352, 33278464, 32014848),
    (1, 16, 2560, 1440): (243213312, 147460352, 133113600, 58112),
}
# the regions in address order, and their offsets as the previous build's carve() placed them (pointer - workspace of every
# member it filled, printed from a throw-away copy of that build; loss_pad = loss_ws + its rounded size)
REGIONS = ("hist", "keys", "partial", "tile_counts", "pair_grad", "wide_off", "counters", "sched_work", "sched_list", "sched_count",
           "sched_counters", "ckpt", "sched_fwd_work", "sched_fwd_list", "sched_fwd_count", "first_slot", "loss_ws", "loss_pad",
           "gt_stats", "scale_cnt", "sort_order", "sort_order_next", "region", "fill", "partial_cam", "d_rec_cam")
OFFSETS = {
    (0, 0, 1, 1): (0, 256, 256, 512, 768, 2304, 2560, 2816, 3072, 23552, 27648, 31744, 18381824, 18382080, 18402560, 18406656,
                   18406912, 18407680, 18407936, 18408192, 18408448, 18408960, 18409472, 18409728, 18409984, 18410240),
    (1, 0, 16, 16): (0, 256, 256, 512, 768, 2304, 2560, 2816, 3072, 23552, 27648, 31744, 18381824, 18382080, 18402560, 18406656,
                     18406912, 18416640, 18416896, 18423040, 18423296, 18423808, 18424320, 18424576, 18424832, 18425088),
    (1, 1, 17, 33): (0, 256, 512, 768, 1024, 2816, 3072, 3328, 3584, 24064, 28160, 32256, 18382336, 18382592, 18403072, 18407168,
                     18407424, 18428160, 18428416, 18441984, 18442240, 18442752, 18443264, 18443520, 18443776, 18444032),
    (513, 1000, 64, 48): (0, 256, 8448, 8704, 8960, 845056, 847360, 847616, 847872, 868352, 872448, 876544, 19226624, 19226880,
                          19247360, 19251456, 19251712, 19362816, 19363072, 19436800, 19437056, 19437568, 19438080, 19438336,
                          19438592, 19438848),
    (60000, 1000000, 854, 480): (0, 764672, 8764672, 8776192, 8782848, 148942848, 149182976, 149183232, 149209344, 149332224,
                                 149336320, 149340416, 167690496, 167716608, 167839488, 167843584, 167850240, 182652928,
                                 182653184, 192491264, 192492288, 192518656, 192545024, 192571136, 192577792, 192581632),
    (480000, 4000000, 854, 480): (0, 6078464, 38078464, 38168576, 38175232, 967455232, 969375232, 969375488, 969401600, 969524480,
                                  969528576, 969532672, 987882752, 987908864, 988031744, 988035840, 988042496, 1002845184,
                                  1002845440, 1012683520, 1012691200, 1012717568, 1012743936, 1012770048, 1012776704, 1012806912),
    (200000, 4000000, 1280, 720): (0, 5630464, 37630464, 37668096, 37682688, 536882688, 537682688, 537682944, 537740544, 537990400,
                                   537994496, 537998592, 556348672, 556406272, 556656128, 556660224, 556674816, 589953280,
                                   589953536, 612071936, 612075264, 612133376, 612191488, 612249088, 612263680, 612276224),
    (1, 16, 2560, 1440): (0, 57600, 57856, 58112, 115712, 118016, 118272, 118528, 348928, 1286912, 1291008, 1295104, 19645184,
                          19875584, 20813568, 20817664, 20875264, 153988864, 153989120, 242462720, 242462976, 242693888,
                          242924800, 243155200, 243212800, 243213056),
}
TUPLES = sorted(TOTALS)


@pytest.fixture(scope="module")
def lib():
    from gflow_amd import _lib
    _lib.build()
    return _lib.load()


def layout(lib, t, room=64):
    names, offsets, sizes = (ctypes.c_char_p * room)(), (ctypes.c_size_t * room)(), (ctypes.c_size_t * room)()
    n = lib.gfl_fit_workspace_layout(*t, names, offsets, sizes, room)
    assert 0 < n <= room
    return [names[i].decode() for i in range(n)], list(offsets[:n]), list(sizes[:n])


@pytest.mark.parametrize("t", TUPLES)
def test_size_queries_answer_what_they_always_did(lib, t):
    cap, K_cap, W, H = t
    got = (lib.gfl_fit_workspace_bytes(cap, K_cap, W, H), lib.gfl_fit_snapshot_workspace_bytes(cap, W, H),
           lib.gfl_loss_workspace_bytes(W, H), lib.gfl_bin_workspace_bytes(cap, K_cap, W, H))
    assert got == TOTALS[t]


def test_invalid_sizes_give_zero(lib):
    for bad in ((-1, 0, 16, 16), (1, -1, 16, 16), (1, 0, 0, 16), (1, 0, 16, 0), (1, 0, -3, 16), (1, 0, 16, -3)):
        assert lib.gfl_fit_workspace_bytes(*bad) == 0, bad
        assert lib.gfl_fit_workspace_layout(*bad, None, None, None, 0) < 0, bad
    for bad in ((-1, 16, 16), (1, 0, 16), (1, 16, 0)):
        assert lib.gfl_fit_snapshot_workspace_bytes(*bad) == 0, bad
    assert lib.gfl_loss_workspace_bytes(0, 16) == 0 and lib.gfl_loss_workspace_bytes(16, -1) == 0
    assert lib.gfl_bin_workspace_bytes(1, -1, 16, 16) == 0 and lib.gfl_bin_workspace_bytes(1, 0, 0, 16) == 0
    assert lib.gfl_bin_workspace_bytes(1, 0, 16, 0) == 0


@pytest.mark.parametrize("t", TUPLES)
def test_layout_invariants(lib, t):
    names, offsets, sizes = layout(lib, t)
    n = len(names)
    # max = 0 counts and writes nothing (NULL tables would be written through); a short table is filled, not overrun
    assert lib.gfl_fit_workspace_layout(*t, None, None, None, 0) == n
    short_n, short_o, short_b = (ctypes.c_char_p * 4)(), (ctypes.c_size_t * 4)(*[7] * 4), (ctypes.c_size_t * 4)(*[7] * 4)
    assert lib.gfl_fit_workspace_layout(*t, short_n, short_o, short_b, 3) == n
    assert list(short_o) == offsets[:3] + [7] and list(short_b) == sizes[:3] + [7] and short_n[3] is None
    assert all(names) and len(set(names)) == n
    assert offsets[0] == 0 and all(o % 256 == 0 for o in offsets) and offsets == sorted(offsets)
    assert all(offsets[i] + sizes[i] <= offsets[i + 1] for i in range(n - 1))
    assert (offsets[-1] + sizes[-1] + 255) // 256 * 256 == lib.gfl_fit_workspace_bytes(*t)
    assert sizes[names.index("counters")] == 256


@pytest.mark.parametrize("t", TUPLES)
def test_offsets_are_the_previous_builds(lib, t):
    names, offsets, _ = layout(lib, t)
    assert tuple(names) == REGIONS
    assert dict(zip(names, offsets)) == dict(zip(REGIONS, OFFSETS[t]))


@pytest.mark.parametrize("t", [(60000, 1000000, 854, 480), (1, 1, 17, 33)])
def test_schedule_info_hands_out_the_layouts_regions(lib, t):
    """the queue lists and lengths of both schedules are base + the layout's offsets (a made-up base: nothing dereferences it)"""
    from gflow_amd.fused import FitState
    cap, K_cap, W, H = t
    base = 0x7F0000000000
    st = FitState(N=0, cap=cap, W=W, H=H, K_cap=K_cap, workspace=base, workspace_bytes=lib.gfl_fit_workspace_bytes(*t))
    names, offsets, _ = layout(lib, t)
    at = dict(zip(names, offsets))
    for fn, lst, cnt in ((lib.gfl_fit_schedule_info, "sched_list", "sched_count"),
                         (lib.gfl_fit_schedule_info_fwd, "sched_fwd_list", "sched_fwd_count")):
        nq, cap_q, lists, counts = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p(), ctypes.c_void_p()
        assert fn(ctypes.byref(st), ctypes.byref(nq), ctypes.byref(cap_q), ctypes.byref(lists), ctypes.byref(counts)) == 0
        assert lists.value == base + at[lst] and counts.value == base + at[cnt]
        assert nq.value >= 64 and nq.value * cap_q.value * 4 <= at[cnt] - at[lst]
    st.workspace_bytes -= 1
    assert lib.gfl_fit_schedule_info(ctypes.byref(st), ctypes.byref(nq), ctypes.byref(cap_q), ctypes.byref(lists),
                                     ctypes.byref(counts)) == -2
