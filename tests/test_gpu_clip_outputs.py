"""A clip fit's optional outputs switched on TOGETHER (``-m gpu``; fit_video.fit_clip_steps' end of a frame): every one of
them is, bit for bit, what the fit gives with that output alone, the fit itself does not notice them, and the frame's final
state is rasterised once more per frame on the fused path however many of them read it -- once per reader on the operator
path.  The clip is tests/score_fit.py's with 4 frames: a frame 0, a first later frame and a steady later one."""
import functools

import numpy as np
import pytest

from tests import score_fit as SF

pytestmark = pytest.mark.gpu
N_FRAMES = 4


@functools.lru_cache(maxsize=None)
def _inputs():
    return SF.clip(n_frames=N_FRAMES), SF.queries(n_frames=N_FRAMES)[1]


@functools.lru_cache(maxsize=None)
def _fit(traj=False, q=False, fused=True, **outputs):
    """(out, keep) of the fit with these outputs on: computed once, shared, never written to"""
    from gflow_amd.fit_video import fit_clip
    frames, queries = _inputs()
    keep = {}
    out = fit_clip(frames, SF.DEV, dict(SF.FIT, traj_num=50) if traj else SF.FIT, seed=0, fused=fused,
                   deterministic=True if fused else None, track_queries=queries if q else None, keep=keep, **outputs)
    return out, keep


def _same_bits(a, b, what):
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64), err_msg=what)


def test_every_output_on_equals_each_output_alone():
    from gflow_amd.camera import SCORE_KEYS
    out, keep = _fit(traj=True, q=True, segment=True, recon=True, camera=True, flow=True)
    base, keep0 = _fit(traj=True, q=True)
    assert sorted(set(out) - set(base)) == ["camera", "flow", "recon", "segmentation"]
    SF.assert_same_fit(out, keep, base, keep0)
    _same_bits(out["flow"]["sums"], _fit(flow=True)[0]["flow"]["sums"], "flow sums")
    assert out["flow"]["sums"].shape == (N_FRAMES - 1, 3, 6) and (out["flow"]["sums"][:, 0, 1] > 0).all()
    alone = _fit(recon=True, camera=True)[0]
    for k in ("sse", "ssim_sum", "PSNR", "SSIM"):
        _same_bits(out["recon"][k], alone["recon"][k], k)
    assert out["camera"]["extr"].tobytes() == alone["camera"]["extr"].tobytes()
    for k in SCORE_KEYS:
        assert out["camera"][k] == alone["camera"][k] and out["camera"][k] is not None, k


def test_overlays_and_backward_tracks_on_top_of_every_output():
    """The overlays and backward tracking beside every other output: the fit does not notice them (the overlays rasterise
    nothing, backward tracking reads the shared forward: ``rasterisations`` is equal), the tracks are those of the fit with
    nothing else on, and the overlays have equal bytes whether the seeds' hull masks come from ``out["segmentation"]``
    (``segment=True``) or from the recorder the overlays asked for themselves."""
    all_on = _fit(traj=True, q=True, track_backward=True, track_vis=True, segment=True, recon=True, camera=True, flow=True)
    base = _fit(traj=True, q=True, track_backward=True)
    alone = _fit(traj=True, q=True, track_backward=True, track_vis=True)
    SF.assert_same_fit(*all_on, *base)
    tracks, tracks_alone = all_on[0]["tracks"], alone[0]["tracks"]
    assert sorted(tracks) == sorted(tracks_alone) and "back_anchor" in tracks
    for k in tracks:
        np.testing.assert_array_equal(tracks[k], tracks_alone[k], err_msg=k)
    vis, vis_alone = all_on[0]["track_vis"], alone[0]["track_vis"]
    assert sorted(vis) == sorted(vis_alone) and {"pred", "seeds", "seeds_still"} <= set(vis)
    for k in vis:
        assert vis[k].dtype == np.uint8 and vis[k].shape == vis_alone[k].shape == (N_FRAMES, SF.H, SF.W, 3), k
        assert vis[k].tobytes() == vis_alone[k].tobytes(), k


# one forward per frame on the fused path, shared by the tracker and the flow recorder; on the operator path each of
# them renders for itself
@pytest.mark.parametrize("fused,outputs,forwards", [(True, dict(q=True, flow=True), N_FRAMES), (True, dict(q=True), N_FRAMES),
                                                    (True, dict(flow=True), N_FRAMES),
                                                    (False, dict(q=True, flow=True), 2 * N_FRAMES)])
def test_forwards_of_a_frames_final_state_without_trajectories(fused, outputs, forwards):
    out, plain = _fit(fused=fused, **outputs)[0], _fit(fused=fused)[0]
    assert out["rasterisations"] == plain["rasterisations"] + forwards
    assert out["iterations"] == plain["iterations"] and out["frames"] == N_FRAMES
    if fused and len(outputs) == 2:                      # the shared forward gives each reader what its own would
        assert out["psnr_sum"] == plain["psnr_sum"]
        for k in ("tracks", "occluded", "anchor", "shift"):
            np.testing.assert_array_equal(out["tracks"][k], _fit(q=True)[0]["tracks"][k])
        _same_bits(out["flow"]["sums"], _fit(flow=True)[0]["flow"]["sums"], "flow sums")
