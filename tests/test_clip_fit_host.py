"""CPU: the clip driver refuses a bad combination of options before a trainer exists -- on the first ``next()`` of
``fit_clip_steps`` (the single-case tests stay where they are: tests/test_tracking_back_host.py, test_deterministic_host.py),
in ``fit_clip`` and in ``fit_clips_concurrent`` before it touches a device -- with the message each has always had."""
import pytest

from gflow_amd import fit_video as FV
from gflow_amd.trainer import SimpleGaussian

STEPS = lambda frames, **kw: next(FV.fit_clip_steps(frames, "cpu", **kw))
CASES = [
    (lambda: STEPS([{}], track_backward=True), r"fit_clip\(track_backward=True\) needs track_queries"),
    (lambda: STEPS([{}], track_vis=True), r"fit_clip\(track_vis=True\) needs track_queries or cfg\['traj_num'\] > 0"),
    (lambda: STEPS([{}], cfg={"traj_num": 0}, track_vis=True), r"fit_clip\(track_vis=True\) needs track_queries or cfg\['traj_num'\] > 0"),
    (lambda: STEPS([{}], camera=True), r"fit_clip\(camera=True\): frames \[0\] carry neither extr_gt nor extr"),
    (lambda: FV.fit_clip([{}], "cpu", deterministic=True, fused=False), r"fit_clip\(deterministic=True\) needs fused=True"),
    (lambda: FV.fit_clips_concurrent([[{}], [{}]], "cpu", track_queries=[None]),
     "fit_clips_concurrent: track_queries needs one entry per clip"),
    (lambda: FV.fit_clips_concurrent([[{}], [{}]], "cpu", track_vis=[True]),
     "fit_clips_concurrent: a list of track_vis needs one entry per clip"),
    (lambda: FV.fit_clips_concurrent([[{}], [{}]], "cpu", track_backward=True),
     r"fit_clips_concurrent\(track_backward=True\) needs track_queries"),
]


@pytest.mark.parametrize("call,message", CASES, ids=["track_backward", "track_vis", "track_vis_traj_num_0", "camera", "deterministic",
                                                     "concurrent_queries", "concurrent_track_vis", "concurrent_track_backward"])
def test_option_errors_come_before_a_trainer_exists(monkeypatch, call, message):
    monkeypatch.setattr(SimpleGaussian, "__init__", lambda self, *a, **k: pytest.fail("a trainer was built before the options were refused"))
    with pytest.raises(ValueError, match=message):
        call()
