"""io.load_sequence resolves a clip's sources once (``-m gpu``): within one call no file is read twice, a video file is
parsed once and the occlusion check runs once -- whichever of the frames, the occlusion masks and the two-view geometry
consume them."""
import os
import shutil

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _clip_as_folder_and_avi(tmp_path, n=4, H=48, W=64):
    """n written frames with their backward flows, and the same frames as ONE .avi beside a copy of the flow folder"""
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    from gflow_amd import video
    sc = S._Scene(H, W, 0)
    frames = [sc.frame(k) for k in range(n)]
    sp = gio.write_sequence(frames, str(tmp_path / "seq"))
    for k in range(1, n):
        gio.write_flow(os.path.join(sp + "_flow_unimatch", f"{k - 1:05d}_pred_bwd.flo"), sc.backward_flow(k).numpy())
    x = torch.stack([(torch.as_tensor(fr["image"]).float().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8) for fr in frames])
    avi = str(tmp_path / "clip.avi")
    video.write_avi(avi, x, fps=5, quality=95)
    shutil.copytree(sp + "_flow_unimatch", str(tmp_path / "clip_flow_unimatch"))
    return sp, avi


def _counted(monkeypatch, module, name, calls):
    inner = getattr(module, name)

    def counted(*args, **kw):
        calls.setdefault(name, []).append(str(args[0]) if isinstance(args[0], (str, os.PathLike)) else None)
        return inner(*args, **kw)

    monkeypatch.setattr(module, name, counted)


def test_one_call_reads_every_source_once(tmp_path, monkeypatch):
    from gflow_amd import io as gio
    from gflow_amd import occlusion, video
    sp, avi = _clip_as_folder_and_avi(tmp_path)
    calls = {}
    for module, name in ((gio, "_read_flo"), (gio, "_decode_image"), (video, "read_avi"), (occlusion, "flow_occlusion")):
        _counted(monkeypatch, module, name, calls)
    kw = dict(device=DEV, occ_masks="flow", depth_camera="estimate")
    for source in (sp, avi):
        for flows in ("files", "estimate"):
            calls.clear()
            frames = gio.load_sequence(source, flows=flows, **kw)
            assert len(frames) == 3 and all("occ_mask" in fr for fr in frames[1:]) and "occ_mask" not in frames[0]
            assert all(fr["flow"].is_cuda and fr["depth"].is_cuda for fr in frames)
            for name in ("_read_flo", "_decode_image"):
                paths = calls.get(name, [])
                assert None not in paths and len(set(paths)) == len(paths), (source, flows, name, paths)
            # forward and backward flow of the three pairs, or none of them; every image of a folder, none of a video file
            assert len(calls.get("_read_flo", [])) == (6 if flows == "files" else 0)
            assert len(calls.get("_decode_image", [])) == (0 if source == avi else 4 if flows == "estimate" else 3)
            assert len(calls.get("read_avi", [])) == (1 if source == avi else 0)
            assert len(calls["flow_occlusion"]) == 1, (source, flows)
    # a file with a bad magic number is no flow on the device path either (and no pair for the occlusion check)
    with open(os.path.join(sp + "_flow_unimatch", "00001_pred.flo"), "r+b") as f:
        f.write(b"\0\0\0\0")
    calls.clear()
    frames = gio.load_sequence(sp, device=DEV, occ_masks="flow")
    assert frames[1]["flow"] is None and frames[0]["flow"].is_cuda and frames[2]["flow"].is_cuda
    assert "occ_mask" in frames[1] and "occ_mask" not in frames[2] and len(calls["flow_occlusion"]) == 1
    assert len(set(calls["_read_flo"])) == len(calls["_read_flo"]) == 6
