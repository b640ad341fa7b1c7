"""io.load_sequence on the host against the single-file readers (no device): the readers are the reference's port
(gflow/utils/read.py, conversion.py) and know nothing of the loader's resolve / prepare / assemble steps, so every tensor of
every frame must be what they give for that frame's files, bit for bit."""
import os

import pytest
import torch


@pytest.fixture()
def clip(tmp_path):
    """4 written frames at 48 x 64: the default slice loads frames 0 .. 2, frame_range=4 all four"""
    from gflow_amd import io as gio
    from gflow_amd import synthetic as S
    return gio.write_sequence(S.make_clip(4, H=48, W=64, seed=0), str(tmp_path / "seq"))


def _check_against_the_readers(frames, p, resize, blur):
    from gflow_amd import io as gio
    focal, pp, poses = gio.read_camera(p["camera"])
    assert len(frames) == len(p["img"])
    for i, fr in enumerate(frames):
        assert fr["name"] == os.path.basename(p["img"][i]).split(".")[0]
        assert torch.equal(fr["image"], gio.image_path_to_tensor(p["img"][i], resize, blur))
        assert torch.equal(fr["depth"], gio.read_depth(p["depth"][i], resize).unsqueeze(-1))
        if i < len(p["move"]):
            assert torch.equal(fr["move_mask"], gio.read_mask(p["move"][i], resize))
        if i < len(p["flow"]):
            want = gio.read_flow(p["flow"][i], resize, blur)
            assert (fr["flow"] is None) if want is None else torch.equal(fr["flow"], want)
        if 1 <= i <= len(p["occ"]):
            assert torch.equal(fr["occ_mask"], gio.image_path_to_tensor(p["occ"][i - 1], resize, blur))
        else:
            assert "occ_mask" not in fr
        assert fr["focal"] == focal and fr["pp"] == pp
        assert fr["extr"].dtype == torch.float32 and torch.equal(fr["extr"], torch.tensor(poses[i], dtype=torch.float32))
        assert "occ_count" not in fr and not any(v.is_cuda for v in fr.values() if torch.is_tensor(v))


@pytest.mark.parametrize("blur", [False, True])
@pytest.mark.parametrize("resize", [None, 24])
def test_every_frame_is_what_the_readers_give_for_its_files(clip, resize, blur):
    from gflow_amd import io as gio
    frames = gio.load_sequence(clip, resize=resize, blur=blur)
    assert len(frames) == 3 and frames[0]["image"].shape == ((48, 64, 3) if resize is None else (24, 32, 3))
    assert all(fr["move_mask"].dtype == torch.bool and fr["flow"].dtype == torch.float32 for fr in frames)
    _check_against_the_readers(frames, gio.sequence_paths(clip), resize, blur)
    # all four frames: the last one has no flow file and gets zeros
    frames = gio.load_sequence(clip, resize=resize, blur=blur, frame_range=4)
    _check_against_the_readers(frames, gio.sequence_paths(clip, frame_range=4), resize, blur)
    assert len(frames) == 4 and frames[3]["flow"].shape == frames[3]["image"].shape[:2] + (2,) and not frames[3]["flow"].any()


@pytest.mark.parametrize("resize", [None, 24])
def test_a_frame_without_its_move_file_gets_zeros_and_a_bad_flo_gives_none(clip, resize, capsys):
    from gflow_amd import io as gio
    p = gio.sequence_paths(clip, frame_range=4)
    assert any(bool(gio.read_mask(f).any()) for f in p["move"])          # (the written masks are not empty)
    os.remove(p["move"][3])                                              # the lists pair by position: the last frame loses its file
    with open(p["flow"][1], "r+b") as f:
        f.write(b"\0\0\0\0")
    capsys.readouterr()
    frames = gio.load_sequence(clip, resize=resize, frame_range=4)
    assert "Magic number incorrect" in capsys.readouterr().out
    assert frames[3]["move_mask"].dtype == torch.bool and frames[3]["move_mask"].shape == frames[3]["image"].shape[:2]
    assert not frames[3]["move_mask"].any()
    assert frames[1]["flow"] is None and all(frames[i]["flow"] is not None for i in (0, 2, 3))
    _check_against_the_readers(frames, gio.sequence_paths(clip, frame_range=4), resize, False)
