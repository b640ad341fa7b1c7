"""Deterministic mode, host side (no GPU): the C ABI of the flag (include/gflow_hip.h, GFL_FIT_DETERMINISTIC), its mirror in
gflow_amd/fused.py, and how the Python entry points take and resolve the switch."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gflow_hip.h")) as f:
        return f.read()


def test_header_defines_the_flag_and_the_version():
    hdr = _header()
    assert re.search(r"^#define GFL_FIT_DETERMINISTIC 1\b", hdr, flags=re.M)
    assert int(re.search(r"^#define GFL_VERSION (\d+)$", hdr, flags=re.M).group(1)) >= 305
    assert re.search(r"int32_t flags;", hdr) and "reserved_" not in hdr.split("} gfl_fit_state;")[0].split("typedef struct gfl_fit_state")[1]
    assert "int gfl_scan_f64(" in hdr
    from gflow_amd import _lib
    assert _lib.MIN_VERSION >= 305
    assert "gfl_scan_f64" in _lib.SIGNATURES and "gfl_scan_f64_workspace_bytes" in _lib.SIGNATURES


def test_fit_state_flags_sits_where_reserved_was():
    from gflow_amd import _lib
    from gflow_amd.fused import GFL_FIT_DETERMINISTIC, FitState
    names = [n for n, _ in FitState._fields_]
    assert "reserved_" not in names and names[-2:] == ["cu_count", "flags"]
    # the word behind cu_count, as reserved_ was: the struct's size and every offset are those of ABI 304
    assert FitState.flags.offset == FitState.cu_count.offset + 4
    assert FitState.flags.offset + 4 <= ctypes.sizeof(FitState)
    assert GFL_FIT_DETERMINISTIC == 1
    lib = _lib.load()
    s, h = ctypes.c_int(), ctypes.c_int()
    assert lib.gfl_abi_sizes(ctypes.byref(s), ctypes.byref(h)) == 0
    from gflow_amd.fused import FitHyper
    assert (s.value, h.value) == (ctypes.sizeof(FitState), ctypes.sizeof(FitHyper))


def test_scan_workspace_is_one_double_per_chunk():
    from gflow_amd import _lib
    lib = _lib.load()
    chunk = int(re.search(r"^#define GFL_SCAN_CHUNK (\d+)$", _header(), flags=re.M).group(1))
    for n, chunks in ((1, 1), (chunk, 1), (chunk + 1, 2), (480 * 854, -(-480 * 854 // chunk))):
        assert lib.gfl_scan_f64_workspace_bytes(n) == 8 * chunks
    # argument checks need no device: a negative length is refused before anything is launched
    assert lib.gfl_scan_f64(None, -1, None, None, 0, None) == -1
    assert lib.gfl_scan_f64(None, 0, None, None, 0, None) == 0


def test_entry_points_take_deterministic(monkeypatch, capsys):
    from gflow_amd import fit_video as FV
    from gflow_amd.fit_video import fit_clip, fit_clip_steps, fit_clips_concurrent, main
    from gflow_amd.fused import FitEngine
    from gflow_amd.trainer import SimpleGaussian
    for fn in (fit_clip, fit_clip_steps, fit_clips_concurrent, SimpleGaussian.__init__):
        p = inspect.signature(fn).parameters["deterministic"]
        assert p.default is None, fn
    assert inspect.signature(FitEngine.__init__).parameters["deterministic"].default is False
    # the command line: the parser has the switch (off by default), and main hands it to the fit as deterministic=True / None
    assert FV._parser().parse_args([]).deterministic is False and FV._parser().parse_args(["--deterministic"]).deterministic is True
    seen = []
    monkeypatch.setattr(FV, "_ranks", lambda: (0, 1, torch.device("cpu"), None, (None, torch.device("cpu"))))
    monkeypatch.setattr(FV, "_load_clips", lambda args, mine, lengths, dev: {ci: [{}] for ci in mine})
    monkeypatch.setattr(FV, "fit_clip", lambda frames, dev, cfg, **kw: seen.append(kw["deterministic"]) or dict.fromkeys(FV.METRIC_NAMES, 0.0))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    main(["--deterministic"])
    main([])
    assert seen == [True, None] and capsys.readouterr().out.count('"psnr_sum"') == 2


def test_none_follows_torchs_switch():
    from gflow_amd import _lib
    before = torch.are_deterministic_algorithms_enabled()
    warn_only = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert _lib.resolve_deterministic(None) is True
        assert _lib.resolve_deterministic(False) is False
        torch.use_deterministic_algorithms(False)
        assert _lib.resolve_deterministic(None) is False
        assert _lib.resolve_deterministic(True) is True
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn_only)


def test_operator_path_refuses_an_explicit_deterministic_fit():
    from gflow_amd.fit_video import fit_clip
    with pytest.raises(ValueError, match="fused=True"):
        fit_clip([], "cpu", fused=False, deterministic=True)
