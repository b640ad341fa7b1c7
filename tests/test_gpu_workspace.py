"""Canary behind the fit workspace and the snapshot workspace (``-m gpu``): every consumer of the carved layout runs once on
buffers whose declared part (the size query's answer) is followed by 4096 bytes of 0xA5 that the test owns.  A region that
the carve places past the size query's total lands in that tail; every other test trusts the size query."""
import ctypes

import pytest
import torch

from tests.scenes import random_scene
from tests.test_gpu_fused import _raw_from_scene, _targets

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, N, CAP, K_CAP, TAIL = 48, 32, 40, 64, 2048, 4096     # six tiles, one partial column


def _with_tail(nbytes):
    t = torch.zeros(nbytes + TAIL, dtype=torch.uint8, device=DEV)
    t[nbytes:] = 0xA5
    return t


def test_no_consumer_of_the_layout_writes_behind_the_declared_workspace():
    from gflow_amd import _lib as L
    from gflow_amd.fused import FitEngine
    s = random_scene(N, W, H, seed=7, sigma_px=2.5, tilt=False)
    raw = _raw_from_scene(s)
    img, dep = _targets(H, W, 3)
    eng = FitEngine(W, H, capacity=CAP, device=DEV, K_cap=K_CAP)
    assert eng.cap == CAP and eng.K_cap == K_CAP and eng.d_rec is None     # (no d_rec of its own: d_rec_cam is in use)
    eng.set_splats({k: v.to(DEV) for k, v in raw.items()})
    eng.intr.copy_(s["intr"].to(DEV))
    eng.set_targets(img, dep)
    for k, v in dict(lambda_rgb=1.0, lambda_depth=0.1, lambda_var=10.0, lr=1e-3).items():
        setattr(eng.hp, k, v)
    eng.reset_optimizer()
    ws_bytes = eng.lib.gfl_fit_workspace_bytes(CAP, K_CAP, W, H)
    snap_bytes = eng.lib.gfl_fit_snapshot_workspace_bytes(N, W, H)
    assert ws_bytes > 0 and snap_bytes > 0
    eng.workspace = _with_tail(ws_bytes)
    eng._state = None
    eng._snap_ws = _with_tail(snap_bytes)

    losses = []
    def ran():
        losses.extend(eng.loss_terms())

    eng.iteration(count=2)                        # the exact binning path, then reserved tile regions
    ran()
    assert eng.iteration(snapshot=True).shape == (3, H, W, 3)
    ran()
    assert eng.snapshot().shape == (3, H, W, 3)
    eng.hp.lr_camera = 1e-3                       # the camera moves: pose gradient, camera launch
    eng.iteration()
    ran()
    eng.hp.lr_camera = 0.0
    eng.deterministic = True
    eng.iteration()
    ran()
    eng.deterministic = False
    # the differentiable operator on this engine, as gflow_amd/render.py drives it: activated rows, the caller's camera
    act = torch.cat([s[k].reshape(N, -1) for k in ("xyz", "scale", "rotate", "opacity", "rgb")] + [torch.zeros(N, 2)], dim=1)
    eng.params[:N] = act.to(DEV)
    intr, extr = s["intr"].to(DEV).reshape(4).contiguous(), s["extr"].to(DEV).reshape(12).contiguous()
    out = torch.empty(4, H, W, dtype=torch.float32, device=DEV)
    rec = torch.empty(N, 12, dtype=torch.float32, device=DEV)
    st = eng.state()
    st.N, st.intr, st.extr, st.render, st.rec = N, intr.data_ptr(), extr.data_ptr(), out.data_ptr(), rec.data_ptr()
    L.check(eng.lib.gfl_render_fwd(ctypes.byref(st), ctypes.byref(eng.hp), L.stream()), "render")
    d_render = torch.ones(4, H, W, dtype=torch.float32, device=DEV)
    d_params = torch.empty(N, 16, dtype=torch.float32, device=DEV)
    d_extr = torch.empty(12, dtype=torch.float32, device=DEV)
    d_intr = torch.empty(4, dtype=torch.float32, device=DEV)
    L.check(eng.lib.gfl_render_bwd_cam(ctypes.byref(st), ctypes.byref(eng.hp), L.ptr(d_render), None, None, L.ptr(d_params),
                                       L.ptr(d_extr), L.ptr(d_intr), L.stream()), "render backward")
    torch.cuda.synchronize()

    assert bool((eng.workspace[ws_bytes:] == 0xA5).all()), "the fit workspace's tail was written"
    assert bool((eng._snap_ws[snap_bytes:] == 0xA5).all()), "the snapshot workspace's tail was written"
    assert eng._snap_ws.numel() == snap_bytes + TAIL                  # (snapshot() kept the buffer it was given)
    assert eng.overflow.tolist() == [0, 0, 0, 0]
    assert bool(torch.isfinite(torch.stack(losses)).all()), losses
    assert bool(torch.isfinite(out).all() and torch.isfinite(d_params).all() and torch.isfinite(d_intr).all())
