"""A float64 numpy restatement of the reconstruction score (include/gflow_hip.h, gfl_recon_frame), from the saved bytes:
what piqa.PSNR() and piqa.SSIM() compute on the PNG the reference saves (gflow/benchmark.py:191-230), written from the
public definition and independently of the kernel -- whole-image separable filtering, no tiles."""
import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2
TAPS, SIGMA = 11, 1.5


def window():
    i = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    g = np.exp(-i ** 2 / (2 * SIGMA ** 2))
    return g / g.sum()


def _filter(a):
    """(H, W, C) -> (H - 10, W - 10, C): the window along both image axes, valid positions only"""
    g = window()
    v = np.lib.stride_tricks.sliding_window_view
    a = np.moveaxis(v(a, TAPS, axis=1), -1, 0)          # (11, H, W - 10, C)
    a = np.tensordot(g, a, axes=1)
    a = np.moveaxis(v(a, TAPS, axis=0), -1, 0)
    return np.tensordot(g, a, axes=1)


def read_back(pred_u8):
    """the saved bytes as the evaluation reads them: uint8 / 255 in float32, then float64"""
    return (np.asarray(pred_u8, dtype=np.uint8).astype(np.float32) / np.float32(255.0)).astype(np.float64)


def ssim_map(x, y):
    """the SSIM map of two (H, W, C) float64 images, (H - 10, W - 10, C)"""
    mx, my = _filter(x), _filter(y)
    sxx, syy, sxy = _filter(x * x) - mx * mx, _filter(y * y) - my * my, _filter(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def sums(pred_u8, gt):
    """(sse, ssim_sum) of the (H, W, 3) uint8 prediction against the (H, W, 3) float target"""
    x = read_back(pred_u8)
    y = np.clip(np.asarray(gt, dtype=np.float32), np.float32(0), np.float32(1)).astype(np.float64)
    assert x.shape == y.shape and x.ndim == 3 and min(x.shape[:2]) >= TAPS
    return float(((x - y) ** 2).sum()), float(ssim_map(x, y).sum())


def psnr(sse, H, W):
    return 10.0 * np.log10(1.0 / (np.asarray(sse, dtype=np.float64) / (3.0 * H * W) + 1e-8))


def ssim(ssim_sum, H, W):
    return np.asarray(ssim_sum, dtype=np.float64) / (3.0 * (H - 10) * (W - 10))


def bytes_of(render_chw):
    """the saved bytes of a (>= 3, H, W) float32 torch render, (H, W, 3) uint8, by torch's own clamp, x 255 and conversion
    (render2img)"""
    import torch
    img = torch.clamp(render_chw[:3].detach().float().permute(1, 2, 0), 0.0, 1.0) * 255.0
    return np.ascontiguousarray(img.to(torch.uint8).cpu().numpy())
