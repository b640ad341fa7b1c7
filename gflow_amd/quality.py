"""The reconstruction score of a clip fit: PSNR and SSIM of every frame ("Reconstruction score").

The contract is the reference's reconstruction evaluation (gflow/benchmark.py:191-230): ``piqa.PSNR()`` and ``piqa.SSIM()``
of every saved ``rendered_*.png`` against the frame's image, averaged over the frames.  LPIPS, the block's third number,
needs network weights and is not computed.

Recorded frame by frame on the device, read once the clip is fitted:

- ``ReconRecorder.frame`` launches gfl_recon_frame (csrc/gfl_recon.hip) on the current stream: it forms the saved byte of
  the render, and leaves the frame's squared-error sum and SSIM-map sum, float64, in one row of a per-clip device array.
  Nothing is allocated or read back;
- ``ReconRecorder.result`` makes ONE copy to the host; PSNR and SSIM follow there.

piqa is not available where this was written: the score follows piqa's public definition (include/gflow_hip.h has it in
full) and is held against a float64 numpy restatement of it (tests/quality_ref.py), not against piqa itself."""
import numpy as np
import torch

from . import _lib as L

WINDOW = 11                       # the SSIM window's taps: no image side may be shorter
PSNR_EPS = 1e-8                   # piqa.psnr's epsilon: identical images score 80 dB

# metrics.csv (benchmark.py:397-403): the reference's keys in the reference's order, without LPIPS
CSV_KEYS = ("PSNR", "SSIM", "Occlusion_Accuracy", "Average_Jaccard", "Average_PTS_within_threshold", "J_zero", "F_zero",
            "J&F_zero", "ATE", "RPE_t", "RPE_r")


def scores_from_sums(sse, ssim_sum, H, W):
    """(PSNR, SSIM) float64 from gfl_recon_frame's two sums: 10 log10(1 / (mse + 1e-8)) and the mean of the SSIM map"""
    sse, ssim_sum = np.asarray(sse, dtype=np.float64), np.asarray(ssim_sum, dtype=np.float64)
    psnr = 10.0 * np.log10(1.0 / (sse / (3.0 * H * W) + PSNR_EPS))
    return psnr, ssim_sum / (3.0 * (H - (WINDOW - 1)) * (W - (WINDOW - 1)))


class ReconRecorder:
    """The per-frame reconstruction sums of one clip."""

    def __init__(self, n_frames, H, W, device):
        self.T, self.H, self.W = int(n_frames), int(H), int(W)
        if self.H < WINDOW or self.W < WINDOW:
            raise ValueError(f"ReconRecorder: SSIM needs an image of at least {WINDOW} x {WINDOW}, got {self.H} x {self.W}")
        self.device = torch.device(device)
        self.sums = torch.zeros((self.T, 2), dtype=torch.float64, device=self.device)
        L.need_device(self.sums)
        self.ws = L.scratch(L.load().gfl_recon_workspace_bytes(self.W, self.H), self.device)

    def frame(self, i, render, gt_image):
        """Frame ``i``'s sums from ``render`` ((>= 3, H, W) float32: planes r, g, b first) and ``gt_image`` ((H, W, 3)
        float32): two launches on the current stream, row ``i`` written."""
        L.need_device(render, gt_image)
        if render.dim() != 3 or render.shape[0] < 3 or tuple(render.shape[1:]) != (self.H, self.W):
            raise ValueError(f"ReconRecorder.frame: render must be (>= 3, {self.H}, {self.W}), got {tuple(render.shape)}")
        if tuple(gt_image.shape) != (self.H, self.W, 3):
            raise ValueError(f"ReconRecorder.frame: gt_image must be ({self.H}, {self.W}, 3), got {tuple(gt_image.shape)}")
        render, gt_image = render.detach().float().contiguous(), gt_image.detach().float().contiguous()
        L.check(L.load().gfl_recon_frame(L.ptr(render), L.ptr(gt_image), self.W, self.H, int(i), self.T, L.ptr(self.sums),
                                         L.ptr(self.ws), self.ws.numel(), L.stream()), "recon frame")

    def result(self):
        """dict(sse, ssim_sum, PSNR, SSIM), float64 arrays of shape (T,): one copy to the host"""
        s = self.sums.cpu().numpy()
        sse, ssim_sum = s[:, 0].copy(), s[:, 1].copy()
        psnr, ssim = scores_from_sums(sse, ssim_sum, self.H, self.W)
        return dict(sse=sse, ssim_sum=ssim_sum, PSNR=psnr, SSIM=ssim)


def evaluate(rec):
    """The clip's score as benchmark.py:224-228 forms it: np.mean over the images of ``rec`` (ReconRecorder.result(), or
    fit_clip's ``out["recon"]``)."""
    n = len(rec["PSNR"])
    mean = lambda a: float(np.mean(np.asarray(a, dtype=np.float64))) if n else float("nan")
    return {"PSNR": mean(rec["PSNR"]), "SSIM": mean(rec["SSIM"]), "frames": n}


def write_metrics_csv(path, metrics):
    """``key,value`` lines as benchmark.py:401-403 writes them: the keys of ``metrics`` that are CSV_KEYS, in that order
    (a block that was not asked for has no lines); None is written as ``None``, as the reference's f-string does."""
    unknown = [k for k in metrics if k not in CSV_KEYS]
    if unknown:
        raise ValueError(f"write_metrics_csv: unknown keys {unknown}")
    with open(path, "w") as f:
        for k in CSV_KEYS:
            if k in metrics:
                f.write(f"{k},{metrics[k]}\n")
