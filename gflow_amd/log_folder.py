"""A clip fit saved as the reference's log folder ("Saving a fit").

gflow/fit_video.py leaves, per clip: ``ckpt/<name>.tar`` per frame, seven images per frame under ``images/``, the hull mask
under ``images_seg/``, the sequence videos and ``sequence_traj.pkl`` -- what its benchmark.py, its viewer and
``gflow_amd.viewer --folder`` read afterwards.  ``ClipLog`` is the recorder of ``ClipFit`` (``fit_clip(save=DIR)``) that keeps
what those files need ON THE DEVICE while the clip is fitted -- nothing is read back per frame -- and writes them once the
clip is fitted: the checkpoints with torch.save, the images as PNG files coded on the device (gflow_amd.png), the videos as
Motion-JPEG AVI files coded on the device (gflow_amd.video; the reference writes mp4).

One divergence: the reference saves the render of the last iteration with ``iteration % 10 == 0``, up to nine iterations
stale; the images here are of the frame's FINAL state, the state the checkpoint holds."""
import os
import pickle

import numpy as np
import torch

from . import png as PN
from . import video as VD

FPS = 5                                            # fit_video.py's save_video(..., fps=5)
# file prefix under images/ and video name -> (what, index): the scene's (rgb, depth colour, centre), the layers'
# [still, moving] x [rgb, centre]
SCENE_KINDS = (("img", "sequence", 0), ("img_depth", "sequence_depth", 1), ("img_center", "sequence_center", 2))
LAYER_KINDS = (("img_still", "sequence_still", (0, 0)), ("img_still_center", "sequence_still_center", (0, 1)),
               ("img_move", "sequence_move", (1, 0)), ("img_move_center", "sequence_move_center", (1, 1)))


def frame_names(frames):
    return [str(fr.get("name", f"{t:05d}")) for t, fr in enumerate(frames)]


def expected_files(names, valid, traj):
    """the files of a log folder, relative, sorted: ``names`` the frames', ``valid`` which frames have a hull mask"""
    out = [f"ckpt/{n}.tar" for n in names]
    out += [f"images/{p}_{n}.png" for p, _, _ in SCENE_KINDS + LAYER_KINDS for n in names]
    out += [f"images_seg/move_mask_{n}.png" for n, v in zip(names, valid) if v]
    out += [f"{v}.avi" for _, v, _ in SCENE_KINDS + LAYER_KINDS] + ["sequence_move_seg.avi"]
    if traj:
        out += ["sequence_traj.avi", "sequence_traj_upon.avi", "sequence_traj.pkl"]
    return sorted(out)


class ClipLog:
    """Per frame, on the device: clones of what ``SimpleGaussian.save_checkpoint`` stores, the three scene images of the
    frame's final state (ClipFit.final_forward(scene=True), shared with the trajectory recorder), the four layer images
    (SecondEngine.parts_u8: two more forwards, as in the reference, once the splats have still / moving labels; black
    before).  The hull masks come from the trainer's MoveSegRecorder, which ClipFit builds with ``save``."""

    def __init__(self, folder, frames, fused=True):
        if not fused:
            raise ValueError("fit_clip(save=...) needs fused=True: the images are taken from the fused engines")
        if not isinstance(folder, (str, os.PathLike)):
            raise ValueError(f"fit_clip(save=...): a folder path, got {folder!r}")
        self.dir = os.fspath(folder)
        self.names = frame_names(frames)
        if len(set(self.names)) != len(self.names) or any(os.sep in n or n in ("", ".", "..") for n in self.names):
            raise ValueError("fit_clip(save=...): the frames' names must be distinct file names")
        self.ckpts, self.scene, self.layers = [], [], []

    def frame(self, cf, i):
        """Frame i's final state.  The layers first -- their forwards leave nothing on the second engine that the frame's
        other recorders read --, then the frame's shared final forward with its scene images."""
        tr = cf.tr
        with torch.no_grad():
            if not tr.engine_current:
                raise RuntimeError("fit_clip(save=...): the fused engine does not hold the current splats")
            still = tr.still_mask
            self.ckpts.append({
                "attributes": {k: v.detach().clone().contiguous() for k, v in tr._attributes.items()},
                "intr": tr.intr.detach().clone(),
                "extr": tr.get_extr().detach().clone(),
                "still_mask": None if still is None else still.detach().clone(),
                "move_seg": None,                        # (the frame's hull mask, filled in once the masks are built)
                "last_uv": None if tr.last_uv is None else tr.last_uv.detach().clone(),
                "width": tr.W,
                "height": tr.H,
            })
            if still is not None and tr.engine.N == still.shape[0]:
                parts = tr.second.parts_u8(tr.engine, tr.bg, still)
                tr.rasterisations_done += 2
                self.layers.append(parts[:, [0, 2]])     # (rgb and centre of [still, moving]: a copy)
            else:
                self.layers.append(None)
            _, scene = cf.final_forward(scene=True)
            self.scene.append(scene)

    def write(self, masks, valid, traj=None):
        """The folder.  ``masks`` (T, H, W) uint8 and ``valid`` (T,): the hull masks (MoveSegRecorder.masks); ``traj``:
        ClipFit.trajectories()'s dict, or None.  One PNG call and one AVI per kind over the whole stack."""
        d, names = self.dir, self.names
        for sub in ("ckpt", "images", "images_seg"):
            os.makedirs(os.path.join(d, sub), exist_ok=True)
        for t, ck in enumerate(self.ckpts):
            ck["move_seg"] = masks[t].copy() if valid[t] else None
            torch.save(ck, os.path.join(d, "ckpt", f"{names[t]}.tar"))
        scene = torch.stack(self.scene)                                    # (T, 3, H, W, 3)
        blank = torch.zeros((2, 2) + tuple(scene.shape[2:]), dtype=torch.uint8, device=scene.device)
        layers = torch.stack([blank if x is None else x for x in self.layers])      # (T, 2, 2, H, W, 3)
        stacks = [(p, v, scene[:, k]) for p, v, k in SCENE_KINDS] + [(p, v, layers[:, a, b]) for p, v, (a, b) in LAYER_KINDS]
        for prefix, vid, stack in stacks:
            stack = stack.contiguous()
            PN.write_pngs(stack, [os.path.join(d, "images", f"{prefix}_{n}.png") for n in names])
            VD.write_avi(os.path.join(d, vid + ".avi"), stack, fps=FPS)
        masks = np.ascontiguousarray(masks)
        keep = [t for t in range(len(names)) if valid[t]]
        if keep:
            PN.write_pngs(masks[keep], [os.path.join(d, "images_seg", f"move_mask_{names[t]}.png") for t in keep])
        VD.write_avi(os.path.join(d, "sequence_move_seg.avi"), masks, fps=FPS)
        if traj is not None:
            VD.write_avi(os.path.join(d, "sequence_traj.avi"), np.ascontiguousarray(traj["images"][:, 0]), fps=FPS)
            VD.write_avi(os.path.join(d, "sequence_traj_upon.avi"), np.ascontiguousarray(traj["images"][:, 1]), fps=FPS)
            with open(os.path.join(d, "sequence_traj.pkl"), "wb") as f:
                pickle.dump([np.asarray(uv) for uv in traj["uv"]], f)       # (fit_video.py:375: a list of per-frame arrays)
        return d
