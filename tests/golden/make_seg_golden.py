"""Generate tests/golden/davis_seg.npz by IMPORTING the reference's utils/measures/jaccard.py and f_boundary.py by path,
the way make_tapvid_golden.py does:

    python tests/golden/make_seg_golden.py

f_boundary.py imports ``binary_dilation`` and ``disk`` from ``skimage.morphology``, and skimage is not installed where
this was run.  This script registers a two-function STAND-IN for that module in ``sys.modules`` before the call:
``disk(r)`` is the footprint X^2 + Y^2 <= r^2 over -r .. r, and ``binary_dilation(image, footprint)`` is
``scipy.ndimage.binary_dilation(image, structure=footprint)`` (zero border).  That is what skimage itself computes (its
binary_dilation is a thin wrapper of scipy's), but it is a stand-in: the golden F values are the reference's code on
scipy's dilation.

Only arrays are written: seeded mask pairs, ``bound_th`` and the reference's J (db_eval_iou(gt, pred)) and F
(db_eval_boundary(pred, gt, bound_th)), the argument order of benchmark.py:268-271.  Nothing at test time runs this."""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("GFLOW_REFERENCE_UTILS", "/root/reference/gflow/utils")
HERE = os.path.dirname(os.path.abspath(__file__))


def install_skimage_stand_in():
    from scipy import ndimage

    def disk(radius):
        r = int(np.floor(radius))
        y, x = np.mgrid[-r:r + 1, -r:r + 1]
        return (x * x + y * y <= radius * radius).astype(np.uint8)

    def binary_dilation(image, footprint=None):
        return ndimage.binary_dilation(image, structure=footprint)

    sk = types.ModuleType("skimage")
    mo = types.ModuleType("skimage.morphology")
    mo.disk, mo.binary_dilation = disk, binary_dilation
    sk.morphology = mo
    sys.modules["skimage"], sys.modules["skimage.morphology"] = sk, mo


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "measures", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def two_discs(rng, H, W, flip=0.01):
    """two overlapping discs, the first touching a border, with ``flip`` of the pixels inverted"""
    y, x = np.mgrid[0:H, 0:W]
    r0 = max(1.0, 0.3 * min(H, W) + 1.0)
    cx, cy = rng.uniform(0, W), (0.0 if rng.random() < 0.5 else H - 1.0)
    m = (x - cx) ** 2 + (y - cy) ** 2 <= max(r0, 0.15 * max(H, W)) ** 2
    cx2, cy2 = cx + rng.uniform(-r0, r0), cy + rng.uniform(-r0, r0) * 0.5 + (r0 if cy == 0 else -r0) * 0.5
    m |= (x - cx2) ** 2 + (y - cy2) ** 2 <= (0.8 * max(r0, 0.1 * max(H, W))) ** 2
    return m ^ (rng.random((H, W)) < flip)


def blob(H, W, cy, cx, r):
    y, x = np.mgrid[0:H, 0:W]
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def main():
    install_skimage_stand_in()
    jaccard, f_boundary = load("jaccard"), load("f_boundary")
    rng = np.random.default_rng(20261017)
    cases = []                                                   # (name, pred, gt, bound_th)
    for H, W, ths in ((37, 53, (0.008, 3)), (70, 130, (8,)), (64, 65, (5,)), (65, 64, (5,)), (1, 200, (0.008,)),
                      (2, 2, (0.008,))):
        for th in ths:
            pred = two_discs(rng, H, W)
            # the other side: the same two discs seen a little later (shifted), flipped pixels of its own
            gt = np.roll(two_discs(rng, H, W), 1, axis=1) | np.roll(pred, 2 if W > 4 else 0, axis=1) & (rng.random((H, W)) < 0.9)
            cases.append((f"{H}x{W}_th{th}", pred, gt, th))
    H, W = 40, 72
    empty, ones = np.zeros((H, W), bool), np.ones((H, W), bool)
    a, b = blob(H, W, 12, 14, 7), blob(H, W, 28, 58, 6)
    cases += [("empty_empty", empty, empty, 0.008), ("empty_blob", empty, a, 0.008), ("blob_empty", a, empty, 0.008),
              ("disjoint_blobs", a, b, 3), ("ones_blob", ones, a, 3)]
    out = {"n_cases": np.array(len(cases)), "names": np.array([c[0] for c in cases])}
    for i, (name, pred, gt, th) in enumerate(cases):
        j = jaccard.db_eval_iou(gt.copy(), pred.copy())
        f = f_boundary.db_eval_boundary(pred.copy(), gt.copy(), th)
        out[f"c{i}_pred"], out[f"c{i}_gt"] = pred, gt
        out[f"c{i}_bound_th"] = np.array(th, dtype=np.float64)
        out[f"c{i}_J"], out[f"c{i}_F"] = np.array(j, dtype=np.float64), np.array(f, dtype=np.float64)
        print(f"{name:>18}: J {float(j):.6f}  F {float(f):.6f}")
    np.savez_compressed(os.path.join(HERE, "davis_seg.npz"), **out)


if __name__ == "__main__":
    main()
