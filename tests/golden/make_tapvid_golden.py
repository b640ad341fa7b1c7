"""Generate tests/golden/tapvid.npz by IMPORTING the reference's utils/tapvid.py and utils/tracking.py (both import here,
SURVEY.md "What can be imported here"), the way make_golden.py does:

    python tests/golden/make_tapvid_golden.py

Only arrays are written: seeded inputs and what compute_tapvid_metrics, find_closest_point and
extract_first_visible_points return for them.  Nothing at test time runs this."""
import importlib.util
import os

import numpy as np

REF = os.environ.get("GFLOW_REFERENCE_UTILS", "/root/reference/gflow/utils")
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ["occlusion_accuracy"] + [f"pts_within_{t}" for t in (1, 2, 4, 8, 16)] + [f"jaccard_{t}" for t in (1, 2, 4, 8, 16)] \
    + ["average_jaccard", "average_pts_within_thresh"]


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    tapvid, tracking = load("tapvid"), load("tracking")
    rng = np.random.default_rng(20261016)
    out = {}
    cases = []
    for b, n, t in ((2, 40, 12), (1, 7, 5)):
        gt = rng.uniform(0, 255, (b, n, t, 2)).astype(np.float32)
        pred = (gt + rng.normal(0, 6, gt.shape)).astype(np.float32)
        go = rng.random((b, n, t)) < 0.3
        po = rng.random((b, n, t)) < 0.3
        qp = np.concatenate([rng.integers(0, t, (b, n, 1)).astype(np.float64), rng.uniform(0, 255, (b, n, 2))], -1)
        cases.append((qp, go, gt, po, pred))
    # a video with no visible point at all (0 / 0 -> NaN)
    qp, go, gt, po, pred = cases[1]
    cases.append((qp, np.ones_like(go), gt, po, pred))
    c = 0
    for qp, go, gt, po, pred in cases:
        for mode in ("first", "strided"):
            for tw in (False, True):
                with np.errstate(divide="ignore", invalid="ignore"):
                    m = tapvid.compute_tapvid_metrics(qp, go, gt, po, pred, mode, get_trackwise_metrics=tw)
                p = f"m{c}_"
                out[p + "query_points"], out[p + "gt_occluded"], out[p + "gt_tracks"] = qp, go, gt
                out[p + "pred_occluded"], out[p + "pred_tracks"] = po, pred
                out[p + "mode"] = np.array(0 if mode == "first" else 1)
                out[p + "trackwise"] = np.array(int(tw))
                for k in KEYS:
                    out[p + "out_" + k] = np.asarray(m[k], dtype=np.float64)
                c += 1
    out["n_metric_cases"] = np.array(c)
    # find_closest_point: ties (duplicated rows), a NaN row, culled rows at (0, 0)
    uv = rng.uniform(0, 100, (300, 2)).astype(np.float32)
    uv[50] = uv[10]
    uv[200:210] = 0
    coords = np.concatenate([uv[[10, 3, 205]].astype(np.float64) + [[0, 0], [0.25, -0.5], [0, 0]],
                             rng.uniform(-5, 105, (20, 2))])
    out["fc_uv"], out["fc_coords"] = uv, coords
    out["fc_index"] = np.asarray(tracking.find_closest_point(uv, coords), np.int64)
    uv_nan = uv.copy()
    uv_nan[120] = np.nan
    uv_nan[130] = np.nan
    out["fc_uv_nan"] = uv_nan
    out["fc_index_nan"] = np.asarray(tracking.find_closest_point(uv_nan, coords), np.int64)
    # extract_first_visible_points: random occlusions and all-occluded tracks
    pts = rng.uniform(0, 1, (30, 9, 2)).astype(np.float32)
    occ = rng.random((30, 9)) < 0.6
    occ[[4, 17]] = True
    out["fv_points"], out["fv_occluded"] = pts, occ
    out["fv_out"] = np.asarray(tracking.extract_first_visible_points(pts, occ), np.float64)
    np.savez_compressed(os.path.join(HERE, "tapvid.npz"), **out)


if __name__ == "__main__":
    main()
