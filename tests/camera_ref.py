"""The camera score without an SVD: ATE as the minimum, over the seven parameters of a similarity (log scale, rotation
vector, translation), of the RMSE between the transformed estimated positions and the reference positions, found with
scipy.optimize.least_squares from several starts; RPE from THAT alignment, with scipy's own rotation code.  Independent of
gflow_amd/camera.py's closed form -- and defined wherever a minimum exists, collinear reference paths included."""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation


def c2w(extr):
    """camera-to-world poses: inv([extr; 0 0 0 1]), the definition (a float32 extr's rotation is orthonormal only to 1e-7)"""
    e = np.asarray(extr, dtype=np.float64).reshape(-1, 3, 4)
    out = []
    for m in e:
        out.append(np.linalg.inv(np.vstack([m, [0.0, 0.0, 0.0, 1.0]])))
    return np.stack(out)


def minimise(x, y, starts=12, seed=0):
    """(rmse, c, R, t) of the best similarity y ~ c R x + t"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)

    def residuals(q):
        r = Rotation.from_rotvec(q[1:4]).as_matrix()
        return (np.exp(q[0]) * x @ r.T + q[4:7] - y).ravel()

    rng = np.random.default_rng(seed)
    sx, sy = np.sqrt(((x - x.mean(0)) ** 2).sum()), np.sqrt(((y - y.mean(0)) ** 2).sum())
    best = None
    for k in range(starts):
        rv = np.zeros(3) if k == 0 else Rotation.random(random_state=rng).as_rotvec()
        lc = np.log(sy / sx)
        t0 = y.mean(0) - np.exp(lc) * Rotation.from_rotvec(rv).as_matrix() @ x.mean(0)
        sol = least_squares(residuals, np.concatenate([[lc], rv, t0]), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                            x_scale="jac", max_nfev=4000)
        if best is None or sol.cost < best.cost:
            best = sol
    q = best.x
    rmse = float(np.sqrt(2.0 * best.cost / x.shape[0]))
    return rmse, float(np.exp(q[0])), Rotation.from_rotvec(q[1:4]).as_matrix(), q[4:7]


def evaluate(extr_est, extr_gt, starts=12):
    """{ATE, RPE_t, RPE_r} as gflow_amd.camera.evaluate defines them, by direct minimisation"""
    est, ref = c2w(extr_est), c2w(extr_gt)
    ate, c, r, t = minimise(est[:, :3, 3], ref[:, :3, 3], starts=starts)
    al = est.copy()
    al[:, :3, 3] = c * est[:, :3, 3] @ r.T + t
    al[:, :3, :3] = r @ est[:, :3, :3]
    e_t, e_r = [], []
    for i in range(len(est) - 1):
        dq = np.linalg.solve(ref[i], ref[i + 1])
        dp = np.linalg.solve(al[i], al[i + 1])
        e = np.linalg.solve(dq, dp)
        e_t.append(np.linalg.norm(e[:3, 3]))
        e_r.append(np.degrees(Rotation.from_matrix(e[:3, :3]).magnitude()))
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    return {"ATE": ate, "RPE_t": rms(e_t), "RPE_r": rms(e_r)}
