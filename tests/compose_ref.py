"""float64 numpy restatement of gfl_compose_rows (include/gflow_hip.h): the float32 inputs are upcast, every operation is done
in float64, one job at a time and one row after the other -- no chunks, no ranks.  Column layout of a row: xyz 0:3 | scale 3:6 |
quaternion wxyz 6:10 | opacity 10 | rgb 11:14 | pad 14:16; of an edit: gain 0 | size 1 | q wxyz 2:6 | pivot 6:9 | shift 9:12 |
tint 12:15 | mix 15."""
import numpy as np

IDENTITY = np.array([1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)


def edit_row(gain=1.0, size=1.0, q=(1.0, 0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0), tint=(0.0, 0.0, 0.0), mix=0.0):
    return np.array([gain, size, *q, *pivot, *shift, *tint, mix], dtype=np.float32)


def quat_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def quat_mul(q, r):
    qw, qx, qy, qz = q
    rw, rx, ry, rz = r
    return np.array([qw * rw - qx * rx - qy * ry - qz * rz, qw * rx + qx * rw + qy * rz - qz * ry,
                     qw * ry - qx * rz + qy * rw + qz * rx, qw * rz + qx * ry - qy * rx + qz * rw], dtype=np.float64)


def job_flag(src, R, rows_max):
    first_a, count_a, first_b, count_b = (int(x) for x in src)
    inside = lambda first, cnt: first >= 0 and cnt >= 0 and first <= R and cnt <= R - first
    return 0 if inside(first_a, count_a) and inside(first_b, count_b) and max(count_a, count_b) <= rows_max else 2


def is_still_transform(e):
    """the edit leaves xyz, scale and rotate alone: size == 1, q == (+-1, 0, 0, 0), shift == 0, exactly"""
    return bool(e[1] == 1 and abs(e[2]) == 1 and not e[3:6].any() and not e[9:12].any())


def compose_job(params, labels, src, s, edits, rows_max):
    """One job.  params (R,16) float32; labels (R,) uint8 or None; src = (first_a, count_a, first_b, count_b); s a float32
    value; edits (G,16) float32 or None.  Returns dict(flag, kept (k,) source indices, rows (k,16) float64, blended (k,16)
    float64 -- the rows before their edit --, group (k,), big (k,16) -- max(|a|, |b|) of the source rows, per column)."""
    R = params.shape[0]
    flag = job_flag(src, R, rows_max)
    empty = dict(flag=flag, kept=np.zeros(0, dtype=np.int64), rows=np.zeros((0, 16)), blended=np.zeros((0, 16)),
                 group=np.zeros(0, dtype=np.int64), big=np.zeros((0, 16)))
    if flag:
        return empty
    first_a, count_a, first_b, count_b = (int(x) for x in src)
    n, both = max(count_a, count_b), min(count_a, count_b)
    if n == 0:
        return empty
    s = float(np.float32(s))
    A = params[first_a:first_a + count_a].astype(np.float64)
    B = params[first_b:first_b + count_b].astype(np.float64)
    # ---- rows in both ranges
    a, b = A[:both], B[:both]
    if s == 0.0:
        v = a.copy()
    elif s == 1.0:
        v = b.copy()
    else:
        v = a + s * (b - a)
        flip = np.where((a[:, 6:10] * b[:, 6:10]).sum(1, keepdims=True) < 0, -1.0, 1.0)
        q = a[:, 6:10] + s * (flip * b[:, 6:10] - a[:, 6:10])
        v[:, 6:10] = q / np.sqrt((q * q).sum(1, keepdims=True))
        v[:, 14:16] = a[:, 14:16]
    big = np.maximum(np.abs(a), np.abs(b))
    # ---- the tail: rows only in b fade in, rows only in a fade out
    tail = (B[both:] if count_b > count_a else A[both:]).copy()
    big = np.concatenate([big, np.abs(tail)])
    tail[:, 10] = tail[:, 10] * (s if count_b > count_a else 1.0 - s)
    v = np.concatenate([v, tail])
    if labels is None:
        group = np.zeros(n, dtype=np.int64)
    else:
        la = np.asarray(labels[first_a:first_a + count_a]).astype(np.int64)
        lb = np.asarray(labels[first_b:first_b + count_b]).astype(np.int64)
        group = np.concatenate([la, lb[count_a:]])
    before = v.copy()
    # ---- the group's edit
    for g in (range(edits.shape[0]) if edits is not None else ()):
        m = group == g
        if not m.any():
            continue
        e = edits[g]
        e64 = e.astype(np.float64)
        v[m, 10] = np.minimum(v[m, 10] * e64[0], 1.0)
        v[m, 11:14] = v[m, 11:14] + e64[15] * (e64[12:15] - v[m, 11:14])
        if not is_still_transform(e):
            size, q, pivot, shift = e64[1], e64[2:6], e64[6:9], e64[9:12]
            v[m, 0:3] = pivot + size * ((v[m, 0:3] - pivot) @ quat_matrix(q).T) + shift
            v[m, 3:6] = size * v[m, 3:6]
            r = quat_mul(q, v[m, 6:10].T).T
            v[m, 6:10] = r / np.sqrt((r * r).sum(1, keepdims=True))
    keep = ~(v[:, 10] <= 0)
    return dict(flag=0, kept=np.nonzero(keep)[0].astype(np.int64), rows=v[keep], blended=before[keep], group=group[keep],
                big=big[keep])


def compose(params, labels, job_src, job_s, job_edit, rows_max):
    """every job of a call: a list of compose_job's dicts (job_edit (J,G,16) or None)"""
    return [compose_job(params, labels, job_src[j], job_s[j], None if job_edit is None else job_edit[j], rows_max)
            for j in range(len(job_src))]
