"""Device self-tests of wave-level primitives (``-m gpu``)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_wave_reduce_scatter10_sums_every_component():
    from gflow_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 10, generator=g)
    # make every (lane, component) entry identifiable: integer weights catch any lane/slot mix-up
    x = x + torch.arange(10).float() * 100.0
    xd = x.cuda().contiguous()
    a = torch.full((10,), float("nan"), device="cuda")
    b = torch.full((10,), float("nan"), device="cuda")
    L.check(lib.gfl_selftest_reduce10(L.ptr(xd), L.ptr(a), L.ptr(b), L.stream()), "selftest")
    ref = x.double().sum(0)
    assert torch.allclose(a.cpu().double(), ref, rtol=1e-5, atol=1e-3), (a.cpu(), ref)
    assert torch.allclose(b.cpu().double(), ref, rtol=1e-5, atol=1e-3), (b.cpu(), ref)


def test_ewa_contraction_on_the_matrix_cores_equals_the_valu_form():
    """Sigma2 = M Sigma M^T with v_mfma_f32_4x4x1_16b_f32 (sixteen splats per instruction, quad broadcasts to lay
    them out) against the 30-FMA form and against float64, over magnitudes the preprocess kernel sees."""
    from gflow_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(0)
    n = 1000                                                  # not a multiple of 64: partial waves pass zeros
    m = (torch.randn(n, 6, generator=g) * 300.0).contiguous()
    r = torch.randn(n, 3, 3, generator=g) * torch.logspace(-3, 0, n).reshape(n, 1, 1)
    S = r @ r.transpose(1, 2)                                 # symmetric positive semi-definite
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).contiguous()
    a = torch.full((n, 3), float("nan"), device="cuda")
    b = torch.full((n, 3), float("nan"), device="cuda")
    md, cd = m.cuda(), cov.cuda()
    L.check(lib.gfl_selftest_cov2d(L.ptr(md), L.ptr(cd), n, L.ptr(a), L.ptr(b), L.stream()), "selftest")
    torch.cuda.synchronize()
    M = m.reshape(n, 2, 3).double()
    ref = M @ S.double() @ M.transpose(1, 2)
    ref = torch.stack([ref[:, 0, 0], ref[:, 0, 1], ref[:, 1, 1]], dim=1)
    scale = ref.abs().max(dim=1, keepdim=True).values
    assert ((a.cpu().double() - ref).abs() / scale).max() < 1e-5
    assert ((b.cpu().double() - ref).abs() / scale).max() < 1e-5
    assert ((a - b).abs().cpu().double() / scale).max() < 1e-6


def test_oracle_parity_holds_with_the_matrix_core_contraction():
    """GFL_EWA_MFMA=1 puts cov2d_mfma into fused_preprocess_fwd (the variant north_star names; the library reads the
    switch once per process, hence a process of its own): the fused forward, all fused gradients and the full-size
    (480x854, 60 000 splats) fused iteration are held against the ORACLE again with the switch on.  conftest.py checks
    inside that process that the library really took the switch (GFL_EXPECT_EWA_MFMA)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GFL_EWA_MFMA="1", GFL_EXPECT_EWA_MFMA="1")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_fused.py::test_fused_forward_matches_oracle_and_operator_path",
           "tests/test_gpu_fused.py::test_fused_gradients_match_oracle",
           "tests/test_gpu_render_op.py::test_render_operator_values_and_gradients_match_oracle",
           "tests/test_gpu_fullsize.py::test_fullsize_fused_iteration_matches_oracle[bench_scene]"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], tail


@pytest.mark.parametrize("block", [256, 512, 1024])
def test_block_scan_twice_on_the_same_scratch(block):
    """block_scan_excl, the one workgroup scan of the library: two scans back to back on the same LDS scratch, with no
    barrier between them but the scan's own, for every workgroup size in use.  Values 1 + (i * 7919) % 13: a lane or wave
    mix-up cannot cancel.  Exact against numpy.cumsum."""
    import numpy as np
    from gflow_amd import _lib as L
    lib = L.load()
    x = (1 + (np.arange(2 * block, dtype=np.int64) * 7919) % 13).astype(np.int32)
    xd = torch.from_numpy(x).to(DEV)
    excl = torch.full((2 * block,), -7, dtype=torch.int32, device=DEV)
    total = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    L.check(lib.gfl_selftest_block_scan(L.ptr(xd), block, L.ptr(excl), L.ptr(total), L.stream()), "selftest")
    torch.cuda.synchronize()
    halves = x.reshape(2, block)
    ref = np.cumsum(halves, axis=1) - halves                       # exclusive
    assert np.array_equal(excl.cpu().numpy().reshape(2, block), ref)
    assert np.array_equal(total.cpu().numpy(), halves.sum(axis=1))


@pytest.mark.parametrize("box", [8, 4])
def test_block_culling_never_drops_a_visible_pixel(box):
    """The blend kernels skip a (splat, pixel box) unit when `block_mask` says the splat cannot reach the box with
    alpha >= 1/255 (an ellipse-vs-box test with a safety margin).  Against brute force over the boxes' pixels with the
    kernels' own alpha arithmetic: the mask must CONTAIN every box that holds a visible pixel, for round, elongated,
    rotated, huge, tiny, barely visible and far-away splats; and it should not be much larger (the bounding-disc test
    of round 1 let 16 % empty units through on the bench scene)."""
    from gflow_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(box)
    n = 200_000
    # covariance = R diag(s1^2, s2^2) R^T + 0.3 I (the EWA blur), conic = its inverse
    s1 = torch.exp(torch.empty(n).uniform_(-2.5, 4.5, generator=g))        # 0.08 .. 90 px
    ratio = torch.exp(torch.empty(n).uniform_(0.0, 4.0, generator=g))      # up to 55 : 1
    s2 = s1 / ratio
    th = torch.empty(n).uniform_(0, 3.14159, generator=g)
    c, s = torch.cos(th), torch.sin(th)
    a = c * c * s1 ** 2 + s * s * s2 ** 2 + 0.3
    b = c * s * (s1 ** 2 - s2 ** 2)
    d = s * s * s1 ** 2 + c * c * s2 ** 2 + 0.3
    det = a * d - b * b
    A, B, C = d / det, -b / det, a / det
    o = torch.empty(n).uniform_(0.0, 1.0, generator=g)
    o[: n // 10] = torch.empty(n // 10).uniform_(0.8 / 255, 3.0 / 255, generator=g)   # around the visibility threshold
    x0, y0 = 160, 96
    u = x0 + torch.empty(n).uniform_(-40, 56, generator=g)
    v = y0 + torch.empty(n).uniform_(-40, 56, generator=g)
    far = slice(n // 2, n // 2 + n // 10)                                   # centres hundreds of pixels away, long axis anywhere
    u[far] = x0 + torch.empty(n // 10).uniform_(-600, 600, generator=g)
    v[far] = y0 + torch.empty(n // 10).uniform_(-600, 600, generator=g)
    lam = 0.5 * (a + d) + torch.sqrt(torch.clamp(0.25 * (a - d) ** 2 + b * b, min=0))
    r = 255.0 * o
    cutoff = torch.where(o < 1 / 255, torch.full_like(o, -1.0),
                         torch.where(r < 1.05, torch.full_like(o, 3e38), 2.0 * torch.log(r) * lam * 1.002 + 0.01))
    rec = torch.zeros(n, 12)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 10] = u, v, A, B, C, o, cutoff
    rec_d = rec.to(DEV)
    mask = torch.zeros(n, dtype=torch.int32, device=DEV)
    truth = torch.zeros(n, dtype=torch.int32, device=DEV)
    L.check(lib.gfl_selftest_block_mask(L.ptr(rec_d), n, x0, y0, box, L.ptr(mask), L.ptr(truth), L.stream()), "selftest")
    torch.cuda.synchronize()
    mask, truth = mask.cpu(), truth.cpu()
    missed = truth & ~mask
    assert int((missed != 0).sum()) == 0, f"{int((missed != 0).sum())} splats lose a visible box; first: {rec[missed != 0][:3]}"
    bits = lambda t: sum(((t >> k) & 1).sum().item() for k in range(4))
    let_through, needed = bits(mask), bits(truth)
    assert needed > 50_000                                                   # the sample does exercise visible boxes
    print(f"box {box}: {let_through} boxes let through for {needed} with a visible pixel ({let_through / needed:.3f}x)")
    assert let_through <= 1.06 * needed, (let_through, needed)               # measured 1.02x (continuous box, margins)



def test_tile_sort_in_any_order_of_the_tiles():
    """gfl_tile_sort_ordered (the fused iteration's sort: every XCD's longest lists first) against
    gfl_tile_sort_only (the tiles in their own order) on the same keys: ids and tile ranges bit-identical, for a random
    permutation of the tiles inside every XCD's run and with lists of every register tier (1 ... 2 500 keys)."""
    import numpy as np
    from gflow_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda", 0)
    W, H = 160, 96
    gx, gy = 10, 6
    T = gx * gy
    g = torch.Generator().manual_seed(11)
    n = 4000
    # every splat covers a 3 x 3 block of tiles around its own (radius 16: [u - 16, u + 16 + 15] / 16)
    cx = torch.randint(1, gx - 1, (n,), generator=g)
    cy = torch.randint(1, gy - 1, (n,), generator=g)
    rec = torch.zeros(n, 12)
    rec[:, 0] = cx * 16 + 8.0
    rec[:, 1] = cy * 16 + 8.0
    rec[:, 11] = torch.full((n,), 16, dtype=torch.int32).view(torch.float32)
    depth = (1 + torch.rand(n, generator=g)).float()
    depth[::9] = depth[0]                                   # ties: the id decides
    lists = [[] for _ in range(T)]
    for i in range(n):
        for ty in range(int(cy[i]) - 1, int(cy[i]) + 2):
            for tx in range(int(cx[i]) - 1, int(cx[i]) + 2):
                lists[ty * gx + tx].append(i)
    # ... and one tile far longer than the rest (the splats of its whole neighbourhood a second time would break the
    # uniqueness of (splat, tile): thin the others out instead)
    for t in range(T):
        if t != 3 * gx + 4:
            lists[t] = lists[t][: max(1, len(lists[t]) // (1 + t % 5))]
    lens = np.array([len(l) for l in lists])
    assert lens.max() > 1024 and lens.min() >= 1
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    K = int(offsets[-1])
    dbits = depth.view(torch.int32).numpy().astype(np.uint64)
    keys = np.zeros(K, dtype=np.uint64)
    rng = np.random.default_rng(3)
    for t in range(T):
        idx = np.array(lists[t], dtype=np.uint64)
        rng.shuffle(idx)
        keys[offsets[t]:offsets[t + 1]] = (dbits[idx.astype(np.int64)] << np.uint64(32)) | idx
    # order: a random permutation of the tiles inside every XCD's run (the runs of xcd_logical_block)
    q, r = T >> 3, T & 7
    order = np.zeros((T, 4), dtype=np.int32)
    for x in range(8):
        s0 = x * q + min(x, r)
        ln = q + (1 if x < r else 0)
        perm = s0 + rng.permutation(ln)
        for j, t in enumerate(perm):
            order[s0 + j] = (t, offsets[t], offsets[t + 1], 0)

    TRAILER = 68                                             # GFL_SORT_ORDER_TRAILER ints behind order[T][4]
    heavy_pos = [p_ for p_ in range(T) if order[p_, 2] - order[p_, 1] > 200]
    assert any(order[p_, 2] - order[p_, 1] > 1024 for p_ in heavy_pos) and len(heavy_pos) >= 3

    def run(ordered, split=False):
        k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
        ids = torch.full((K,), -7, dtype=torch.int32, device=dev)
        tr = torch.full((T, 2), -7, dtype=torch.int32, device=dev)
        if ordered:
            o_np = np.concatenate([order.reshape(-1), np.zeros(TRAILER, dtype=np.int32)])
            if split:
                # the lists of more than 200 keys (up to > 1024: every register tier of the halves) cut in two
                o_np[4 * T] = len(heavy_pos)
                for j, p_ in enumerate(heavy_pos):
                    o_np[4 * p_ + 3] = 1 + j
                    o_np[4 * T + 1 + j] = p_
            o = torch.from_numpy(o_np).to(dev)
            L.check(lib.gfl_tile_sort_ordered(L.ptr(o), W, H, K, L.ptr(k), L.ptr(ids), L.ptr(tr), L.stream()), "sort ordered")
        else:
            off = torch.from_numpy(offsets).to(dev)
            L.check(lib.gfl_tile_sort_only(L.ptr(off), T, K, L.ptr(k), L.ptr(ids), L.ptr(tr), L.stream()), "sort")
        torch.cuda.synchronize()
        return ids.cpu(), tr.cpu()

    ids0, tr0 = run(False)
    ids1, tr1 = run(True)
    assert torch.equal(tr0, tr1) and torch.equal(ids0, ids1)
    ids2, tr2 = run(True, split=True)                    # ... and with the long lists cut at a pivot, two workgroups each
    assert torch.equal(tr0, tr2) and torch.equal(ids0, ids2)
    # and the plain one is right: every list ascending in (depth, id)
    for t in (0, 3 * gx + 4, T - 1):
        seg = ids0[offsets[t]:offsets[t + 1]].long()
        d = depth[seg]
        assert bool(((d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (seg[1:] > seg[:-1]))).all())
        assert sorted(seg.tolist()) == sorted(lists[t])
