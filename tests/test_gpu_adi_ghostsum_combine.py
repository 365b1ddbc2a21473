"""Tile sums T in the one-pass kernel and the combine form of `fine_ghostsum_kernel` (`csrc/qp_adi_fine.inc`).

The x-ghosts are linear in the x-interface values, gl = (ic0 yf(tx) + yl(tx - 1)) ic2 and likewise gr, so their
y-eliminations S follow from the y-eliminations T of yf / yl that every tile of the one-pass kernel leaves.  The GPU tests
hold the one-pass steps to the contract of test_gpu_adi_onepass.py (1e-14 relative to the two-sweep sequence) at the
benchmark's call length, on many fields, on grids where every chunk is a first or last chunk, and across calls on one plan;
the CPU test checks the algebra of the combine against the row-wise sum."""
import numpy as np
import pytest

REL_TOL = 1e-14
FS = 32


def _engine(ny, nx, side_bc=None, dx=1.0):
    from qpsim_amd.engine import Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    if side_bc is None:
        bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    else:
        bcs = {e.edge_id: side_bc[e.normal] for e in edges}
    return Engine(compile_geometry(mask, edges, bcs, dx))


def _operator(monkeypatch, eng, nf, dt, Dc, mode):
    from qpsim_amd.engine import DiffusionOperator
    monkeypatch.setenv("QPSIM_FINE_TILES", "1")
    monkeypatch.setenv("QPSIM_ADI_FUSED", mode)
    op = DiffusionOperator(eng, nf, dt, dcoef=Dc)
    monkeypatch.delenv("QPSIM_ADI_FUSED")
    assert op.rect is not None and op.rect.fine
    return op


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _torch_run(eng, op, u0, nsteps):
    import torch
    u = u0.clone()
    eng.adi_steps(op, u, nsteps)
    torch.cuda.synchronize()
    return u.cpu().numpy()


@pytest.mark.gpu
def test_onepass_at_benchmark_call_length(monkeypatch):
    """4096^2, one field, the benchmark's plan and its 50 steps per call."""
    import torch
    N, k = 4096, 50
    eng = _engine(N, N)
    onepass = _operator(monkeypatch, eng, 1, 0.1, [6.0], "2")
    plain = _operator(monkeypatch, eng, 1, 0.1, [6.0], "0")
    g = torch.Generator(device="cpu").manual_seed(50)
    u0 = (1e-4 * (1.0 + torch.rand(1, N * N, generator=g, dtype=torch.float64))).cuda()
    err = _rel(_torch_run(eng, onepass, u0, k), _torch_run(eng, plain, u0, k))
    print(f"4096^2 k={k}: rel err {err:.3e}")
    assert err <= REL_TOL, err


def _mixed_sides():
    from qpsim_amd.models import BoundaryCondition
    return {"left": BoundaryCondition("dirichlet", 0.3), "right": BoundaryCondition("robin", 0.2, 0.4),
            "up": BoundaryCondition("neumann", -0.1), "down": BoundaryCondition("absorbing")}


@pytest.mark.gpu
def test_onepass_many_fields_ten_steps(monkeypatch):
    """1024^2 x 12 fields with distinct diffusivities and mixed sides, k = 10."""
    import torch
    N, nf, k = 1024, 12, 10
    eng = _engine(N, N, _mixed_sides(), dx=1.0)
    Dc = [0.25 * (i + 1) for i in range(nf)]
    onepass = _operator(monkeypatch, eng, nf, 0.1, Dc, "2")
    plain = _operator(monkeypatch, eng, nf, 0.1, Dc, "0")
    g = torch.Generator(device="cpu").manual_seed(11)
    u0 = torch.rand(nf, N * N, generator=g, dtype=torch.float64).cuda()
    err = _rel(_torch_run(eng, onepass, u0, k), _torch_run(eng, plain, u0, k))
    print(f"1024^2 x {nf} k={k}: rel err {err:.3e}")
    assert err <= REL_TOL, err


# the extents of test_gpu_adi_onepass.py; (64, 64) has px = py = 2, (64, 320) py = 2, (192, 64) px = 2: every chunk of
# that direction is a first or last chunk, so the combine runs its end cases only
EXTENTS = [(64, 64), (64, 320), (192, 64), (128, 192), (256, 128), (320, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(len(EXTENTS)))
def test_onepass_fuzz_small_extents(monkeypatch, seed):
    """The seeded sides, fields (D = 0 included) and diffusivities of test_gpu_adi_onepass.py, k in {2, 3, 7}."""
    from qpsim_amd.models import BoundaryCondition
    rng = np.random.default_rng(4000 + seed)
    ny, nx = EXTENTS[seed]

    def bc():
        kind = ["dirichlet", "neumann", "robin", "absorbing", "reflective"][int(rng.integers(0, 5))]
        if kind == "robin":
            return BoundaryCondition("robin", float(rng.uniform(-0.5, 0.5)), float(rng.uniform(0.05, 1.0)))
        if kind in ("dirichlet", "neumann"):
            return BoundaryCondition(kind, float(rng.uniform(-0.5, 0.9)))
        return BoundaryCondition(kind)

    side_bc = {side: bc() for side in ("left", "right", "up", "down")}
    dx, dt = float(rng.uniform(0.7, 1.3)), float(rng.uniform(0.05, 0.15))
    r = 0.5 * dt / dx ** 2
    nf = int(rng.integers(1, 5))
    Dc = [float(v) for v in rng.uniform(0.0, 0.31 / r, nf)]
    if seed % 3 == 0:
        Dc[0] = 0.0
    eng = _engine(ny, nx, side_bc, dx)
    onepass = _operator(monkeypatch, eng, nf, dt, Dc, "2")
    plain = _operator(monkeypatch, eng, nf, dt, Dc, "0")
    u0 = rng.random((nf, ny * nx))
    for k in (2, 3, 7):
        a, b = eng.upload_packed(u0), eng.upload_packed(u0)
        eng.adi_steps(onepass, a, k)
        eng.adi_steps(plain, b, k)
        err = _rel(eng.download_packed(a), eng.download_packed(b))
        print(f"{ny} x {nx} x {nf} k={k}: rel err {err:.3e}")
        assert err <= REL_TOL, (k, err)


@pytest.mark.gpu
def test_consecutive_calls_leave_nothing_behind(monkeypatch):
    """k = 3 then k = 4 on one plan equal the same two calls on a fresh plan each, bit for bit: no stale T or S."""
    import torch
    N, nf = 1024, 4
    eng = _engine(N, N, _mixed_sides(), dx=1.0)
    Dc = [0.4 * (i + 1) for i in range(nf)]
    g = torch.Generator(device="cpu").manual_seed(3)
    u0 = torch.rand(nf, N * N, generator=g, dtype=torch.float64).cuda()
    used = _operator(monkeypatch, eng, nf, 0.1, Dc, "2")
    eng.adi_steps(used, 7.0 * u0 + 1.0, 5)      # T and S of another run are in the plan's buffers
    a = u0.clone()
    eng.adi_steps(used, a, 3)
    eng.adi_steps(used, a, 4)
    b = u0.clone()
    eng.adi_steps(_operator(monkeypatch, eng, nf, 0.1, Dc, "2"), b, 3)
    eng.adi_steps(_operator(monkeypatch, eng, nf, 0.1, Dc, "2"), b, 4)
    torch.cuda.synchronize()
    assert torch.equal(a, b), _rel(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.gpu
def test_ghostsum_grid_at_headline_size(monkeypatch):
    """The combine runs one thread per (field, x-chunk, y-chunk): 128 * 128 / 256 = 64 blocks of 256 threads at 4096^2."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    from qpsim_amd.engine import DiffusionOperator
    monkeypatch.delenv("QPSIM_ADI_FUSED", raising=False)
    monkeypatch.delenv("QPSIM_FINE_TILES", raising=False)
    N, nsteps = 4096, 3
    eng = _engine(N, N)
    op = DiffusionOperator(eng, 1, 0.1, dcoef=[6.0])
    u = torch.full((1, N * N), 1e-4, dtype=torch.float64, device="cuda")
    eng.adi_steps(op, u, nsteps)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        eng.adi_steps(op, u, nsteps)
        torch.cuda.synchronize()
    import json
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "trace.json")
        prof.export_chrome_trace(path)
        with open(path) as fh:
            events = json.load(fh)["traceEvents"]
    launches = [e for e in events if e.get("cat") == "kernel" and "fine_ghostsum_kernel" in e.get("name", "")]
    assert len(launches) == nsteps - 1, [e.get("name") for e in events if e.get("cat") == "kernel"]
    for e in launches:
        assert list(e["args"]["grid"]) == [64, 1, 1], e["args"]
        assert list(e["args"]["block"]) == [256, 1, 1], e["args"]


def _combine(T, ic, px):
    """S of every (tx, q) from T[tx, q] = (ends_f yf, ends_l yf, ends_f yl, ends_l yl), as fine_ghostsum_kernel does."""
    S = np.zeros_like(T)
    for tx in range(px):
        if tx > 0:
            S[tx, :, 0] = (ic[tx, 0] * T[tx, :, 0] + T[tx - 1, :, 2]) * ic[tx, 2]
            S[tx, :, 1] = (ic[tx, 0] * T[tx, :, 1] + T[tx - 1, :, 3]) * ic[tx, 2]
        if tx < px - 1:
            S[tx, :, 2] = (ic[tx + 1, 1] * T[tx, :, 2] + T[tx + 1, :, 0]) * ic[tx + 1, 2]
            S[tx, :, 3] = (ic[tx + 1, 1] * T[tx, :, 3] + T[tx + 1, :, 1]) * ic[tx + 1, 2]
    return S


@pytest.mark.parametrize("px,py", [(2, 2), (3, 2), (2, 5), (7, 4)])
def test_combine_of_tile_sums_equals_rowwise_sum(px, py):
    """S from T against the direct sum over rows, S_direct = sum_k w_k g_k with g_k = (ic0 yf_k + yl'_k) ic2.

    Bound.  With u = 2^-53 and the products and sums of either form evaluated in any order:
      * g_k carries two roundings (the fma, the product): |fl(g_k) - g_k| <= 2 u |g|_max, where |g|_max here is the bound
        G = (|ic0| max|yf| + max|yl'|) |ic2| that holds for every intermediate of both forms;
      * a 32-term dot product sum_k w_k x_k carries at most 32 roundings per term (one product, at most 31 additions
        whatever the tree): error <= 32 u sum|w| max|x|.
    Direct form: 32 u W G for the sum plus 2 u W G for the g_k, W = sum_k |w_k|: 34 u W G.
    Combine form: the two dot products err by 32 u W max|yf| and 32 u W max|yl'|, scaled by |ic0 ic2| and |ic2| they add up
    to at most 32 u W G; the fma and the product of the combine add 2 u W G: 34 u W G.
    The two forms therefore differ by at most 68 u W G (first order in u; the factor 1.01 covers the higher orders)."""
    rng = np.random.default_rng(100 * px + py)
    ny = py * FS
    yf = rng.standard_normal((px, ny))
    yl = rng.standard_normal((px, ny))
    ic = rng.uniform(-1.5, 1.5, (px + 1, 3))
    w = rng.standard_normal((py, 2, FS)) * np.exp(-0.3 * np.arange(FS))      # decaying end rows, as A^-1 has them
    T = np.zeros((px, py, 4))
    direct = np.zeros((px, py, 4))
    bound = np.zeros((px, py, 4))
    u = 2.0 ** -53
    for tx in range(px):
        for q in range(py):
            rows = slice(q * FS, (q + 1) * FS)
            wf, wl = w[q, 0], w[q, 1]
            T[tx, q] = [wf @ yf[tx, rows], wl @ yf[tx, rows], wf @ yl[tx, rows], wl @ yl[tx, rows]]
            W = (np.abs(wf).sum(), np.abs(wl).sum())
            if tx > 0:
                gl = (ic[tx, 0] * yf[tx, rows] + yl[tx - 1, rows]) * ic[tx, 2]
                G = (abs(ic[tx, 0]) * np.abs(yf[tx, rows]).max() + np.abs(yl[tx - 1, rows]).max()) * abs(ic[tx, 2])
                direct[tx, q, 0], direct[tx, q, 1] = wf @ gl, wl @ gl
                bound[tx, q, 0], bound[tx, q, 1] = W[0] * G, W[1] * G
            if tx < px - 1:
                gr = (ic[tx + 1, 1] * yl[tx, rows] + yf[tx + 1, rows]) * ic[tx + 1, 2]
                G = (abs(ic[tx + 1, 1]) * np.abs(yl[tx, rows]).max() + np.abs(yf[tx + 1, rows]).max()) * abs(ic[tx + 1, 2])
                direct[tx, q, 2], direct[tx, q, 3] = wf @ gr, wl @ gr
                bound[tx, q, 2], bound[tx, q, 3] = W[0] * G, W[1] * G
    S = _combine(T, ic, px)
    assert np.all(S[0, :, :2] == 0.0) and np.all(S[px - 1, :, 2:] == 0.0)      # no ghost beyond the walls
    assert np.all(np.abs(S - direct) <= 1.01 * 68 * u * bound), float(np.max(np.abs(S - direct) / np.maximum(bound, 1e-300)) / u)
    assert np.any(S != 0.0)
