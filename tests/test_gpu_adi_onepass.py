"""One-pass ADI steps on fine tiles (`fine_onepass_kernel` + `fine_ghostsum_kernel`, `csrc/qp_adi_fine.inc`) against the
two-sweep sequence (`QPSIM_ADI_FUSED=0`).  The y-interface rows are formed as P + phi S instead of directly, so the steps
after the first round differently: the results must agree to 1e-14 relative, and a single step (entry, reduce pass, exit
pass) must equal the reduce + fused path (`QPSIM_ADI_FUSED=1`) bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-14


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


def _operators(monkeypatch, eng, nf, dt, Dc):
    """(one-pass, reduce + fused, two-sweep) operators on the same plan parameters, all on fine tiles."""
    from qpsim_amd.engine import DiffusionOperator
    monkeypatch.setenv("QPSIM_FINE_TILES", "1")
    ops = []
    for mode in ("2", "1", "0"):
        monkeypatch.setenv("QPSIM_ADI_FUSED", mode)
        ops.append(DiffusionOperator(eng, nf, dt, dcoef=Dc))
    monkeypatch.delenv("QPSIM_ADI_FUSED")
    assert all(op.rect is not None and op.rect.fine for op in ops)
    return ops


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _check(eng, ops, u0, nsteps, upload, download):
    onepass, fused, plain = ops
    a, b = upload(u0), upload(u0)
    eng.adi_steps(onepass, a, nsteps)
    eng.adi_steps(plain, b, nsteps)
    ha, hb = download(a), download(b)
    err = _rel(ha, hb)
    assert err <= REL_TOL, (nsteps, err)
    if nsteps == 1:
        c = upload(u0)
        eng.adi_steps(fused, c, 1)
        assert np.array_equal(ha, download(c)), _rel(ha, download(c))
    return ha


def _torch_io():
    import torch

    def upload(u0):
        return u0.clone()

    def download(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return upload, download


@pytest.mark.parametrize("nsteps", [1, 2, 20])
def test_onepass_steps_at_headline_size(monkeypatch, nsteps):
    """4096^2, one field, the benchmark's plan (D = 6, dt = 0.1, dx = 1, reflective walls)."""
    import torch
    N = 4096
    eng = _engine(N, N)
    ops = _operators(monkeypatch, eng, 1, 0.1, [6.0])
    g = torch.Generator(device="cpu").manual_seed(29 + nsteps)
    u0 = (1e-4 * (1.0 + torch.rand(1, N * N, generator=g, dtype=torch.float64))).cuda()
    got = _check(eng, ops, u0, nsteps, *_torch_io())
    assert not np.array_equal(got, u0.cpu().numpy())


def test_onepass_steps_many_fields(monkeypatch):
    """1024^2 x 12 fields with distinct diffusivities (the c2 diffusion shape), mixed sides."""
    import torch
    from qpsim_amd.models import BoundaryCondition
    N, nf = 1024, 12
    side_bc = {"left": BoundaryCondition("dirichlet", 0.3), "right": BoundaryCondition("robin", 0.2, 0.4),
               "up": BoundaryCondition("neumann", -0.1), "down": BoundaryCondition("absorbing")}
    eng = _engine(N, N, side_bc, dx=1.0)
    Dc = [0.25 * (k + 1) for k in range(nf)]
    ops = _operators(monkeypatch, eng, nf, 0.1, Dc)
    g = torch.Generator(device="cpu").manual_seed(7)
    u0 = torch.rand(nf, N * N, generator=g, dtype=torch.float64).cuda()
    for nsteps in (1, 3):
        _check(eng, ops, u0, nsteps, *_torch_io())


EXTENTS = [(64, 64), (64, 320), (192, 64), (128, 192), (256, 128), (320, 256)]


@pytest.mark.parametrize("seed", range(len(EXTENTS)))
def test_onepass_steps_fuzz(monkeypatch, seed):
    """The seeded extents, sides, fields (D = 0 included) and diffusivities of test_gpu_adi_fused.py, k in {1, 2, 5}."""
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
    ops = _operators(monkeypatch, eng, nf, dt, Dc)
    u0 = rng.random((nf, ny * nx))
    for nsteps in (1, 2, 5):
        _check(eng, ops, u0, nsteps, eng.upload_packed, eng.download_packed)


def test_default_headline_plan_runs_onepass_steps(monkeypatch):
    """The default 4096^2 plan: per call of k steps one fine_reduce_kernel, k - 1 ghost-sum passes, k one-pass kernels."""
    import torch
    from torch.autograd import DeviceType
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
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]

    def count(s):
        return sum(s in n for n in names)
    assert count("fine_reduce_kernel") == 1, names
    assert count("fine_onepass_kernel") == nsteps, names
    assert count("fine_ghostsum_kernel") == nsteps - 1, names
    assert count("fine_fused_kernel") == 0 and count("fine_x_kernel") == 0, names
