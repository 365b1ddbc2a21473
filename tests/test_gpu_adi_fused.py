"""Fused ADI steps on fine tiles (`fine_reduce_kernel` + `fine_fused_kernel`, `csrc/qp_adi_fine.inc`) against the two-sweep
sequence they replace (`QPSIM_ADI_FUSED=0`): the same floating-point operations in the same order, so the results must be
bitwise identical - any difference is a bug, not a tolerance question."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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
    """(fused, two-sweep) operators on the same plan parameters, both on fine tiles."""
    from qpsim_amd.engine import DiffusionOperator
    monkeypatch.setenv("QPSIM_FINE_TILES", "1")
    monkeypatch.setenv("QPSIM_ADI_FUSED", "1")
    fused = DiffusionOperator(eng, nf, dt, dcoef=Dc)
    monkeypatch.setenv("QPSIM_ADI_FUSED", "0")
    plain = DiffusionOperator(eng, nf, dt, dcoef=Dc)
    monkeypatch.delenv("QPSIM_ADI_FUSED")
    assert fused.rect is not None and fused.rect.fine and plain.rect.fine
    return fused, plain


def _kernel_names(eng, op, u, nsteps):
    """Names of the device kernels one eng.adi_steps call launches (profiler trace, no API needed)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        eng.adi_steps(op, u, nsteps)
        torch.cuda.synchronize()
    return " ".join(e.name for e in prof.events())


def _assert_fused_path(eng, fused, plain, u):
    names = _kernel_names(eng, fused, u.clone(), 2)
    assert "fine_reduce_kernel" in names and "fine_fused_kernel" in names, names[:2000]
    assert "fine_x_kernel" not in names
    names = _kernel_names(eng, plain, u.clone(), 2)
    assert "fine_x_kernel" in names and "fine_fused_kernel" not in names, names[:2000]


@pytest.mark.parametrize("nsteps", [1, 2, 20])
def test_fused_steps_bitwise_at_headline_size(monkeypatch, nsteps):
    """4096^2, one field, the benchmark's plan (D = 6, dt = 0.1, dx = 1, reflective walls)."""
    import torch
    N = 4096
    eng = _engine(N, N)
    fused, plain = _operators(monkeypatch, eng, 1, 0.1, [6.0])
    g = torch.Generator(device="cpu").manual_seed(17 + nsteps)
    u0 = (1e-4 * (1.0 + torch.rand(1, N * N, generator=g, dtype=torch.float64))).cuda()
    if nsteps == 2:
        _assert_fused_path(eng, fused, plain, u0)
    a, b = u0.clone(), u0.clone()
    eng.adi_steps(fused, a, nsteps)
    eng.adi_steps(plain, b, nsteps)
    torch.cuda.synchronize()
    assert not torch.equal(a, u0)
    assert torch.equal(a, b), float((a - b).abs().max())


def test_fused_steps_bitwise_many_fields(monkeypatch):
    """1024^2 x 12 fields with distinct diffusivities (the c2 diffusion shape), mixed sides."""
    import torch
    from qpsim_amd.models import BoundaryCondition
    N, nf = 1024, 12
    side_bc = {"left": BoundaryCondition("dirichlet", 0.3), "right": BoundaryCondition("robin", 0.2, 0.4),
               "up": BoundaryCondition("neumann", -0.1), "down": BoundaryCondition("absorbing")}
    eng = _engine(N, N, side_bc, dx=1.0)
    Dc = [0.25 * (k + 1) for k in range(nf)]          # r D up to 0.15: fine tiles qualify
    fused, plain = _operators(monkeypatch, eng, nf, 0.1, Dc)
    g = torch.Generator(device="cpu").manual_seed(5)
    u0 = torch.rand(nf, N * N, generator=g, dtype=torch.float64).cuda()
    _assert_fused_path(eng, fused, plain, u0)
    for nsteps in (1, 3):
        a, b = u0.clone(), u0.clone()
        eng.adi_steps(fused, a, nsteps)
        eng.adi_steps(plain, b, nsteps)
        torch.cuda.synchronize()
        assert torch.equal(a, b), (nsteps, float((a - b).abs().max()))


EXTENTS = [(64, 64), (64, 320), (192, 64), (128, 192), (256, 128), (320, 256)]


@pytest.mark.parametrize("seed", range(len(EXTENTS)))
def test_fused_steps_bitwise_fuzz(monkeypatch, seed):
    """Seeded extents (multiples of 64: lines of 2 chunks, tiles whose two half-waves hold first / last chunks), 1-4 fields,
    reflective, absorbing and source-carrying sides, k in {1, 2, 5}: fused == two-sweep, bit for bit."""
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
    fused, plain = _operators(monkeypatch, eng, nf, dt, Dc)
    u0 = rng.random((nf, ny * nx))
    for nsteps in (1, 2, 5):
        a, b = eng.upload_packed(u0), eng.upload_packed(u0)
        eng.adi_steps(fused, a, nsteps)
        eng.adi_steps(plain, b, nsteps)
        ha, hb = eng.download_packed(a), eng.download_packed(b)
        assert np.array_equal(ha, hb), (ny, nx, side_bc, Dc, nsteps, float(np.max(np.abs(ha - hb))))
    if seed == 0:
        import torch
        _assert_fused_path(eng, fused, plain, eng.upload_packed(u0))
        torch.cuda.synchronize()
