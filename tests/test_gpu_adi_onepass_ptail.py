"""P of the next one-pass step, formed y-elimination first and mapped through `xmap` + `pbias` (`fine_p_map`,
`csrc/qp_adi_fine.inc`; the algebra and its rounding bound are in test_adi_onepass_ptail_host.py).

The contract is that of test_gpu_adi_onepass.py: 1e-14 relative to the two-sweep sequence.  The shapes are the smallest
that reach every branch of the tail: 64 x 64 (every tile mixes the first / last y-variants, x-variants first and last only),
128 x 192 and 192 x 128 (interior x-chunks, an interior tile row whose half-waves share one y-variant), 64 x 320.  P is
consumed from step 2 on and ping-pongs between two buffers, hence k in {2, 3, 6}.  Three fields: D = 0, a mid value and
r D = 0.31, the edge of the decoupled regime.  Reflective walls test the map M alone (pbias = 0); sides with sources and
u0 = 0 leave pbias alone in P after the first step; the same sides with a random field test both."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-14
DT, DX = 0.1, 1.0
R = 0.5 * DT / DX ** 2
DCOEF = [0.0, 0.15 / R, 0.31 / R]
SHAPES = [(64, 64), (128, 192), (192, 128), (64, 320)]
CASES = ["reflective_random", "sources_zero_field", "sources_random"]


def _sides():
    from qpsim_amd.models import BoundaryCondition
    return {"left": BoundaryCondition("dirichlet", 0.3), "right": BoundaryCondition("robin", 0.2, 0.4),
            "up": BoundaryCondition("neumann", -0.1), "down": BoundaryCondition("absorbing")}


def _engine(ny, nx, side_bc):
    from qpsim_amd.engine import Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    if side_bc is None:
        bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    else:
        bcs = {e.edge_id: side_bc[e.normal] for e in edges}
    return Engine(compile_geometry(mask, edges, bcs, DX))


def _operator(monkeypatch, eng, mode):
    from qpsim_amd.engine import DiffusionOperator
    monkeypatch.setenv("QPSIM_FINE_TILES", "1")
    monkeypatch.setenv("QPSIM_ADI_FUSED", mode)
    op = DiffusionOperator(eng, len(DCOEF), DT, dcoef=DCOEF)
    monkeypatch.delenv("QPSIM_ADI_FUSED")
    assert op.rect is not None and op.rect.fine
    return op


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _run(eng, op, u0, calls):
    u = eng.upload_packed(u0)
    for k in calls:
        eng.adi_steps(op, u, k)
    return eng.download_packed(u)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_p_from_map_and_bias(monkeypatch, shape, case):
    ny, nx = shape
    rng = np.random.default_rng(ny * 1000 + nx + CASES.index(case))
    eng = _engine(ny, nx, None if case == "reflective_random" else _sides())
    nf = len(DCOEF)
    u0 = np.zeros((nf, ny * nx)) if case == "sources_zero_field" else rng.random((nf, ny * nx))
    onepass, fused, plain = (_operator(monkeypatch, eng, m) for m in ("2", "1", "0"))
    for k in (2, 3, 6):
        got = _run(eng, onepass, u0, [k])
        two_sweep = _run(eng, plain, u0, [k])
        reduce_fused = _run(eng, fused, u0, [k])
        assert np.max(np.abs(two_sweep)) > 0.0
        e0, e1 = _rel(got, two_sweep), _rel(got, reduce_fused)
        print(f"{ny} x {nx} {case} k={k}: rel err {e0:.3e} (two-sweep) {e1:.3e} (reduce + fused)")
        assert e0 <= REL_TOL, (k, e0)
        assert e1 <= REL_TOL, (k, e1)
    # k = 3 then k = 4 on the plan used above equal the same calls on a fresh plan each, bit for bit
    a = _run(eng, onepass, u0, [3, 4])
    u = eng.upload_packed(u0)
    eng.adi_steps(_operator(monkeypatch, eng, "2"), u, 3)
    eng.adi_steps(_operator(monkeypatch, eng, "2"), u, 4)
    b = eng.download_packed(u)
    assert np.array_equal(a, b), _rel(a, b)
