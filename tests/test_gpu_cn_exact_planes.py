"""`Engine.cn_exact_step` held to its tolerance plane by plane, on planes that differ by many decades.

The iteration stops on max |res| against max |R|; `test_exact_cn_iteration_*` compares per plane, but with every plane
O(1).  Energy planes of a real run differ by many decades (thermal weights): a stopping rule that takes both maxima over the
whole batch never looks at a plane far below the largest one.  Here: four planes on D = 0.5, 2, 6, 12 (the small planes on the
large D, which converge slowest), zero-source sides, rtol = 1e-13, six consecutive calls on one operator so that the adaptive
cycle length and the blind iteration counts evolve.  After every call each plane is compared with `O.CNStepper` of that
plane alone, from the state the call started from: rel_err < 1e-11 per plane, the tolerance `test_exact_cn_iteration_*`
uses.  A per-plane residual rule reaches it with room: ||A^-1||_inf <= 1, so the error is at most rtol (1 + 8 r D) <= 7e-13
of the plane."""
from __future__ import annotations

import numpy as np
import pytest

import adi_exact as X
from golden_utils import rel_err

pytestmark = pytest.mark.gpu

DCOEF = [0.5, 2.0, 6.0, 12.0]
SCALES = {"rough_small": (1.0, 1e-6, 1e-12, 1e-18), "smooth": (1.0, 1e-3, 1e-6, 1e-9)}
CALLS = 6
TOL = 1e-11
GEOMETRIES = ["rect64x64", "rect70x130", "donut", "holes", "donut_plain", "strip1x100"]


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


def _geometry(name):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    if name.startswith("donut"):      # the centre part of the ring of tests/test_gpu_parity.py (keeps SuperLU quick)
        from test_gpu_parity import _masked_problem
        mask = _masked_problem("donut", 23)[1][96:352, 128:384]
        edges = extract_edge_segments(mask)
        return mask, edges, {e.edge_id: BoundaryCondition("absorbing" if i % 3 == 0 else "reflective")
                             for i, e in enumerate(edges)}
    if name == "holes":
        return X._geometry(("masked", "holes"), "homogeneous")
    ny, nx = {"rect64x64": (64, 64), "rect70x130": (70, 130), "strip1x100": (1, 100)}[name]
    return X._geometry(("rect", ny, nx), "homogeneous")


def _inputs(mask, kind, seed):
    """[4, n] packed planes: smooth = a broad Gaussian on an offset, each plane with its own centre and width."""
    rng = np.random.default_rng(seed)
    ny, nx = mask.shape
    y, x = np.indices(mask.shape)
    out = []
    for k, s in enumerate(SCALES[kind]):
        cy, cx, w = (0.3 + 0.1 * k) * ny, (0.6 - 0.1 * k) * nx, (0.2 + 0.05 * k) * max(ny, nx)
        smooth = 0.5 + np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * w * w))
        plane = smooth if (kind == "smooth" or k == 0) else rng.random(mask.shape)
        out.append(s * plane[mask])
    return np.stack(out)


@pytest.mark.parametrize("kind", sorted(SCALES))
@pytest.mark.parametrize("name", GEOMETRIES)
def test_exact_cn_step_reaches_its_tolerance_on_every_plane(O, name, kind):
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    mask, edges, bcs = _geometry(name)
    eng = Engine(compile_geometry(mask, edges, bcs, X.DX))
    op = DiffusionOperator(eng, 4, X.DT, dcoef=DCOEF)
    assert eng.cn_contraction_bound(op) > eng.CHEBYSHEV_FROM
    if name.startswith("rect") or name.startswith("strip"):
        assert op.rect is not None
    else:
        assert op.rect is None and op.tile is not None, op.tile_refused
    if name == "donut_plain":
        op._cn_plain = True
    ops = O.build_grid_ops(mask, edges, bcs, X.DX)
    steppers = [O.CNStepper(ops, d, X.DT) for d in DCOEF]
    u = _inputs(mask, kind, 7)
    v = eng.upload_packed(u)
    worst = np.zeros(4)
    for call in range(CALLS):
        its = eng.cn_exact_step(op, v, rtol=1e-13)
        got = eng.download_packed(v)
        errs = np.array([rel_err(got[k], steppers[k].step(u[k])) for k in range(4)])
        print(f"{name} {kind} call {call}: {its} iterations, per-plane error " + " ".join(f"{e:.1e}" for e in errs))
        worst = np.maximum(worst, errs)
        u = got
    # the path the case is about
    cycle = op._pr_cycles.get(getattr(op, "_pr_J", None)) if op.rect is not None else None
    if name == "rect64x64":
        assert cycle and any(plan.fine for plan in cycle)             # Peaceman-Rachford cycle, fine tiles where they qualify
    elif name == "rect70x130":
        assert cycle and not any(plan.fine for plan in cycle)         # the same cycle on 64-cell tiles
    elif name == "strip1x100":
        assert op.rect is not None
    elif name == "donut_plain":
        assert op._cn_plain and getattr(op, "_cn_cheb_its", None) is None
    else:
        assert not getattr(op, "_cn_plain", False) and hasattr(op, "_cn_cheb_its")       # Chebyshev semi-iteration
    assert np.all(worst < TOL), f"{name} {kind}: worst per-plane error over {CALLS} calls " + " ".join(f"{e:.1e}" for e in worst)


@pytest.mark.parametrize("geom", [("rect", 64, 64), ("rect", 70, 130), ("rect", 1, 100), ("rect", 300, 5), ("hole", 70, 65),
                                  ("masked", "holes")])
def test_per_plane_norms_are_the_maxima_of_each_plane(geom):
    """`qp_adi_rect_combine_norms` / `qp_stencil_combine_norms` against NumPy on the plane the same pass stored, planes 13
    decades apart and one of zeros; the scalar entries still give the maximum over all planes; more planes than a field
    has rows (blocks per field = 1)."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    mask, edges, bcs = X._geometry(geom, "mixed")
    eng = Engine(compile_geometry(mask, edges, bcs, X.DX))
    rng = np.random.default_rng(5)
    for nf in (1, 5, 7):
        scales = np.array([1.0, 1e-13, 0.0, 3.0, 1e-200, 1e3, 1e-7])[:nf]
        op = DiffusionOperator(eng, nf, X.DT, dcoef=list(np.linspace(0.5, 6.0, nf)))
        assert (op.rect is not None) == (geom[0] == "rect")
        u = eng.upload_packed(scales[:, None] * rng.random((nf, int(mask.sum()))))
        rin = eng.upload_packed(scales[:, None] * rng.random((nf, int(mask.sum()))))
        out, norms, one = eng.empty(nf, eng.ncell), eng.empty(nf), eng.empty(1)
        eng.stencil(op, u, out, -1.0, 1.0, 1.0, 0.0, rin=rin, cr=1.0, norms_out=norms)
        want = np.abs(out.cpu().numpy()).max(axis=1)
        assert np.array_equal(norms.cpu().numpy(), want) and np.count_nonzero(want) == np.count_nonzero(scales)
        eng.stencil(op, u, out, -1.0, 1.0, 1.0, 0.0, rin=rin, cr=1.0, norm_out=one)
        assert float(one.cpu()[0]) == want.max()
        if op.rect is not None:                  # norms only, no plane stored
            norms.zero_()
            eng.stencil(op, u, None, -1.0, 1.0, 1.0, 0.0, rin=rin, cr=1.0, norms_out=norms)
            assert np.array_equal(norms.cpu().numpy(), want)


@pytest.mark.parametrize("fast,nf", [(True, 1100), (True, 2049), (False, 1100), (False, 9000)])
def test_more_planes_than_partial_slots(O, fast, nf):
    """An ensemble hands one operator NE x members planes: more than the 1024 partial slots of the reduction workspace (and,
    on the general path, more than the 8192 blocks of the plain combine).  The per-plane norms then come from launches of
    at most 1024 planes each, the single norm and the plain combine from one launch whose blocks stride over the planes:
    8 x 8 cells, rectangle plan and general kernel; both mappings store the same plane, the norms are its maxima, and
    `cn_exact_step` solves every plane."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    mask, edges, bcs = X._geometry(("rect", 8, 8), "mixed")
    eng = Engine(compile_geometry(mask, edges, bcs, X.DX))
    dc = [DCOEF[k % 4] for k in range(nf)]
    op = DiffusionOperator(eng, nf, X.DT, dcoef=dc, allow_fast=fast)
    assert (op.rect is not None) == fast and op.tile is None
    rng = np.random.default_rng(nf)
    scales = 10.0 ** -(np.arange(nf) % 19)
    u0 = scales[:, None] * rng.random((nf, 64))
    u, rin = eng.upload_packed(u0), eng.upload_packed(scales[:, None] * rng.random((nf, 64)))
    grouped, strided, norms, one = eng.empty(nf, 64), eng.empty(nf, 64), eng.empty(nf), eng.empty(1)
    eng.stencil(op, u, grouped, -1.0, 1.0, 1.0, 0.5, rin=rin, cr=1.0, norms_out=norms)
    eng.stencil(op, u, strided, -1.0, 1.0, 1.0, 0.5, rin=rin, cr=1.0, norm_out=one)
    want = np.abs(grouped.cpu().numpy()).max(axis=1)
    assert np.array_equal(grouped.cpu().numpy(), strided.cpu().numpy()) and np.all(want > 0.0)
    assert np.array_equal(norms.cpu().numpy(), want) and float(one.cpu()[0]) == want.max()
    strided.zero_()
    eng.stencil(op, u, strided, -1.0, 1.0, 1.0, 0.5, rin=rin, cr=1.0)                 # no norm at all
    assert np.array_equal(grouped.cpu().numpy(), strided.cpu().numpy())
    if nf > 2100:
        return
    eng.cn_exact_step(op, u, rtol=1e-13)
    got = eng.download_packed(u)
    ops = O.build_grid_ops(mask, edges, bcs, X.DX)
    steppers = [O.CNStepper(ops, d, X.DT) for d in DCOEF]
    errs = np.array([rel_err(got[k], steppers[k % 4].step(u0[k])) for k in range(nf)])
    print(f"{nf} planes, {'rectangle' if fast else 'general'} path: worst per-plane error {errs.max():.1e}")
    assert errs.max() < TOL
