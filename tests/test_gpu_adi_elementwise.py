"""Diffusion kernels bounded cell by cell and plane by plane: |got - exact| / (u max(T, 1e-4 max_plane T)), with `exact` and T
from the long-double evaluation of tests/adi_exact.py on the same fp64 coefficients.

Every other ADI test divides by the largest value of the whole batch, on dense inputs of dynamic range 2: a wrong tail
behind a chunk interface, a boundary term dropped on a plane that is 1e-9 of its neighbour or a ghost superposed with the
wrong weight where the field is small pass it (tests/test_adi_exact_host.py plants three such faults).  Here each batch
holds four planes on distinct D - flat, a pulse on a 1e-8 floor, a ramp over twelve decades, a delta at or off a chunk
interface - with the suite's usual sides at scale 1, or with zero-source sides and the planes at 1, 1e-9, 1e-18, 1e-100.
K_hip <= 4 K_ref64 + 4 per plane, K_ref64 being the same statistic of the fp64 oracle (the reference, never the kernel);
a plane with D = 0 must come back to 4 units of its input per step, and the single cell of the 1 x 1 grid is held to 4
units outright.  The preconditioner solves (`qp_adi_rect_solve`,
`qp_adi_tile_solve`, the per-line sweeps) are held to the same limit with T = Sy^-1 Sx^-1 |x|.  Every case asserts its path."""
from __future__ import annotations

import numpy as np
import pytest

import adi_exact as X
from test_gpu_collision_instantiations import HAVE_X87

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")]


def _operator(monkeypatch, eng, case, p):
    """The operator of the case's path, after asserting that the plan is the one the case is about."""
    from qpsim_amd.engine import DiffusionOperator
    path, mask = case["path"], p["mask"]
    ny, nx = mask.shape
    if case["dset"] == "field":
        kw = dict(dfield=np.stack([np.asarray(d).reshape(-1) for d in p["D"]]))
    else:
        kw = dict(dcoef=list(p["D"]))
    if path == "lines":
        op = DiffusionOperator(eng, 4, p["dt"], allow_fast=False, **kw)
        assert op.rect is None and op.tile is None
    elif path in ("rect64", "banded"):
        monkeypatch.setenv("QPSIM_FINE_TILES", "0")
        op = DiffusionOperator(eng, 4, p["dt"], force_banded=path == "banded", **kw)
        assert op.rect is not None and not op.rect.fine
        if path == "banded":
            assert op.rect.decoupled == (False, False)
        else:      # a short remainder chunk keeps a visible coupling through it: that direction stays banded
            assert op.rect.decoupled == tuple(n <= 64 or n % 64 == 0 or n % 64 >= 48 for n in (nx, ny))
    elif path in X.FINE_MODES:
        monkeypatch.setenv("QPSIM_FINE_TILES", "1")
        monkeypatch.setenv("QPSIM_ADI_FUSED", X.FINE_MODES[path])
        op = DiffusionOperator(eng, 4, p["dt"], **kw)
        assert op.rect is not None and op.rect.fine
    else:
        assert path == "tile"
        op = DiffusionOperator(eng, 4, p["dt"], **kw)
        assert op.rect is None and op.tile is not None, op.tile_refused
        counts = op.tile.tile_counts
        assert sum(counts.values()) == -(-ny // 64) * -(-nx // 64) and op.tile.far_coupling < 1e-22
        if case["dset"] == "field":
            assert counts["clean"] == 0
        elif case["geom"][1] == "donut":
            assert counts["empty"] > 0 and counts["clean"] > 0 and counts["general"] > 0
    return op


def _judge(case, got, refs, mask, which, frozen):
    """K of every plane against limit(K_ref64); `which` = a step count or "solve"."""
    worst, tag = [], case["id"]
    for k, name in enumerate(X.PLANES):
        tr, t, kref = refs[k]["solve"] if which == "solve" else refs[k]["steps"][which]
        grid = np.zeros(mask.shape)
        grid[mask] = got[k]
        kk, bad = X.K(grid, tr, t, mask)
        print(f"K {tag} {which} {name}: {kk:.2f} (K_ref64 {kref:.2f})")
        if frozen[k]:
            assert kref == 0.0
        lim = X.case_limit(case, kref)
        if bad or not kk <= lim:
            d = np.abs(grid.astype(X.LD) - tr) / (X.U * np.maximum(t, X.FLOOR * t.max()))
            worst.append(f"{name}: K = {kk:.3g} > {lim:.3g} (K_ref64 {kref:.3g}) at cell {np.unravel_index(int(np.argmax(d)), d.shape)}, "
                         f"{bad} cells with T = 0 differ")
    assert not worst, f"{tag} {which}: " + "; ".join(worst)


@pytest.mark.parametrize("case", X.CASES, ids=[c["id"] for c in X.CASES])
def test_adi_paths_cell_by_cell(monkeypatch, case):
    from qpsim_amd.engine import Engine, compile_geometry
    p = X.problem(case)
    mask = p["mask"]
    eng = Engine(compile_geometry(mask, p["edges"], p["bcs"], p["dx"]))
    op = _operator(monkeypatch, eng, case, p)
    refs = X.references(case)
    frozen = [X.is_frozen(d) for d in p["D"]]
    u0 = np.ascontiguousarray(p["u0"][:, mask])
    hole = ~mask.reshape(-1)
    for n in case["steps"]:
        a = eng.upload_packed(u0)
        eng.adi_steps(op, a, n)
        got = eng.download_packed(a)
        assert np.all(np.isfinite(got)) and np.all(a.detach().cpu().numpy()[:, hole] == 0.0)
        _judge(case, got, refs, mask, n, frozen)
    x = eng.upload_packed(u0)
    eng._precondition(op, x)
    got = eng.download_packed(x)
    assert np.all(np.isfinite(got)) and np.all(x.detach().cpu().numpy()[:, hole] == 0.0)
    _judge(case, got, refs, mask, "solve", frozen)
