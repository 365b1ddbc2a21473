"""Boundary outflow traces on the GPU: ``qp_boundary_flux`` through ``Engine.boundary_flux`` against the helper's exact sums,
runs with a flux sink against runs that store the same steps, the number balance of the exact Crank-Nicolson step, and
ensembles against lone runs.

The error bound of a sum is derived, not measured: the kernel forms every term with the helper's three roundings, so the
terms are the same doubles, and whatever the order, a floating-point sum of n doubles lies within (n - 1) 2^-53 sum |x| of
the exact sum (first order).  The exact sum is ``math.fsum``.
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import pytest

import boundary_flux_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _bc(*args):
    from qpsim_amd.models import BoundaryCondition
    return BoundaryCondition(*args)


def _same(a, b) -> bool:
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and (
            a.tobytes() == b.tobytes() if a.dtype.kind == "f" else np.array_equal(a, b))
    return a == b


# ------------------------------------------------------------------------------------------------ the kernel alone
_CHECKERS: dict = {}


def _checker(shape):
    """A checkerboard: every interior cell has four boundary faces, each an edge of its own (3200 faces on 40 x 40).  The
    kinds cycle through all five; the Dirichlet value lies above the state (signed terms); the last 40 edges are
    reflective (a surface made of them is left without faces)."""
    if shape not in _CHECKERS:
        from qpsim_amd.engine import compile_geometry
        from qpsim_amd.geometry import extract_edge_segments
        rows, cols = np.indices(shape)
        mask = (rows + cols) % 2 == 0
        edges = extract_edge_segments(mask)
        kinds = [_bc("absorbing"), _bc("dirichlet", 1.5), _bc("robin", 0.3, 0.2), _bc("neumann", -0.05), _bc("robin", 0.7, 0.0),
                 _bc("neumann", 0.04)]
        bcs = {e.edge_id: kinds[k % len(kinds)] for k, e in enumerate(edges)}
        for e in edges[-40:]:
            bcs[e.edge_id] = _bc("reflective")
        _CHECKERS[shape] = (mask, edges, bcs, compile_geometry(mask, edges, bcs, 0.5))
    return _CHECKERS[shape]


def _surfaces(kind: str, edges) -> list:
    ids = [e.edge_id for e in edges]
    live = ids[:-40]
    if kind == "edge":          # 1, 1023, 1024, 1025 and 2049 faces around the chunk edge, overlapping, and an empty one
        return [live[:1], live[1:1024], ids[-40:], live[:1024], live[5:1030], live[100:2149]]
    if kind == "one":
        return [ids]
    n = int(kind)
    return [live[37 * k:37 * k + 1 + (11 * k) % 45] + (ids[-3:] if k % 9 == 0 else []) for k in range(n)]


KERNEL_CASES = [((40, 40), "edge", 13, 1, "dcoef"), ((40, 40), "edge", 1, 1, "dfield"), ((39, 41), "edge", 13, 3, "dfield"),
                ((39, 41), "64", 1, 3, "dcoef"), ((40, 40), "63", 13, 1, "dcoef"), ((40, 40), "one", 1, 1, "dcoef")]


@pytest.mark.parametrize("shape,kind,nplane,members,form", KERNEL_CASES,
                         ids=[f"{c[0][0]}x{c[0][1]}-{c[1]}-p{c[2]}-m{c[3]}-{c[4]}" for c in KERNEL_CASES])
def test_boundary_flux_against_exact_sums(shape, kind, nplane, members, form):
    import torch
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_boundary_faces
    mask, edges, bcs, geom = _checker(shape)
    ncell = mask.size
    assert ncell % 2 == (1 if members > 1 else 0)               # members: every second plane starts on an odd element
    surfaces = _surfaces(kind, edges)
    want_faces = R.walk_faces(mask, edges, bcs, 0.5, surfaces)
    counts = [len(f) for f in want_faces]
    if kind == "edge":
        assert counts == [1, 1023, 0, 1024, 1025, 2049] and sum(counts) > 3000
    elif kind == "one":
        assert counts == [len(edges) - 40] and counts[0] > 3000
    else:
        assert len(counts) == int(kind)
    eng = Engine(geom)
    faces = compile_boundary_faces(mask, edges, bcs, 0.5, surfaces)
    assert faces.counts == counts
    dev_faces = eng.upload_boundary_faces(faces)
    rng = np.random.default_rng(ncell + 7 * nplane + members)
    nfield = nplane * members
    state = 0.2 + rng.random((nplane, members, ncell))
    dcoef = 0.5 + rng.random(nfield) if form == "dcoef" else None
    dfield = 0.5 + rng.random((nfield, ncell)) if form == "dfield" else None
    op = DiffusionOperator(eng, nfield, 0.1, dcoef=dcoef, dfield=dfield, allow_fast=False)
    d_state = torch.as_tensor(state, device=eng.device)

    def launch(op, planes, m):
        out = torch.full((m, len(surfaces), nplane), float("nan"), dtype=torch.float64, device=eng.device)
        eng.boundary_flux(dev_faces, op, planes, m, out)
        return out.cpu().numpy()

    got = launch(op, d_state, members)
    assert not np.isnan(got).any(), "every entry of the row is written"
    assert launch(op, d_state, members).tobytes() == got.tobytes(), "a sample is reproducible bit for bit"
    worst, negative = 0.0, 0
    for m in range(members):
        for i in range(nplane):
            f = i * members + m
            D = dcoef[f] if form == "dcoef" else dfield[f]
            for s, flist in enumerate(want_faces):
                if not flist:
                    assert got[m, s, i] == 0.0 and not np.signbit(got[m, s, i])
                    continue
                exact, magnitude = R.outflow(flist, state[i, m], D)
                bound = R.bound(len(flist), magnitude)
                err = abs(got[m, s, i] - exact)
                negative += int((R.terms(flist, state[i, m], D) < 0).any())
                if len(flist) == 1:
                    assert got[m, s, i] == exact            # one face: the term itself, the same three roundings
                else:
                    worst = max(worst, err / bound)
                assert err <= bound, (m, s, i, got[m, s, i], exact, bound)
    print(f"{shape} {kind} planes {nplane} members {members} {form}: worst error / bound = {worst:.3g}")
    assert negative > 0, "the Dirichlet value above the state gives signed terms"
    # only cells on listed, non-reflective faces are read: NaN everywhere else changes nothing
    used = np.zeros(ncell, dtype=bool)
    used[faces.face_cell] = True
    assert (~used).any()
    poisoned = state.copy()
    poisoned[:, :, ~used] = np.nan
    assert launch(op, torch.as_tensor(poisoned, device=eng.device), members).tobytes() == got.tobytes()
    if form == "dfield":
        bad = dfield.copy()
        bad[:, ~used] = np.nan
        op_bad = DiffusionOperator(eng, nfield, 0.1, dfield=bad, allow_fast=False)
        assert launch(op_bad, d_state, members).tobytes() == got.tobytes()
    # a member of a batch gives the bits of a lone call on its planes, odd cell counts included
    if members > 1:
        for m in range(members):
            pick = [i * members + m for i in range(nplane)]
            lone_op = DiffusionOperator(eng, nplane, 0.1, dcoef=None if dcoef is None else dcoef[pick],
                                        dfield=None if dfield is None else dfield[pick], allow_fast=False)
            lone = launch(lone_op, torch.as_tensor(np.ascontiguousarray(state[:, m:m + 1]), device=eng.device), 1)
            assert lone[0].tobytes() == got[m].tobytes(), f"member {m}"


def test_boundary_flux_refuses_what_it_does_not_serve():
    import torch
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_boundary_faces
    mask, edges, bcs, geom = _checker((40, 40))
    eng, other = Engine(geom), Engine(geom)
    faces = eng.upload_boundary_faces(compile_boundary_faces(mask, edges, bcs, 0.5, [[e.edge_id for e in edges]]))
    op = DiffusionOperator(eng, 2, 0.1, dcoef=[1.0, 2.0], allow_fast=False)
    state = torch.zeros(2, mask.size, dtype=torch.float64, device=eng.device)
    out = torch.zeros(1, 1, 2, dtype=torch.float64, device=eng.device)
    eng.boundary_flux(faces, op, state, 1, out)
    with pytest.raises(ValueError, match="domain-decomposed"):
        other.boundary_flux(faces, op, state, 1, out)
    for bad_state, bad_out in ((state[:1], out), (state, out[:, :, :1]), (state, torch.zeros(1, 2, 2, dtype=torch.float64,
                                                                                               device=eng.device))):
        with pytest.raises(ValueError, match="out_row"):
            eng.boundary_flux(faces, op, bad_state, 1, bad_out)


# ------------------------------------------------------------------------------------------------ whole runs
BALANCE_KINDS = [("absorbing", None, None), ("dirichlet", 1e-6, None), ("robin", 0.3, 1e-7), ("neumann", -1e-8, None)]


def _balance_run_arguments():
    from qpsim_amd.geometry import extract_edge_segments
    mask = R.balance_case()["mask"]
    edges = extract_edge_segments(mask)
    assert mask.shape == (24, 20) and len(edges) == 4
    bcs = {e.edge_id: _bc(*kind) for e, kind in zip(edges, BALANCE_KINDS)}
    init = 1e-4 * (1.0 + np.random.default_rng(3).random(mask.shape))
    return dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=0.5, dt=0.1,
                total_time=0.75, dx=0.5, energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=4,
                diffusion_scheme="cn_exact", cn_rtol=1e-13)


def _check_outflow(flux, mask, faces, planes_per_sample, D_of_plane):
    """``flux["outflow"]`` against the helper on the frames a run stored at the same steps; returns the error bounds."""
    bounds = np.zeros(flux["outflow"].shape)
    worst = 0.0
    for k, frames in enumerate(planes_per_sample):
        for i, frame in enumerate(frames):
            plane = R.frame_plane(mask, frame)
            for s, flist in enumerate(faces):
                exact, magnitude = R.outflow(flist, plane, D_of_plane(i)) if flist else (0.0, 0.0)
                bounds[k, s, i] = R.bound(len(flist), magnitude)
                err = abs(flux["outflow"][k, s, i] - exact)
                assert err <= bounds[k, s, i], (k, s, i, flux["outflow"][k, s, i], exact, bounds[k, s, i])
                if bounds[k, s, i] > 0:
                    worst = max(worst, err / bounds[k, s, i])
    print(f"outflow against the helper: worst error / bound = {worst:.3g}")
    return bounds


def test_lone_run_outflow_and_the_number_balance_of_exact_cn():
    """NE = 4 on the 24 x 20 rectangle, absorbing / dirichlet / robin / neumann sides, no collisions, ``cn_exact``, 7 steps
    of 0.1 and one of 0.05, ``flux_every = 1``.

    Balance.  The outflow is affine in u, so the unsplit CN step A u' = R, A = I - r L, R = (I + r L) u + 2 r S, closes
    mass_k - mass_{k+1} = dt_k (F_k + F_{k+1}) / 2 exactly, with mass = dx^2 sum u of a plane and F its total outflow.
    The tolerance has three parts, none taken from the balance the run shows:
      rounding   4 x ``R.CN_CLOSURE_UNITS`` x 2^-53 x the mass scale: four times what the oracle's CN step leaves on this
                 rectangle (tests/test_boundary_flux_host.py measures 2.06 units), the device's sums running in another order;
      sums       dt_k / 2 x the (faces - 1) 2^-53 sum |term| bounds of the kernel at both ends, and 3 x 2^-53 sum_s |F_s| for
                 adding the four surfaces;
      stopping   ``Engine.cn_exact_step`` accepts an iterate u' when ``_cn_plane_error`` = max |R - A u'| / max |R| of the
                 plane is <= ``cn_rtol``.  With delta = A^-1 (R - A u') the error of u': A is an M-matrix with row sums
                 >= 1 (all boundary diag >= 0), so max |delta| <= max |R - A u'| <= cn_rtol max |R|.  delta moves the mass
                 by at most dx^2 n max |delta| and dt F / 2 by at most (dt D_i / 2) sum_f diag_f max |delta| = a_i dx^2
                 sum_f diag_f max |delta|, a_i = dt D_i / (2 dx^2).  Here a_i (4 + e) <= 0.1 x 8 < 1 (e <= 4: the largest
                 sum of boundary diag of one cell), so I + r L has no negative entry and row sums <= 1, hence
                 max |u_{k+1}| <= max |u_k| + 2 a_i s and max |R| <= max |u_0| + 2 (k + 1) a_i s with s the largest sum of
                 |src| of one cell (two sides meet in a corner); max |u_0| is read from the initial state (the frames at
                 t = 0), which no step has touched.  The mass scale is n dx^2 times that bound."""
    from qpsim_amd import tables
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw = _balance_run_arguments()
    mask, edges, bcs, dx, dt = kw["mask"], kw["edges"], kw["edge_conditions"], kw["dx"], kw["dt"]
    surfaces = {e.edge_id: [e.edge_id] for e in edges}
    flux: dict = {"stale": True}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        stored = run_2d_crank_nicolson(**kw, store_every=1)
        sampled = run_2d_crank_nicolson(**kw, store_every=1, flux_out=flux, flux_surfaces=surfaces, flux_every=1)
        sparse_flux: dict = {}
        sparse = run_2d_crank_nicolson(**kw, store_every=100, flux_out=sparse_flux, flux_surfaces=surfaces, flux_every=1)
    assert _same(list(sampled), list(stored)), "the frames are those of the run without a sink"
    assert sorted(flux) == ["energy_bins", "faces", "number_outflow", "outflow", "surfaces", "times"]
    assert flux["times"] == list(stored[0]) and len(flux["times"]) == 9 and flux["surfaces"] == list(surfaces)
    assert flux["faces"] == [len(e.faces) for e in edges] and np.array_equal(flux["energy_bins"], stored[5])
    assert _same(sparse_flux, flux) and list(sparse[0]) == [stored[0][0], stored[0][-1]]
    E_bins = stored[5]
    dE = float(E_bins[1] - E_bins[0])
    D = [float(v) for v in tables.diffusion_coefficients(E_bins, kw["energy_gap"], kw["diffusion_coefficient"])]
    faces = R.walk_faces(mask, edges, bcs, dx, list(surfaces.values()))
    bounds = _check_outflow(flux, mask, faces, stored[4], lambda i: D[i])
    assert flux["outflow"].shape == (9, 4, 4) and (flux["outflow"] < 0).any() and (flux["outflow"] > 0).any()
    np.testing.assert_allclose(flux["number_outflow"], dE * flux["outflow"].sum(axis=-1), rtol=8 * U, atol=0)
    # the balance, plane by plane
    n = int(mask.sum())
    diag_sum = sum(f[1] for flist in faces for f in flist)
    srcs = sorted(abs(R.face_terms(b, dx)[1]) for b in bcs.values())
    s_cell = srcs[-1] + srcs[-2]
    times = flux["times"]
    worst = 0.0
    for i in range(4):
        moved = 0.0
        u0 = float(np.max(np.abs(stored[4][0][i][mask])))
        mass = [dx * dx * math.fsum(frames[i][mask].tolist()) for frames in stored[4]]
        F = flux["outflow"][:, :, i].sum(axis=1)
        for k in range(8):
            dt_k = times[k + 1] - times[k]
            a = dt * D[i] / (2 * dx * dx)
            assert a * 8 < 1
            r_max = u0 + 2 * (k + 1) * a * s_cell
            rounding = 4 * R.CN_CLOSURE_UNITS * U * n * dx * dx * r_max
            sums = dt_k / 2 * (bounds[k, :, i].sum() + bounds[k + 1, :, i].sum()
                               + 3 * U * (np.abs(flux["outflow"][k, :, i]).sum() + np.abs(flux["outflow"][k + 1, :, i]).sum()))
            stopping = kw["cn_rtol"] * r_max * dx * dx * (n + a * diag_sum)
            tol = rounding + sums + stopping
            err = mass[k] - mass[k + 1] - dt_k * (F[k] + F[k + 1]) / 2
            print(f"plane {i} step {k + 1} (dt {dt_k:.3g}): mass {mass[k]:.6e} -> {mass[k + 1]:.6e}, closure {err:.3g}, "
                  f"tolerance {tol:.3g} (rounding {rounding:.2g}, sums {sums:.2g}, stopping {stopping:.2g})")
            worst = max(worst, abs(err) / tol)
            assert abs(err) <= tol, (i, k, err, tol)
            moved = max(moved, abs(mass[k] - mass[k + 1]) / tol)
        assert moved > 1e3 or D[i] == 0.0, "the balance is not trivially closed"
    assert abs(times[8] - times[7] - 0.05) < 1e-12
    print(f"balance: worst closure / tolerance = {worst:.3g}")


def _donut_arguments():
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import ExternalGenerationSpec
    mask = np.ones((32, 32), dtype=bool)
    mask[12:20, 12:20] = False
    edges = extract_edge_segments(mask)
    inner = [e for e in edges if len(e.faces) == 8]              # the four walls of the hole; an outer side has 32 faces
    assert len(edges) == 8 and len(inner) == 4
    outer_kinds = [_bc("reflective"), _bc("dirichlet", 1e-6), _bc("robin", 0.3, 1e-7), _bc("reflective")]
    outer = [e for e in edges if e not in inner]
    bcs = {e.edge_id: _bc("absorbing") for e in inner}
    bcs.update({e.edge_id: kind for e, kind in zip(outer, outer_kinds)})
    init = 1e-4 * (1.0 + np.random.default_rng(4).random(mask.shape))
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1,
              total_time=1.25, dx=0.5, energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=6,
              enable_recombination=True, enable_scattering=True, T_c=1.2, diffusion_scheme="adi",
              gap_expression="170.0 + 10.0 * (x > 0.5)",
              external_generation=ExternalGenerationSpec(mode="constant", rate=2e-6))
    surfaces = {"hole": [e.edge_id for e in inner], "outer": [e.edge_id for e in outer],
                "mirror": [outer[0].edge_id, outer[3].edge_id]}
    return kw, surfaces


def test_donut_with_a_non_uniform_gap_beside_a_trace():
    """32 x 32 with an absorbing hole, two gap values (a field of coefficients), collisions on, ADI; 12 steps of 0.1 and one
    of 0.05, ``flux_every = 3`` beside ``trace_every = 2``.  The outflow against the helper on the frames of a run that stores
    every 3; the trace against the trace of a run that halts at the same steps (stores every 3, no flux sink)."""
    from qpsim_amd import solver as S
    kw, surfaces = _donut_arguments()
    mask, edges, bcs, dx = kw["mask"], kw["edges"], kw["edge_conditions"], kw["dx"]
    flux: dict = {}
    trace, trace_alone = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        stored = S.run_2d_crank_nicolson(**kw, store_every=3, trace_out=trace_alone, trace_every=2)
        S.run_2d_crank_nicolson(**kw, store_every=100, flux_out=flux, flux_surfaces=surfaces, flux_every=3, trace_out=trace,
                                trace_every=2)
    assert _same(trace, trace_alone), "the traces are unchanged by the flux sampler"
    assert flux["times"] == list(stored[0]) and len(flux["times"]) == 6 and len(trace["times"]) == 8
    assert flux["surfaces"] == ["hole", "outer", "mirror"] and flux["faces"] == [32, 64, 0]
    pre = S._auto_precomputed(None, kw["gap_expression"], mask, edges, bcs, diffusion_coefficient=kw["diffusion_coefficient"],
                              dt=kw["dt"], total_time=kw["total_time"], mesh_size=dx, energy_gap=kw["energy_gap"],
                              energy_min_factor=kw["energy_min_factor"], energy_max_factor=kw["energy_max_factor"],
                              num_energy_bins=kw["num_energy_bins"], dynes_gamma=0.0, tau_0=440.0, tau_s=440.0, tau_r=440.0,
                              T_c=kw["T_c"], bath_temperature=0.1)
    assert not bool(pre["is_uniform"]) and np.unique(pre["D_array"][-1]).size == 2
    D_planes = R.grid_plane(mask, np.asarray(pre["D_array"], dtype=float))
    faces = R.walk_faces(mask, edges, bcs, dx, list(surfaces.values()))
    _check_outflow(flux, mask, faces, stored[4], lambda i: D_planes[i])
    assert np.all(flux["outflow"][:, 2] == 0.0) and not np.signbit(flux["outflow"][:, 2]).any()
    assert np.all(flux["outflow"][:, 0, 1:] > 0.0), "quasiparticles leave through the absorbing hole"


def test_scalar_mode_on_a_padded_mask():
    """Scalar mode (the plane is u, ``energy_bins`` None) on a 9 x 11 grid with holes inside a padded frame: the device grid
    is the cropped bounding box, the faces are indexed on it."""
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.solver import run_2d_crank_nicolson
    mask = np.zeros((12, 15), dtype=bool)
    mask[2:11, 3:14] = True
    mask[4:6, 6:8] = False
    mask[8, 10] = False
    mask[2, 3] = False
    edges = extract_edge_segments(mask)
    kinds = [_bc("reflective"), _bc("dirichlet", 3e-4), _bc("absorbing"), _bc("robin", 0.3, 1e-6), _bc("neumann", 2e-5)]
    bcs = {e.edge_id: kinds[k % 5] for k, e in enumerate(edges)}
    init = 1e-4 * (1.0 + np.random.default_rng(3).random(mask.shape))
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1,
              total_time=0.75, dx=0.5, diffusion_scheme="cn_exact")
    ids = [e.edge_id for e in edges]
    surfaces = {"even": ids[::2], "odd": ids[1::2], "first": ids[:1]}
    flux: dict = {}
    default: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        stored = run_2d_crank_nicolson(**kw, store_every=2)
        sampled = run_2d_crank_nicolson(**kw, store_every=100, flux_out=flux, flux_surfaces=surfaces, flux_every=2)
        run_2d_crank_nicolson(**kw, store_every=100, flux_out=default, flux_every=2)
    assert flux["energy_bins"] is None and sampled[4] is None and flux["times"] == list(stored[0]) and len(flux["times"]) == 5
    for k in (0, -1):
        assert np.array_equal(sampled[1][k], stored[1][k], equal_nan=True) and sampled[2][k] == stored[2][k]
    faces = R.walk_faces(mask, edges, bcs, kw["dx"], list(surfaces.values()))
    assert flux["faces"] == [len(f) for f in faces] and flux["outflow"].shape == (5, 3, 1)
    _check_outflow(flux, mask, faces, [[frame] for frame in stored[1]], lambda i: kw["diffusion_coefficient"])
    assert np.array_equal(flux["number_outflow"], flux["outflow"][..., 0])
    assert (flux["outflow"] < 0).any() and (flux["outflow"] > 0).any()
    # None: one surface "all" of every edge
    every = R.walk_faces(mask, edges, bcs, kw["dx"], [ids])
    assert default["surfaces"] == ["all"] and default["faces"] == [len(every[0])]
    _check_outflow(default, mask, every, [[frame] for frame in stored[1]], lambda i: kw["diffusion_coefficient"])


def _ensemble_arguments(sweep: bool = False):
    """Per-member tables (a sweep) are bit-equal to the lone tables in the register kernels when the member grid holds a
    multiple of 64 cells: 24 x 40 with NE = 8 there, 20 x 28 with NE = 6 otherwise."""
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import ExternalGenerationSpec
    mask = np.ones((24, 40) if sweep else (20, 28), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: _bc(*kind) for e, kind in zip(edges, [("absorbing",), ("dirichlet", 1e-6), ("robin", 0.3, 1e-7),
                                                            ("reflective",)])}
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, diffusion_coefficient=6.0, dt=0.1, total_time=1.25, dx=0.5,
              energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=8 if sweep else 6,
              enable_recombination=True, enable_scattering=True, T_c=1.2, diffusion_scheme="adi", store_every=13, flux_every=3,
              flux_surfaces={"sink": [edges[0].edge_id], "walls": [e.edge_id for e in edges[1:]]},
              external_generation=ExternalGenerationSpec(mode="constant", rate=2e-6))
    rng = np.random.default_rng(11)
    inits = [1e-4 * (1.0 + rng.random(mask.shape)) for _ in range(3)]
    return kw, inits


@pytest.mark.parametrize("sweep", [False, True], ids=["coefficients", "swept_tau_0"])
def test_ensemble_members_get_the_outflow_of_their_lone_runs(sweep):
    """Three members with other initial fields and other diffusion coefficients (or a swept tau_0) on a small rectangle:
    ADI on the same tile family in both calls, so the states are bit-equal and the outflow with them."""
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw, inits = _ensemble_arguments(sweep)
    if sweep:
        members = [dict(initial_field=f) for f in inits]
        swept = {"tau_0": [440.0, 300.0, 600.0]}
    else:
        members = [dict(initial_field=f, diffusion_coefficient=d) for f, d in zip(inits, (6.0, 4.0, 8.0))]
        kw.pop("diffusion_coefficient")
        swept = None
    sinks: list = ["stale"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=swept, flux_out=sinks, **kw)
        assert len(sinks) == 3 and len(got) == 3
        for m, member in enumerate(members):
            lone: dict = {}
            extra = {} if swept is None else {key: values[m] for key, values in swept.items()}
            run_2d_crank_nicolson(**dict(kw, **member, **extra), flux_out=lone)
            assert len(lone["times"]) == 6 and lone["outflow"].shape == (6, 2, kw["num_energy_bins"])
            assert _same(sinks[m], lone), f"member {m}"
    assert sinks[0]["outflow"].tobytes() != sinks[1]["outflow"].tobytes()


def test_a_failed_member_gets_none():
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    kw, inits = _ensemble_arguments()
    members = [dict(initial_field=inits[0]), dict(initial_field=inits[0] * 1e9), dict(initial_field=inits[0] * 0.5)]
    kw.update(pauli_error_threshold=1.0, enforce_pauli=True)
    sinks: list = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, errors="return", flux_out=sinks, **kw)
    kinds = ["error" if isinstance(r, Exception) else "ok" for r in got]
    assert kinds == ["ok", "error", "ok"], got
    assert sinks[1] is None and sinks[0]["surfaces"] == ["sink", "walls"] and len(sinks[2]["times"]) == 6
