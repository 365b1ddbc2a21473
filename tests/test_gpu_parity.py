"""GPU parity tests: every call goes through the C ABI of libqpsim_hip.so and is checked against the
reference's golden vectors and the CPU oracle on the same inputs."""
from __future__ import annotations

import json
import warnings

import numpy as np
import pytest

from golden_utils import GOLDEN, GoldenRun, bcs_from_json, edges_from_json, oracle_kwargs, rel_err, run_names

pytestmark = pytest.mark.gpu

STRIP_TOL = 1e-10   # north_star: parity <= 1e-10 rel on the MKID cross-check (strip) configuration
GRID_TOL = 1e-9     # 2-D grids, exact-CN mode iterated to 1e-13 residual
ADI_TOL = 1e-11     # HIP ADI vs the oracle's ADI restatement (same algorithm, fp64 rounding only)
# phonon occupations go through (e^{b dt} - 1)/b of solver.py:697 (no expm1): for small |b dt| a last-bit difference
# between the host and device exp() is amplified by eps/|b dt|.  Priced in tests/test_gpu_configs.py against an 80-bit
# evaluation of the same algorithm: the fp64 reference restatement and the HIP kernels both sit ~1e-11 from it (NE = 12: 1.3e-11,
# NE = 50: 1.2e-11) and much closer to each other, so the kernel-vs-oracle bound is north_star's 1e-10 (round 1 used 1e-9)
PHONON_TOL = 1e-10
# whole runs accumulate that conditioning over their steps (mkid_24x24_ne12_full_physics: 20 coupled steps): phonon HISTORIES
# of multi-step runs keep the round-1 bound
RUN_PHONON_TOL = 1e-9
# (recombination, scattering, update_phonons): every template instantiation of the register kernels, including the
# frozen-phonon single-process ones the BASELINE configs[1] workload (`bench.py --workload c2`) runs
PROCESS_COMBOS = [(True, True, True), (True, False, True), (False, True, True), (True, True, False), (True, False, False),
                  (False, True, False)]


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


def _random_problem(seed, ny, nx, holes=True):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    rng = np.random.default_rng(seed)
    mask = np.ones((ny, nx), dtype=bool)
    if holes:
        mask &= rng.random((ny, nx)) > 0.15
        mask[ny // 2, :] |= True
    edges = extract_edge_segments(mask)
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 0.4), BoundaryCondition("absorbing"),
             BoundaryCondition("neumann", -0.05), BoundaryCondition("robin", 0.5, 0.1)]
    bcs = {e.edge_id: kinds[int(rng.integers(0, 5))] for e in edges}
    return rng, mask, edges, bcs


@pytest.mark.parametrize("variable_d", [False, True])
def test_stencil_and_sweeps_match_oracle(O, variable_d):
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    rng, mask, edges, bcs = _random_problem(3, 23, 37)
    dx, dt, B = 0.7, 0.13, 3
    geom = compile_geometry(mask, edges, bcs, dx)
    eng = Engine(geom)
    ops = O.build_grid_ops(mask, edges, bcs, dx)
    n = int(mask.sum())
    u = rng.random((B, n))
    if variable_d:
        Dp = 1.0 + 5.0 * rng.random((B, n))
        dfull = np.zeros((B, mask.size))
        dfull[:, mask.reshape(-1)] = Dp
        op = DiffusionOperator(eng, B, dt, dfield=dfull)
    else:
        Dc = [2.0, 6.0, 0.0]
        op = DiffusionOperator(eng, B, dt, dcoef=Dc)
    d_u = eng.upload_packed(u)
    for b in range(B):
        Dg = np.zeros(mask.shape)
        Dg[mask] = Dp[b] if variable_d else Dc[b]
        st = O.ADIStepper(ops, Dg if variable_d else Dc[b], dt)
        ug = np.zeros(mask.shape)
        ug[mask] = u[b]
        # explicit halves + source
        out = eng.empty(B, eng.ncell)
        eng.stencil(op, d_u, out, 1.0, 0.0, 1.0, 1.0)
        want = st._explicit(ug, "y") + st.src
        assert rel_err(eng.download_packed(out)[b], want[mask]) < 1e-14
        eng.stencil(op, d_u, out, 1.0, 1.0, 0.0, 1.0)
        want = st._explicit(ug, "x") + st.src
        assert rel_err(eng.download_packed(out)[b], want[mask]) < 1e-14
        # implicit sweeps
        x = eng.empty(B, eng.ncell)
        eng.sweep(op, 0, d_u, x)
        want = O.thomas_batched(*st.ax, ug)
        assert rel_err(eng.download_packed(x)[b], want[mask]) < 1e-13
        eng.sweep(op, 1, d_u, x)
        a, bb, c = (np.swapaxes(t, -1, -2) for t in st.ay)
        want = np.swapaxes(O.thomas_batched(a, bb, c, ug.T), -1, -2)
        assert rel_err(eng.download_packed(x)[b], want[mask]) < 1e-13
        # full ADI step and exact CN step
        v = d_u.clone()
        eng.adi_step(op, v)
        assert rel_err(eng.download_packed(v)[b], st.step(u[b])) < 1e-13
        v = d_u.clone()
        eng.cn_exact_step(op, v)
        assert rel_err(eng.download_packed(v)[b], O.CNStepper(ops, Dg if variable_d else Dc[b], dt).step(u[b])) < 1e-11
    assert np.all(eng.download_packed(v) == eng.download_packed(v))  # no NaN
    full = v.cpu().numpy()
    assert np.all(full[:, ~mask.reshape(-1)] == 0.0), "cells outside the mask must stay zero"


def test_collision_kernel_matches_reference_vectors():
    from qpsim_amd import tables as T
    from qpsim_amd.solver import (apply_collision_step_fischer_catelani_nonuniform,
                                  apply_collision_step_fischer_catelani_uniform)
    z = np.load(GOLDEN / "collision_vectors.npz", allow_pickle=False)
    meta = json.loads(str(z["meta_json"]))
    worst = 0.0
    for tag, m in meta.items():
        if tag == "nonuni":
            continue
        E, dE = T.build_energy_grid(m["gap"], 1.0, m["fmax"], m["ne"])
        om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
        s, p = z[f"{tag}_state_in"].copy(), z[f"{tag}_ph_in"].copy()
        apply_collision_step_fischer_catelani_uniform(
            s, p, T.recombination_kernel_base(E, m["gap"], m["tau_r"], m["T_c"]) if m["en_r"] else None,
            T.scattering_kernel_base(E, m["gap"], m["tau_s"], m["T_c"]) if m["en_s"] else None,
            T.dynes_density_of_states(E, m["gap"], m["gamma"]), idx_d, idx_s, sg, dE, m["dt"],
            enable_recombination=m["en_r"], enable_scattering=m["en_s"])
        e = max(rel_err(s, z[f"{tag}_state_out"]), rel_err(p, z[f"{tag}_ph_out"]))
        if e > worst:
            worst, worst_tag = e, (tag, m)
    # The reference's own update forms (1 - e^{-mu dt})/mu and (e^{b dt} - 1)/b without expm1 (solver.py:661,697):
    # for |x| << 1 the result carries ~eps/|x| of exp()'s last-bit rounding, so two correct exp() implementations
    # (glibc vs the device math library) legitimately differ by more than 1e-13 there.
    assert worst < 2e-11, (worst, worst_tag)
    m = meta["nonuni"]
    E, dE = T.build_energy_grid(m["gap"], 1.0, m["fmax"], m["ne"])
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    gaps = z["nonuni_gaps"]
    s, p = z["nonuni_state_in"].copy(), z["nonuni_ph_in"].copy()
    apply_collision_step_fischer_catelani_nonuniform(
        s, p, np.stack([T.recombination_kernel_base(E, g, m["tau_r"], m["T_c"]) for g in gaps]),
        np.stack([T.scattering_kernel_base(E, g, m["tau_s"], m["T_c"]) for g in gaps]),
        np.stack([T.dynes_density_of_states(E, g, m["gamma"]) for g in gaps]), idx_d, idx_s, sg, dE, m["dt"],
        enable_recombination=True, enable_scattering=True)
    assert rel_err(s, z["nonuni_state_out"]) < 1e-12 and rel_err(p, z["nonuni_ph_out"]) < 1e-12
    # frozen phonons: quasiparticles move, phonons do not
    tag = "c000"
    m = meta[tag]
    E, dE = T.build_energy_grid(m["gap"], 1.0, m["fmax"], m["ne"])
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    s, p = z[f"{tag}_state_in"].copy(), z[f"{tag}_ph_in"].copy()
    apply_collision_step_fischer_catelani_uniform(
        s, p, T.recombination_kernel_base(E, m["gap"], m["tau_r"], m["T_c"]),
        T.scattering_kernel_base(E, m["gap"], m["tau_s"], m["T_c"]), T.dynes_density_of_states(E, m["gap"], m["gamma"]),
        idx_d, idx_s, sg, dE, m["dt"], enable_recombination=True, enable_scattering=True, update_phonons=False)
    assert rel_err(s, z[f"{tag}_state_out"]) < 1e-12 and np.array_equal(p, z[f"{tag}_ph_in"])


def _compare_run(run: GoldenRun, res, ph, tol):
    times, frames, mass, clim, eframes, E = res
    sel = slice(-1, None) if run.final_only else slice(None)
    assert np.allclose(times, run.expected("times"), rtol=0, atol=1e-12)
    assert rel_err(np.stack(frames)[sel], run.expected("frames")) < tol
    dx = float(run.kwargs["dx"])
    scale = max(float(np.sum(np.abs(run.kwargs["initial_field"][run.kwargs["mask"]]))) * dx * dx,
                float(np.max(np.abs(run.expected("mass")))))
    assert np.max(np.abs(np.asarray(mass) - run.expected("mass"))) <= tol * scale
    cscale = float(np.max(np.abs(run.expected("color_limits"))))
    assert np.max(np.abs(np.asarray(clim) - run.expected("color_limits"))) <= tol * cscale
    if run.expected("energy_frames") is not None:
        got = np.stack([np.stack(ts) for ts in eframes])[sel]
        assert rel_err(got, run.expected("energy_frames")) < tol
        assert np.array_equal(E, run.expected("E_bins"))
    else:
        assert eframes is None and E is None
    if run.want_phonon_history:
        assert rel_err(np.stack(ph["phonon_frames"])[sel], run.expected("phonon_frames")) < tol
        if run.expected("phonon_energy_frames") is not None:
            got = np.stack([np.stack(ts) for ts in ph["phonon_energy_frames"]])[sel]
            assert rel_err(got, run.expected("phonon_energy_frames")) < tol
            assert np.array_equal(ph["phonon_energy_bins"], run.expected("phonon_energy_bins"))
        else:
            assert ph["phonon_energy_frames"] is None
        assert ph["phonon_metadata"] == run.meta["phonon_metadata"]


@pytest.mark.parametrize("name", run_names())
def test_default_run_reproduces_reference(name):
    """Drop-in call (default exact-CN scheme) against the recorded reference outputs."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    run = GoldenRun(name)
    kw = dict(run.kwargs)
    ph = {} if run.want_phonon_history else None
    if ph is not None:
        kw["phonon_history_out"] = ph
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = run_2d_crank_nicolson(**kw)
    _compare_run(run, res, ph, GRID_TOL if run.is_2d else STRIP_TOL)


@pytest.mark.parametrize("name", [n for n in run_names() if GoldenRun(n).is_2d])
def test_adi_scheme_matches_oracle_adi_on_2d(O, name):
    """The benchmarked ADI kernel sequence vs the oracle's ADI restatement on the same 2-D inputs."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    run = GoldenRun(name)
    kw = dict(run.kwargs)
    ph = {} if run.want_phonon_history else None
    if ph is not None:
        kw["phonon_history_out"] = ph
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson(**kw, diffusion_scheme="adi")
        ref = O.run(**oracle_kwargs(run, "adi"))
    assert rel_err(np.stack(got[1]), np.stack(ref[1])) < ADI_TOL
    if got[4] is not None:
        assert rel_err(np.stack([np.stack(t) for t in got[4]]), np.stack([np.stack(t) for t in ref[4]])) < ADI_TOL
    if ph is not None and ph["phonon_energy_frames"] is not None:
        assert rel_err(np.stack([np.stack(t) for t in ph["phonon_energy_frames"]]),
                       np.stack([np.stack(t) for t in ref[6]["phonon_energy_frames"]])) < RUN_PHONON_TOL


def test_mkid_crosscheck_bound_of_the_reference_test():
    """tests/test_mkid_crosscheck.py:194-207: rel < 1e-6 against the MKID-style 1-D update."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    run = GoldenRun("xcheck_mkid_1x48_ne12")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = run_2d_crank_nicolson(**run.kwargs)
    state = np.stack([np.stack(t) for t in res[4]])[:, :, 0, :]
    ref1d = np.asarray(run.meta["extra"]["mkid_like_reference_1d"])
    assert np.max(np.abs(state - ref1d)) / np.max(np.abs(ref1d)) < 1e-6
    dE = float(res[5][1] - res[5][0])
    assert np.max(np.abs(state.sum(1) * dE - ref1d.sum(1) * dE)) / np.max(np.abs(ref1d.sum(1) * dE)) < 1e-6


def _one_pixel():
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((1, 1), dtype=bool)
    edges = extract_edge_segments(mask)
    return mask, edges, {e.edge_id: BoundaryCondition("reflective") for e in edges}


def test_pauli_violation_raises_or_warns_like_the_reference():
    """tests/test_physics_safety.py:57-106."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    mask, edges, bcs = _one_pixel()
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=np.array([[2.0]]), diffusion_coefficient=6.0,
              dt=0.1, total_time=0.2, dx=1.0, energy_gap=180.0, energy_min_factor=1.5, energy_max_factor=1.5,
              num_energy_bins=1, enable_diffusion=False, enable_recombination=False, enable_scattering=False,
              pauli_error_threshold=1.0)
    with pytest.raises(ValueError, match="Pauli occupation exceeded limit"):
        run_2d_crank_nicolson(**kw, enforce_pauli=True)
    with pytest.warns(UserWarning, match="Pauli occupation exceeded limit"):
        run_2d_crank_nicolson(**kw, enforce_pauli=False)


def test_forbidden_state_is_detected():
    """rho == 0 bins (E below the local gap) holding density trip the guard (solver.py:1305-1317)."""
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    from qpsim_amd.solver import run_2d_crank_nicolson
    mask = np.ones((1, 4), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    with pytest.raises(ValueError, match="forbidden state"):
        run_2d_crank_nicolson(mask=mask, edges=edges, edge_conditions=bcs, initial_field=np.full((1, 4), 1e-6),
                              diffusion_coefficient=6.0, dt=0.1, total_time=0.1, dx=1.0, energy_gap=180.0,
                              energy_min_factor=0.5, energy_max_factor=2.0, num_energy_bins=6,
                              energy_weights=np.ones(6))


def test_argument_errors_match_reference_types():
    from qpsim_amd.engine import BoundaryAssignmentError
    from qpsim_amd.solver import run_2d_crank_nicolson
    mask, edges, bcs = _one_pixel()
    base = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=np.ones((1, 1)), diffusion_coefficient=1.0,
                dt=0.1, total_time=0.2, dx=1.0)
    with pytest.raises(ValueError):
        run_2d_crank_nicolson(**{**base, "dt": 0.0})
    with pytest.raises(ValueError):
        run_2d_crank_nicolson(**{**base, "diffusion_coefficient": 0.0})
    with pytest.raises(ValueError):
        run_2d_crank_nicolson(**{**base, "initial_field": np.ones((2, 1))})
    with pytest.raises(BoundaryAssignmentError):
        run_2d_crank_nicolson(**{**base, "edge_conditions": {}})
    with pytest.raises(ValueError, match="Unsupported collision solver"):
        run_2d_crank_nicolson(**base, energy_gap=180.0, num_energy_bins=4, collision_solver="boltzphlow_relaxation")
    with pytest.raises(ValueError, match="energy_weights must have length"):
        run_2d_crank_nicolson(**base, energy_gap=180.0, num_energy_bins=4, energy_weights=np.ones(3))


def test_progress_callback_and_final_time():
    """tests/test_regressions.py:254-301."""
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    from qpsim_amd.solver import run_2d_crank_nicolson
    mask = np.ones((2, 2), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    seen = []
    times, frames, *_ = run_2d_crank_nicolson(mask, edges, bcs, np.ones((2, 2)), 1.0, 0.3, 1.0, 1.0, 1,
                                              progress_callback=lambda t, f: seen.append((t, f.copy())))
    assert abs(times[-1] - 1.0) < 1e-12 and len(times) == 5
    assert [t for t, _ in seen] == times
    assert np.allclose(seen[-1][1], frames[-1])

    def boom(t, f):
        raise RuntimeError("callback errors are swallowed")
    run_2d_crank_nicolson(mask, edges, bcs, np.ones((2, 2)), 1.0, 0.3, 1.0, 1.0, 1, progress_callback=boom)


def test_pauli_stats_kernel_tie_breaking_and_classes():
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((3, 5), dtype=bool)
    mask[1, 2] = False
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    n = int(mask.sum())
    rho = np.array([[1.0, 2.0, 0.0], [4.0, 0.0, 1.0]])
    cls = np.arange(n) % 2
    idx = np.zeros((3, 3), dtype=np.int32)
    tab = eng.make_collision_tables(None, None, rho, idx, idx, idx.astype(np.int8), cls)
    state = np.zeros((3, n))
    state[0, 3] = 2.0      # class 1: f = 0.5
    state[1, 4] = 1.0      # class 0: f = 0.5  (later in C order -> loses the tie)
    state[0, 6] = 0.5      # class 0: f = 0.5  (same row, later pixel -> loses)
    state[2, 8] = 1e-3     # class 0, rho = 0  -> forbidden
    state[1, 9] = 5e-3     # class 1, rho = 0  -> forbidden, but earlier in C order (row 1 < row 2)
    d = eng.upload_packed(state)
    mx, top, forb = eng.pauli_stats(d, tab, 1e-18)
    px_of_cell = np.cumsum(mask.reshape(-1)) - 1
    assert mx == 0.5 and (top[0], px_of_cell[top[1]]) == (0, 3)
    assert (forb[0], px_of_cell[forb[1]]) == (1, 9)
    mx, top, forb = eng.pauli_stats(d, tab, 1.0)
    assert forb is None


@pytest.mark.parametrize("ny,nx", [(64, 64), (128, 192), (1, 48), (50, 1), (1, 1), (3, 200), (70, 65), (129, 257), (64, 63)])
def test_rect_fast_path_matches_oracle_adi_and_general_kernels(O, ny, nx):
    """Tiled partition-method ADI (full rectangle, one BC per side) vs the oracle ADI and the general kernels."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    rng = np.random.default_rng(ny * 1000 + nx)
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    side_bc = {"left": BoundaryCondition("dirichlet", 0.7), "right": BoundaryCondition("robin", 0.4, 0.2),
               "up": BoundaryCondition("neumann", -0.3), "down": BoundaryCondition("absorbing")}
    bcs = {e.edge_id: side_bc[e.normal] for e in edges}
    dx, dt = 0.9, 0.11
    geom = compile_geometry(mask, edges, bcs, dx)
    eng = Engine(geom)
    ops = O.build_grid_ops(mask, edges, bcs, dx)
    Dc = [6.0, 0.35, 0.0, 40.0]
    u0 = rng.random((len(Dc), ny * nx))
    fast = DiffusionOperator(eng, len(Dc), dt, dcoef=Dc)
    banded = DiffusionOperator(eng, len(Dc), dt, dcoef=Dc, force_banded=True)
    slow = DiffusionOperator(eng, len(Dc), dt, dcoef=Dc, allow_fast=False)
    assert fast.rect is not None and slow.rect is None and banded.rect.decoupled == (False, False)
    # D = 40 (r D = 2.7) keeps couplings between 64-cell chunks above the drop threshold: banded reduced solve
    if max(ny, nx) > 64:
        assert fast.rect.decoupled != (True, True)
    mild = DiffusionOperator(eng, 2, dt, dcoef=Dc[:2])
    # a short remainder chunk (n % 64 small) keeps a visible coupling through it -> that direction stays banded
    expect = tuple(n <= 64 or n % 64 == 0 or n % 64 >= 48 for n in (nx, ny))
    assert mild.rect.decoupled == expect
    for nsteps in (1, 3):
        a = eng.upload_packed(u0)
        b = eng.upload_packed(u0)
        c = eng.upload_packed(u0)
        d = eng.upload_packed(u0[:2])
        eng.adi_steps(fast, a, nsteps)
        eng.adi_steps(slow, b, nsteps)
        eng.adi_steps(banded, c, nsteps)
        eng.adi_steps(mild, d, nsteps)
        ha, hb = eng.download_packed(a), eng.download_packed(b)
        assert rel_err(eng.download_packed(c), ha) < 2e-13
        assert rel_err(eng.download_packed(d), eng.download_packed(c)[:2]) < 2e-13
        for k, D in enumerate(Dc):
            st = O.ADIStepper(ops, D, dt)
            want = u0[k].copy()
            for _ in range(nsteps):
                want = st.step(want)
            assert rel_err(ha[k], want) < 2e-13, (k, nsteps)
            assert rel_err(hb[k], want) < 2e-13, (k, nsteps)


@pytest.mark.parametrize("ny,nx,D", [(64, 64, 6.0), (70, 130, 2.0), (128, 192, 40.0), (1, 100, 6.0)])
def test_exact_cn_iteration_on_the_fast_path_matches_superlu(O, ny, nx, D):
    """Exact-CN step whose preconditioner runs on the tiled solve (decoupled and banded regimes) vs the oracle's SuperLU."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    rng = np.random.default_rng(ny + nx)
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    side_bc = {"left": BoundaryCondition("dirichlet", 0.7), "right": BoundaryCondition("robin", 0.4, 0.2),
               "up": BoundaryCondition("neumann", -0.3), "down": BoundaryCondition("absorbing")}
    bcs = {e.edge_id: side_bc[e.normal] for e in edges}
    dx, dt = 0.9, 0.11
    eng = Engine(compile_geometry(mask, edges, bcs, dx))
    op = DiffusionOperator(eng, 2, dt, dcoef=[D, 0.5 * D])
    assert op.rect is not None
    u0 = rng.random((2, ny * nx))
    v = eng.upload_packed(u0)
    its = eng.cn_exact_step(op, v)
    ops = O.build_grid_ops(mask, edges, bcs, dx)
    got = eng.download_packed(v)
    for k, d in enumerate([D, 0.5 * D]):
        assert rel_err(got[k], O.CNStepper(ops, d, dt).step(u0[k])) < 1e-11
    assert its < 400      # stiff a = r D (2.7 in the third case) converges slowly: plain Richardson, factor ~(a l/(1+a l))^2


def test_rect_fast_path_large_reflective_conserves_mass_and_matches_general():
    """4096-class property check at a size the oracle cannot reach quickly: 1024^2, 5 steps, reflective walls."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    N = 1024
    mask = np.ones((N, N), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    eng = Engine(compile_geometry(mask, edges, bcs, 1.0))
    u0 = 1e-4 * (1.0 + np.random.default_rng(0).random((1, N * N)))
    fast = DiffusionOperator(eng, 1, 0.1, dcoef=[6.0])
    slow = DiffusionOperator(eng, 1, 0.1, dcoef=[6.0], allow_fast=False)
    a, b = eng.upload_packed(u0), eng.upload_packed(u0)
    eng.adi_steps(fast, a, 5)
    eng.adi_steps(slow, b, 5)
    ha, hb = eng.download_packed(a), eng.download_packed(b)
    assert rel_err(ha, hb) < 1e-13
    assert abs(ha.sum() - u0.sum()) / u0.sum() < 1e-13           # zero-flux walls conserve the integral
    assert ha.min() >= u0.min() and ha.max() <= u0.max()         # discrete maximum principle for r D = 0.3


@pytest.mark.parametrize("ne,fmax", [(2, 3.0), (5, 3.0), (8, 4.0), (12, 3.0), (16, 10.0), (20, 3.0), (32, 3.0), (40, 3.0),
                                     (50, 10.0)])
@pytest.mark.parametrize("en_r,en_s,upd", PROCESS_COMBOS)
def test_fast_collision_kernel_matches_generic_and_oracle(O, ne, fmax, en_r, en_s, upd):
    """Register-resident diagonal kernel (uniform tables; NE = 50, the reference default, runs the split
    quasiparticle / phonon pair with q re-formed on the fly) vs the generic kernel and the oracle."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags, structured_bin_maps
    rng = np.random.default_rng(ne * 7 + int(en_r) + 2 * int(en_s))
    mask = rng.random((9, 31)) > 0.2
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    n = int(mask.sum())
    gap, gamma = 180.0, 0.1
    E, dE = T.build_energy_grid(gap, 1.0, fmax, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    assert structured_bin_maps(idx_d, idx_s, sg) is not None
    rho = T.dynes_density_of_states(E, gap, gamma)
    kr, ks = T.recombination_kernel_base(E, gap, 500.0, 1.2), T.scattering_kernel_base(E, gap, 400.0, 1.2)
    state = rng.random((ne, n)) * rho[:, None] * rng.choice([1e-5, 1e-2, 0.5, 0.95], size=n)[None, :]
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    outs = []
    for fast in (True, False):
        tab = eng.make_collision_tables(kr[None], ks[None], rho[None], idx_d, idx_s, sg, allow_fast=fast)
        assert tab["fast"] == fast and tab["kernel"] == ("register" if fast else "generic")
        s_in, p_dev = eng.upload_packed(state), eng.upload_packed(ph)
        s_out = eng.empty(ne, eng.ncell)
        eng.collide(tab, s_in, s_out, p_dev, dE, 0.37, en_r, en_s, upd)
        outs.append((eng.download_packed(s_out), eng.download_packed(p_dev), s_out.cpu().numpy()))
    # phonon planes: (e^{b dt} - 1)/b without expm1 (solver.py:697) amplifies summation-order differences in b by
    # eps/|b dt|; with 50 bins and occupations up to 0.95 every kernel (and the oracle) sits within PHONON_TOL of the others
    ptol = 1e-11 if ne <= 16 else PHONON_TOL
    assert rel_err(outs[0][0], outs[1][0]) < 1e-12 and rel_err(outs[0][1], outs[1][1]) < ptol
    assert np.all(outs[0][2][:, ~mask.reshape(-1)] == 0.0)
    tables = {"rho": rho[None], "Kr0": kr[None] if en_r else None, "Ks0": ks[None] if en_s else None,
              "cls": np.zeros(n, dtype=int), "idx_diff": idx_d, "idx_sum": idx_s, "sign": sg, "dE": dE}
    s_ref, p_ref = state.copy(), ph.copy()
    O.collision_step(s_ref, p_ref, tables, 0.37, en_r=en_r, en_s=en_s, update_phonons=upd)
    # vs the host oracle the exp() last-bit caveat of solver.py:661,697 applies (see the golden-vector test above)
    assert rel_err(outs[0][0], s_ref) < 2e-11 and rel_err(outs[0][1], p_ref) < (2e-11 if ne <= 16 else PHONON_TOL)


@pytest.mark.parametrize("ne,fmax", [(12, 3.0), (50, 10.0)])
@pytest.mark.parametrize("dt", [0.0, 1e-7, 3e-3, 25.0])
def test_collision_update_over_the_range_of_rate_times_step(O, ne, fmax, dt):
    """The exponential updates (solver.py:640-665, :686-700) over the regimes of x = rate * dt: dt = 0 (state returned
    unchanged - x = 0 with finite rates, where the small-|x| path of the NE < 30 kernels has no reciprocal), |x| ~ 1e-8
    (the reference's e^x - 1 is rounding-dominated there: the kernels reproduce that rounding instead of the closed form),
    the small-|x| polynomial path proper, and |x| >> 1/8 (general path; waves mix both paths pixel by pixel through the
    occupation levels).  The clip of the exponent to +-80 is barely reached: at dt = 25 b dt spans -18.4 ... 6.7 at NE = 12
    (no clip) and -354 ... 69.3 at NE = 50 (the lower clip only); tests/test_gpu_collision_elementwise.py reaches both
    clips with dt = 400 and 800.  Against the oracle at the tolerances of the other collision tests."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    rng = np.random.default_rng(ne + 101)
    mask = rng.random((9, 31)) > 0.2
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    n = int(mask.sum())
    E, dE = T.build_energy_grid(180.0, 1.0, fmax, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = T.dynes_density_of_states(E, 180.0, 0.1)
    kr, ks = T.recombination_kernel_base(E, 180.0, 500.0, 1.2), T.scattering_kernel_base(E, 180.0, 400.0, 1.2)
    state = rng.random((ne, n)) * rho[:, None] * rng.choice([1e-9, 1e-5, 1e-2, 0.5, 0.95], size=n)[None, :]
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    tab = eng.make_collision_tables(kr[None], ks[None], rho[None], idx_d, idx_s, sg)
    assert tab["kernel"] == "register"
    s_in, p_dev = eng.upload_packed(state), eng.upload_packed(ph)
    s_out = eng.empty(ne, eng.ncell)
    eng.collide(tab, s_in, s_out, p_dev, dE, dt, True, True, True)
    got_s, got_p = eng.download_packed(s_out), eng.download_packed(p_dev)
    assert np.all(np.isfinite(got_s)) and np.all(np.isfinite(got_p))
    if dt == 0.0:
        assert np.array_equal(got_s, state) and np.array_equal(got_p, ph)
        return
    tables = {"rho": rho[None], "Kr0": kr[None], "Ks0": ks[None], "cls": np.zeros(n, dtype=int), "idx_diff": idx_d,
              "idx_sum": idx_s, "sign": sg, "dE": dE}
    s_ref, p_ref = state.copy(), ph.copy()
    O.collision_step(s_ref, p_ref, tables, dt, en_r=True, en_s=True, update_phonons=True)
    assert rel_err(got_s, s_ref) < 2e-11 and rel_err(got_p, p_ref) < (2e-11 if ne <= 16 else PHONON_TOL)


@pytest.mark.parametrize("ne,fmax", [(12, 5.0), (18, 10.0), (24, 4.0), (40, 5.0), (50, 5.0)])
@pytest.mark.parametrize("en_r,en_s,upd", PROCESS_COMBOS)
def test_register_collision_kernel_with_merged_phonon_bins(O, ne, fmax, en_r, en_s, upd):
    """2 E_min / dE integer: phonon bins shared between a diagonal and an anti-diagonal.  The register kernels park the
    diagonal's sums in scratch and finalise the bin once; checked against the generic kernel and the oracle."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags, structured_bin_maps
    rng = np.random.default_rng(ne * 13 + int(en_r) + 2 * int(en_s))
    mask = rng.random((9, 31)) > 0.2
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    n = int(mask.sum())
    gap, gamma = 180.0, 0.1
    E, dE = T.build_energy_grid(gap, 1.0, fmax, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    assert structured_bin_maps(idx_d, idx_s, sg) is None and structured_bin_maps(idx_d, idx_s, sg, allow_shared=True) is not None
    rho = T.dynes_density_of_states(E, gap, gamma)
    kr, ks = T.recombination_kernel_base(E, gap, 500.0, 1.2), T.scattering_kernel_base(E, gap, 400.0, 1.2)
    state = rng.random((ne, n)) * rho[:, None] * rng.choice([1e-5, 1e-2, 0.5, 0.95], size=n)[None, :]
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    outs = []
    for kern in ("auto", "generic"):
        tab = eng.make_collision_tables(kr[None], ks[None], rho[None], idx_d, idx_s, sg, kernel=kern)
        assert tab["kernel"] == ("register" if kern == "auto" else "generic") and tab["merged_slots"] > 0
        s_in, p_dev = eng.upload_packed(state), eng.upload_packed(ph)
        s_out = eng.empty(ne, eng.ncell)
        eng.collide(tab, s_in, s_out, p_dev, dE, 0.37, en_r, en_s, upd)
        outs.append((eng.download_packed(s_out), eng.download_packed(p_dev)))
    ptol = 1e-11 if ne <= 16 else PHONON_TOL
    assert rel_err(outs[0][0], outs[1][0]) < 1e-12 and rel_err(outs[0][1], outs[1][1]) < ptol
    tables = {"rho": rho[None], "Kr0": kr[None] if en_r else None, "Ks0": ks[None] if en_s else None,
              "cls": np.zeros(n, dtype=int), "idx_diff": idx_d, "idx_sum": idx_s, "sign": sg, "dE": dE}
    s_ref, p_ref = state.copy(), ph.copy()
    O.collision_step(s_ref, p_ref, tables, 0.37, en_r=en_r, en_s=en_s, update_phonons=upd)
    # (1 - e^{-mu dt})/mu without expm1 (solver.py:661) amplifies summation-order differences of mu like the phonon form
    assert rel_err(outs[0][0], s_ref) < (2e-11 if ne <= 16 else 1e-10)
    assert rel_err(outs[0][1], p_ref) < (2e-11 if ne <= 16 else PHONON_TOL)
    if not upd:
        assert np.array_equal(outs[0][1], ph)


def test_merged_phonon_bins_fall_back_to_generic_kernel():
    from qpsim_amd import tables as T
    from qpsim_amd.engine import structured_bin_maps
    E, _ = T.build_energy_grid(180.0, 1.0, 10.0, 18)      # 2 E_min / dE = 4: sums and differences share bins
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    assert om.size < 18 + 35 and structured_bin_maps(idx_d, idx_s, sg) is None
    E, _ = T.build_energy_grid(180.0, 1.0, 3.0, 12)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    d, a = structured_bin_maps(idx_d, idx_s, sg)
    assert om.size == 35 and d.size == 12 and a.size == 23


def test_euler_step_helpers_match_reference_vectors():
    """Public explicit-Euler helpers (solver.py:551-637) on the GPU vs recorded reference outputs."""
    from qpsim_amd import tables as T
    from qpsim_amd.solver import _collision_rhs, apply_recombination_step, apply_scattering_step
    z = np.load(GOLDEN / "collision_vectors.npz", allow_pickle=False)
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, 8)
    rho = T.dynes_density_of_states(E, 180.0, 0.0)
    K_s, K_r = T.scattering_kernel(E, 180.0, 400.0, 1.2, 0.2), T.recombination_kernel(E, 180.0, 500.0, 1.2, 0.2)
    a = z["euler_state_in"].copy()
    apply_scattering_step(a, K_s, rho, dE, 0.05)
    b = z["euler_state_in"].copy()
    apply_recombination_step(b, K_r, z["euler_G"], dE, 0.05)
    assert rel_err(a, z["euler_scat_out"]) < 1e-13 and rel_err(b, z["euler_recomb_out"]) < 1e-13
    assert rel_err(_collision_rhs(z["euler_state_in"][:, 0], K_r, K_s, rho, z["euler_G"], dE), z["euler_rhs_px0"]) < 1e-12
    assert np.array_equal(_collision_rhs(z["euler_state_in"][:, 0], None, None, None, None, dE), np.zeros(8))


def test_fast_validation_suite_on_gpu_matches_reference_report():
    """tests/test_physics_safety.py:109-117 + the reference's recorded report values."""
    from qpsim_amd.validation import run_fast_validation_suite
    ref = json.loads((GOLDEN / "validation_report.json").read_text())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = run_fast_validation_suite().as_dict()
    assert rep["overall_passed"] is True
    for key in ("detailed_balance", "thermal_stability", "pure_diffusion", "pure_scattering", "pure_recombination"):
        assert rep[key]["passed"] is True
    assert rep["detailed_balance"]["max_relative_error"] == ref["detailed_balance"]["max_relative_error"]
    assert abs(rep["pure_scattering"]["mass_relative_drift"] - ref["pure_scattering"]["mass_relative_drift"]) < 1e-9
    assert abs(rep["pure_recombination"]["mass_end"] - ref["pure_recombination"]["mass_end"]) < 1e-14
    assert rep["thermal_stability"]["max_relative_drift"] < 1e-9 and rep["pure_diffusion"]["mass_relative_drift"] < 1e-12


def test_padded_rectangle_geometry_is_cropped_onto_the_fast_path(O):
    """The reference's built-in geometry (solid rectangle in a padded frame, geometry.py:245-262) must give the same
    result as the general masked path, and its packed ordering must survive the crop."""
    from qpsim_amd.engine import Engine
    from qpsim_amd.geometry import create_intrinsic_geometry, extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    from qpsim_amd.solver import _crop_to_bounding_box, run_2d_crank_nicolson
    g = create_intrinsic_geometry(width=40, height=28)
    mask = np.asarray(g.mask, dtype=bool)
    edges = g.edges
    kinds = {"left": BoundaryCondition("dirichlet", 0.2), "right": BoundaryCondition("absorbing"),
             "up": BoundaryCondition("reflective"), "down": BoundaryCondition("robin", 0.3, 0.05)}
    bcs = {e.edge_id: kinds[e.normal] for e in edges}
    cm, ce = _crop_to_bounding_box(mask, edges)
    assert cm.all() and cm.shape == (14, 24) and [e.edge_id for e in ce] == [e.edge_id for e in edges]
    init = np.random.default_rng(4).random(mask.shape)
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=3.0, dt=0.1,
              total_time=0.6, dx=1.0, store_every=3)
    got = run_2d_crank_nicolson(**kw, diffusion_scheme="adi")
    ref = O.run(**kw, scheme="adi")
    assert rel_err(np.stack(got[1]), np.stack(ref[1])) < 1e-12
    got = run_2d_crank_nicolson(**kw)
    ref = O.run(**kw, scheme="cn")
    assert rel_err(np.stack(got[1]), np.stack(ref[1])) < 1e-10
    assert np.allclose(got[2], ref[2], rtol=1e-10)


def test_energy_integral_and_weighted_sum_kernels():
    """qp_energy_integrate / qp_weighted_sum (solver.py:1358,1367,1480) vs NumPy on a masked grid."""
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    rng = np.random.default_rng(9)
    mask = rng.random((13, 17)) > 0.3
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    n = int(mask.sum())
    state = rng.random((7, n))
    w = rng.random(7)
    d = eng.upload_packed(state)
    got = eng.energy_integral(d, 0.37).cpu().numpy()[mask.reshape(-1)]
    assert np.array_equal(got, np.sum(state, axis=0) * 0.37)      # same sequential order as np.sum(axis=0)
    got = eng.weighted_sum(d, w).cpu().numpy()[mask.reshape(-1)]
    assert rel_err(got, np.sum(state * w[:, None], axis=0)) < 1e-15


@pytest.mark.parametrize("ne,fmax,nclass", [(6, 3.0, 1), (12, 3.0, 1), (24, 4.0, 1), (50, 10.0, 1), (64, 10.0, 1),
                                            (18, 10.0, 1), (10, 3.0, 3), (50, 10.0, 2)])
@pytest.mark.parametrize("en_r,en_s,upd", [(True, True, True), (True, False, True), (False, True, False)])
def test_wave_collision_kernel_matches_generic_and_oracle(O, ne, fmax, nclass, en_r, en_s, upd):
    """One-wave-per-pixel kernel (NE <= 64, gap classes, merged bins via LDS atomics) vs generic kernel and oracle."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags, structured_bin_maps
    rng = np.random.default_rng(ne * 11 + nclass)
    mask = rng.random((7, 23)) > 0.2
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    n = int(mask.sum())
    gaps = np.array([180.0, 171.0, 188.5])[:nclass]
    E, dE = T.build_energy_grid(180.0, 1.0, fmax, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in gaps])
    kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in gaps])
    ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in gaps])
    cls = rng.integers(0, nclass, size=n)
    state = rng.random((ne, n)) * rho[cls].T * rng.choice([1e-5, 1e-2, 0.5, 0.95], size=n)[None, :]
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    # sums and differences share phonon bins when 2 E_min / dE is an integer inside the difference range
    ratio = 2.0 * ne / (fmax - 1.0)
    merged = structured_bin_maps(idx_d, idx_s, sg) is None
    assert merged == (abs(ratio - round(ratio)) < 1e-9 and ratio <= ne - 2)
    outs = {}
    for kern in ("wave", "wave_unstructured", "generic"):
        tab = eng.make_collision_tables(kr, ks, rho, idx_d, idx_s, sg, cls if nclass > 1 else None, kernel=kern)
        assert tab["kernel"] == kern.split("_")[0]
        s_in, p_dev = eng.upload_packed(state), eng.upload_packed(ph)
        s_out = eng.empty(ne, eng.ncell)
        eng.collide(tab, s_in, s_out, p_dev, dE, 0.37, en_r, en_s, upd)
        outs[kern] = (eng.download_packed(s_out), eng.download_packed(p_dev), s_out.cpu().numpy(), p_dev.cpu().numpy())
    assert rel_err(outs["wave"][0], outs["generic"][0]) < 1e-12 and rel_err(outs["wave"][1], outs["generic"][1]) < 1e-11
    assert rel_err(outs["wave_unstructured"][0], outs["generic"][0]) < 1e-12
    assert rel_err(outs["wave_unstructured"][1], outs["generic"][1]) < 1e-11
    hole = ~mask.reshape(-1)
    assert np.all(outs["wave"][2][:, hole] == 0.0) and np.all(outs["wave"][3][:, hole] == 0.0)
    tables = {"rho": rho, "Kr0": kr if en_r else None, "Ks0": ks if en_s else None, "cls": cls, "idx_diff": idx_d,
              "idx_sum": idx_s, "sign": sg, "dE": dE}
    s_ref, p_ref = state.copy(), ph.copy()
    O.collision_step(s_ref, p_ref, tables, 0.37, en_r=en_r, en_s=en_s, update_phonons=upd)
    assert rel_err(outs["wave"][0], s_ref) < 2e-11 and rel_err(outs["wave"][1], p_ref) < 2e-11
    if not upd:
        assert np.array_equal(outs["wave"][1], ph)


def test_collision_kernel_selection():
    import ctypes as C
    from qpsim_amd import _hip
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((1, 8), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    family = {_hip.ROUTE_WAVE: "wave", _hip.ROUTE_GENERIC: "generic"}
    family.update({r: "register" for r in (_hip.ROUTE_ONEPASS, _hip.ROUTE_REGISTER, _hip.ROUTE_REGISTER_MEMBERS,
                                           _hip.ROUTE_ONEPASS_CLASSES, _hip.ROUTE_REGISTER_CLASSES)})

    def pick(ne, fmax, nclass=1):
        E, _ = T.build_energy_grid(180.0, 1.0, fmax, ne)
        om, idd, ids, sg = T.build_phonon_frequency_map(E)
        rho = np.ones((nclass, ne))
        k = np.zeros((nclass, ne, ne))
        h = eng.make_collision_tables(k, k, rho, idd, ids, sg, np.zeros(8, dtype=int) if nclass > 1 else None)
        # the engine's own rule agrees with the library's: all processes on, scratch present
        route = _hip.load().qp_collision_route(C.byref(h["struct"]), 8, 1, 1, 1, 1)
        assert family[route] == h["kernel"], (ne, fmax, nclass, route)
        return h["kernel"]

    assert pick(12, 3.0) == "register" and pick(16, 10.0) == "register"
    assert pick(24, 3.0) == "register" and pick(50, 10.0) == "register"      # instantiated sizes incl. the reference default
    assert pick(20, 3.0) == "register" and pick(33, 10.0) == "wave" and pick(64, 10.0) == "wave"   # 33, 64: no instantiation
    assert pick(17, 3.0) == "wave"             # rounding splits some |Ei-Ej| into extra bins here: no diagonal structure
    assert pick(18, 10.0) == "register"        # merged bins: register kernel with the scratch stash
    assert pick(12, 3.0, nclass=2) == "wave"   # gap classes without the separable tables (gap_params)
    assert pick(65, 10.0) == "generic"


# ------------------------------------------------------------------------------------------------------------------
# tiled path for masked grids (qp_adi_tile.hip)
# ------------------------------------------------------------------------------------------------------------------
def _donut(ny, nx, r_out, r_in):
    y, x = np.indices((ny, nx))
    rr = np.hypot(y - (ny - 1) / 2.0, x - (nx - 1) / 2.0)
    return (rr <= r_out) & (rr >= r_in)


def _masked_problem(kind, seed):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    rng = np.random.default_rng(seed)
    if kind == "holes":               # random holes everywhere: every tile is general, many short segments
        ny, nx = 150, 200
        mask = rng.random((ny, nx)) > 0.12
    elif kind == "donut":             # clean tiles in the ring, empty ones in the hole and the corners
        ny, nx = 448, 512
        mask = _donut(ny, nx, 215.0, 70.0)
    elif kind == "slab":              # full rectangle with a different BC on half of one side (not a "rect" geometry)
        ny, nx = 192, 260
        mask = np.ones((ny, nx), dtype=bool)
    elif kind == "strip":             # 1 x N strip with a gap
        ny, nx = 1, 300
        mask = np.ones((ny, nx), dtype=bool)
        mask[0, 140:150] = False
    elif kind == "small":             # smaller than one tile
        ny, nx = 9, 11
        mask = rng.random((ny, nx)) > 0.2
    else:
        raise ValueError(kind)
    edges = extract_edge_segments(mask)
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 0.4), BoundaryCondition("absorbing"),
             BoundaryCondition("neumann", -0.05), BoundaryCondition("robin", 0.5, 0.1)]
    if kind == "slab":
        bcs = {e.edge_id: kinds[0] for e in edges}
        # split the left wall: rows < 100 Dirichlet, the rest reflective (edge segments are per wall, so set by cell below)
        bcs = {e.edge_id: (kinds[1] if e.normal == "left" else kinds[4] if e.normal == "down" else kinds[0]) for e in edges}
    else:
        bcs = {e.edge_id: kinds[int(rng.integers(0, 5))] for e in edges}
    return rng, mask, edges, bcs


@pytest.mark.parametrize("kind", ["holes", "donut", "slab", "strip", "small"])
def test_tile_path_matches_oracle_adi_and_general_kernels(O, kind):
    """Masked-grid tiled ADI vs the oracle ADI restatement and vs the per-line kernels, 1 and 3 carried steps."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    rng, mask, edges, bcs = _masked_problem(kind, 11)
    dx, dt = 0.9, 0.11
    geom = compile_geometry(mask, edges, bcs, dx)
    if kind == "slab":   # make the geometry non-rect: a second boundary term on part of the left wall
        geom.ex[:100, 0] *= 0.5
        geom.sx[:100, 0] *= 0.25
    eng = Engine(geom)
    Dc = [6.0, 0.35, 0.0]
    n = int(mask.sum())
    u0 = rng.random((len(Dc), n))
    fast = DiffusionOperator(eng, len(Dc), dt, dcoef=Dc)
    slow = DiffusionOperator(eng, len(Dc), dt, dcoef=Dc, allow_fast=False)
    assert fast.rect is None and fast.tile is not None, fast.tile_refused
    assert slow.tile is None
    counts = fast.tile.tile_counts
    py, px = -(-mask.shape[0] // 64), -(-mask.shape[1] // 64)
    assert sum(counts.values()) == py * px
    if kind == "donut":
        assert counts["empty"] > 0 and counts["clean"] > 0 and counts["general"] > 0
    assert fast.tile.far_coupling < 1e-22
    for nsteps in (1, 3):
        a, b = eng.upload_packed(u0), eng.upload_packed(u0)
        eng.adi_steps(fast, a, nsteps)
        eng.adi_steps(slow, b, nsteps)
        ha, hb = eng.download_packed(a), eng.download_packed(b)
        assert rel_err(ha, hb) < 2e-13, nsteps
        full = a.detach().cpu().numpy()
        assert np.all(full[:, ~mask.reshape(-1)] == 0.0)          # holes stay exactly 0
        if kind != "slab":                                         # the oracle has no per-cell override of BC terms
            ops = O.build_grid_ops(mask, edges, bcs, dx)
            for k, D in enumerate(Dc):
                st = O.ADIStepper(ops, D, dt)
                want = u0[k].copy()
                for _ in range(nsteps):
                    want = st.step(want)
                assert rel_err(ha[k], want) < 2e-13, (k, nsteps)


def test_tile_path_refuses_stiff_steps_and_falls_back(O):
    """r D = 2.7 keeps 64-cell chunks coupled wherever a line segment spans a whole chunk (ring): the plan is refused and
    the per-line kernels run; with random holes no segment is that long, so the same step size is accepted."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    for kind, accepted in (("donut", False), ("holes", True)):
        rng, mask, edges, bcs = _masked_problem(kind, 5)
        if kind == "donut":
            mask = mask[:, :256]
            from qpsim_amd.geometry import extract_edge_segments
            from qpsim_amd.models import BoundaryCondition
            edges = extract_edge_segments(mask)
            bcs = {e.edge_id: BoundaryCondition("absorbing" if i % 2 else "reflective") for i, e in enumerate(edges)}
        eng = Engine(compile_geometry(mask, edges, bcs, 0.9))
        op = DiffusionOperator(eng, 1, 0.11, dcoef=[40.0])
        if accepted:
            assert op.tile is not None
        else:
            assert op.tile is None and "too large" in op.tile_refused
        u0 = rng.random((1, int(mask.sum())))
        a = eng.upload_packed(u0)
        eng.adi_steps(op, a, 1)
        want = O.ADIStepper(O.build_grid_ops(mask, edges, bcs, 0.9), 40.0, 0.11).step(u0[0])
        assert rel_err(eng.download_packed(a)[0], want) < 2e-13


@pytest.mark.parametrize("kind", ["holes", "donut"])
def test_exact_cn_iteration_on_the_tile_path_matches_superlu(O, kind):
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    rng, mask, edges, bcs = _masked_problem(kind, 23)
    if kind == "donut":
        mask = mask[96:352, 128:384]          # keep SuperLU quick: centre part of the ring
        from qpsim_amd.geometry import extract_edge_segments
        from qpsim_amd.models import BoundaryCondition
        edges = extract_edge_segments(mask)
        bcs = {e.edge_id: BoundaryCondition("absorbing" if i % 3 == 0 else "reflective") for i, e in enumerate(edges)}
    dx, dt = 0.9, 0.11
    eng = Engine(compile_geometry(mask, edges, bcs, dx))
    op = DiffusionOperator(eng, 2, dt, dcoef=[6.0, 1.5])
    assert op.tile is not None
    u0 = rng.random((2, int(mask.sum())))
    v = eng.upload_packed(u0)
    its = eng.cn_exact_step(op, v)
    ops = O.build_grid_ops(mask, edges, bcs, dx)
    got = eng.download_packed(v)
    for k, d in enumerate([6.0, 1.5]):
        assert rel_err(got[k], O.CNStepper(ops, d, dt).step(u0[k])) < 1e-11
    assert its < 100


def test_tile_path_large_donut_conserves_mass_and_matches_general():
    """2048^2 ring with reflective walls: mass conservation and agreement with the per-line kernels over 4 steps."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    N = 2048
    mask = _donut(N, N, 1000.0, 300.0)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    eng = Engine(compile_geometry(mask, edges, bcs, 1.0))
    n = int(mask.sum())
    u0 = 1e-4 * (1.0 + np.random.default_rng(0).random((1, n)))
    fast = DiffusionOperator(eng, 1, 0.1, dcoef=[6.0])
    slow = DiffusionOperator(eng, 1, 0.1, dcoef=[6.0], allow_fast=False)
    assert fast.tile is not None
    a, b = eng.upload_packed(u0), eng.upload_packed(u0)
    eng.adi_steps(fast, a, 4)
    eng.adi_steps(slow, b, 4)
    ha, hb = eng.download_packed(a), eng.download_packed(b)
    assert rel_err(ha, hb) < 1e-12
    assert abs(ha.sum() - u0.sum()) / u0.sum() < 1e-12


@pytest.mark.parametrize("kind", ["holes", "donut", "full", "strip", "small"])
def test_tile_path_variable_diffusivity_matches_oracle_and_per_line_kernels(O, kind):
    """Spatially varying D (non-uniform gap, build_variable_diffusion_laplacian): tiled path vs oracle ADI and per-line kernels."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    if kind == "full":
        from qpsim_amd.geometry import extract_edge_segments
        from qpsim_amd.models import BoundaryCondition
        rng = np.random.default_rng(3)
        mask = np.ones((130, 200), dtype=bool)
        edges = extract_edge_segments(mask)
        side_bc = {"left": BoundaryCondition("dirichlet", 0.7), "right": BoundaryCondition("robin", 0.4, 0.2),
                   "up": BoundaryCondition("neumann", -0.3), "down": BoundaryCondition("absorbing")}
        bcs = {e.edge_id: side_bc[e.normal] for e in edges}
    else:
        rng, mask, edges, bcs = _masked_problem(kind, 17)
    dx, dt, B = 0.9, 0.11, 3
    eng = Engine(compile_geometry(mask, edges, bcs, dx))
    n = int(mask.sum())
    u0 = rng.random((B, n))
    Dp = 0.2 + 5.8 * rng.random((B, n))
    Dp[2] *= 0.05                                   # a nearly frozen bin (D -> 0 towards the gap edge)
    dfull = np.zeros((B, mask.size))
    dfull[:, mask.reshape(-1)] = Dp
    fast = DiffusionOperator(eng, B, dt, dfield=dfull)
    slow = DiffusionOperator(eng, B, dt, dfield=dfull, allow_fast=False)
    assert fast.rect is None and fast.tile is not None, fast.tile_refused
    assert fast.tile.tile_counts["clean"] == 0 and slow.tile is None
    ops = O.build_grid_ops(mask, edges, bcs, dx)
    for nsteps in (1, 3):
        a, b = eng.upload_packed(u0), eng.upload_packed(u0)
        eng.adi_steps(fast, a, nsteps)
        eng.adi_steps(slow, b, nsteps)
        ha, hb = eng.download_packed(a), eng.download_packed(b)
        assert rel_err(ha, hb) < 2e-13, nsteps
        assert np.all(a.detach().cpu().numpy()[:, ~mask.reshape(-1)] == 0.0)
        for k in range(B):
            Dg = np.zeros(mask.shape)
            Dg[mask] = Dp[k]
            st = O.ADIStepper(ops, Dg, dt)
            want = u0[k].copy()
            for _ in range(nsteps):
                want = st.step(want)
            assert rel_err(ha[k], want) < 2e-13, (k, nsteps)
    # exact-CN with the tiled preconditioner vs SuperLU on the variable-D operator
    v = eng.upload_packed(u0)
    its = eng.cn_exact_step(fast, v)
    got = eng.download_packed(v)
    for k in range(B):
        Dg = np.zeros(mask.shape)
        Dg[mask] = Dp[k]
        assert rel_err(got[k], O.CNStepper(ops, Dg, dt).step(u0[k])) < 1e-11
    assert its < 200


def test_solver_runs_from_a_worker_thread_like_the_gui():
    """ui/main_app.py:1937-1968 calls the solver from a daemon thread with a progress callback: same result as on the main
    thread, callback invoked at t = 0 and at every stored step on that worker thread."""
    import threading
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    from qpsim_amd.solver import run_2d_crank_nicolson
    mask = _donut(40, 48, 18.0, 6.0)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    init = np.where(mask, 1e-4 * (1 + np.random.default_rng(2).random(mask.shape)), 0.0)
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1,
              total_time=1.0, dx=1.0, store_every=5, energy_gap=180.0, energy_max_factor=3.0, num_energy_bins=8,
              enable_recombination=True, enable_scattering=True)
    ref = run_2d_crank_nicolson(**kw)
    seen, box = [], {}

    def work():
        box["out"] = run_2d_crank_nicolson(**kw, progress_callback=lambda t, f: seen.append((t, threading.get_ident())))

    th = threading.Thread(target=work, daemon=True)
    th.start()
    th.join(120)
    assert not th.is_alive() and "out" in box
    assert [t for t, _ in seen] == pytest.approx(ref[0]) and {tid for _, tid in seen} == {th.ident}
    assert np.array_equal(np.stack(box["out"][1]), np.stack(ref[1]), equal_nan=True)
    assert box["out"][2] == ref[2]


@pytest.mark.parametrize("seed", range(15))
def test_tiled_paths_agree_with_per_line_kernels_on_random_geometries(seed):
    """Differential fuzz: random masks (noise, blobs, necks exactly on tile boundaries, boxes with holes, ellipses), random
    per-edge boundary conditions, grid sizes, dx, dt, uniform or per-cell D: tiled path vs one-thread-per-line kernels."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 0.4), BoundaryCondition("absorbing"),
             BoundaryCondition("neumann", -0.05), BoundaryCondition("robin", 0.5, 0.1)]
    rng = np.random.default_rng(1000 + seed)
    ny, nx = int(rng.integers(1, 200)), int(rng.integers(1, 260))
    style = seed % 5
    if style == 0:
        mask = rng.random((ny, nx)) > rng.uniform(0.02, 0.4)
    elif style == 1:
        f = rng.standard_normal((ny, nx))
        for _ in range(6):
            f = (f + np.roll(f, 1, 0) + np.roll(f, -1, 0) + np.roll(f, 1, 1) + np.roll(f, -1, 1)) / 5
        mask = f > np.quantile(f, 0.3)
    elif style == 2:
        mask = np.ones((ny, nx), dtype=bool)
        mask[:, 63::64] = rng.random((ny, len(range(63, nx, 64)))) > 0.7
        mask[64::64, :] = rng.random((len(range(64, ny, 64)), nx)) > 0.5
    elif style == 3:
        mask = np.ones((ny, nx), dtype=bool)
        for _ in range(int(rng.integers(1, 6))):
            j, i = int(rng.integers(0, ny)), int(rng.integers(0, nx))
            mask[j:j + int(rng.integers(1, 40)), i:i + int(rng.integers(1, 40))] = False
    else:
        y, x = np.indices((ny, nx))
        mask = np.hypot((y - ny / 2) / ny, (x - nx / 2) / nx) < rng.uniform(0.2, 0.6)
    if not mask.any():
        mask[ny // 2, nx // 2] = True
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: kinds[int(rng.integers(0, 5))] for e in edges}
    dx, dt = float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.02, 0.2))
    eng = Engine(compile_geometry(mask, edges, bcs, dx))
    n, B = int(mask.sum()), 2
    u0 = rng.random((B, n))
    if seed % 3 == 0:
        d = np.zeros((B, mask.size))
        d[:, mask.reshape(-1)] = rng.uniform(0.01, 6.0, size=(B, n))
        fast, slow = DiffusionOperator(eng, B, dt, dfield=d), DiffusionOperator(eng, B, dt, dfield=d, allow_fast=False)
    else:
        Dc = [float(rng.uniform(0.1, 6.0)), float(rng.uniform(0.0, 1.0))]
        fast, slow = DiffusionOperator(eng, B, dt, dcoef=Dc), DiffusionOperator(eng, B, dt, dcoef=Dc, allow_fast=False)
    assert fast.rect is not None or fast.tile is not None, fast.tile_refused
    a, b = eng.upload_packed(u0), eng.upload_packed(u0)
    k = int(rng.integers(1, 5))
    eng.adi_steps(fast, a, k)
    eng.adi_steps(slow, b, k)
    assert rel_err(eng.download_packed(a), eng.download_packed(b)) < 5e-13


@pytest.mark.parametrize("ne,fmax", [(6, 3.0), (12, 3.0), (12, 5.0), (16, 10.0), (24, 3.0), (30, 3.0), (32, 3.0), (40, 5.0),
                                     (50, 10.0)])
@pytest.mark.parametrize("en_r,en_s,upd", PROCESS_COMBOS)
def test_register_collision_kernel_with_gap_classes(O, ne, fmax, en_r, en_s, upd):
    """Non-uniform gap (per-pixel K_r0_all / K_s0_all / rho_all of solver.py:1203-1232): the register kernel forms K per
    pixel from the gap-independent amplitude tables; checked against the wave and generic kernels (per-class tables) and
    the oracle."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    rng = np.random.default_rng(ne * 17 + int(en_r) + 2 * int(en_s))
    mask = rng.random((9, 31)) > 0.2
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    n = int(mask.sum())
    gaps = np.array([180.0, 171.0, 165.5, 176.25])
    E, dE = T.build_energy_grid(180.0, 1.0, fmax, ne)          # energy grid of the run; every class gap lies at or below it
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in gaps])
    kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in gaps])
    ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in gaps])
    cls = rng.integers(0, gaps.size, size=n)
    state = rng.random((ne, n)) * rho[cls].T * rng.choice([1e-5, 1e-2, 0.5, 0.9], size=n)[None, :]
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    params = dict(E=E, gaps=gaps, tau_r=500.0, tau_s=400.0, T_c=1.2)
    outs = {}
    for kern in ("auto", "wave", "generic"):
        tab = eng.make_collision_tables(kr, ks, rho, idx_d, idx_s, sg, cls, kernel=kern, gap_params=params)
        assert tab["kernel"] == ("register" if kern == "auto" else kern)
        s_in, p_dev = eng.upload_packed(state), eng.upload_packed(ph)
        s_out = eng.empty(ne, eng.ncell)
        eng.collide(tab, s_in, s_out, p_dev, dE, 0.37, en_r, en_s, upd)
        outs[kern] = (eng.download_packed(s_out), eng.download_packed(p_dev))
    for other in ("wave", "generic"):
        assert rel_err(outs["auto"][0], outs[other][0]) < 1e-12
        assert rel_err(outs["auto"][1], outs[other][1]) < (1e-11 if ne <= 16 else PHONON_TOL)
    tables = {"rho": rho, "Kr0": kr if en_r else None, "Ks0": ks if en_s else None, "cls": cls, "idx_diff": idx_d,
              "idx_sum": idx_s, "sign": sg, "dE": dE}
    s_ref, p_ref = state.copy(), ph.copy()
    O.collision_step(s_ref, p_ref, tables, 0.37, en_r=en_r, en_s=en_s, update_phonons=upd)
    assert rel_err(outs["auto"][0], s_ref) < (2e-11 if ne <= 16 else 1e-10)
    assert rel_err(outs["auto"][1], p_ref) < (2e-11 if ne <= 16 else PHONON_TOL)
    # without the separable tables gap classes stay on the wave kernel
    assert eng.make_collision_tables(kr, ks, rho, idx_d, idx_s, sg, cls)["kernel"] == "wave"


def test_full_size_4096_adi_is_linear_and_conservative():
    """BASELINE headline size, properties that need no oracle: the step is linear in the field (zero boundary sources) and
    conserves the integral under reflective walls; both tiled sweeps, carried over 3 steps."""
    import torch
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    N = 4096
    mask = np.ones((N, N), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    eng = Engine(compile_geometry(mask, edges, bcs, 1.0))
    op = DiffusionOperator(eng, 3, 0.1, dcoef=[6.0, 6.0, 6.0])
    assert op.rect is not None
    g = torch.Generator(device=eng.device).manual_seed(7)
    u = torch.rand((1, N * N), dtype=torch.float64, device=eng.device, generator=g)
    v = torch.rand((1, N * N), dtype=torch.float64, device=eng.device, generator=g)
    a, b = 0.37, -1.9
    planes = torch.cat([u, v, a * u + b * v])
    before = planes.sum(dim=1)
    eng.adi_steps(op, planes, 3)
    after = planes.sum(dim=1)
    assert float(((after - before).abs() / before.abs()).max()) < 1e-12
    lin = (planes[2] - (a * planes[0] + b * planes[1])).abs().max() / planes[2].abs().max()
    assert float(lin) < 1e-13
    assert float(planes[0].min()) >= 0.0 and float(planes[0].max()) <= 1.0      # maximum principle, r D = 0.3


def test_large_collision_update_is_pixel_local():
    """2048^2 pixels, NE = 12, full physics: the update of a pixel depends on that pixel only - permuting the pixels
    permutes the result (register kernel, planes of 4.2 M cells)."""
    import torch
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    N = 2048
    mask = np.ones((1, N * N), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    ne = 12
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = T.dynes_density_of_states(E, 180.0, 0.0)
    tab = eng.make_collision_tables(T.recombination_kernel_base(E, 180.0, 440.0, 1.2)[None],
                                    T.scattering_kernel_base(E, 180.0, 440.0, 1.2)[None], rho[None], idx_d, idx_s, sg)
    assert tab["kernel"] == "register"
    g = torch.Generator(device=eng.device).manual_seed(3)
    dev = eng.device
    occ = torch.rand((1, N * N), dtype=torch.float64, device=dev, generator=g) * 0.6
    state = torch.as_tensor(rho, device=dev)[:, None] * occ
    ph = torch.as_tensor(T.thermal_phonon_occupation(om, 0.2), device=dev)[:, None] * (
        0.5 + torch.rand((om.size, N * N), dtype=torch.float64, device=dev, generator=g))
    perm = torch.randperm(N * N, device=dev, generator=g)
    out1, ph1 = torch.empty_like(state), ph.clone()
    eng.collide(tab, state, out1, ph1, dE, 0.05, True, True, True)
    state_p, ph_p = state[:, perm].contiguous(), ph[:, perm].contiguous()
    out2 = torch.empty_like(state)
    eng.collide(tab, state_p, out2, ph_p, dE, 0.05, True, True, True)
    assert torch.equal(out2, out1[:, perm]) and torch.equal(ph_p, ph1[:, perm])
    assert float(out1.min()) >= 0.0 and float(ph1.min()) >= 0.0
