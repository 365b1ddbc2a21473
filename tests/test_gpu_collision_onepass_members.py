"""Ensemble parameter sweeps at NE = 30, 32, 40, 50 on the GPU: the one-pass collision kernel staging per-member tables
(QP_COLL_MEMBER_CLASSES, a member's cell count a multiple of 256) against one call per member with that member's single
table, against the CPU oracle, the unchanged class-map fallback, and ``run_2d_crank_nicolson_ensemble(sweep=...)`` at these
sizes against lone ``run_2d_crank_nicolson`` calls.  Set-up as in tests/test_gpu_ensemble_sweep.py."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest

from collision_grids import MERGED_FMAX, unmerged_fmax
from test_gpu_ensemble_sweep import (ADI_TOL, FLOOR, MEMBER_PHYSICS, PROCESSES, SWEEP, _assert_contract, _common, _lone,
                                     _rect_problem, _rel, _sweep_members, rel_err)

pytestmark = pytest.mark.gpu

ONEPASS_NE = [30, 32, 40, 50]
# cells per member -> grid.  256: every neighbouring block of the kernel belongs to another member; 512: two blocks per
# member, so block -> member is a real division; 320: blocks would straddle members (the fallback)
SHAPES = {256: (16, 16), 512: (16, 32), 320: (16, 20)}
MEMBER_SHAPES = [(ne, ncm) for ne in ONEPASS_NE for ncm in (256, 512)]
DT = 0.37
STATE_TOL, PHONON_TOL = 1e-12, 1e-10      # the bounds of tests/test_gpu_ensemble_sweep.py above NE = 16, of the largest value


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def lib():
    from qpsim_amd import _hip
    return _hip.load()


_SETUPS: dict = {}


def _setup(ne, ncm, fmax=None):
    """Engine of one member's grid, the member-class tables of three members, each member's lone table, and inputs laid out
    [bin][member][cell], seeded per shape and built once.  Inactive: the last wave of member 0, the last 256-cell block of
    member 1 (all of member 1 at 256 cells), and single lanes on both sides of the member boundaries."""
    fmax = unmerged_fmax(ne) if fmax is None else fmax
    key = (ne, ncm, fmax)
    if key in _SETUPS:
        return _SETUPS[key]
    import torch
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    M = len(MEMBER_PHYSICS)
    mask = np.ones(SHAPES[ncm], dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    assert eng.ncell == ncm
    E, dE = T.build_energy_grid(180.0, 1.0, fmax, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, 180.0, g) for g, _, _, _ in MEMBER_PHYSICS])
    kr = np.stack([T.recombination_kernel_base(E, 180.0, tr, tc) for _, tr, _, tc in MEMBER_PHYSICS])
    ks = np.stack([T.scattering_kernel_base(E, 180.0, ts, tc) for _, _, ts, tc in MEMBER_PHYSICS])
    assert not np.array_equal(rho[0], rho[1]) and not np.array_equal(kr[1], kr[2]) and not np.array_equal(ks[0], ks[2])
    tab = eng.make_collision_tables(kr, ks, rho, idx_d, idx_s, sg, None, members=M, member_classes=True)
    lone = [eng.make_collision_tables(kr[m][None], ks[m][None], rho[m][None], idx_d, idx_s, sg) for m in range(M)]
    rng = np.random.default_rng(1000 * ne + ncm)
    n = M * ncm
    level = rng.choice([1e-5, 1e-2, 0.5, 0.95], size=n)
    state = rng.random((ne, n)) * np.repeat(rho.T, ncm, axis=1) * level[None, :] + 1e-12
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    flags = np.where(rng.random(n) < 0.9, 16, 0).astype(np.uint8)
    flags[ncm - 64:ncm] = 0                        # one whole wave: the last of member 0
    flags[2 * ncm - 256:2 * ncm] = 0               # one whole 256-cell block: the last of member 1
    flags[ncm - 65] = 16
    flags[ncm] = 0                                 # lane 0 of member 1's first wave
    flags[2 * ncm] = 0                             # lane 0 of member 2's first wave ...
    flags[2 * ncm + 1] = 16                        # ... next to an active one
    flags[n - 1] = 0
    flags[n - 2] = 16
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")          # noqa: E731
    out = dict(eng=eng, tab=tab, lone=lone, dE=float(dE), nw=om.size, M=M, ncm=ncm, ne=ne, state=d(state), ph=d(ph),
               flags=d(flags), rho=rho, kr=kr, ks=ks, maps=(idx_d, idx_s, sg), state_host=state, ph_host=ph,
               flags_host=flags)
    _SETUPS[key] = out
    return out


_LONE: dict = {}


def _lone_step(s, en_r, en_s, upd, guarded=False, fmax=None):
    """One qp_collision_step(_guarded) call per member on its slice with its single table: (state, phonons, guards);
    computed once per case and shared."""
    key = (s["ne"], s["ncm"], fmax, en_r, en_s, upd, guarded)
    if key in _LONE:
        return _LONE[key]
    eng, ncm = s["eng"], s["ncm"]
    outs, phs, guards = [], [], []
    for m in range(s["M"]):
        sl = slice(m * ncm, (m + 1) * ncm)
        si, pi, fl = (a[..., sl].contiguous() for a in (s["state"], s["ph"], s["flags"]))
        so = eng.torch.full_like(si, -7.0)
        if guarded:
            guards.append(eng.pauli_stats_result(eng.collide_guarded(s["lone"][m], si, so, pi, s["dE"], DT, en_r, en_s, upd,
                                                                     FLOOR, ncell=ncm, flags=fl)))
        else:
            eng.collide(s["lone"][m], si, so, pi, s["dE"], DT, en_r, en_s, upd, ncell=ncm, flags=fl)
        outs.append(so.cpu().numpy())
        phs.append(pi.cpu().numpy())
    assert outs[0].shape == (s["ne"], ncm)
    _LONE[key] = np.concatenate(outs, axis=1), np.concatenate(phs, axis=1), guards
    return _LONE[key]


def _route(lib, tab, ncell, en_r, en_s, upd):
    scratch = int(bool(tab["merged_slots"]))
    return lib.qp_collision_route(C.byref(tab["struct"]), ncell, int(en_r), int(en_s), int(upd), scratch)


def _assert_one_pass_members(lib, s, en_r, en_s, upd):
    """Both sides of the comparison run the one-pass kernel: the member tables and every member's lone table."""
    from qpsim_amd import _hip
    ne, ncm, M = s["ne"], s["ncm"], s["M"]
    tab = s["tab"]
    assert tab["kernel"] == "register" and not tab["pair"]
    assert tab["struct"].flags & 8 and tab["nclass"] == M == 3
    assert tuple(tab["ks0_diag"].shape) == (3, ne, ne) and tuple(tab["kr0_anti2"].shape) == (3, 2 * ne - 1, ne)
    assert _route(lib, tab, M * ncm, en_r, en_s, upd) == _hip.ROUTE_ONEPASS
    for lone in s["lone"]:
        assert _route(lib, lone, ncm, en_r, en_s, upd) == _hip.ROUTE_ONEPASS


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("upd", [True, False])
@pytest.mark.parametrize("en_r,en_s", PROCESSES)
@pytest.mark.parametrize("ne,ncm", MEMBER_SHAPES)
def test_member_table_one_pass_step_is_bit_equal_to_lone_table_calls(torch, lib, ne, ncm, en_r, en_s, upd):
    s = _setup(ne, ncm)
    _assert_one_pass_members(lib, s, en_r, en_s, upd)
    eng, n = s["eng"], s["M"] * ncm
    want_s, want_p, _ = _lone_step(s, en_r, en_s, upd)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(s["tab"], s["state"], out, ph, s["dE"], DT, en_r, en_s, upd, ncell=n, flags=s["flags"])
    assert np.array_equal(out.cpu().numpy(), want_s)
    assert np.array_equal(ph.cpu().numpy(), want_p)
    if not upd:
        assert np.array_equal(want_p, s["ph_host"])
    inactive = s["flags_host"] == 0
    assert np.array_equal(want_s[:, inactive], s["state_host"][:, inactive])
    assert np.array_equal(want_p[:, inactive], s["ph_host"][:, inactive])
    assert not np.array_equal(want_s[:, ~inactive], s["state_host"][:, ~inactive])
    assert inactive[ncm - 64:ncm].all() and inactive[2 * ncm - 256:2 * ncm].all() and not inactive[2 * ncm + 1]


@pytest.mark.parametrize("upd", [True, False])
@pytest.mark.parametrize("en_r,en_s", PROCESSES)
@pytest.mark.parametrize("ne,ncm", MEMBER_SHAPES)
def test_member_table_one_pass_guarded_step_gives_the_lone_guards(torch, lib, ne, ncm, en_r, en_s, upd):
    """The one-pass kernels write no guard partials: the per-member statistics pass follows, over bit-equal states."""
    s = _setup(ne, ncm)
    _assert_one_pass_members(lib, s, en_r, en_s, upd)
    eng = s["eng"]
    want_s, want_p, want_g = _lone_step(s, en_r, en_s, upd, guarded=True)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    got_g = eng.pauli_stats_members_result(eng.collide_guarded_members(s["tab"], s["state"], out, ph, s["dE"], DT, en_r, en_s,
                                                                       upd, FLOOR, ncm, s["M"], s["flags"]))
    assert np.array_equal(out.cpu().numpy(), want_s)
    assert np.array_equal(ph.cpu().numpy(), want_p)
    assert got_g == want_g


@pytest.mark.parametrize("ne", [50, 32])
def test_member_table_one_pass_step_matches_the_cpu_oracle(torch, lib, ne):
    from oracle import qp_oracle as O
    ncm = 256
    s = _setup(ne, ncm)
    _assert_one_pass_members(lib, s, True, True, True)
    eng, n = s["eng"], s["M"] * ncm
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(s["tab"], s["state"], out, ph, s["dE"], DT, True, True, True, ncell=n, flags=s["flags"])
    got_s, got_p = out.cpu().numpy(), ph.cpu().numpy()
    idx_d, idx_s, sg = s["maps"]
    active = s["flags_host"] != 0
    checked = 0
    for m in range(s["M"]):
        px = np.nonzero(active[m * ncm:(m + 1) * ncm])[0] + m * ncm
        if px.size == 0:                          # member 1 at 256 cells: its one block is the inactive one
            assert m == 1
            continue
        tables = {"rho": s["rho"][m][None], "Kr0": s["kr"][m][None], "Ks0": s["ks"][m][None], "cls": np.zeros(px.size, dtype=int),
                  "idx_diff": idx_d, "idx_sum": idx_s, "sign": sg, "dE": s["dE"]}
        s_ref, p_ref = s["state_host"][:, px].copy(), s["ph_host"][:, px].copy()
        O.collision_step(s_ref, p_ref, tables, DT, en_r=True, en_s=True, update_phonons=True)
        es, ep = rel_err(got_s[:, px], s_ref), rel_err(got_p[:, px], p_ref)
        print(f"ne={ne} member {m}: state {es:.3e} phonons {ep:.3e}")
        assert es < STATE_TOL and ep < PHONON_TOL
        checked += 1
    assert checked == 2


def test_member_table_one_pass_step_with_merged_phonon_bins(torch, lib):
    """Merged bins (QP_COLL_SHARED_BINS, the grid of tests/collision_grids.py for NE = 30): phase 2 parks the diagonal's sums
    in the stash, addressed by the global cell, exactly as with one table."""
    s = _setup(30, 256, fmax=MERGED_FMAX[30])
    assert s["tab"]["merged_slots"] > 0 and s["tab"]["struct"].flags & 4
    _assert_one_pass_members(lib, s, True, True, True)
    eng, n = s["eng"], s["M"] * 256
    want_s, want_p, _ = _lone_step(s, True, True, True, fmax=MERGED_FMAX[30])
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(s["tab"], s["state"], out, ph, s["dE"], DT, True, True, True, ncell=n, flags=s["flags"])
    assert np.array_equal(out.cpu().numpy(), want_s) and np.array_equal(ph.cpu().numpy(), want_p)
    assert not np.array_equal(want_p, s["ph_host"])


# ------------------------------------------------------------------------------------------------ fallback
def test_members_that_straddle_blocks_keep_the_class_map_kernel(torch, lib):
    """320 cells per member: the second 256-cell block would hold cells of two members."""
    from qpsim_amd import _hip
    ne, ncm = 50, 320
    s = _setup(ne, ncm)
    eng, n = s["eng"], s["M"] * ncm
    assert s["tab"]["kernel"] == "wave" and s["tab"]["ks0_diag"] is None and s["tab"]["kr0_anti2"] is None
    assert _route(lib, s["tab"], n, True, True, True) == _hip.ROUTE_WAVE
    want_s, want_p, _ = _lone_step(s, True, True, True)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(s["tab"], s["state"], out, ph, s["dE"], DT, True, True, True, ncell=n, flags=s["flags"])
    es, ep = rel_err(out.cpu().numpy(), want_s), rel_err(ph.cpu().numpy(), want_p)
    print(f"ne={ne} ncm={ncm}: state {es:.3e} phonons {ep:.3e}")
    assert es < STATE_TOL and ep < PHONON_TOL


# ------------------------------------------------------------------------------------------------ API
@pytest.mark.parametrize("ne", [50, 32])
def test_swept_ensemble_at_one_pass_sizes_matches_lone_runs(ne):
    from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble
    ny, nx = 16, 16
    mask, edges, bcs = _rect_problem(ny, nx)
    common = _common(mask, edges, bcs, ne=ne, scheme="adi", total_time=0.6, store_every=3)
    members = _sweep_members(ny, nx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=SWEEP, **common)
    stats = last_run_stats()
    assert stats["batches"] == 1 and stats["pair_passes"] == 0
    for m, mem in enumerate(members):
        want, ph = _lone(common, mem, SWEEP, m)
        assert ph and mem["phonon_history_out"]
        _assert_contract(got[m], want, ADI_TOL, mem["phonon_history_out"], ph)
    # the members really differ through the sweep alone
    same_field = [dict(members[0], phonon_history_out=None) for _ in members]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        swept = run_2d_crank_nicolson_ensemble(same_field, sweep=SWEEP, **common)
    assert _rel(np.stack(swept[1][1]), np.stack(swept[0][1])) > 1e-6


@pytest.mark.parametrize("ne", [50, 32])
def test_solver_member_tables_take_the_one_pass_route(lib, ne):
    from qpsim_amd import _hip, solver as S, tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((16, 16), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    E, _ = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    _, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    params = [(g, t, t, tc) for t, tc, g in zip(SWEEP["tau_0"], SWEEP["T_c"], SWEEP["dynes_gamma"])]
    tab, rho = S._collision_tables(eng, E, 180.0, None, 256, 0.0, 440.0, 440.0, 1.2, True, True, idx_d, idx_s, sg,
                                   members=4, member_params=params)
    assert rho.shape == (4, ne) and tab["kernel"] == "register" and tuple(tab["ks0_diag"].shape) == (4, ne, ne)
    assert _route(lib, tab, 4 * 256, True, True, True) == _hip.ROUTE_ONEPASS
