"""Ensemble parameter sweeps on the GPU: the register collision kernels reading per-member tables (QP_COLL_MEMBER_CLASSES)
against one call per member with that member's single table, the class-map fallback, and
``run_2d_crank_nicolson_ensemble(sweep=...)`` against lone ``run_2d_crank_nicolson`` calls."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest

from collision_grids import unmerged_fmax
from test_collision_route_host import AVAILABLE

pytestmark = pytest.mark.gpu

ADI_TOL, CN_TOL = 2e-13, 1e-12          # the ensemble contract (tests/test_gpu_ensemble.py)
FLOOR = 1e-18
# (dynes_gamma, tau_r, tau_s, T_c) of the three members of the kernel tests: every table differs between members
MEMBER_PHYSICS = [(0.0, 440.0, 440.0, 1.2), (0.1, 300.0, 520.0, 1.0), (0.4, 650.0, 250.0, 1.5)]
PROCESSES = [(True, True), (True, False), (False, True)]       # (recombination, scattering)
SHAPES = {40: (4, 10), 64: (4, 16), 100: (4, 25), 128: (8, 16), 192: (12, 16)}
# (ne, cells per member) of the kernel tests: every size of QP_MEMBER_NE_LIST at 192 cells (three waves per member, so the
# 128-thread blocks straddle members), three of them also at one and two waves per member
MEMBER_NE = AVAILABLE["qp_collision_member_tables_available"]
MEMBER_SHAPES = [(ne, ncm) for ne in MEMBER_NE for ncm in ((64, 128, 192) if ne in (4, 12, 16) else (192,))]
assert {4, 7, 9, 12, 13, 16} <= set(MEMBER_NE)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def lib():
    from qpsim_amd import _hip
    return _hip.load()


def _p(t):
    return 0 if t is None else int(t.data_ptr())


def _stream(torch):
    return int(torch.cuda.current_stream().cuda_stream)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ------------------------------------------------------------------------------------------------ kernels
_SETUPS: dict = {}


def _setup(ne, ncm, fmax=None):
    """Engine of one member's grid, the member-class tables of three members, each member's lone table, and inputs laid out
    [bin][member][cell] (built once per shape).  Default grid: the unmerged one of tests/collision_grids.py."""
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
    flags[ncm - min(ncm, 64):ncm] = 0              # one whole wave of member 0 is inactive (all of it when ncm = 64)
    flags[ncm] = 0                                 # lane 0 of member 1's first wave
    flags[ncm + 1] = 16
    flags[2 * ncm] = 16
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")          # noqa: E731
    out = dict(eng=eng, tab=tab, lone=lone, dE=float(dE), nw=om.size, M=M, ncm=ncm, ne=ne, state=d(state), ph=d(ph),
               flags=d(flags), rho=rho, kr=kr, ks=ks, maps=(idx_d, idx_s, sg), state_host=state, ph_host=ph,
               flags_host=flags)
    _SETUPS[key] = out
    return out


def _member(s, m, *arrays):
    sl = slice(m * s["ncm"], (m + 1) * s["ncm"])
    return [a[..., sl].contiguous() for a in arrays]


def _lone_step(s, dt, en_r, en_s, upd, guarded=False):
    """One qp_collision_step(_guarded) call per member on its slice with its single table: (state, phonons, guards)."""
    eng, ne = s["eng"], s["ne"]
    outs, phs, guards = [], [], []
    for m in range(s["M"]):
        si, pi, fl = _member(s, m, s["state"], s["ph"], s["flags"])
        so = s["eng"].torch.full_like(si, -7.0)
        if guarded:
            guards.append(eng.pauli_stats_result(eng.collide_guarded(s["lone"][m], si, so, pi, s["dE"], dt, en_r, en_s, upd,
                                                                     FLOOR, ncell=s["ncm"], flags=fl)))
        else:
            eng.collide(s["lone"][m], si, so, pi, s["dE"], dt, en_r, en_s, upd, ncell=s["ncm"], flags=fl)
        outs.append(so.cpu().numpy())
        phs.append(pi.cpu().numpy())
    assert outs[0].shape == (ne, s["ncm"])
    return np.concatenate(outs, axis=1), np.concatenate(phs, axis=1), guards


@pytest.mark.parametrize("upd", [True, False])
@pytest.mark.parametrize("en_r,en_s", PROCESSES)
@pytest.mark.parametrize("ne,ncm", MEMBER_SHAPES)
def test_member_table_step_is_bit_equal_to_lone_table_calls(torch, lib, ne, ncm, en_r, en_s, upd):
    """ncm = 64 / 192: 128-thread blocks hold waves of two members, and at 3 x 64 cells the last block's second wave lies
    beyond the grid."""
    from qpsim_amd import _hip
    s = _setup(ne, ncm)
    assert lib.qp_collision_member_tables_available(ne) == 1 and s["tab"]["kernel"] == "register"
    assert s["tab"]["struct"].flags & 8 and s["tab"]["nclass"] == 3
    eng, n = s["eng"], s["M"] * ncm
    assert lib.qp_collision_route(C.byref(s["tab"]["struct"]), n, int(en_r), int(en_s), int(upd), 0) == _hip.ROUTE_REGISTER_MEMBERS
    for lone in s["lone"]:
        assert lib.qp_collision_route(C.byref(lone["struct"]), ncm, int(en_r), int(en_s), int(upd), 0) == _hip.ROUTE_REGISTER
    want_s, want_p, _ = _lone_step(s, 0.37, en_r, en_s, upd)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(s["tab"], s["state"], out, ph, s["dE"], 0.37, en_r, en_s, upd, ncell=n, flags=s["flags"])
    assert np.array_equal(out.cpu().numpy(), want_s)
    assert np.array_equal(ph.cpu().numpy(), want_p)
    if not upd:
        assert np.array_equal(want_p, s["ph_host"])
    inactive = s["flags_host"] == 0
    assert np.array_equal(want_s[:, inactive], s["state_host"][:, inactive])
    assert not np.array_equal(want_s[:, ~inactive], s["state_host"][:, ~inactive])


@pytest.mark.parametrize("upd", [True, False])
@pytest.mark.parametrize("en_r,en_s", PROCESSES)
@pytest.mark.parametrize("ne,ncm", MEMBER_SHAPES)
def test_member_table_guarded_step_is_bit_equal_with_per_member_guards(torch, lib, ne, ncm, en_r, en_s, upd):
    s = _setup(ne, ncm)
    eng = s["eng"]
    want_s, want_p, want_g = _lone_step(s, 0.37, en_r, en_s, upd, guarded=True)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    got_g = eng.pauli_stats_members_result(eng.collide_guarded_members(s["tab"], s["state"], out, ph, s["dE"], 0.37, en_r, en_s,
                                                                       upd, FLOOR, ncm, s["M"], s["flags"]))
    assert np.array_equal(out.cpu().numpy(), want_s)
    assert np.array_equal(ph.cpu().numpy(), want_p)
    assert got_g == want_g


@pytest.mark.parametrize("upd", [True, False])
@pytest.mark.parametrize("en_r,en_s", PROCESSES)
@pytest.mark.parametrize("ne,ncm", MEMBER_SHAPES)
def test_member_table_double_step_is_bit_equal_to_the_two_call_sequence(torch, lib, ne, ncm, en_r, en_s, upd):
    """qp_collision_double_step_guarded_members with member tables against, per member and with its single table,
    qp_collision_step_guarded(dt_first); += gen_amount on interior cells; qp_collision_step(dt_second)."""
    s = _setup(ne, ncm)
    eng, M = s["eng"], s["M"]
    assert eng.pair_members_supported(s["tab"], ncm, M)
    dt_a, dt_b, gen = 0.05, 0.07, 1e-6
    want_s, want_p, want_g = [], [], []
    for m in range(M):
        si, pi, fl = _member(s, m, s["state"], s["ph"], s["flags"])
        tmp, so = torch.full_like(si, -7.0), torch.full_like(si, -7.0)
        want_g.append(eng.pauli_stats_result(eng.collide_guarded(s["lone"][m], si, tmp, pi, s["dE"], dt_a, en_r, en_s, upd,
                                                                 FLOOR, ncell=ncm, flags=fl)))
        assert lib.qp_add_constant(_p(fl), ncm, ne, _p(tmp), gen, _stream(torch)) == 0
        eng.collide(s["lone"][m], tmp, so, pi, s["dE"], dt_b, en_r, en_s, upd, ncell=ncm, flags=fl)
        want_s.append(so.cpu().numpy())
        want_p.append(pi.cpu().numpy())
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    got_g = eng.pauli_stats_members_result(eng.collide_pair_guarded_members(
        s["tab"], s["state"], out, ph, s["dE"], dt_a, dt_b, gen, en_r, en_s, upd, FLOOR, ncm, M, s["flags"]))
    assert np.array_equal(out.cpu().numpy(), np.concatenate(want_s, axis=1))
    assert np.array_equal(ph.cpu().numpy(), np.concatenate(want_p, axis=1))
    assert got_g == want_g


def test_member_table_step_with_merged_phonon_bins(torch, lib):
    """Merged bins (QP_COLL_SHARED_BINS): the single-pass kernel parks the diagonal's sums in scratch exactly as with one
    table; the double half-step call has no kernel for them."""
    s = _setup(12, 64, fmax=5.0)
    assert s["tab"]["merged_slots"] > 0 and not s["tab"]["pair"]
    eng, n = s["eng"], s["M"] * 64
    want_s, want_p, _ = _lone_step(s, 0.37, True, True, True)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(s["tab"], s["state"], out, ph, s["dE"], 0.37, True, True, True, ncell=n, flags=s["flags"])
    assert np.array_equal(out.cpu().numpy(), want_s) and np.array_equal(ph.cpu().numpy(), want_p)


@pytest.mark.parametrize("ne", [4, 7, 9, 13, 16])
def test_member_table_step_matches_the_cpu_oracle(torch, ne):
    from oracle import qp_oracle as O
    s = _setup(ne, 128)
    eng, n = s["eng"], s["M"] * 128
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(s["tab"], s["state"], out, ph, s["dE"], 0.37, True, True, True, ncell=n, flags=s["flags"])
    got_s, got_p = out.cpu().numpy(), ph.cpu().numpy()
    idx_d, idx_s, sg = s["maps"]
    active = s["flags_host"] != 0
    for m in range(s["M"]):
        px = np.nonzero(active[m * 128:(m + 1) * 128])[0] + m * 128
        tables = {"rho": s["rho"][m][None], "Kr0": s["kr"][m][None], "Ks0": s["ks"][m][None], "cls": np.zeros(px.size, dtype=int),
                  "idx_diff": idx_d, "idx_sum": idx_s, "sign": sg, "dE": s["dE"]}
        s_ref, p_ref = s["state_host"][:, px].copy(), s["ph_host"][:, px].copy()
        O.collision_step(s_ref, p_ref, tables, 0.37, en_r=True, en_s=True, update_phonons=True)
        es, ep = rel_err(got_s[:, px], s_ref), rel_err(got_p[:, px], p_ref)
        print(f"ne={ne} member {m}: state {es:.3e} phonons {ep:.3e}")
        assert es < 2e-11 and ep < 1e-11


# ------------------------------------------------------------------------------------------------ fallback routing
def _double_step_rc(torch, lib, s, struct, ncell=None, ncm=None):
    n = s["M"] * s["ncm"] if ncell is None else ncell
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(s["M"], dtype=torch.float64, device="cuda")
    idx = torch.zeros(2 * s["M"], dtype=torch.int64, device="cuda")
    out = torch.full_like(s["state"], -7.0)
    rc = lib.qp_collision_double_step_guarded_members(C.byref(struct), _p(s["flags"]), n, _p(s["state"]), _p(out), _p(s["ph"]),
                                                      s["dE"], 0.05, 0.05, 0.0, 1, 1, 1, FLOOR, _p(ws),
                                                      s["ncm"] if ncm is None else ncm, s["M"], _p(vals), _p(idx),
                                                      _stream(torch))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                              # nothing launched
    return rc


@pytest.mark.parametrize("ne,ncm", [(12, 40), (12, 100), (50, 64)])
@pytest.mark.parametrize("en_r,en_s,upd", [(True, True, True), (True, False, True), (False, True, False)])
def test_unaligned_members_and_large_ne_run_the_class_map_kernels(torch, lib, ne, ncm, en_r, en_s, upd):
    s = _setup(ne, ncm)
    eng, n, M = s["eng"], s["M"] * ncm, s["M"]
    assert s["tab"]["kernel"] == ("register" if ne == 12 else "wave") and s["tab"]["ks0_diag"] is None
    assert s["tab"]["gap_sq"] is None and lib.qp_collision_member_tables_available(ne) == (1 if ne == 12 else 0)
    assert not eng.pair_members_supported(s["tab"], ncm, M)
    want_s, want_p, want_g = _lone_step(s, 0.37, en_r, en_s, upd, guarded=True)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    got_g = eng.pauli_stats_members_result(eng.collide_guarded_members(s["tab"], s["state"], out, ph, s["dE"], 0.37, en_r, en_s,
                                                                       upd, FLOOR, ncm, M, s["flags"]))
    es, ep = rel_err(out.cpu().numpy(), want_s), rel_err(ph.cpu().numpy(), want_p)
    print(f"ne={ne} ncm={ncm}: state {es:.3e} phonons {ep:.3e}")
    assert es < 1e-12 and ep < (1e-11 if ne <= 16 else 1e-10)
    for g, w in zip(got_g, want_g):                               # same cells, occupations within the state tolerance
        assert g[1:] == w[1:] and (g[0] == w[0] or abs(g[0] - w[0]) <= 1e-12 * abs(w[0]))     # -inf: no active cell
    assert _double_step_rc(torch, lib, s, s["tab"]["struct"]) == -3


def test_member_class_flag_misuse_is_refused_before_any_launch(torch, lib):
    from qpsim_amd import _hip
    s = _setup(12, 64)
    n = s["M"] * 64

    def variant(**changes):
        t = _hip.CollisionTables()
        C.memmove(C.byref(t), C.byref(s["tab"]["struct"]), C.sizeof(t))
        for k, v in changes.items():
            setattr(t, k, v)
        return t

    def step_rc(t, ncell):
        out = torch.full_like(s["state"], -7.0)
        rc = lib.qp_collision_step(C.byref(t), _p(s["flags"]), ncell, _p(s["state"]), _p(out), _p(s["ph"]), 0, s["dE"], 0.1, 1,
                                   1, 0, _stream(torch))
        torch.cuda.synchronize()
        assert rc != 0 and bool((out == -7.0).all())
        return rc

    assert step_rc(variant(), n - 1) == -1 and b"multiple of nclass" in lib.qp_last_error()
    assert step_rc(variant(nclass=5), n) == -1 and b"multiple of nclass" in lib.qp_last_error()
    assert step_rc(variant(cls=None), n) == -1 and b"cls" in lib.qp_last_error()
    assert _double_step_rc(torch, lib, s, variant(cls=None)) == -1 and b"cls" in lib.qp_last_error()
    assert _double_step_rc(torch, lib, s, variant(nclass=5)) == -1
    assert _double_step_rc(torch, lib, s, variant(flags=8 | 2)) == -3        # FORCE_WAVE: no pair pass


# ------------------------------------------------------------------------------------------------ API parity
def _rect_problem(ny, nx, kind="dirichlet", value=1e-5):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition(kind, value if kind == "dirichlet" else None) for e in edges}
    return mask, edges, bcs


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    scale = np.nanmax(np.abs(b))
    return 0.0 if scale == 0 else float(np.nanmax(np.abs(a - b)) / scale)


def _assert_contract(got, want, tol, ph_got=None, ph_want=None):
    assert not isinstance(got, Exception), got
    assert len(got) == 6 and got[0] == want[0]
    assert _rel(np.stack(got[1]), np.stack(want[1])) <= tol
    assert _rel(got[2], want[2]) <= tol
    assert type(got[3]) is type(want[3]) and _rel(got[3], want[3]) <= tol
    if want[4] is None:
        assert got[4] is None and got[5] is None
    else:
        assert _rel(np.stack([np.stack(f) for f in got[4]]), np.stack([np.stack(f) for f in want[4]])) <= tol
        assert np.array_equal(got[5], want[5])
    if ph_want is not None:
        assert sorted(ph_got) == sorted(ph_want)
        assert ph_got["phonon_metadata"] == ph_want["phonon_metadata"]
        assert _rel(np.stack(ph_got["phonon_frames"]), np.stack(ph_want["phonon_frames"])) <= tol
        if ph_want["phonon_energy_frames"] is not None:
            assert _rel(np.stack([np.stack(f) for f in ph_got["phonon_energy_frames"]]),
                        np.stack([np.stack(f) for f in ph_want["phonon_energy_frames"]])) <= tol


def _common(mask, edges, bcs, ne=12, scheme="adi", **kw):
    c = dict(mask=mask, edges=edges, edge_conditions=bcs, diffusion_coefficient=6.0, dt=0.1, total_time=1.0, dx=1.0,
             store_every=3, energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=ne,
             enable_recombination=True, enable_scattering=True, diffusion_scheme=scheme)
    c.update(kw)
    return c


SWEEP = {"tau_0": [440.0, 300.0, 600.0, 150.0], "T_c": [1.2, 1.0, 1.4, 1.1], "dynes_gamma": [0.0, 0.1, 0.3, 0.05]}


def _sweep_members(ny, nx, M=4):
    rng = np.random.default_rng(ny * 1000 + nx)
    return [{"initial_field": 1e-4 * (1.0 + rng.random((ny, nx))), "phonon_history_out": {}} for _ in range(M)]


def _lone(common, member, sweep, m):
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw = dict(common, **member)
    kw.update({k: v[m] for k, v in sweep.items()})
    if member.get("phonon_history_out") is not None:
        kw["phonon_history_out"] = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return run_2d_crank_nicolson(**kw), kw.get("phonon_history_out")


@pytest.mark.parametrize("ny,nx,scheme", [(8, 16, "adi"), (6, 10, "adi"), (8, 16, "cn_exact")])
def test_swept_ensemble_matches_lone_runs(ny, nx, scheme):
    """128 cells per member: member tables in the register and pair kernels; 60 cells: the class-map kernels, no pair pass."""
    from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble
    mask, edges, bcs = _rect_problem(ny, nx)
    common = _common(mask, edges, bcs, scheme=scheme)
    members = _sweep_members(ny, nx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=SWEEP, **common)
    stats = last_run_stats()
    assert stats["batches"] == 1
    if (ny * nx) % 64 == 0:
        assert stats["pair_passes"] > 0
    else:
        assert stats["pair_passes"] == 0
    tol = ADI_TOL if scheme == "adi" else CN_TOL
    for m, mem in enumerate(members):
        want, ph = _lone(common, mem, SWEEP, m)
        _assert_contract(got[m], want, tol, mem["phonon_history_out"], ph)
    # the members really differ through the sweep alone
    same_field = [dict(members[0], phonon_history_out=None) for _ in members]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        swept = run_2d_crank_nicolson_ensemble(same_field, sweep=SWEEP, **common)
    assert _rel(np.stack(swept[1][1]), np.stack(swept[0][1])) > 1e-6


def test_swept_ensemble_in_batches_gives_the_one_batch_results():
    from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble
    mask, edges, bcs = _rect_problem(8, 16)
    common = _common(mask, edges, bcs, total_time=0.6)
    members = [{"initial_field": mem["initial_field"]} for mem in _sweep_members(8, 16)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = run_2d_crank_nicolson_ensemble(members, sweep=SWEEP, **common)
        split = run_2d_crank_nicolson_ensemble(members, sweep=SWEEP, max_members_per_batch=3, **common)
    assert last_run_stats()["batches"] == 2
    for a, b in zip(split, one):
        _assert_contract(a, b, ADI_TOL)


@pytest.mark.parametrize("ny,nx", [(8, 16), (6, 10)])
def test_all_equal_sweep_is_the_call_without_sweep(ny, nx):
    from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble
    mask, edges, bcs = _rect_problem(ny, nx)
    members = _sweep_members(ny, nx, M=3)
    for mem in members:
        mem.pop("phonon_history_out")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = run_2d_crank_nicolson_ensemble(members, **_common(mask, edges, bcs, tau_0=300.0, T_c=1.1, dynes_gamma=0.2))
        want_stats = last_run_stats()
        got = run_2d_crank_nicolson_ensemble(members, sweep={"tau_0": [300.0] * 3, "T_c": [1.1] * 3, "dynes_gamma": [0.2] * 3},
                                             **_common(mask, edges, bcs))
        got_stats = last_run_stats()
    assert got_stats == want_stats
    for a, b in zip(got, want):
        assert a[0] == b[0] and a[2] == b[2]
        assert np.array_equal(np.stack(a[1]), np.stack(b[1]), equal_nan=True)
        assert np.array_equal(np.stack([np.stack(f) for f in a[4]]), np.stack([np.stack(f) for f in b[4]]), equal_nan=True)


def test_scalar_mode_validates_swept_values_and_ignores_them():
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    mask, edges, bcs = _rect_problem(6, 10)
    common = _common(mask, edges, bcs, energy_gap=0.0, total_time=0.3)
    members = [{"initial_field": mem["initial_field"]} for mem in _sweep_members(6, 10, M=2)]
    want = run_2d_crank_nicolson_ensemble(members, **common)
    got = run_2d_crank_nicolson_ensemble(members, sweep={"tau_0": [100.0, 200.0], "T_c": [1.0, 2.0]}, **common)
    for a, b in zip(got, want):
        assert np.array_equal(np.stack(a[1]), np.stack(b[1]), equal_nan=True)
    with pytest.raises(ValueError, match=r"^member 1: tau_s must be positive"):
        run_2d_crank_nicolson_ensemble(members, sweep={"tau_0": [100.0, -1.0]}, **common)


# ------------------------------------------------------------------------------------------------ guard
GUARD_GAMMAS = [0.0, 20.0, 40.0, 60.0]


def _guard_setup():
    """Reflective box, diffusion only, one uniform field and one constant generation rate for every member; the members differ
    by their Dynes broadening alone.  The initial state follows rho, so f0 = amp / (sum rho dE) - 0.460, 0.479, 0.504, 0.523 for
    the four broadenings - and grows by 0.004 per step: with the thresholds 0.5 / 0.52 member 0 stays silent over the 8 steps,
    member 1 warns at step 6, member 2 warns at step 0 and raises at step 5, member 3 raises at step 0."""
    from qpsim_amd import tables as T
    from qpsim_amd.models import ExternalGenerationSpec
    mask, edges, bcs = _rect_problem(8, 8, kind="reflective")
    ne, dt = 8, 0.1
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    rho = T.dynes_density_of_states(E, 180.0, 0.0)
    common = _common(mask, edges, bcs, ne=ne, total_time=0.8, store_every=4, enable_recombination=False,
                     enable_scattering=False, pauli_warn_threshold=0.5, pauli_error_threshold=0.52)
    member = {"initial_field": np.full(mask.shape, 0.46 * np.sum(rho) * dE),
              "external_generation": ExternalGenerationSpec(mode="constant", rate=0.004 * float(rho.min()) / dt)}
    return common, [dict(member) for _ in GUARD_GAMMAS], {"dynes_gamma": list(GUARD_GAMMAS)}


def test_guard_verdicts_of_a_swept_broadening_are_the_lone_runs(torch):
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from qpsim_amd.solver import run_2d_crank_nicolson
    common, members, sweep = _guard_setup()
    want_warn, want = [], []
    for m, mem in enumerate(members):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            try:
                want.append(run_2d_crank_nicolson(**common, **mem, dynes_gamma=sweep["dynes_gamma"][m]))
            except ValueError as exc:
                want.append(exc)
        if m == 0:
            assert not rec                                         # precondition: one member is silent ...
        want_warn += [f"member {m}: {w.message}" for w in rec]
    assert not isinstance(want[0], Exception) and not isinstance(want[1], Exception)
    assert any(w.startswith("member 1: ") for w in want_warn)      # ... one warns and finishes ...
    assert isinstance(want[2], ValueError) and isinstance(want[3], ValueError)      # ... and two raise, at different steps
    assert "step=5" in str(want[2]) and "step=0" in str(want[3])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = run_2d_crank_nicolson_ensemble(members, sweep=sweep, errors="return", **common)
    assert sorted(str(w.message) for w in rec) == sorted(want_warn)
    for m in (2, 3):
        assert isinstance(got[m], ValueError) and str(got[m]) == f"member {m}: {want[m]}"
    for m in (0, 1):
        _assert_contract(got[m], want[m], ADI_TOL)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError) as exc:
            run_2d_crank_nicolson_ensemble(members, sweep=sweep, **common)
    assert str(exc.value) == f"member 3: {want[3]}"
