"""Ensembles on the GPU: the per-member guard and generation kernels against their lone counterparts, and
``run_2d_crank_nicolson_ensemble`` against lone ``run_2d_crank_nicolson`` calls (rounding contract of qpsim_amd.ensemble)."""
from __future__ import annotations

import ctypes as C
import os
import pickle
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ADI_TOL, CN_TOL = 2e-13, 1e-12


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


# ------------------------------------------------------------------------------------------------ kernels
def _guard_inputs(torch, ne, ncm, members, seed):
    rng = np.random.default_rng(seed)
    n = members * ncm
    s = rng.random((ne, n)) * 0.8
    s[rng.random((ne, n)) < 0.01] = np.nan                     # NaN occupations win, first NaN in C order
    top = rng.random((ne, n)) < 0.02
    s[top] = 0.8                                               # ties at the maximum: smallest index wins
    flags = np.where(rng.random(n) < 0.85, 16, 0).astype(np.uint8)    # cells outside the mask
    rho = np.stack([np.linspace(1.0, 2.0, ne), np.linspace(1.5, 0.5, ne)])
    rho[1, 2] = 0.0                                            # forbidden bin of class 1
    cls = (rng.random(n) < 0.5).astype(np.int32)
    d = lambda a: torch.as_tensor(a, device="cuda")           # noqa: E731
    return d(s), d(rho), d(cls), d(flags)


@pytest.mark.parametrize("ncm", [40, 100, 128, 2048])
def test_pauli_stats_members_equals_lone_stats_per_slice(torch, lib, ncm):
    ne, members = 7, 5
    s, rho, cls, flags = _guard_inputs(torch, ne, ncm, members, ncm)
    ws = torch.empty(int(lib.qp_pauli_members_workspace_bytes(ncm, members)), dtype=torch.uint8, device="cuda")
    vals = torch.zeros(members, dtype=torch.float64, device="cuda")
    idx = torch.zeros(2 * members, dtype=torch.int64, device="cuda")
    assert lib.qp_pauli_stats_members(_p(s), _p(rho), _p(cls), _p(flags), ne, 2, ncm, members, 1e-18, _p(ws), _p(vals),
                                      _p(idx), _stream(torch)) == 0
    lws = torch.empty(int(lib.qp_pauli_workspace_bytes()), dtype=torch.uint8, device="cuda")
    lv = torch.zeros(1, dtype=torch.float64, device="cuda")
    li = torch.zeros(2, dtype=torch.int64, device="cuda")
    got_v, got_i = vals.cpu().numpy(), idx.cpu().numpy()
    for m in range(members):
        sl = slice(m * ncm, (m + 1) * ncm)
        ss, cs, fs = s[:, sl].contiguous(), cls[sl].contiguous(), flags[sl].contiguous()
        assert lib.qp_pauli_stats(_p(ss), _p(rho), _p(cs), _p(fs), ne, 2, ncm, 1e-18, _p(lws), _p(lv), _p(li),
                                  _stream(torch)) == 0
        want_v, want_i = lv.cpu().numpy(), li.cpu().numpy()
        assert np.array_equal(np.array([got_v[m]]), want_v, equal_nan=True), m
        assert got_v[m].tobytes() == want_v[0].tobytes(), m
        assert (got_i[2 * m], got_i[2 * m + 1]) == (want_i[0], want_i[1]), m


def test_add_constant_members_equals_lone_add_constant(torch, lib):
    ncm, members, nf = 100, 4, 3
    rng = np.random.default_rng(1)
    s = torch.as_tensor(rng.random((nf, members * ncm)), device="cuda")
    flags = torch.as_tensor(np.where(rng.random(members * ncm) < 0.8, 16, 0).astype(np.uint8), device="cuda")
    amounts = [1e-3, 0.0, 0.37, 1e-17]
    a = torch.as_tensor(np.asarray(amounts), device="cuda")
    want = s.clone()
    for m in range(members):
        sl = want[:, m * ncm:(m + 1) * ncm].contiguous()
        assert lib.qp_add_constant(_p(flags[m * ncm:(m + 1) * ncm].contiguous()), ncm, nf, _p(sl), amounts[m],
                                   _stream(torch)) == 0
        want[:, m * ncm:(m + 1) * ncm] = sl
    assert lib.qp_add_constant_members(_p(flags), ncm, members, nf, _p(s), _p(a), _stream(torch)) == 0
    assert torch.equal(s, want)


def _coupled_engine(torch, ny, nx, ne=12):
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((ny, nx), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = T.dynes_density_of_states(E, 180.0, 0.0)
    tab = eng.make_collision_tables(T.recombination_kernel_base(E, 180.0, 440.0, 1.2)[None],
                                    T.scattering_kernel_base(E, 180.0, 440.0, 1.2)[None], rho[None], idx_d, idx_s, sg)
    return eng, tab, dE, om.size, rho


def test_fused_member_finish_equals_standalone_pass(torch, lib):
    """ncell_member % 64 == 0: the per-member finish of the fused guard (single and double step) equals the standalone
    per-member pass over the state it describes."""
    ny, nx, members = 8, 16, 6
    eng, tab, dE, nw, rho = _coupled_engine(torch, ny, nx)
    assert tab["kernel"] == "register" and tab["pair"]
    ncm = ny * nx
    rng = np.random.default_rng(4)
    w = rho / (rho.sum() * dE)
    s0 = torch.as_tensor(w[:, None] * (0.05 + rng.random(members * ncm))[None, :], device="cuda")
    ph = torch.as_tensor(0.01 * (1.0 + rng.random((nw, members * ncm))), device="cuda")
    flags = eng.d_flags.reshape(-1).repeat(members)
    out = torch.empty_like(s0)
    ph1 = ph.clone()
    fused = eng.pauli_stats_members_result(eng.collide_guarded_members(tab, s0, out, ph1, dE, 0.05, True, True, True, 1e-18,
                                                                       ncm, members, flags))
    plain = eng.pauli_stats_members_result(eng.pauli_stats_members_launch(out, tab, 1e-18, ncm, members, flags))
    assert fused == plain
    # double step: its guard describes the state after the first half-step
    ph2 = ph.clone()
    out2 = torch.empty_like(s0)
    dbl = eng.pauli_stats_members_result(eng.collide_pair_guarded_members(tab, s0, out2, ph2, dE, 0.05, 0.05, 0.0, True, True,
                                                                          True, 1e-18, ncm, members, flags))
    assert dbl == plain
    # and the lone guard of one member equals its entry
    lone = eng.pauli_stats_result(eng.pauli_stats_launch(out[:, 2 * ncm:3 * ncm].contiguous(), tab, 1e-18))
    assert lone == plain[2]


def test_double_step_members_unsupported_cases(torch, lib):
    eng, tab, dE, nw, rho = _coupled_engine(torch, 4, 25)          # 100 cells per member: not a multiple of 64
    members, ncm = 3, 100
    s = torch.ones((12, members * ncm), dtype=torch.float64, device="cuda") * 1e-3
    o, ph = torch.empty_like(s), torch.zeros((nw, members * ncm), dtype=torch.float64, device="cuda")
    flags = eng.d_flags.reshape(-1).repeat(members)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(members, dtype=torch.float64, device="cuda")
    idx = torch.zeros(2 * members, dtype=torch.int64, device="cuda")
    rc = lib.qp_collision_double_step_guarded_members(C.byref(tab["struct"]), _p(flags), members * ncm, _p(s), _p(o), _p(ph),
                                                      dE, 0.05, 0.05, 0.0, 1, 1, 1, 1e-18, _p(ws), ncm, members, _p(vals),
                                                      _p(idx), _stream(torch))
    assert rc == -3 and "multiple of 64" in lib.qp_last_error().decode()
    # 64 members of 2048^2 = 2^28 pixels: beyond the pair kernel's 32-bit pixel range - refused before any launch
    big = 2048 * 2048
    rc = lib.qp_collision_double_step_guarded_members(C.byref(tab["struct"]), _p(flags), 64 * big, _p(s), _p(o), _p(ph),
                                                      dE, 0.05, 0.05, 0.0, 1, 1, 1, 1e-18, _p(ws), big, 64, _p(vals),
                                                      _p(idx), _stream(torch))
    assert rc == -3
    assert not eng.pair_members_supported(tab, big, 64) and eng.pair_members_supported(tab, 128, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ API parity
def _rect_problem(ny, nx, kind="dirichlet", value=1e-5):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition(kind, value if kind == "dirichlet" else None) for e in edges}
    return mask, edges, bcs


def _members(ny, nx, n=5):
    from qpsim_amd.models import ExternalGenerationSpec
    rng = np.random.default_rng(ny * 1000 + nx)
    gens = [None,
            ExternalGenerationSpec(mode="pulse", pulse_start=0.2, pulse_duration=0.3, pulse_rate=2e-4),
            ExternalGenerationSpec(mode="pulse", pulse_start=0.0, pulse_duration=0.5, pulse_rate=5e-4),
            ExternalGenerationSpec(mode="constant", rate=1e-4),
            ExternalGenerationSpec(mode="pulse", pulse_start=0.2, pulse_duration=0.3, pulse_rate=2e-4)]
    out = []
    for m in range(n):
        d = {"initial_field": 1e-4 * (1.0 + rng.random((ny, nx))), "bath_temperature": 0.1 + 0.02 * m,
             "phonon_history_out": {}}
        if gens[m % len(gens)] is not None:
            d["external_generation"] = gens[m % len(gens)]
        out.append(d)
    return out


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


def _lone(common, member):
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw = dict(common, **member)
    if member.get("phonon_history_out") is not None:
        kw["phonon_history_out"] = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return run_2d_crank_nicolson(**kw), kw.get("phonon_history_out")


def _common(mask, edges, bcs, ne=12, scheme="adi", **kw):
    c = dict(mask=mask, edges=edges, edge_conditions=bcs, diffusion_coefficient=6.0, dt=0.1, total_time=1.0, dx=1.0,
             store_every=3, energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=ne,
             enable_recombination=True, enable_scattering=True, T_c=1.2, diffusion_scheme=scheme)
    c.update(kw)
    return c


@pytest.mark.parametrize("ny,nx,scheme", [(36, 56, "adi"), (64, 64, "adi"), (36, 56, "cn_exact")])
def test_ensemble_matches_lone_runs(ny, nx, scheme):
    from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble
    mask, edges, bcs = _rect_problem(ny, nx)
    common = _common(mask, edges, bcs, scheme=scheme)
    members = _members(ny, nx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, **common)
    stats = last_run_stats()
    assert stats["batches"] == 1
    # one member generates at a constant rate and one not at all: the amounts always differ, so no step pair is fused
    # (the pair pass is covered at the c4 shape); the aligned 64^2 members take the fused per-member guard finish
    assert stats["pair_passes"] == 0 and stats["guarded_calls"] == 10
    tol = ADI_TOL if scheme == "adi" else CN_TOL
    for m, mem in enumerate(members):
        want, ph = _lone(common, mem)
        _assert_contract(got[m], want, tol, mem["phonon_history_out"], ph)


def test_ensemble_ne50_unfused_guard_and_scalar_mode():
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    mask, edges, bcs = _rect_problem(12, 20)
    common = _common(mask, edges, bcs, ne=50, total_time=0.5, store_every=2)
    members = _members(12, 20, n=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, **common)
    for m, mem in enumerate(members):
        want, ph = _lone(common, mem)
        _assert_contract(got[m], want, ADI_TOL, mem["phonon_history_out"], ph)
    scalar = dict(common, energy_gap=0.0)
    smembers = [{"initial_field": mem["initial_field"], "diffusion_coefficient": 3.0 + m, "phonon_history_out": {},
                 "bath_temperature": 0.1 + 0.01 * m} for m, mem in enumerate(members)]
    got = run_2d_crank_nicolson_ensemble(smembers, **scalar)
    for m, mem in enumerate(smembers):
        want, ph = _lone(scalar, mem)
        _assert_contract(got[m], want, ADI_TOL, mem["phonon_history_out"], ph)


def _guard_setup():
    """Reflective box, diffusion only, uniform fields: f = n / rho grows by dt * rate / min(rho) per step from f0 = 0.12 -
    8 steps: member 0 never warns, 1 warns at step 4, 2 at step 8, 3 warns at step 2 and crosses the error threshold at step 3."""
    from qpsim_amd import tables as T
    from qpsim_amd.models import ExternalGenerationSpec
    mask, edges, bcs = _rect_problem(8, 8, kind="reflective")
    ne, dt = 8, 0.1
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    rho = T.dynes_density_of_states(E, 180.0, 0.0)
    common = _common(mask, edges, bcs, ne=ne, total_time=0.8, store_every=4, enable_recombination=False,
                     enable_scattering=False)
    amp = 0.12 * np.sum(rho) * dE                              # f0 = amp w_i / rho_i = amp / (sum rho dE)
    members = []
    for inc in (0.0, 0.1, 0.05, 0.3):
        d = {"initial_field": np.full(mask.shape, amp)}
        if inc > 0:
            d["external_generation"] = ExternalGenerationSpec(mode="constant", rate=inc * float(rho.min()) / dt)
        members.append(d)
    return common, members


def test_guard_warnings_and_errors_are_the_lone_runs(torch):
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from qpsim_amd.solver import run_2d_crank_nicolson
    common, members = _guard_setup()
    want_warn, want = [], []
    for m, mem in enumerate(members):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            try:
                want.append(run_2d_crank_nicolson(**common, **mem))
            except ValueError as exc:
                want.append(exc)
        want_warn += [f"member {m}: {w.message}" for w in rec]
    assert isinstance(want[3], ValueError) and not any(isinstance(w, Exception) for w in want[:3])
    assert len({w.split("step=")[1].split(",")[0] for w in want_warn}) >= 3       # different steps
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = run_2d_crank_nicolson_ensemble(members, errors="return", **common)
    assert sorted(str(w.message) for w in rec) == sorted(want_warn)
    assert isinstance(got[3], ValueError) and str(got[3]) == f"member 3: {want[3]}"
    for m in range(3):
        _assert_contract(got[m], want[m], ADI_TOL)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match=r"^member 3: Pauli occupation exceeded limit"):
            run_2d_crank_nicolson_ensemble(members, **common)


def test_c4_shape_members_meet_contract_and_take_the_pair_pass(torch):
    from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble
    N, M, steps = 256, 64, 3
    mask, edges, bcs = _rect_problem(N, N, kind="reflective")
    common = _common(mask, edges, bcs, total_time=steps * 0.1, store_every=steps)
    rng = np.random.default_rng(7)
    members = [{"initial_field": 1e-4 * (1.0 + rng.random((N, N)))} for _ in range(M)]
    got = run_2d_crank_nicolson_ensemble(members, **common)
    assert last_run_stats()["pair_passes"] == steps - 1
    for m in (0, 31, 63):
        want, _ = _lone(common, members[m])
        _assert_contract(got[m], want, ADI_TOL)


def test_batches_give_the_one_batch_results():
    from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble
    mask, edges, bcs = _rect_problem(36, 56)
    common = _common(mask, edges, bcs, total_time=0.6)
    members = _members(36, 56)
    for mem in members:
        mem.pop("phonon_history_out")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one = run_2d_crank_nicolson_ensemble(members, **common)
        split = run_2d_crank_nicolson_ensemble(members, max_members_per_batch=2, **common)
    assert last_run_stats()["batches"] == 3
    for a, b in zip(split, one):
        _assert_contract(a, b, ADI_TOL)


def _dist_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
        mask, edges, bcs = _rect_problem(36, 56)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = run_2d_crank_nicolson_ensemble(_members(36, 56), process_group=dist.group.WORLD,
                                                 **_common(mask, edges, bcs, total_time=0.6))
        with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
            pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


def test_two_process_gloo_ensemble_returns_the_one_process_list(tmp_path):
    import torch.multiprocessing as mp
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from test_distributed_cpu import _free_port
    mp.spawn(_dist_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    mask, edges, bcs = _rect_problem(36, 56)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = run_2d_crank_nicolson_ensemble(_members(36, 56), **_common(mask, edges, bcs, total_time=0.6))
    for r in range(2):
        with open(tmp_path / f"rank{r}.pkl", "rb") as f:
            got = pickle.load(f)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            _assert_contract(a, b, ADI_TOL)
