"""Padded bins on the GPU (QP_COLL_PAD_BINS, QP_ROUTE_ONEPASS_PADDED): the one-pass kernel of a ceiling size (30, 32, 40,
50) on the live bins of every size in 17 ... 49 that has no kernel of its own.

Element by element against the extended-precision evaluation, as tests/test_gpu_collision_elementwise.py bounds the
instantiated sizes: K = max |got - exact| / T <= 4 K_ref64 + 4 for the state and for the phonon planes, K_ref64 being the
same statistic of the fp64 oracle (1.0 ... 4.2 on these grids), and no T = 0 element may differ.  Grids and inputs:
tests/collision_padded_cases.py; the 407-cell mask of the instantiation tests.  Every case asserts its route."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest

import collision_exact as X
import collision_padded_cases as PC
from golden_utils import rel_err
from test_gpu_collision_instantiations import FLOOR, HAVE_X87, _check_untouched, _engine, _route, _run
from test_gpu_ensemble_sweep import _assert_contract, _common, _rect_problem, _rel

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")]

DT = 0.37
_SETUPS: dict = {}


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


def _padded_route():
    from qpsim_amd import _hip as H
    return H.ROUTE_ONEPASS_PADDED


def _setup(ne, kind):
    """`collision_padded_cases.host_setup` uploaded to the engine of the instantiation tests, with the padded and the
    one-wave-per-pixel tables of its one gap class; built once."""
    key = (ne, kind)
    if key not in _SETUPS:
        eng, h = _engine(), PC.host_setup(ne, kind)
        assert np.array_equal(h["active"], eng.mask_flat)
        d = lambda a: eng.torch.as_tensor(np.ascontiguousarray(a), device=eng.device)          # noqa: E731
        args = PC.one_class_args(h)
        tabs = {("one", "padded"): eng.make_collision_tables(*args, pad_bins=True),
                ("one", "wave"): eng.make_collision_tables(*args, kernel="wave")}
        pad = tabs[("one", "padded")]
        assert pad["kernel"] == "register" and pad["struct"].flags & 16 and not pad["pair"] and pad["nw"] == h["nw"]
        assert (pad["merged_slots"] > 0) == (kind == "merged")
        assert tuple(pad["ks0_diag"].shape) == (ne, ne) and tuple(pad["kr0_anti2"].shape) == (2 * ne - 1, ne)
        assert tabs[("one", "wave")]["kernel"] == "wave" and not tabs[("one", "wave")]["struct"].flags & 16
        _SETUPS[key] = dict(h, eng=eng, state_dev={"one": d(h["state"]["one"])}, ph_dev=d(h["ph"]), tabs=tabs)
    return _SETUPS[key]


def _elementwise(O, h, combo, dt, got_s, got_p, tag):
    """K of the state and of the phonon planes against limit(K_ref64); elements with T = 0 must be equal."""
    ex = X.exact(O, h, "one", combo, dt)
    (r_s, r_p), ref_differ = X.k_ref64(O, h, "one", combo, dt)
    (k_s, k_p), differ = X.error_k(O, got_s, got_p, ex)
    print(f"K {tag}: state {k_s:.2f} (K_ref64 {r_s:.2f}) phonons {k_p:.2f} (K_ref64 {r_p:.2f})")
    assert ref_differ == 0 and differ == 0
    assert k_s <= X.limit(r_s), f"{tag}: state K = {k_s:.3g} > 4 x {r_s:.3g} + 4"
    assert k_p <= X.limit(r_p), f"{tag}: phonons K = {k_p:.3g} > 4 x {r_p:.3g} + 4"


def _case(O, monkeypatch, ne, kind, combo, dt):
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    s = _setup(ne, kind)
    assert _route(s, s["tabs"][("one", "padded")], combo) == _padded_route()
    out, ph, _, _ = _run(s, "one", "padded", combo, dt=dt)
    _check_untouched(s, "one", out, ph, combo[2])
    px = s["active"]
    got_s, got_p = out[:, px], ph[:, px]
    assert got_s.shape[0] == ne and np.all(np.isfinite(got_s)) and np.all(np.isfinite(got_p))
    _elementwise(O, s, combo, dt, got_s, got_p, f"padded {kind} ne={ne} C={PC.ceiling(ne)} {combo} dt={dt:g}")


# ------------------------------------------------------------------------------------------------ against the exact evaluation
@pytest.mark.parametrize("ne,kind", PC.GRIDS)
def test_every_padded_size_element_by_element(O, monkeypatch, ne, kind):
    """All 27 sizes without a kernel of their own (30 grids: 25, 36 and 45 with and without merged bins), every process on."""
    _case(O, monkeypatch, ne, kind, X.ALL_ON, DT)


@pytest.mark.parametrize("dt", [1e-7, DT])
@pytest.mark.parametrize("en_r,en_s,upd", X.COMBOS)
@pytest.mark.parametrize("ne", PC.BOUNDARY_NE)
def test_first_and_last_live_size_of_every_ceiling(O, monkeypatch, ne, en_r, en_s, upd, dt):
    """17 / 29 (ceiling 30), 31 (32), 33 / 39 (40), 41 / 49 (50); 42 = three whole 14-bin target blocks of ceiling 50; 28 and
    29 end inside the second 16-bin block of ceiling 30.  `_check_untouched`: inactive cells pass through bit-equal."""
    _case(O, monkeypatch, ne, PC.kind_of(ne), (en_r, en_s, upd), dt)


@pytest.mark.parametrize("en_r,en_s", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("ne", PC.BOUNDARY_NE)
def test_frozen_phonons_stay_bit_equal(monkeypatch, ne, en_r, en_s):
    """update_phonons off (the UPD = false kernels): the phonon planes are untouched."""
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    s = _setup(ne, PC.kind_of(ne))
    assert _route(s, s["tabs"][("one", "padded")], (en_r, en_s, False)) == _padded_route()
    out, ph, _, _ = _run(s, "one", "padded", (en_r, en_s, False))
    _check_untouched(s, "one", out, ph, False)
    assert np.array_equal(ph, s["ph"]) and np.all(np.isfinite(out))


@pytest.mark.parametrize("dt", X.SWEEP_DT)
@pytest.mark.parametrize("ne", [25, 45])
def test_time_step_sweep_element_by_element(O, monkeypatch, ne, dt):
    """3e-3 ... 800: from rounding-dominated e^x - 1 to both clips of the exponent (asserted on the host)."""
    x = X.exact(O, PC.host_setup(ne, "regimes"), "one", X.ALL_ON, dt)["x"]
    assert bool(np.any(x == -80.0)) == (dt >= 400.0) and bool(np.any(x == 80.0)) == (dt == 800.0)
    _case(O, monkeypatch, ne, "regimes", X.ALL_ON, dt)


# ------------------------------------------------------------------------------------------------ against the wave kernel
@pytest.mark.parametrize("ne", [25, 36, 45])
def test_padded_kernel_against_the_wave_kernel(monkeypatch, ne):
    """The kernel the same tables run without the flag, with the relative bounds tests/test_gpu_parity.py uses between
    kernel families (1e-12 state, 1e-11 phonons, of the largest value)."""
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    s = _setup(ne, "regimes")
    assert _route(s, s["tabs"][("one", "wave")], X.ALL_ON) == H.ROUTE_WAVE
    assert _route(s, s["tabs"][("one", "padded")], X.ALL_ON) == _padded_route()
    pad_s, pad_p, _, _ = _run(s, "one", "padded", X.ALL_ON)
    wav_s, wav_p, _, _ = _run(s, "one", "wave", X.ALL_ON)
    es, ep = rel_err(pad_s, wav_s), rel_err(pad_p, wav_p)
    print(f"ne={ne}: padded vs wave: state {es:.3e} phonons {ep:.3e}")
    assert es < 1e-12 and ep < 1e-11


# ------------------------------------------------------------------------------------------------ pad planes
PATTERN = 0x7FF8DEADBEEF0001      # a quiet NaN with a payload: any write, and any arithmetic on it, changes the bits


def _torch():
    import torch
    return torch


@pytest.mark.parametrize("ne,kind", [(25, "regimes"), (31, "merged"), (41, "merged")])
def test_pad_planes_are_neither_read_nor_written(monkeypatch, ne, kind):
    """Buffers with C - ne extra state planes, 8 extra phonon planes and 2 extra stash planes behind the live ones: NaN where
    the call could read, a fixed bit pattern where it could write.  Afterwards the extra planes are bit-identical and the
    live results are those of the call on tight buffers."""
    from qpsim_amd.engine import _ptr
    torch = _torch()
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    s = _setup(ne, kind)
    eng, tab, n, nw = s["eng"], s["tabs"][("one", "padded")], s["eng"].ncell, s["nw"]
    extra = PC.ceiling(ne) - ne
    slots = tab["merged_slots"]
    assert extra > 0 and (slots > 0) == (kind == "merged")
    assert _route(s, tab, X.ALL_ON) == _padded_route()
    want_s, want_p, _, _ = _run(s, "one", "padded", X.ALL_ON)
    pattern = torch.tensor([PATTERN], dtype=torch.int64, device=eng.device).view(torch.float64)

    def filled(planes):
        return pattern.expand(planes * n).clone().reshape(planes, n)

    s_in = torch.cat([s["state_dev"]["one"], torch.full((extra, n), float("nan"), dtype=torch.float64, device=eng.device)])
    s_out = filled(ne + extra)
    ph = torch.cat([s["ph_dev"], filled(8)])
    stash = filled(2 * slots + 2)
    rc = eng.lib.qp_collision_step(C.byref(tab["struct"]), _ptr(eng.d_flags), n, _ptr(s_in), _ptr(s_out), _ptr(ph),
                                   _ptr(stash), float(s["dE"]), DT, 1, 1, 1, eng.stream)
    assert rc == 0
    torch.cuda.synchronize()
    as_bits = lambda t: t.contiguous().view(torch.int64).cpu().numpy()          # noqa: E731
    assert np.all(as_bits(s_out[ne:]) == PATTERN)
    assert np.all(as_bits(ph[nw:]) == PATTERN)
    assert np.all(as_bits(stash[2 * slots:]) == PATTERN)
    assert np.array_equal(as_bits(s_in[:ne]), as_bits(s["state_dev"]["one"]))
    assert np.array_equal(s_out[:ne].cpu().numpy(), want_s)
    assert np.array_equal(ph[:nw].cpu().numpy(), want_p)
    assert np.all(np.isfinite(want_s)) and np.all(np.isfinite(want_p))


# ------------------------------------------------------------------------------------------------ member tables
MEMBER_TAU = [440.0, 300.0, 650.0]
_MEMBERS: dict = {}


def _member_setup(ne):
    """3 members x 256 cells with tau_0 differing per member; the last 256-cell block of member 1 (all of it) and lane 0 of
    member 2 inactive, as in tests/test_gpu_collision_onepass_members.py."""
    if ne in _MEMBERS:
        return _MEMBERS[ne]
    torch = _torch()
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    M, ncm = len(MEMBER_TAU), 256
    mask = np.ones((16, 16), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    E, dE = T.build_energy_grid(180.0, 1.0, PC.UNMERGED[ne], ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, 180.0, 0.1)] * M)
    kr = np.stack([T.recombination_kernel_base(E, 180.0, tau, 1.2) for tau in MEMBER_TAU])
    ks = np.stack([T.scattering_kernel_base(E, 180.0, tau, 1.2) for tau in MEMBER_TAU])
    assert not np.array_equal(kr[0], kr[1]) and not np.array_equal(ks[1], ks[2])
    tab = eng.make_collision_tables(kr, ks, rho, idx_d, idx_s, sg, None, members=M, member_classes=True, pad_bins=True)
    lone = [eng.make_collision_tables(kr[m][None], ks[m][None], rho[m][None], idx_d, idx_s, sg, pad_bins=True)
            for m in range(M)]
    rng = np.random.default_rng(1000 * ne + ncm)
    n = M * ncm
    level = rng.choice([1e-5, 1e-2, 0.5, 0.95], size=n)
    state = rng.random((ne, n)) * np.repeat(rho.T, ncm, axis=1) * level[None, :] + 1e-12
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    flags = np.where(rng.random(n) < 0.9, 16, 0).astype(np.uint8)
    flags[ncm - 64:ncm] = 0                        # the last wave of member 0
    flags[2 * ncm - 256:2 * ncm] = 0               # the last (only) block of member 1
    flags[2 * ncm] = 0                             # lane 0 of member 2 ...
    flags[2 * ncm + 1] = 16                        # ... next to an active one
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")          # noqa: E731
    _MEMBERS[ne] = dict(eng=eng, tab=tab, lone=lone, dE=float(dE), M=M, ncm=ncm, ne=ne, state=d(state), ph=d(ph),
                        flags=d(flags), state_host=state, ph_host=ph, flags_host=flags)
    return _MEMBERS[ne]


@pytest.mark.parametrize("ne", [25, 45])
def test_member_tables_are_bit_equal_to_lone_padded_calls(monkeypatch, ne):
    torch = _torch()
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    s = _member_setup(ne)
    eng, M, ncm, tab = s["eng"], s["M"], s["ncm"], s["tab"]
    n = M * ncm
    assert tab["kernel"] == "register" and tab["struct"].flags & 16 and tab["struct"].flags & 8
    assert tuple(tab["ks0_diag"].shape) == (M, ne, ne) and tuple(tab["kr0_anti2"].shape) == (M, 2 * ne - 1, ne)
    route = lambda t, nc: eng.lib.qp_collision_route(C.byref(t["struct"]), nc, 1, 1, 1, 0)          # noqa: E731
    assert route(tab, n) == _padded_route() and all(route(t, ncm) == _padded_route() for t in s["lone"])
    outs, phs = [], []
    for m in range(M):
        sl = slice(m * ncm, (m + 1) * ncm)
        si, pi, fl = (a[..., sl].contiguous() for a in (s["state"], s["ph"], s["flags"]))
        so = torch.full_like(si, -7.0)
        eng.collide(s["lone"][m], si, so, pi, s["dE"], DT, True, True, True, ncell=ncm, flags=fl)
        outs.append(so.cpu().numpy())
        phs.append(pi.cpu().numpy())
    want_s, want_p = np.concatenate(outs, axis=1), np.concatenate(phs, axis=1)
    out, ph = torch.full_like(s["state"], -7.0), s["ph"].clone()
    eng.collide(tab, s["state"], out, ph, s["dE"], DT, True, True, True, ncell=n, flags=s["flags"])
    assert np.array_equal(out.cpu().numpy(), want_s) and np.array_equal(ph.cpu().numpy(), want_p)
    inactive = s["flags_host"] == 0
    assert inactive[ncm:2 * ncm].all() and inactive[2 * ncm] and not inactive[2 * ncm + 1]
    assert np.array_equal(want_s[:, inactive], s["state_host"][:, inactive])
    assert np.array_equal(want_p[:, inactive], s["ph_host"][:, inactive])
    assert not np.array_equal(want_s[:, ~inactive], s["state_host"][:, ~inactive])
    # the members differ through their tables alone: member 2 with member 0's table gives another result
    sl = slice(2 * ncm, 3 * ncm)
    si, pi, fl = (a[..., sl].contiguous() for a in (s["state"], s["ph"], s["flags"]))
    so = torch.full_like(si, -7.0)
    eng.collide(s["lone"][0], si, so, pi, s["dE"], DT, True, True, True, ncell=ncm, flags=fl)
    assert not np.array_equal(so.cpu().numpy(), want_s[:, sl])


# ------------------------------------------------------------------------------------------------ guarded call
@pytest.mark.parametrize("ne,kind", [(25, "regimes"), (31, "merged"), (45, "regimes")])
def test_guarded_call_runs_the_separate_statistics_pass(monkeypatch, ne, kind):
    """The one-pass kernels write no guard partials: qp_collision_step_guarded = qp_collision_step + qp_pauli_stats."""
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    s = _setup(ne, kind)
    tab = s["tabs"][("one", "padded")]
    assert _route(s, tab, X.ALL_ON) == _padded_route()
    out, ph, out_dev, stats = _run(s, "one", "padded", X.ALL_ON, guarded=True)
    want_s, want_p, plain_dev, _ = _run(s, "one", "padded", X.ALL_ON)
    assert np.array_equal(out, want_s) and np.array_equal(ph, want_p)
    assert stats == s["eng"].pauli_stats(plain_dev, tab, FLOOR)
    px = s["active"]
    f = np.where(s["rho"][0][:, None] > 1e-30, out[:, px] / np.maximum(s["rho"][0][:, None], 1e-30), 0.0)
    k = int(np.argmax(f))
    assert stats[0] == f.reshape(-1)[k] and stats[1] == (k // int(px.sum()), np.flatnonzero(px)[k % int(px.sum())])


# ------------------------------------------------------------------------------------------------ public interface
def _capture_tables(monkeypatch):
    from qpsim_amd.engine import Engine
    seen = []
    make = Engine.make_collision_tables

    def wrapper(self, *a, **kw):
        h = make(self, *a, **kw)
        seen.append((self, h))
        return h
    monkeypatch.setattr(Engine, "make_collision_tables", wrapper)
    return seen


def _run_lone(**kw):
    from qpsim_amd.solver import run_2d_crank_nicolson
    ph = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return run_2d_crank_nicolson(**kw, phonon_history_out=ph), ph


def _route_of(eng, h, ncell):
    return eng.lib.qp_collision_route(C.byref(h["struct"]), ncell, 1, 1, 1, int(bool(h["merged_slots"])))


def test_run_keyword_takes_the_padded_route_and_agrees_with_the_default(monkeypatch):
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    seen = _capture_tables(monkeypatch)
    ny, nx, ne = 16, 16, 25
    mask, edges, bcs = _rect_problem(ny, nx)
    init = 1e-4 * (1.0 + np.random.default_rng(25).random((ny, nx)))
    common = _common(mask, edges, bcs, ne=ne, scheme="adi", total_time=0.6, store_every=3, initial_field=init)
    on, ph_on = _run_lone(**common, collision_padded_bins=True)
    off, ph_off = _run_lone(**common, collision_padded_bins=False)
    never, ph_never = _run_lone(**common)
    assert len(seen) == 3
    (e_on, h_on), (e_off, h_off), (e_nv, h_nv) = seen
    assert h_on["struct"].flags & 16 and h_on["kernel"] == "register" and _route_of(e_on, h_on, ny * nx) == H.ROUTE_ONEPASS_PADDED
    for e, h in ((e_off, h_off), (e_nv, h_nv)):
        assert h["struct"].flags == 0 and h["kernel"] == "wave" and _route_of(e, h, ny * nx) == H.ROUTE_WAVE
        assert h["ks0_diag"] is None and h["kr0_anti2"] is None
    assert len(on[0]) == 3 and ph_on["phonon_frames"]
    _assert_contract(on, off, 1e-9, ph_on, ph_off)
    print("switch on vs off: frames", _rel(np.stack(on[1]), np.stack(off[1])), "phonon frames",
          _rel(np.stack(ph_on["phonon_frames"]), np.stack(ph_off["phonon_frames"])))
    _assert_contract(off, never, 0.0, ph_off, ph_never)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(off[1], never[1]))


def test_swept_ensemble_with_the_keyword_matches_lone_padded_runs(monkeypatch):
    from qpsim_amd import _hip as H
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    seen = _capture_tables(monkeypatch)
    ny, nx, ne = 16, 16, 25
    mask, edges, bcs = _rect_problem(ny, nx)
    common = _common(mask, edges, bcs, ne=ne, scheme="adi", total_time=0.6, store_every=3, collision_padded_bins=True)
    sweep = {"tau_0": [440.0, 300.0, 650.0]}
    rng = np.random.default_rng(16 * 1000 + 25)
    members = [{"initial_field": 1e-4 * (1.0 + rng.random((ny, nx))), "phonon_history_out": {}} for _ in range(3)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=sweep, **common)
    assert len(seen) == 1
    eng, h = seen[0]
    assert h["struct"].flags & 16 and h["struct"].flags & 8 and h["nclass"] == 3
    assert _route_of(eng, h, 3 * ny * nx) == H.ROUTE_ONEPASS_PADDED
    for m, mem in enumerate(members):
        kw = dict(common, initial_field=mem["initial_field"], tau_0=sweep["tau_0"][m])
        want, ph = _run_lone(**kw)
        assert seen[-1][1]["struct"].flags & 16 and _route_of(*seen[-1], ny * nx) == H.ROUTE_ONEPASS_PADDED
        _assert_contract(got[m], want, 0.0, mem["phonon_history_out"], ph)
    assert _rel(np.stack(got[1][1]), np.stack(got[0][1])) > 1e-6
