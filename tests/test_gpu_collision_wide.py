"""Wide bins on the GPU (QP_COLL_WIDE_BINS, QP_ROUTE_WAVE_WIDE): the one-wave-per-pixel kernel with two energy bins per
lane, NE = 65 ... 128, where the generic one-thread-per-cell kernel runs without the flag.

Element by element against the extended-precision evaluation, as tests/test_gpu_collision_elementwise.py bounds the other
kernels: K = max |got - exact| / T <= 4 K_ref64 + 4 for the state and for the phonon planes, K_ref64 being the same
statistic of the fp64 oracle on the same inputs, and no T = 0 element may differ.  Inputs: `collision_exact.host_setup(ne,
"regimes")` on the 407-cell ragged mask of the instantiation tests (one wave entirely inactive, a fifth of the rest
inactive, the last pixel group ragged for 4 and for 8 pixels per wave).  Sizes: 65 (unstructured maps, the atomic form; one
live lane in the second half), 72 (structured; 8 live lanes), 100, 127 (unstructured; 7 phonon bins per lane), 128 (both
halves full).  Every case asserts its route."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import pytest

import collision_exact as X
from golden_utils import rel_err
from test_gpu_collision_instantiations import (FLOOR, HAVE_X87, X87_RULE, _check_untouched, _engine, _oracle, _route, _run,
                                               _tolerances, check)
from test_gpu_ensemble_sweep import _assert_contract, _common, _rel

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")]

DT = 0.37
SIZES = {65: (233, False), 72: (215, True), 100: (299, True), 127: (424, False), 128: (383, True)}   # ne: (nw, structured)
STRUCTURED = [ne for ne, (_, st) in SIZES.items() if st]
_SETUPS: dict = {}


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


def _wide_route():
    from qpsim_amd import _hip as H
    return H.ROUTE_WAVE_WIDE


def _torch():
    import torch
    return torch


def _setup(ne):
    """`collision_exact.host_setup(ne, "regimes")` uploaded to the engine of the instantiation tests with the wide and the
    generic tables of its one gap class and the wide tables of its four gap classes; built once."""
    if ne not in _SETUPS:
        eng, h = _engine(), X.host_setup(ne, "regimes")
        assert np.array_equal(h["active"], eng.mask_flat)
        nw, structured = SIZES[ne]
        assert h["nw"] == nw
        d = lambda a: eng.torch.as_tensor(np.ascontiguousarray(a), device=eng.device)          # noqa: E731
        one = (h["kr"][:1], h["ks"][:1], h["rho"][:1], *h["maps"])
        tabs = {("one", "wide"): eng.make_collision_tables(*one, wide_bins=True),
                ("one", "generic"): eng.make_collision_tables(*one, kernel="generic"),
                ("classes", "wide"): eng.make_collision_tables(h["kr"], h["ks"], h["rho"], *h["maps"], h["cls"][h["active"]],
                                                               wide_bins=True)}
        for family in ("one", "classes"):
            t = tabs[(family, "wide")]
            assert t["kernel"] == "wave" and t["fast"] and not t["pair"] and t["struct"].flags == 32 and t["nw"] == nw
            assert (t["diag_bin"] is not None) == structured
        gen = tabs[("one", "generic")]
        assert gen["kernel"] == "generic" and not gen["fast"] and gen["struct"].flags == 1
        _SETUPS[ne] = dict(h, eng=eng, state_dev={f: d(a) for f, a in h["state"].items()}, ph_dev=d(h["ph"]), tabs=tabs)
    return _SETUPS[ne]


def _elementwise(O, h, family, combo, dt, got_s, got_p, tag):
    """K of the state and of the phonon planes against limit(K_ref64); elements with T = 0 must be equal."""
    ex = X.exact(O, h, family, combo, dt)
    (r_s, r_p), ref_differ = X.k_ref64(O, h, family, combo, dt)
    (k_s, k_p), differ = X.error_k(O, got_s, got_p, ex)
    x = ex["x"]
    print(f"K {tag}: state {k_s:.2f} (K_ref64 {r_s:.2f}) phonons {k_p:.2f} (K_ref64 {r_p:.2f}); exponents clipped at -80: "
          f"{np.mean(x == -80.0):.2%}, at +80: {np.mean(x == 80.0):.2%}")
    assert ref_differ == 0 and differ == 0
    assert k_s <= X.limit(r_s), f"{tag}: state K = {k_s:.3g} > 4 x {r_s:.3g} + 4"
    assert k_p <= X.limit(r_p), f"{tag}: phonons K = {k_p:.3g} > 4 x {r_p:.3g} + 4"


def _case(O, family, ne, combo, dt):
    s = _setup(ne)
    assert _route(s, s["tabs"][(family, "wide")], combo) == _wide_route()
    out, ph, _, _ = _run(s, family, "wide", combo, dt=dt)
    _check_untouched(s, family, out, ph, combo[2])
    px = s["active"]
    got_s, got_p = out[:, px], ph[:, px]
    assert got_s.shape[0] == ne and np.all(np.isfinite(got_s)) and np.all(np.isfinite(got_p))
    tag = f"wide {family} ne={ne} {combo} dt={dt:g}"
    ref_s, ref_p = _oracle(O, s, family, combo, dt)
    tol_s, tol_p = _tolerances(family, "regimes", ne)[1]
    for i, (name, got, ref, tol) in enumerate((("state", got_s, ref_s, tol_s), ("phonons", got_p, ref_p, tol_p))):
        check(got, ref, s["level"], tol, f"{tag} {name} vs oracle", rule=X87_RULE.get((family, "regimes", name), ()), ref64=ref,
              ref80=lambda i=i: _oracle(O, s, family, combo, dt, np.longdouble)[i])
    _elementwise(O, s, family, combo, dt, got_s, got_p, tag)


# ------------------------------------------------------------------------------------------------ 1. against the exact evaluation
@pytest.mark.parametrize("dt", [1e-7, DT])
@pytest.mark.parametrize("en_r,en_s,upd", X.COMBOS)
@pytest.mark.parametrize("ne", sorted(SIZES))
def test_every_size_element_by_element(O, ne, en_r, en_s, upd, dt):
    _case(O, "one", ne, (en_r, en_s, upd), dt)


@pytest.mark.parametrize("dt", X.SWEEP_DT)
@pytest.mark.parametrize("ne", [72, 128])
def test_time_step_sweep_element_by_element(O, ne, dt):
    """3e-3 ... 800: from rounding-dominated e^x - 1 to the clips of the exponent (their share is printed with K)."""
    _case(O, "one", ne, X.ALL_ON, dt)


@pytest.mark.parametrize("ne", [72, 127])
def test_gap_classes_element_by_element(O, ne):
    """Four gap classes mixed pixel by pixel: per-class [NE][NE] tables through `cls`."""
    s = _setup(ne)
    assert s["tabs"][("classes", "wide")]["nclass"] == 4 and np.unique(s["cls"][s["active"]]).size == 4
    _case(O, "classes", ne, X.ALL_ON, DT)


# ------------------------------------------------------------------------------------------------ 2. against the generic kernel
@pytest.mark.parametrize("ne", sorted(SIZES))
def test_wide_kernel_against_the_generic_kernel(ne):
    """The kernel the same inputs run without the flag, with the relative bounds tests/test_gpu_parity.py uses between
    kernel families (1e-12 state, 1e-11 phonons, of the largest value)."""
    from qpsim_amd import _hip as H
    s = _setup(ne)
    assert _route(s, s["tabs"][("one", "generic")], X.ALL_ON) == H.ROUTE_GENERIC
    assert _route(s, s["tabs"][("one", "wide")], X.ALL_ON) == _wide_route()
    wid_s, wid_p, _, _ = _run(s, "one", "wide", X.ALL_ON)
    gen_s, gen_p, _, _ = _run(s, "one", "generic", X.ALL_ON)
    es, ep = rel_err(wid_s, gen_s), rel_err(wid_p, gen_p)
    print(f"ne={ne}: wide vs generic: state {es:.3e} phonons {ep:.3e}")
    assert es < 1e-12 and ep < 1e-11


# ------------------------------------------------------------------------------------------------ 3. frozen phonons
@pytest.mark.parametrize("en_r,en_s", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("ne", [72, 128])
def test_frozen_phonons_stay_bit_equal(ne, en_r, en_s):
    s = _setup(ne)
    assert _route(s, s["tabs"][("one", "wide")], (en_r, en_s, False)) == _wide_route()
    out, ph, _, _ = _run(s, "one", "wide", (en_r, en_s, False))
    _check_untouched(s, "one", out, ph, False)
    assert np.array_equal(ph, s["ph"]) and np.all(np.isfinite(out))
    assert not np.array_equal(out[:, s["active"]], s["state"]["one"][:, s["active"]])


# ------------------------------------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("ne", STRUCTURED)
def test_structured_sizes_are_deterministic(ne):
    """With the structure hint the per-bin sums are plain read-modify-writes of one wave: two calls are bit-equal."""
    s = _setup(ne)
    assert s["tabs"][("one", "wide")]["diag_bin"] is not None
    a_s, a_p, _, _ = _run(s, "one", "wide", X.ALL_ON)
    b_s, b_p, _, _ = _run(s, "one", "wide", X.ALL_ON)
    assert np.array_equal(a_s, b_s) and np.array_equal(a_p, b_p)
    assert not np.array_equal(a_p[:, s["active"]], s["ph"][:, s["active"]])


# ------------------------------------------------------------------------------------------------ 5. guarded call
def test_guarded_call_runs_the_separate_statistics_pass():
    """The wide kernel writes no guard partials: qp_collision_step_guarded = qp_collision_step + qp_pauli_stats."""
    s = _setup(100)
    tab = s["tabs"][("one", "wide")]
    assert _route(s, tab, X.ALL_ON) == _wide_route()
    out, ph, out_dev, stats = _run(s, "one", "wide", X.ALL_ON, guarded=True)
    want_s, want_p, plain_dev, _ = _run(s, "one", "wide", X.ALL_ON)
    assert np.array_equal(out, want_s) and np.array_equal(ph, want_p)
    assert stats == s["eng"].pauli_stats(plain_dev, tab, FLOOR)
    px = s["active"]
    f = np.where(s["rho"][0][:, None] > 1e-30, out[:, px] / np.maximum(s["rho"][0][:, None], 1e-30), 0.0)
    k = int(np.argmax(f))
    assert stats[0] == f.reshape(-1)[k] and stats[1] == (k // int(px.sum()), np.flatnonzero(px)[k % int(px.sum())])


# ------------------------------------------------------------------------------------------------ 6. member tables
MEMBER_TAU = [440.0, 300.0, 650.0]


def test_member_classes_are_bit_equal_to_lone_wide_calls():
    """Three members of 128 cells with tau_0 differing per member, read through `cls`: each member's cells come out as in
    a lone call with that member's single table."""
    torch = _torch()
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    ne, M, ncm = 72, len(MEMBER_TAU), 128
    mask = np.ones((8, 16), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, 180.0, 0.1)] * M)
    kr = np.stack([T.recombination_kernel_base(E, 180.0, tau, 1.2) for tau in MEMBER_TAU])
    ks = np.stack([T.scattering_kernel_base(E, 180.0, tau, 1.2) for tau in MEMBER_TAU])
    tab = eng.make_collision_tables(kr, ks, rho, idx_d, idx_s, sg, None, members=M, member_classes=True, wide_bins=True)
    lone = [eng.make_collision_tables(kr[m][None], ks[m][None], rho[m][None], idx_d, idx_s, sg, wide_bins=True)
            for m in range(M)]
    assert tab["kernel"] == "wave" and tab["struct"].flags == 32 | 8 and tab["nclass"] == M and tab["fast"]
    n = M * ncm
    route = lambda t, nc: eng.lib.qp_collision_route(C.byref(t["struct"]), nc, 1, 1, 1, 0)          # noqa: E731
    assert route(tab, n) == _wide_route() and all(route(t, ncm) == _wide_route() for t in lone)
    rng = np.random.default_rng(1000 * ne + ncm)
    level = rng.choice([1e-5, 1e-2, 0.5, 0.95], size=n)
    state_host = rng.random((ne, n)) * np.repeat(rho.T, ncm, axis=1) * level[None, :] + 1e-12
    ph_host = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    flags_host = np.where(rng.random(n) < 0.9, 16, 0).astype(np.uint8)
    flags_host[ncm - 64:ncm] = 0                   # the last wave of member 0
    flags_host[2 * ncm], flags_host[2 * ncm + 1] = 0, 16
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=eng.device)          # noqa: E731
    state, ph0, flags = d(state_host), d(ph_host), d(flags_host)
    outs, phs = [], []
    for m in range(M):
        sl = slice(m * ncm, (m + 1) * ncm)
        si, pi, fl = (a[..., sl].contiguous() for a in (state, ph0, flags))
        so = torch.full_like(si, -7.0)
        eng.collide(lone[m], si, so, pi, float(dE), DT, True, True, True, ncell=ncm, flags=fl)
        outs.append(so.cpu().numpy())
        phs.append(pi.cpu().numpy())
    want_s, want_p = np.concatenate(outs, axis=1), np.concatenate(phs, axis=1)
    out, ph = torch.full_like(state, -7.0), ph0.clone()
    eng.collide(tab, state, out, ph, float(dE), DT, True, True, True, ncell=n, flags=flags)
    assert np.array_equal(out.cpu().numpy(), want_s) and np.array_equal(ph.cpu().numpy(), want_p)
    inactive = flags_host == 0
    assert np.array_equal(want_s[:, inactive], state_host[:, inactive])
    assert np.array_equal(want_p[:, inactive], ph_host[:, inactive])
    assert not np.array_equal(want_s[:, ~inactive], state_host[:, ~inactive])
    # the members differ through their tables alone: member 2 with member 0's table gives another result
    sl = slice(2 * ncm, 3 * ncm)
    si, pi, fl = (a[..., sl].contiguous() for a in (state, ph0, flags))
    so = torch.full_like(si, -7.0)
    eng.collide(lone[0], si, so, pi, float(dE), DT, True, True, True, ncell=ncm, flags=fl)
    assert not np.array_equal(so.cpu().numpy(), want_s[:, sl])


# ------------------------------------------------------------------------------------------------ 7. public interface
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


def _route_of(eng, h, ncell, scratch):
    return eng.lib.qp_collision_route(C.byref(h["struct"]), ncell, 1, 1, 1, scratch)


def _hole_problem():
    """12 x 10 cells with a hole of 3 x 2, reflective and Dirichlet edges alternating."""
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((12, 10), dtype=bool)
    mask[4:7, 5:7] = False
    edges = extract_edge_segments(mask)
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 1e-5)]
    return mask, edges, {e.edge_id: kinds[i % 2] for i, e in enumerate(edges)}


def test_run_keyword_takes_the_wide_route_and_agrees_with_the_default(monkeypatch):
    from qpsim_amd import _hip as H
    seen = _capture_tables(monkeypatch)
    mask, edges, bcs = _hole_problem()
    init = 1e-4 * (1.0 + np.random.default_rng(72).random(mask.shape))
    common = _common(mask, edges, bcs, ne=72, total_time=0.6, store_every=2, initial_field=init)
    on, ph_on = _run_lone(**common, collision_wide_bins=True)
    off, ph_off = _run_lone(**common, collision_wide_bins=False)
    never, ph_never = _run_lone(**common)
    assert len(seen) == 3
    (e_on, h_on), (e_off, h_off), (e_nv, h_nv) = seen
    assert h_on["struct"].flags == 32 and h_on["kernel"] == "wave" and h_on["fast"]
    assert _route_of(e_on, h_on, e_on.ncell, 0) == H.ROUTE_WAVE_WIDE
    for e, h in ((e_off, h_off), (e_nv, h_nv)):
        assert h["struct"].flags == 0 and h["kernel"] == "generic" and _route_of(e, h, e.ncell, 1) == H.ROUTE_GENERIC
    assert len(on[0]) == 4 and ph_on["phonon_frames"] and on[4] is not None
    _assert_contract(on, off, 1e-9, ph_on, ph_off)
    print("switch on vs off: frames", _rel(np.stack(on[1]), np.stack(off[1])), "phonon frames",
          _rel(np.stack(ph_on["phonon_frames"]), np.stack(ph_off["phonon_frames"])))
    _assert_contract(off, never, 0.0, ph_off, ph_never)
    assert _rel(np.stack(on[1])[-1], np.stack(on[1])[0]) > 1e-6


def test_swept_ensemble_with_the_keyword_matches_lone_wide_runs(monkeypatch):
    from qpsim_amd import _hip as H
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    seen = _capture_tables(monkeypatch)
    mask, edges, bcs = _hole_problem()
    common = _common(mask, edges, bcs, ne=72, total_time=0.6, store_every=2, collision_wide_bins=True)
    sweep = {"tau_0": [440.0, 300.0, 650.0]}
    rng = np.random.default_rng(12 * 1000 + 72)
    members = [{"initial_field": 1e-4 * (1.0 + rng.random(mask.shape)), "phonon_history_out": {}} for _ in range(3)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=sweep, **common)
    assert len(seen) == 1
    eng, h = seen[0]
    assert h["struct"].flags == 32 | 8 and h["nclass"] == 3 and h["kernel"] == "wave"
    assert _route_of(eng, h, 3 * eng.ncell, 0) == H.ROUTE_WAVE_WIDE
    for m, mem in enumerate(members):
        kw = dict(common, initial_field=mem["initial_field"], tau_0=sweep["tau_0"][m])
        want, ph = _run_lone(**kw)
        assert seen[-1][1]["struct"].flags == 32 and _route_of(*seen[-1], seen[-1][0].ncell, 0) == H.ROUTE_WAVE_WIDE
        _assert_contract(got[m], want, 0.0, mem["phonon_history_out"], ph)
    assert _rel(np.stack(got[1][1]), np.stack(got[0][1])) > 1e-6
