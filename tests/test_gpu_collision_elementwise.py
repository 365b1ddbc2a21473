"""Collision kernels bounded element by element: |got - exact| / T, with `exact` and T from the extended-precision
evaluation `oracle.qp_oracle.collision_pixels_exact` of the same fp64 inputs.

`check` of tests/test_gpu_collision_instantiations.py (still run here, unchanged) divides by the largest plane of an
occupation level; the phonon bins that receive only recombination terms sit 1e-7 ... 1e-10 below it on dilute pixels, and
a fault confined to small rates or small values passes (tests/test_collision_exact_host.py shows two).  Here every element
is judged against its own conditioning: K_hip = max |got - exact| / T <= 4 K_ref64 + 4, K_ref64 being the same statistic
of the fp64 oracle on the same inputs (2 ... 5; it is the reference, never the kernel), for the state planes and for the
phonon planes.  Same 407-cell grid and inputs as the instantiation tests; every case asserts its route."""
from __future__ import annotations

import numpy as np
import pytest

import collision_exact as X
from test_gpu_collision_instantiations import (CLASSES_NE, HAVE_X87, ONEPASS_CLASSES_NE, ONEPASS_NE, REGISTER_NE, X87_RULE,
                                               _check_untouched, _engine, _expected_route, _oracle, _route, _run, _set_onepass,
                                               _setup, _tab, _tolerances, check)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")]

# `check` was never run with gap classes on the `regimes` grid at every size: at NE = 15 (scattering on, dt = 0.37) the
# phonon planes miss 2e-11 by the reference's conditioning, as on the plain grid (X87_RULE) - whole array 3.69e-11 (kernel -
# x87 1.51e-11, fp64 oracle - x87 2.18e-11), level 1e-5 3.74e-11 (1.53e-11, 2.21e-11).  Any group of these planes that misses
# the constant must satisfy the 80-bit rule; the per-element limit below applies to all of them regardless.
RULE = {**X87_RULE, ("classes", "regimes", "phonons"): {"all", 1e-9, 1e-5, 1e-2, 0.5, 0.95}}
_SAME: set = set()
_LONE: dict = {}


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


def _host(s):
    """`host_setup` of the grid of `s`, after one bit-for-bit comparison with the inputs `_setup` uploaded."""
    h = X.host_setup(s["ne"], s["kind"])
    if (s["ne"], s["kind"]) not in _SAME:
        assert np.array_equal(h["active"], s["active"]) and np.array_equal(h["level"], s["level"])
        assert all(np.array_equal(h[k], s[k]) for k in ("E", "rho", "kr", "ks", "cls", "ph"))
        assert all(np.array_equal(h["state"][f], s["state"][f]) for f in ("one", "classes"))
        assert h["dE"] == s["dE"] and all(np.array_equal(a, b) for a, b in zip(h["maps"], s["maps"]))
        _SAME.add((s["ne"], s["kind"]))
    return h


def _elementwise(O, h, family, combo, dt, got_s, got_p, tag):
    """K of the state and of the phonon planes against limit(K_ref64); elements with T = 0 must be equal."""
    ex = X.exact(O, h, family, combo, dt)
    (r_s, r_p), ref_differ = X.k_ref64(O, h, family, combo, dt)
    (k_s, k_p), differ = X.error_k(O, got_s, got_p, ex)
    print(f"K {tag}: state {k_s:.2f} (K_ref64 {r_s:.2f}) phonons {k_p:.2f} (K_ref64 {r_p:.2f})")
    assert ref_differ == 0 and differ == 0
    assert k_s <= X.limit(r_s), f"{tag}: state K = {k_s:.3g} > 4 x {r_s:.3g} + 4"
    assert k_p <= X.limit(r_p), f"{tag}: phonons K = {k_p:.3g} > 4 x {r_p:.3g} + 4"


def _assert_clips(O, h, family, ne, dt):
    x = X.exact(O, h, family, X.ALL_ON, dt)["x"]
    if dt >= 400.0:
        assert np.any(x == -80.0)
    if dt == 800.0 or (dt == 400.0 and ne == 12):
        assert np.any(x == 80.0)


def _case(O, monkeypatch, family, kind, ne, onepass, combo, dt):
    s = _setup(ne, kind)
    h = _host(s)
    _set_onepass(monkeypatch, onepass)
    assert _route(s, _tab(s, family, "auto"), combo) == _expected_route(family, ne, onepass)
    _assert_clips(O, h, family, ne, dt)
    out, ph, _, _ = _run(s, family, "auto", combo, dt=dt)
    _check_untouched(s, family, out, ph, combo[2])
    px = s["active"]
    got_s, got_p = out[:, px], ph[:, px]
    assert np.all(np.isfinite(got_s)) and np.all(np.isfinite(got_p))
    tag = f"{family} {kind} ne={ne} onepass={onepass} {combo} dt={dt:g}"
    ref_s, ref_p = _oracle(O, s, family, combo, dt)
    tol_s, tol_p = _tolerances(family, kind, ne)[1]
    for i, (name, got, ref, tol) in enumerate((("state", got_s, ref_s, tol_s), ("phonons", got_p, ref_p, tol_p))):
        check(got, ref, s["level"], tol, f"{tag} {name} vs oracle", rule=RULE.get((family, kind, name), ()), ref64=ref,
              ref80=lambda i=i: _oracle(O, s, family, combo, dt, np.longdouble)[i])
    _elementwise(O, h, family, combo, dt, got_s, got_p, tag)


def _settings(family, sizes):
    onepass = ONEPASS_NE if family == "one" else ONEPASS_CLASSES_NE
    return [(family, ne, op) for ne in sizes for op in (("1", "0") if ne in onepass else (None,))]


EVERY = _settings("one", REGISTER_NE) + _settings("classes", CLASSES_NE)
MERGED = _settings("one", sorted(X.MERGED_FMAX)) + _settings("classes", sorted(X.MERGED_FMAX))
SWEEP = _settings("one", X.SWEEP_NE) + _settings("classes", X.SWEEP_NE)


@pytest.mark.parametrize("dt", [1e-7, 0.37])
@pytest.mark.parametrize("en_r,en_s,upd", X.COMBOS)
@pytest.mark.parametrize("family,ne,onepass", EVERY)
def test_every_size_element_by_element(O, monkeypatch, family, ne, onepass, en_r, en_s, upd, dt):
    """Every register and one-pass instantiation with phonon update, at the step of the instantiation tests and at 1e-7,
    where every rate x step is far below 1/8 (the `exp_small` / `phi_small` path of the single-pass register kernels, NE < 32)."""
    _case(O, monkeypatch, family, "regimes", ne, onepass, (en_r, en_s, upd), dt)


@pytest.mark.parametrize("family,ne,onepass", MERGED)
def test_merged_bins_element_by_element(O, monkeypatch, family, ne, onepass):
    """Bins fed by a diagonal and an anti-diagonal: the recombination planes are smallest here (down to 1e-10 of the
    level's maximum)."""
    _case(O, monkeypatch, family, "merged", ne, onepass, X.ALL_ON, 0.37)


@pytest.mark.parametrize("dt", X.SWEEP_DT)
@pytest.mark.parametrize("family,ne,onepass", SWEEP)
def test_time_step_sweep_element_by_element(O, monkeypatch, family, ne, onepass, dt):
    """3e-3 ... 800: from rounding-dominated e^x - 1 to both clips of the exponent (asserted on the host for 400 and
    800)."""
    _case(O, monkeypatch, family, "regimes", ne, onepass, X.ALL_ON, dt)


def _lone(ne):
    """`host_setup` uploaded for the kernels that need no structured bin maps (NE = 65 has none on this grid), with the
    tables of one gap class for the generic and, up to NE = 64, the one-wave-per-pixel kernel."""
    if ne not in _LONE:
        eng, h = _engine(), X.host_setup(ne, "regimes")
        assert np.array_equal(h["active"], eng.mask_flat)
        d = lambda a: eng.torch.as_tensor(np.ascontiguousarray(a), device=eng.device)          # noqa: E731
        args = (h["kr"][:1], h["ks"][:1], h["rho"][:1], *h["maps"])
        tabs = {("one", k): eng.make_collision_tables(*args, kernel=k) for k in ("generic", "wave") if k == "generic" or ne <= 64}
        assert all(t["kernel"] == k for (_, k), t in tabs.items())
        _LONE[ne] = dict(h, eng=eng, state_dev={"one": d(h["state"]["one"])}, ph_dev=d(h["ph"]), tabs=tabs)
    return _LONE[ne]


@pytest.mark.parametrize("dt", X.LONE_DT)
@pytest.mark.parametrize("kernel,ne", [("generic", ne) for ne in X.GENERIC_NE] + [("wave", ne) for ne in X.WAVE_NE])
def test_generic_and_wave_kernels_element_by_element(O, kernel, ne, dt):
    """What every other collision test compares against, itself against the exact evaluation."""
    from qpsim_amd import _hip as H
    s, combo = _lone(ne), X.ALL_ON
    assert _route(s, s["tabs"][("one", kernel)], combo) == (H.ROUTE_GENERIC if kernel == "generic" else H.ROUTE_WAVE)
    _assert_clips(O, s, "one", ne, dt)
    out, ph, _, _ = _run(s, "one", kernel, combo, dt=dt)
    _check_untouched(s, "one", out, ph, True)
    px = s["active"]
    got_s, got_p = out[:, px], ph[:, px]
    assert np.all(np.isfinite(got_s)) and np.all(np.isfinite(got_p))
    tag = f"{kernel} ne={ne} dt={dt:g}"
    ref_s, ref_p = _oracle(O, s, "one", combo, dt)
    tol_s, tol_p = _tolerances("one", "regimes", ne)[1]
    for i, (name, got, ref, tol) in enumerate((("state", got_s, ref_s, tol_s), ("phonons", got_p, ref_p, tol_p))):
        check(got, ref, s["level"], tol, f"{tag} {name} vs oracle", rule=RULE.get(("one", "regimes", name), ()), ref64=ref,
              ref80=lambda i=i: _oracle(O, s, "one", combo, dt, np.longdouble)[i])
    _elementwise(O, s, "one", combo, dt, got_s, got_p, tag)
