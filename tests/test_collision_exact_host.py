"""The per-element error criterion of the collision tests, checked without a GPU.

`check` of tests/test_gpu_collision_instantiations.py divides by the largest plane of an occupation level, and the phonon
planes of one pixel span many orders of magnitude: the bins that receive only recombination terms sit 1e-7 ... 1e-10 below
the largest plane on dilute pixels.  tests/test_gpu_collision_elementwise.py bounds |got - exact| / T element by element
instead, with `exact` and T from `oracle.qp_oracle.collision_pixels_exact`.  Here: that evaluation against the oracle's
routine on extended-precision inputs, K_ref64 (the K of the fp64 oracle) for every case of the GPU test, and three wrong
variants of the fp64 oracle that pass `check` at its constants and miss the new limit (two of them on the dilute pixels;
the third is the fault this criterion found in the register kernels)."""
from __future__ import annotations

import math
import platform

import numpy as np
import pytest

import collision_exact as X
from test_collision_route_host import AVAILABLE
from test_gpu_collision_instantiations import HAVE_X87, X87_RULE, _tolerances, check

REGISTER_NE = AVAILABLE["qp_collision_register_kernel_available"]
CLASSES_NE = AVAILABLE["qp_collision_register_kernel_classes"]
CASES = X.register_cases({"one": REGISTER_NE, "classes": CLASSES_NE}) + X.lone_cases()
GROUPS = sorted({(c[0], c[1], c[2]) for c in CASES})

if platform.machine() in ("x86_64", "AMD64"):
    assert HAVE_X87, "x86-64 has an 80-bit long double"
pytestmark = pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


def _family(name):
    """The generic and wave kernels run the tables of one gap class."""
    return name if name in ("one", "classes") else "one"


def _oracle80(O, h, family, combo, dt):
    """`O.collision_step`, the reference's formulas, on extended-precision inputs."""
    LD = np.longdouble
    t = X.oracle_tables(h, family, combo)
    t = {k: (np.asarray(v, dtype=LD) if k in ("rho", "Kr0", "Ks0") and v is not None else v) for k, v in t.items()}
    t["dE"] = LD(t["dE"])
    px = h["active"]
    s, p = h["state"][family][:, px].astype(LD), h["ph"][:, px].astype(LD)
    O.collision_step(s, p, t, LD(dt), en_r=combo[0], en_s=combo[1], update_phonons=combo[2])
    return s, p


@pytest.mark.parametrize("dt", [1e-7, 3e-3, 0.37, 25.0, 400.0])
@pytest.mark.parametrize("family,kind,ne", [("one", "regimes", 12), ("classes", "regimes", 12), ("one", "merged", 12),
                                            ("classes", "regimes", 50), ("one", "merged", 50), ("one", "regimes", 3)])
def test_exact_evaluation_is_the_oracle_routine_in_extended_precision(O, family, kind, ne, dt):
    """Same function, two codes.  Where |x| >= 1e-3 the reference's (e^x - 1) / b loses at most 2^-63 / 1e-3 = 1e-16 in
    80-bit arithmetic and the two agree to 1e-15 of each element.  Below, the 80-bit routine has the cancellation the
    exact one avoids: 2^-63 max(1, e^x) A / |b| = 2^-10 of the second term of T (same form, u = 2^-53), so the
    difference is bounded by 1e-15 of the element + 2^-10 T.  The two codes sum b in different orders, so an element
    could take different branches of the |b| < 1e-14 switch only with |b| within 2^-60 of the threshold: no element may
    differ by the J rule, and none in the window [0.5e-14, 2e-14] differs by more than the bound above either."""
    h = X.host_setup(ne, kind)
    ex = X.exact(O, h, family, X.ALL_ON, dt)
    s80, p80 = _oracle80(O, h, family, X.ALL_ON, dt)
    d_p = np.abs(p80 - ex["p"])
    big = np.abs(ex["x"]) >= 1e-3
    assert np.all(d_p[big] <= 1e-15 * ex["p"][big])
    assert np.all(d_p <= 1e-15 * ex["p"] + 2.0 ** -10 * ex["T_ph"])
    assert np.all(np.abs(s80 - ex["n"]) <= 1e-15 * ex["n"] + 2.0 ** -10 * ex["T_n"])
    assert np.all(ex["T_ph"] >= O.U53 * ex["p"]) and np.all(ex["T_n"] >= O.U53 * ex["n"])
    print(f"{family} {kind} ne={ne} dt={dt:g}: {int(big.sum())} of {big.size} phonon elements with |x| >= 1e-3, "
          f"max |80-bit routine - exact| / T = {float(np.max(d_p[ex['T_ph'] > 0] / ex['T_ph'][ex['T_ph'] > 0])):.2e}")


@pytest.mark.parametrize("name,kind,ne", GROUPS)
def test_k_of_the_fp64_reference_for_every_gpu_case(O, name, kind, ne):
    """K_ref64 of every (process combination, dt) the GPU test runs at this size: finite, no element with T = 0 that
    differs, fewer than 1 % of the phonon elements in the window of the |b| < 1e-14 switch (a condition on the seeds of
    `_setup`, not a tolerance: inside the window T grows by J and checks less)."""
    h = X.host_setup(ne, kind)
    for _, _, _, combo, dt in [c for c in CASES if (c[0], c[1], c[2]) == (name, kind, ne)]:
        ex = X.exact(O, h, _family(name), combo, dt)
        (k_s, k_p), differ = X.k_ref64(O, h, _family(name), combo, dt)
        share = float(ex["window"].mean())
        print(f"{name} {kind} ne={ne} {combo} dt={dt:g}: K_ref64 state {k_s:.2f} phonons {k_p:.2f}, window {share:.2%}, "
              f"x in [{float(ex['x'].min()):.3g}, {float(ex['x'].max()):.3g}]")
        assert math.isfinite(k_s) and math.isfinite(k_p) and differ == 0
        assert share < 0.01


@pytest.mark.parametrize("name,ne,dt", sorted({(c[0], c[2], c[4]) for c in CASES if c[4] >= 400.0}))
def test_long_steps_reach_both_clips_of_the_exponent(O, name, ne, dt):
    """dt = 400 on the `regimes` inputs: b dt < -80 for a third of the phonon elements at every size, b dt > 80 at NE = 12
    (at NE = 24 the largest b dt is 73, at NE = 30 61).  dt = 800 reaches both clips at every size of the sweep, so the
    single-pass register kernels, which have the small-|x| path, see the upper clip at three sizes."""
    x = X.exact(O, X.host_setup(ne, "regimes"), _family(name), X.ALL_ON, dt)["x"]
    lo, hi = float(np.mean(x == -80.0)), float(np.mean(x == 80.0))
    print(f"{name} ne={ne} dt={dt:g}: {lo:.1%} of the phonon elements clipped at -80, {hi:.2%} at +80")
    assert lo > 0.05
    if ne == 12 or dt == 800.0:
        assert hi > 0.0


# ------------------------------------------------------------------------------------------------ sensitivity
def _small_x_affine(last):
    """`affine_growth` with the small-|x| form of the NE < 30 kernels (phi(x) = (e^x - 1) / x by its Taylor series, the
    reference's rounding of e^x re-applied) in NumPy, the series ending at x^last / (last + 1)!; the kernels' ends at
    x^9 / 10!."""
    def affine_growth(y, a, b, dt):
        x = np.clip(b * dt, -80.0, 80.0)
        ex = np.exp(x)
        tiny = np.abs(b) < 1e-14
        general = np.maximum(ex * y + np.where(tiny, dt, (ex - 1.0) / np.where(tiny, 1.0, b)) * a, 0.0)
        phi = np.zeros_like(x)
        for k in range(last, -1, -1):
            phi = phi * x + 1.0 / math.factorial(k + 1)
        u = x * phi
        e = 1.0 + u
        with np.errstate(divide="ignore", invalid="ignore"):
            g = phi + ((e - 1.0) - u) / x
        small = np.maximum(e * y + np.where(tiny, dt, dt * g) * a, 0.0)
        return np.where(np.abs(x) < 0.125, small, general)
    return affine_growth


def _old_check_passes(h, family, got, ref):
    """`check` against the fp64 oracle at the constants of the GPU tests, state and phonons."""
    tol_s, tol_p = _tolerances(family, h["kind"], h["ne"])[1]
    for name, g, r, tol in (("state", got[0], ref[0], tol_s), ("phonons", got[1], ref[1], tol_p)):
        check(g, r, h["level"], tol, f"wrong variant, {name} vs oracle", rule=X87_RULE.get((family, h["kind"], name), ()))


def _dilute_k(O, h, family, dt, got):
    ex = X.exact(O, h, family, X.ALL_ON, dt)
    (k_s, k_p), _ = X.error_k(O, got[0], got[1], ex, h["level"] <= X.DILUTE)
    (r_s, r_p), _ = X.k_ref64(O, h, family, X.ALL_ON, dt)
    return (k_s, X.limit(r_s)), (k_p, X.limit(r_p))


@pytest.mark.parametrize("family,ne,dt", [("one", 12, 1e-7), ("classes", 12, 1e-7), ("one", 24, 1e-7), ("classes", 50, 1e-7)])
def test_a_table_entry_wrong_by_1e_6_passes_the_level_norm_and_misses_the_element_limit(O, family, ne, dt):
    """K^r_0 of the last anti-diagonal (one entry, the top recombination bin) scaled by 1 + 1e-6 in every class, at the
    step of 1e-7 at which no level's own maximum shows the recombination planes (at 0.37 the same fault moves the state
    of the dense pixels by 2e-9 and `check` sees it)."""
    h = X.host_setup(ne, "regimes")
    kr = h["kr"].copy()
    kr[:, -1, -1] *= 1.0 + 1e-6
    got = X.run_oracle64(O, h, family, X.ALL_ON, dt, kr=kr)
    _old_check_passes(h, family, got, X.run_oracle64(O, h, family, X.ALL_ON, dt))
    _, (k_p, lim) = _dilute_k(O, h, family, dt, got)
    print(f"{family} ne={ne} dt={dt:g}: K on the pixels of level <= {X.DILUTE:g} = {k_p:.3g} (limit {lim:.3g})")
    assert k_p > lim


@pytest.mark.parametrize("ne", [12, 24])
def test_a_truncated_small_x_series_passes_the_level_norm_and_misses_the_element_limit(O, monkeypatch, ne):
    """The series of the small-|x| coefficient cut short.  Dropping ONE term (x^9 / 10!) cannot be seen by any criterion
    that admits the reference's own rounding: the relative error of the coefficient is at most (1/8)^9 / 10! = 18.5 u,
    the coefficient's term of p' is at most |x| <= 1/8 of the second term of T / u, so K rises by at most 18.5 / 8 = 2.3
    (asserted).  Dropping two terms (remainder (1/8)^8 / 9! = 1480 u, K up to 185) is seen, on the dilute pixels too,
    while `check` still passes at its constants."""
    h, dt = X.host_setup(ne, "regimes"), 0.37
    ref = X.run_oracle64(O, h, "one", X.ALL_ON, dt)
    k = {}
    for last in (9, 8, 7):
        monkeypatch.setattr(O, "affine_growth", _small_x_affine(last))
        got = X.run_oracle64(O, h, "one", X.ALL_ON, dt)
        monkeypatch.undo()
        _old_check_passes(h, "one", got, ref)
        _, (k[last], lim) = _dilute_k(O, h, "one", dt, got)
        print(f"ne={ne}: series to x^{last}: K on the pixels of level <= {X.DILUTE:g} = {k[last]:.3g} (limit {lim:.3g})")
    assert k[9] <= lim                       # the kernels' own form, evaluated in NumPy, is within the limit
    assert k[8] <= k[9] + 2.3
    assert k[7] > lim


def _contracted_relaxation(dE):
    """`relaxation_update` with mu - loss formed as fma(-dE, la, mu) for loss = dE la: the rounding error of the product
    instead of 0.  What the single-pass register kernels computed until this criterion was run against them."""
    def relaxation_update(n, gain, loss, dt):
        la = loss / dE
        mu = np.maximum(dE * la, 0.0)
        slip = (mu.astype(np.longdouble) - np.longdouble(dE) * la.astype(np.longdouble)).astype(np.float64)
        P = np.maximum(gain + slip * n, 0.0)
        decay = np.exp(-mu * dt)
        small = mu < 1e-14
        return np.maximum(decay * n + np.where(small, dt, (1.0 - decay) / np.where(small, 1.0, mu)) * P, 0.0)
    return relaxation_update


@pytest.mark.parametrize("ne,dt", [(12, 25.0), (24, 400.0)])
def test_a_contracted_loss_product_passes_the_level_norm_and_misses_the_element_limit(O, monkeypatch, ne, dt):
    """Half an ulp of the loss times n in P: 1e-16 of n in absolute terms, 1e-11 of n' in the top bins of dense pixels that
    a long step depletes.  Against the level's maximum it is 1e-16; element by element K is in the hundreds."""
    h = X.host_setup(ne, "regimes")
    ref = X.run_oracle64(O, h, "one", X.ALL_ON, dt)
    monkeypatch.setattr(O, "relaxation_update", _contracted_relaxation(h["dE"]))
    got = X.run_oracle64(O, h, "one", X.ALL_ON, dt)
    monkeypatch.undo()
    _old_check_passes(h, "one", got, ref)
    (k_s, _), _ = X.error_k(O, got[0], got[1], X.exact(O, h, "one", X.ALL_ON, dt))
    (r_s, _), _ = X.k_ref64(O, h, "one", X.ALL_ON, dt)
    print(f"ne={ne} dt={dt:g}: state K = {k_s:.3g} (limit {X.limit(r_s):.3g})")
    assert k_s > X.limit(r_s)
