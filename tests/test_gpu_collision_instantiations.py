"""Every instantiation of the register and one-pass collision kernels against the generic kernel and the fp64 oracle.

Each (NE, scattering, recombination, phonon update, gap classes) is its own fully unrolled code object with its own register
allocation, prefetch-ring edges and (one-pass) ragged target blocks, so every size in the availability lists of
tests/test_collision_route_host.py runs here, on one small masked grid, and every test asserts the route it is written for.
Errors are bounded over the whole array AND per occupation level (each level against its own maximum): pixels at 1e-5 of
the density of states would otherwise be discounted by five orders of magnitude against those at 0.95."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from collision_grids import MERGED_FMAX, unmerged_fmax
from golden_utils import rel_err
from test_collision_route_host import AVAILABLE
from test_gpu_parity import PHONON_TOL, PROCESS_COMBOS

pytestmark = pytest.mark.gpu

REGISTER_NE = AVAILABLE["qp_collision_register_kernel_available"]
CLASSES_NE = AVAILABLE["qp_collision_register_kernel_classes"]
ONEPASS_NE = AVAILABLE["qp_collision_onepass_available"]
ONEPASS_CLASSES_NE = [50]                      # QP_ONEPASS_CLASSES_NE_LIST has no query of its own
COPY_NE = [2, 12, 50]
REGIME_ONE_NE, REGIME_CLASSES_NE = [24, 30], [12, 30, 50]
assert set(ONEPASS_CLASSES_NE) <= set(ONEPASS_NE) & set(CLASSES_NE)
assert set(COPY_NE) | set(REGIME_ONE_NE) <= set(REGISTER_NE) and set(REGIME_CLASSES_NE) <= set(CLASSES_NE)
assert set(MERGED_FMAX) <= set(REGISTER_NE) and set(MERGED_FMAX) <= set(CLASSES_NE)

GAPS = np.array([180.0, 171.0, 165.5, 176.25])          # class 0 is the one gap class of the "one" family
LEVELS = {"plain": [1e-5, 1e-2, 0.5, 0.95], "merged": [1e-5, 1e-2, 0.5, 0.95], "regimes": [1e-9, 1e-5, 1e-2, 0.5, 0.95]}
DT, FLOOR = 0.37, 1e-18


def _settings(sizes, onepass_sizes):
    """(ne, QPSIM_COLL_ONEPASS): both settings where a one-pass kernel exists, the environment's default elsewhere."""
    return [(ne, op) for ne in sizes for op in (("1", "0") if ne in onepass_sizes else (None,))]


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


# ------------------------------------------------------------------------------------------------ shared set-up
_ENGINE: list = []
_SETUPS: dict = {}
_REFS: dict = {}


def _engine():
    """11 x 37 = 407 cells: 4 blocks of 128 threads (23 lanes in the last), 2 ragged blocks of 256; the wave of cells
    64 ... 127 and about a fifth of the others inactive, cell 0 active, cell 128 (lane 0 of a wave and of a block) not."""
    if not _ENGINE:
        from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
        active = np.random.default_rng(407).random(407) > 0.2
        active[64:128] = False
        active[0], active[128] = True, False
        mask = active.reshape(11, 37)
        z = np.zeros(mask.shape)
        eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
        assert eng.ncell == 407 and active[384:].any() and not active[384:].all()
        _ENGINE.append(eng)
    return _ENGINE[0]


def _setup(ne, kind):
    """Grid, tables of the four gap classes and inputs over ALL cells (inactive ones hold data too), built once."""
    key = (ne, kind)
    if key in _SETUPS:
        return _SETUPS[key]
    from qpsim_amd import tables as T
    from qpsim_amd.engine import structured_bin_maps
    eng = _engine()
    n = eng.ncell
    E, dE = T.build_energy_grid(180.0, 1.0, MERGED_FMAX[ne] if kind == "merged" else unmerged_fmax(ne), ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    if kind == "merged":
        assert structured_bin_maps(idx_d, idx_s, sg) is None
        assert structured_bin_maps(idx_d, idx_s, sg, allow_shared=True) is not None
    else:
        assert structured_bin_maps(idx_d, idx_s, sg) is not None and om.size == 3 * ne - 1
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in GAPS])
    kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in GAPS])
    ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in GAPS])
    rng = np.random.default_rng(1000 * ne + len(kind))
    cls = rng.integers(0, GAPS.size, size=n)
    level = rng.choice(LEVELS[kind], size=n)
    u = rng.random((ne, n))
    state = {"one": u * rho[0][:, None] * level[None, :], "classes": u * rho[cls].T * level[None, :]}
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    d = lambda a: eng.torch.as_tensor(np.ascontiguousarray(a), device=eng.device)          # noqa: E731
    active = eng.mask_flat.copy()
    s = dict(eng=eng, ne=ne, kind=kind, E=E, dE=float(dE), nw=om.size, maps=(idx_d, idx_s, sg), rho=rho, kr=kr, ks=ks, cls=cls,
             level=level[active], active=active, state=state, ph=ph, state_dev={f: d(a) for f, a in state.items()},
             ph_dev=d(ph), tabs={})
    _SETUPS[key] = s
    return s


def _tab(s, family, kernel):
    """Tables of one family ("one" gap class / gap "classes") for the default kernel choice or the generic kernel."""
    if (family, kernel) not in s["tabs"]:
        eng = s["eng"]
        if family == "one":
            tab = eng.make_collision_tables(s["kr"][:1], s["ks"][:1], s["rho"][:1], *s["maps"], allow_fast=kernel == "auto")
        else:
            tab = eng.make_collision_tables(s["kr"], s["ks"], s["rho"], *s["maps"], s["cls"][s["active"]], kernel=kernel,
                                            gap_params=dict(E=s["E"], gaps=GAPS, tau_r=500.0, tau_s=400.0, T_c=1.2))
        assert tab["kernel"] == ("register" if kernel == "auto" else "generic")
        assert (tab["merged_slots"] > 0) == (s["kind"] == "merged") and tab["nw"] == s["nw"]
        s["tabs"][(family, kernel)] = tab
    return s["tabs"][(family, kernel)]


def _route(s, tab, combo):
    """The library's answer for the call `Engine.collide` makes with these tables and switches."""
    from qpsim_amd.collision_tables import scratch_planes
    en_r, en_s, upd = combo
    scratch = scratch_planes(tab, en_r, en_s, upd) > 0
    return s["eng"].lib.qp_collision_route(C.byref(tab["struct"]), s["eng"].ncell, int(en_r), int(en_s), int(upd), int(scratch))


def _expected_route(family, ne, onepass):
    from qpsim_amd import _hip as H
    if family == "one":
        return H.ROUTE_ONEPASS if ne in ONEPASS_NE and onepass != "0" else H.ROUTE_REGISTER
    return H.ROUTE_ONEPASS_CLASSES if ne in ONEPASS_CLASSES_NE and onepass != "0" else H.ROUTE_REGISTER_CLASSES


def _set_onepass(monkeypatch, onepass):
    if onepass is None:
        monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    else:
        monkeypatch.setenv("QPSIM_COLL_ONEPASS", onepass)         # read by the library at every call


def _run(s, family, kernel, combo, dt=DT, guarded=False, state_dev=None):
    """One collision call on fresh copies: (state_out, phonons) as host arrays over ALL cells, state_out on the device,
    the guard ticket's result."""
    eng, tab = s["eng"], _tab(s, family, kernel)
    en_r, en_s, upd = combo
    s_in = s["state_dev"][family] if state_dev is None else state_dev
    out, ph = eng.torch.full_like(s_in, -7.0), s["ph_dev"].clone()
    stats = None
    if guarded:
        stats = eng.pauli_stats_result(eng.collide_guarded(tab, s_in, out, ph, s["dE"], dt, en_r, en_s, upd, FLOOR))
    else:
        eng.collide(tab, s_in, out, ph, s["dE"], dt, en_r, en_s, upd)
    return out.cpu().numpy(), ph.cpu().numpy(), out, stats


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _generic(s, family, combo):
    """The generic kernel's result on the active cells, computed once per case."""
    key = ("generic", s["ne"], s["kind"], family, combo)
    if key not in _REFS:
        from qpsim_amd import _hip as H
        assert _route(s, _tab(s, family, "generic"), combo) == H.ROUTE_GENERIC
        out, ph, _, _ = _run(s, family, "generic", combo)
        _REFS[key] = _frozen(out[:, s["active"]], ph[:, s["active"]])
    return _REFS[key]


def _oracle(O, s, family, combo, dt=DT, dtype=np.float64):
    """`O.collision_step` on the active cells in fp64 (computed once per case), or in extended precision."""
    key = ("oracle", s["ne"], s["kind"], family, combo, dt, np.dtype(dtype).name)
    if key not in _REFS:
        en_r, en_s, upd = combo
        A = lambda a: np.asarray(a, dtype=dtype)          # noqa: E731
        px = s["active"]
        nc = 1 if family == "one" else GAPS.size
        idx_d, idx_s, sg = s["maps"]
        tables = {"rho": A(s["rho"][:nc]), "Kr0": A(s["kr"][:nc]) if en_r else None, "Ks0": A(s["ks"][:nc]) if en_s else None,
                  "cls": s["cls"][px] if nc > 1 else np.zeros(int(px.sum()), dtype=int), "idx_diff": idx_d, "idx_sum": idx_s,
                  "sign": sg, "dE": dtype(s["dE"])}
        s_ref, p_ref = A(s["state"][family][:, px]).copy(), A(s["ph"][:, px]).copy()
        O.collision_step(s_ref, p_ref, tables, dtype(dt), en_r=en_r, en_s=en_s, update_phonons=upd)
        _REFS[key] = _frozen(s_ref, p_ref)
    return _REFS[key]


# Where the constants are missed by the reference's own conditioning, not by a kernel ("Collision kernel
# coverage", records the distances): (family, grid kind, planes) -> the groups of `check` that may instead satisfy the rule
# of test_phonon_tolerance_is_the_conditioning_of_the_reference_formula_not_a_kernel_error.  On energy_max_factor = 3.0 at
# NE = 50 the fp64 oracle itself sits 1.5e-10 from the 80-bit evaluation of the phonon update, above PHONON_TOL.
X87_RULE = {("one", "plain", "phonons"): {"all", 0.95}, ("one", "merged", "phonons"): {"all", 1e-5, 0.95},
            ("classes", "plain", "phonons"): {"all", 0.5, 0.95}, ("classes", "merged", "phonons"): {1e-5},
            ("one", "regimes", "state"): {1e-9}, ("classes", "regimes", "state"): {1e-9}}
HAVE_X87 = bool(np.finfo(np.longdouble).eps < 2e-19)


def check(got, want, levels, tol, what, rule=(), ref64=None, ref80=None):
    """max |got - want| / max |want| < tol over the whole array and over the pixels of each occupation level alone (each
    level against its own maximum).  A group named in `rule` that misses `tol` passes if the kernel is as close to the
    extended-precision evaluation `ref80()` as the fp64 oracle `ref64` is: e_hip <= 4 e_ref64 + 1e-14, both normalised by
    the group's maximum.  Without an 80-bit long double on the host only the constant is available."""
    for name, g in [("all", slice(None))] + [(float(lv), levels == lv) for lv in np.unique(levels)]:
        e = rel_err(got[:, g], want[:, g])
        line = f"{what} [{name}]: {e:.2e} (tol {tol:g})"
        if not e < tol and ref80 is not None and HAVE_X87:
            x = ref80()[:, g]
            e_hip, e_ref = (float(np.max(np.abs(a[:, g].astype(np.longdouble) - x)) / np.max(np.abs(x))) for a in (got, ref64))
            line += f"  |hip - x87| = {e_hip:.2e}  |fp64 oracle - x87| = {e_ref:.2e}"
            if name in rule:
                print(line)
                assert e_hip <= 4.0 * e_ref + 1e-14, line
                continue
        print(line)
        assert e < tol, line


def _tolerances(family, kind, ne):
    """The project's bounds of tests/test_gpu_parity.py: ((state, phonons) against the generic kernel, against the oracle)."""
    plain_one = family == "one" and kind != "merged"
    return ((1e-12, 1e-11 if ne <= 16 else PHONON_TOL),
            (2e-11 if (plain_one or ne <= 16) else 1e-10, 2e-11 if ne <= 16 else PHONON_TOL))


def _check_untouched(s, family, out, ph, upd):
    """Inactive cells (the inactive wave, holes, up to the ragged end) pass through; frozen phonons stay bit-equal."""
    hole = ~s["active"]
    assert np.array_equal(out[:, hole], s["state"][family][:, hole])
    assert np.array_equal(ph[:, hole], s["ph"][:, hole])
    assert not np.any(out[:, s["active"]] == -7.0)
    if not upd:
        assert np.array_equal(ph, s["ph"])


def _check_guard(s, family, out_dev, out, stats):
    """As test_fused_pauli_guard_equals_the_separate_reduction: the fused ticket, qp_pauli_stats and NumPy agree exactly."""
    eng, px = s["eng"], s["active"]
    assert stats == eng.pauli_stats(out_dev, _tab(s, family, "auto"), FLOOR)
    rho = s["rho"][0][:, None] if family == "one" else s["rho"][s["cls"][px]].T
    f = np.where(rho > 1e-30, out[:, px] / np.maximum(rho, 1e-30), 0.0)
    k, n = int(np.argmax(f)), int(px.sum())
    mx, top, forb = stats
    assert mx == f.reshape(-1)[k] and top == (k // n, np.flatnonzero(px)[k % n]) and forb is None


def _family_case(O, monkeypatch, family, kind, ne, onepass, combo):
    s = _setup(ne, kind)
    _set_onepass(monkeypatch, onepass)
    assert _route(s, _tab(s, family, "auto"), combo) == _expected_route(family, ne, onepass)
    out, ph, out_dev, stats = _run(s, family, "auto", combo, guarded=ne < 32)
    _check_untouched(s, family, out, ph, combo[2])
    got_s, got_p, lv = out[:, s["active"]], ph[:, s["active"]], s["level"]
    tag = f"{family} {kind} ne={ne} onepass={onepass} {combo}"
    vs_generic, vs_oracle = _tolerances(family, kind, ne)
    gen_s, gen_p = _generic(s, family, combo)
    ref_s, ref_p = _oracle(O, s, family, combo)
    planes = [("state", got_s, gen_s, ref_s, 0)] + ([("phonons", got_p, gen_p, ref_p, 1)] if combo[2] else [])
    for name, got, gen, ref, i in planes:
        x87 = dict(rule=X87_RULE.get((family, kind, name), ()), ref64=ref,
                   ref80=lambda i=i: _oracle(O, s, family, combo, dtype=np.longdouble)[i])
        check(got, gen, lv, vs_generic[i], f"{tag} {name} vs generic", **x87)
        check(got, ref, lv, vs_oracle[i], f"{tag} {name} vs oracle", **x87)
    if stats is not None:
        _check_guard(s, family, out_dev, out, stats)


# ------------------------------------------------------------------------------------------------ 1. one gap class
@pytest.mark.parametrize("en_r,en_s,upd", PROCESS_COMBOS)
@pytest.mark.parametrize("ne,onepass", _settings(REGISTER_NE, ONEPASS_NE))
def test_one_gap_class_kernel_of_every_size(O, monkeypatch, ne, onepass, en_r, en_s, upd):
    """diag<NE> (NE >= 32: the three-launch split) and, where it exists, the one-pass kernel: against the generic kernel
    and the oracle, with the fused Pauli guard below NE = 32."""
    _family_case(O, monkeypatch, "one", "plain", ne, onepass, (en_r, en_s, upd))


@pytest.mark.parametrize("en_r,en_s,upd", PROCESS_COMBOS)
@pytest.mark.parametrize("ne", ONEPASS_NE)
def test_one_pass_kernel_of_every_size_equals_its_register_form(monkeypatch, ne, en_r, en_s, upd):
    """At the constants of test_one_pass_ne50_kernel_equals_the_split_kernels_on_a_ragged_masked_grid."""
    from qpsim_amd import _hip as H
    s, combo = _setup(ne, "plain"), (en_r, en_s, upd)
    res = {}
    for onepass, route in (("1", H.ROUTE_ONEPASS), ("0", H.ROUTE_REGISTER)):
        _set_onepass(monkeypatch, onepass)
        assert _route(s, _tab(s, "one", "auto"), combo) == route
        out, ph, _, _ = _run(s, "one", "auto", combo)
        res[onepass] = (out[:, s["active"]], ph[:, s["active"]])
    check(res["1"][0], res["0"][0], s["level"], 1e-13, f"ne={ne} {combo} one-pass vs register, state")
    if upd:
        check(res["1"][1], res["0"][1], s["level"], 1e-10, f"ne={ne} {combo} one-pass vs register, phonons")
    else:
        assert np.array_equal(res["1"][1], res["0"][1])


@pytest.mark.parametrize("en_r,en_s,upd", [(True, True, True), (True, True, False)])
@pytest.mark.parametrize("ne,onepass", _settings(sorted(MERGED_FMAX), ONEPASS_NE))
def test_one_gap_class_kernel_of_every_size_with_merged_phonon_bins(O, monkeypatch, ne, onepass, en_r, en_s, upd):
    """QP_COLL_SHARED_BINS (1 ... 15 shared bins): the diagonal's sums parked in scratch, or never formed when phonons are
    frozen."""
    _family_case(O, monkeypatch, "one", "merged", ne, onepass, (en_r, en_s, upd))


@pytest.mark.parametrize("ne", COPY_NE)
def test_no_process_runs_the_copy_kernel(O, ne):
    """QP_ROUTE_COPY (collision_none_kernel): n' = max(n, 0) on active cells, everything else bit-unchanged."""
    from qpsim_amd import _hip as H
    s, combo = _setup(ne, "plain"), (False, False, True)
    assert _route(s, _tab(s, "one", "auto"), combo) == H.ROUTE_COPY
    state = s["state"]["one"].copy()
    state[::2, 1::3] *= -1.0
    assert (state[:, s["active"]] < 0).any() and (state[:, ~s["active"]] < 0).any()
    out, ph, _, _ = _run(s, "one", "auto", combo, state_dev=s["eng"].torch.as_tensor(state, device=s["eng"].device))
    want = np.where(s["active"][None, :], np.maximum(state, 0.0), state)
    assert np.array_equal(out, want) and np.array_equal(ph, s["ph"])
    px = s["active"]
    idx_d, idx_s, sg = s["maps"]
    tables = {"rho": s["rho"][:1], "Kr0": s["kr"][:1], "Ks0": s["ks"][:1], "cls": np.zeros(int(px.sum()), dtype=int),
              "idx_diff": idx_d, "idx_sum": idx_s, "sign": sg, "dE": s["dE"]}
    s_ref, p_ref = state[:, px].copy(), s["ph"][:, px].copy()
    O.collision_step(s_ref, p_ref, tables, DT, en_r=False, en_s=False, update_phonons=True)
    assert np.array_equal(out[:, px], s_ref) and np.array_equal(ph[:, px], p_ref)


# ------------------------------------------------------------------------------------------------ 2. gap classes
@pytest.mark.parametrize("en_r,en_s,upd", PROCESS_COMBOS)
@pytest.mark.parametrize("ne,onepass", _settings(CLASSES_NE, ONEPASS_CLASSES_NE))
def test_gap_class_kernel_of_every_size(O, monkeypatch, ne, onepass, en_r, en_s, upd):
    """Four gap classes mixed lane by lane, K formed per pixel from the amplitude tables."""
    _family_case(O, monkeypatch, "classes", "plain", ne, onepass, (en_r, en_s, upd))


@pytest.mark.parametrize("ne,onepass", _settings(sorted(MERGED_FMAX), ONEPASS_CLASSES_NE))
def test_gap_class_kernel_of_every_size_with_merged_phonon_bins(O, monkeypatch, ne, onepass):
    _family_case(O, monkeypatch, "classes", "merged", ne, onepass, (True, True, True))


@pytest.mark.parametrize("dt", [0.0, 1e-7, 3e-3, 25.0])
@pytest.mark.parametrize("family,ne,onepass", [("one", ne, op) for ne, op in _settings(REGIME_ONE_NE, ONEPASS_NE)]
                         + [("classes", ne, op) for ne, op in _settings(REGIME_CLASSES_NE, ONEPASS_CLASSES_NE)])
def test_rate_times_step_regimes_on_both_sides_of_the_small_x_switch(O, monkeypatch, family, ne, onepass, dt):
    """test_collision_update_over_the_range_of_rate_times_step for the kernels with (NE < 30) and without (NE >= 30) the
    small-|x| polynomial path, with gap classes, and with occupation levels down to 1e-9."""
    s, combo = _setup(ne, "regimes"), (True, True, True)
    _set_onepass(monkeypatch, onepass)
    assert _route(s, _tab(s, family, "auto"), combo) == _expected_route(family, ne, onepass)
    out, ph, _, _ = _run(s, family, "auto", combo, dt=dt)
    _check_untouched(s, family, out, ph, True)
    px = s["active"]
    got_s, got_p = out[:, px], ph[:, px]
    assert np.all(np.isfinite(got_s)) and np.all(np.isfinite(got_p))
    if dt == 0.0:
        assert np.array_equal(got_s, s["state"][family][:, px]) and np.array_equal(got_p, s["ph"][:, px])
        return
    ref_s, ref_p = _oracle(O, s, family, combo, dt)
    tol_s, tol_p = _tolerances(family, "regimes", ne)[1]
    tag = f"{family} ne={ne} onepass={onepass} dt={dt:g}"
    for i, (name, got, ref, tol) in enumerate((("state", got_s, ref_s, tol_s), ("phonons", got_p, ref_p, tol_p))):
        check(got, ref, s["level"], tol, f"{tag} {name} vs oracle", rule=X87_RULE.get((family, "regimes", name), ()), ref64=ref,
              ref80=lambda i=i: _oracle(O, s, family, combo, dt, np.longdouble)[i])


# ------------------------------------------------------------------------------------------------ 3. upload of a plan
@pytest.mark.parametrize("kind,ne,cells", [("plain", 12, 64), ("member", 30, 256), ("gap", 12, 64)])
def test_handle_is_the_plan_uploaded_once(kind, ne, cells):
    """Every tensor of the handle is the plan's array, bit for bit, and the struct holds its address (no kernel runs)."""
    from qpsim_amd import _hip as H
    from qpsim_amd import tables as T
    from qpsim_amd.collision_tables import ARRAY_NAMES, plan_collision_tables
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((cells // 64, 64), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    E, _ = T.build_energy_grid(180.0, 1.0, unmerged_fmax(ne), ne)
    maps = T.build_phonon_frequency_map(E)[1:]
    kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in GAPS[:3]])
    ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in GAPS[:3]])
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in GAPS[:3]])
    if kind == "plain":
        args, kw = (kr[:1], ks[:1], rho[:1], *maps), {}
    elif kind == "member":
        args, kw = (kr, ks, rho, *maps), dict(members=3, member_classes=True)
    else:
        args = (kr, ks, rho, *maps, np.arange(eng.ncell) % 3)
        kw = dict(gap_params=dict(E=E, gaps=GAPS[:3], tau_r=500.0, tau_s=400.0, T_c=1.2))
    plan = plan_collision_tables(eng.lib, eng.ncell, eng.mask_flat, *args, **kw)
    tab = eng.make_collision_tables(*args, **kw)
    assert tab["kernel"] == plan.kernel == "register"
    assert (plan.arrays["kr0_anti2"] is not None) == (kind == "member") and (plan.arrays["gap_sq"] is not None) == (kind == "gap")
    pointers = [name for name, ctype in H.CollisionTables._fields_ if ctype is H.c_dp]
    assert pointers == list(ARRAY_NAMES)
    for name in ARRAY_NAMES:
        want, got = plan.arrays[name], tab[name]
        if want is None:
            assert got is None and not getattr(tab["struct"], name)
            continue
        back = got.cpu().numpy()
        assert back.dtype == want.dtype and back.shape == want.shape and back.tobytes() == want.tobytes(), name
        assert getattr(tab["struct"], name) == got.data_ptr(), name
    assert (tab["struct"].ne, tab["struct"].nw, tab["struct"].nclass, tab["struct"].flags) == (
        plan.ne, plan.nw, plan.nclass, plan.flag_bits)
