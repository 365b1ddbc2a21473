"""Phonon rate traces, host side (no GPU): the reference helper against the oracle's phonon update, the soundness of the
error bound on every input the GPU tests use, the number balance between the phonon channels and the quasiparticle
channels, the argument checks of both public calls, the size query and the workspace formula of the library."""
from __future__ import annotations

import inspect

import numpy as np
import pytest

import collision_exact as CE
import collision_rates_ref as R
import phonon_rates_ref as PR
from oracle import qp_oracle as O
from qpsim_amd import ensemble as ENS
from qpsim_amd import solver as S
from qpsim_amd.geometry import extract_edge_segments
from qpsim_amd.models import BoundaryCondition

U = 2.0 ** -53
CASE_IDS = lambda c: f"ne{c[0]}-{c[1]}-{c[2]}x{c[3]}-r{c[4]}-{c[6]}"  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


def _affine(y, a, b, dt):
    """The growth update of the phonon planes, restated: y' = a + b y over one step with frozen coefficients."""
    x = np.clip(b * dt, -80.0, 80.0)
    ex = np.exp(x)
    small = np.abs(b) < 1e-14
    coeff = np.where(small, dt, (ex - 1.0) / np.where(small, 1.0, b))
    return np.maximum(ex * y + coeff * a, 0.0)


@pytest.mark.parametrize("combo", CE.COMBOS, ids=lambda c: "r%ds%d" % c[:2])
@pytest.mark.parametrize("family", ["one", "classes"])
@pytest.mark.parametrize("ne", [12, 50])
def test_helper_reproduces_the_oracle_phonon_update(ne, family, combo):
    """a = E + R and b = a - A - B from the helper's base sums through the growth update give the phonon planes of
    ``O.collision_step``, which is pinned to the reference, on the same pre-state, to 1e-12 relative element by element.

    The pre-state.  The reference's update forms (e^x - 1) / b with x = b dt, and b is a difference: two evaluations whose
    b differ by a relative d give planes that differ by d wherever |x| is small (e^x - 1 is the same rounded number in
    both), and d = (roundings of the sums) x kappa, kappa = (E + A + R + B) / |b|.  An independent association of NE^2 terms
    differs from the oracle's by some NE u per sum, so 1e-12 is implied only where kappa is below about 40 at NE = 50.  On
    the `regimes` state of `collision_exact.host_setup` (random occupations) a few of the 10^4 elements have emission and
    absorption equal to 4 - 5 digits by chance (measured: NE = 12, one class, bin 11: E + R = 2.48850e-3, A = 2.48856e-3,
    kappa = 9e4, difference to the oracle 7.5e-12), which says nothing about which pairs the helper adds to which bin.  So
    the state here is built to have kappa <= 3 everywhere: the phonons, cells, classes and levels of `regimes`, occupations
    f_i = n_i / rho_i = 0.3 level 8^-i (0.5 ... 1), for which n_i q_j <= 0.36 n_j q_i (i > j: E_w <= 0.36 A_w) and
    n_i n_j <= 0.19 q_i q_j (R_w <= 0.19 B_w), so b = (E - A) + (R - B) adds two negative numbers.  kappa is asserted."""
    h = CE.host_setup(ne, "regimes")
    px = h["active"]
    nc = 1 if family == "one" else CE.GAPS.size
    cls = h["cls"][px] if nc > 1 else np.zeros(int(px.sum()), dtype=int)
    rng = np.random.default_rng([ne, nc])
    f = 0.3 * h["level"][None, :] * 8.0 ** -np.arange(ne)[:, None] * (0.5 + 0.5 * rng.random((ne, cls.size)))
    n, p = f * h["rho"][cls].T, h["ph"][:, px]
    en_r, en_s, _ = combo
    tables = dict(kr=h["kr"][:nc] if en_r else None, ks=h["ks"][:nc] if en_s else None, rho=h["rho"][:nc], maps=h["maps"],
                  dE=h["dE"])
    dt = 0.37
    n_ref, want = n.copy(), p.copy()
    O.collision_step(n_ref, want, CE.oracle_tables(h, family, combo), dt, en_r=en_r, en_s=en_s, update_phonons=True)
    ch, base = PR.channels(n, p, tables, cls, en_r, en_s)
    assert np.all(ch >= 0.0) and np.all(base >= 0.0)
    a = base[0] + base[2]
    b = a - base[1] - base[3]
    fed = base.sum(axis=0) > 0
    assert np.all(base.sum(axis=0)[fed] <= 3.0 * np.abs(b[fed])), "kappa <= 3 on this state"
    got = _affine(p, a, b, dt)
    assert not np.array_equal(want, p), "the oracle moved the phonons"
    err = np.abs(got - want)
    print(f"ne {ne} {family} {combo}: max relative difference to the oracle {np.max(err / np.maximum(want, 1e-300)):.3g}")
    assert np.all(err <= 1e-12 * want)


@pytest.mark.parametrize("case_key", PR.KERNEL_CASES + PR.MANY_CHUNK_CASES, ids=CASE_IDS)
def test_the_bound_is_sound_on_the_inputs_of_the_gpu_tests(case_key):
    """fp64 in the kernel's association against extended precision: every pixel value within (NE + 8) u of exact, every
    region sum of c cells (added in fp64 in index order) within (NE + 8 + c - 1) u."""
    ne, _, ncm, members, _, (en_r, en_s), _ = case_key
    case, ch64, chld, _ = PR.case_exact(case_key)
    assert np.all(chld >= 0) and np.all(ch64 >= 0)
    assert np.all(np.abs(ch64 - chld) <= np.longdouble(R.bound(ne, 1)) * chld)
    if not en_r:
        assert not ch64[2:].any()
    if not en_s:
        assert not ch64[:2].any()
    worst = 0.0
    for m in range(members):
        for region in case["regions"]:
            cells = int(region.sum())
            exact = R.region_sums(chld[:, :, m], region)
            seq = np.zeros((4, case["nw"]))
            for c in np.flatnonzero(region):
                seq += ch64[:, :, m, c]
            limit = R.bound(ne, cells) * exact
            err = np.abs(seq - exact)
            worst = max(worst, float(np.max(err[limit > 0] / limit[limit > 0], initial=0.0)))
            assert np.all(err <= limit)
    print(f"worst error / bound of the fp64 helper: {worst:.3g}")


def test_the_cases_reach_every_instantiation_and_the_largest_phonon_grid():
    """(regions rounded up to 1, 2, 4, 8) x (1, 2, 3 phonon bins per lane): all twelve; the structured sizes nearest to each boundary, NW = 64 among them."""
    seen, nws = set(), set()
    for ne, kind, ncm, members, nregion, _, family in PR.KERNEL_CASES:
        nw = R.case_inputs(ne, kind, ncm, members, nregion, family)["nw"]
        seen.add((1 if nregion == 1 else 2 if nregion == 2 else 4 if nregion <= 4 else 8, PR.bins_per_lane(nw)))
        nws.add(nw)
    assert seen == {(nr, b) for nr in (1, 2, 4, 8) for b in (1, 2, 3)}
    assert {64, 71, 119, 134, 191} <= nws
    assert (64, 191, 8) in {(c[0], R.case_inputs(c[0], c[1], c[2], c[3], c[4], c[6])["nw"], c[4]) for c in PR.KERNEL_CASES}


@pytest.mark.parametrize("case_key", [c for c in PR.KERNEL_CASES if c[2] <= 130], ids=CASE_IDS)
def test_number_balance_between_phonon_and_quasiparticle_channels(case_key):
    """In extended precision, per pixel: every recombination removes two quasiparticles and emits one phonon, every pair
    breaking absorbs one phonon and adds two, every scattering event moves one quasiparticle out of its bin and emits or
    absorbs one phonon.  The two sides are different associations of the same terms: NE^2 terms each, so they agree within
    2 (NE^2 + 8) roundings of the extended format."""
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case, _, chld, _ = PR.case_exact(case_key)
    flat = lambda a: a.reshape(a.shape[0], -1)  # noqa: E731
    qp = R.channels(flat(case["state"]), flat(case["ph"]), R.case_tables(case, en_r, en_s), case["cls"].reshape(-1), en_r,
                    en_s, dtype=np.longdouble)
    ph = chld.reshape(4, case["nw"], -1)
    tol = 2 * (ne * ne + 8) * np.longdouble(np.finfo(np.longdouble).eps)
    pairs = ((qp[2].sum(axis=0), 2 * ph[2].sum(axis=0)), (qp[3].sum(axis=0), 2 * ph[3].sum(axis=0)),
             (qp[1].sum(axis=0), ph[0].sum(axis=0) + ph[1].sum(axis=0)))
    for a, b in pairs:
        assert np.all(np.abs(a - b) <= tol * np.maximum(a, b))
    if en_r:
        assert np.all(pairs[0][0] > 0) and np.all(pairs[1][0] > 0)
    if en_s:
        assert np.all(pairs[2][0] > 0)


# ------------------------------------------------------------------------------------------------ arguments
def _small(**kw):
    mask = np.ones((3, 4), dtype=bool)
    edges = extract_edge_segments(mask)
    base = dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BoundaryCondition("reflective") for e in edges},
                initial_field=np.ones(mask.shape), diffusion_coefficient=1.0, dt=0.1, total_time=0.75, dx=1.0,
                energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=8,
                enable_recombination=True, enable_scattering=True)
    base.update(kw)
    return base


KEYS = ("phonon_rates_out", "phonon_rates_regions", "phonon_rates_every")


def test_the_three_parameters_and_their_defaults():
    """Fails on the parent commit: the keywords do not exist."""
    params = inspect.signature(S.run_2d_crank_nicolson).parameters
    assert [params[k].default for k in KEYS] == [None, None, 1]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in KEYS)
    sink = inspect.signature(ENS.run_2d_crank_nicolson_ensemble).parameters["phonon_rates_out"]
    assert sink.default is None and sink.kind is inspect.Parameter.KEYWORD_ONLY
    assert S.PHONON_RATE_CHANNELS == ("scattering_emission", "scattering_absorption", "recombination_emission",
                                      "pair_breaking_absorption") == PR.CHANNELS


ONES = np.ones((3, 4), dtype=bool)


@pytest.mark.parametrize("kw,match", [
    (dict(phonon_rates_out={}, phonon_rates_every=0), "phonon_rates_every"),
    (dict(phonon_rates_every=-1), "phonon_rates_every"),
    (dict(phonon_rates_every=True), "phonon_rates_every"),
    (dict(phonon_rates_regions={"a": ONES}), "phonon_rates_regions needs phonon_rates_out"),
    (dict(phonon_rates_out={}, phonon_rates_regions={"a": np.ones((3, 3), dtype=bool)}), r"phonon_rates_regions\['a'\].*shape"),
    (dict(phonon_rates_out={}, phonon_rates_regions={f"r{k}": ONES for k in range(9)}), "phonon_rates_regions.*1 to 8"),
    (dict(phonon_rates_out={}, phonon_rates_regions={}), "phonon_rates_regions.*1 to 8"),
    (dict(phonon_rates_out={}, energy_gap=0.0), "phonon_rates_out.*energy_gap"),
    (dict(phonon_rates_out={}, enable_recombination=False, enable_scattering=False),
     "phonon_rates_out.*enable_recombination"),
    (dict(phonon_rates_out={}, num_energy_bins=65), "phonon_rates_out.*num_energy_bins=65"),
    (dict(phonon_rates_out={}, num_energy_bins=100, collision_wide_bins=True), "phonon_rates_out.*num_energy_bins=100"),
    (dict(phonon_rates_out={}, num_energy_bins=1), "phonon_rates_out.*num_energy_bins=1"),
    # 100001 samples x 8 regions x 4 channels x 35 phonon bins x 8 B = 855 MiB
    (dict(phonon_rates_out={}, phonon_rates_regions={f"r{k}": ONES for k in range(8)}, dt=1e-5, total_time=1.0,
          num_energy_bins=12), "phonon_rates_every.*256 MiB.*larger phonon_rates_every"),
])
def test_bad_arguments_are_refused_before_a_sink_is_cleared_or_a_device_is_needed(lib, kw, match):
    """Fails on the parent commit: the keywords do not exist (TypeError)."""
    kw = dict(kw)
    sink = kw.get("phonon_rates_out")
    if sink is not None:
        sink["stale"] = True
    other = {"stale": True}
    with pytest.raises(ValueError, match=match):
        S.run_2d_crank_nicolson(**_small(**kw), trace_out=other)
    if "larger phonon_rates_every" not in match:   # the buffer check needs the schedule: it comes after the plans
        assert other == {"stale": True} and (sink is None or sink == {"stale": True})


def test_the_keys_are_shared_by_all_members(lib):
    """Fails on the parent commit: the keywords do not exist."""
    common = _small()
    for key, value in (("phonon_rates_regions", {"a": ONES}), ("phonon_rates_every", 2), ("phonon_rates_out", {})):
        with pytest.raises(ValueError, match=f"member 1: '{key}' is shared by all members"):
            ENS.member_arguments([{}, {key: value}], common)
    kws = ENS.member_arguments([{}, {}], dict(common, phonon_rates_every=4))
    assert [k["phonon_rates_every"] for k in kws] == [4, 4]
    assert kws[0]["phonon_rates_regions"] is None and kws[0]["phonon_rates_out"] is None
    with pytest.raises(ValueError, match="phonon_rates_regions needs phonon_rates_out"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], phonon_rates_regions={"a": ONES}, **common)
    with pytest.raises(ValueError, match="phonon_rates_every"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], phonon_rates_out=[], phonon_rates_every=0, **common)
    with pytest.raises(ValueError, match="phonon_rates_out.*energy_gap"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], phonon_rates_out=[], **dict(common, energy_gap=0.0))


def test_the_plan_has_the_method_set_of_the_other_plans_and_comes_fourth(lib):
    """Fails on the parent commit: ``_sampling_plans`` takes no fourth kind."""
    from qpsim_amd import tables as T
    from qpsim_amd.timeloop import Schedule
    mask = np.ones((3, 4), dtype=bool)
    a = _small()
    sinks = [{}, {}, {}, {}]
    plans = S._sampling_plans(mask, sinks[0], None, 1, sinks[1], 2, 1, sinks[2], None, 2, a, sinks[3],
                              {"a": ONES, "b": ~ONES}, 3)
    assert [type(p).__name__ for p, _ in plans] == ["_TracePlan", "_CoarsePlan", "_RatesPlan", "_PhononRatesPlan"]
    assert [sink is s for (_, sink), s in zip(plans, sinks)] == [True] * 4
    plan = plans[3][0]
    for name in ("every", "row_shape", "sampler", "result", "too_large"):
        assert hasattr(plan, name)
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, 8)
    omega = T.build_phonon_frequency_map(E)[0]
    nw = omega.size
    assert plan.every == 3 and plan.nw == nw and plan.row_shape(8) == (2, 4, nw) and plan.cells == [12, 0]
    assert np.array_equal(plan.omega_bins, omega)
    widths = T.integration_widths_from_centers(omega, fallback_width=dE)
    assert np.array_equal(plan.widths, widths)
    sched = Schedule(0.75, 0.1, 1)
    assert S._sample_buffer_bytes(plan, sched, 5, 8) == 8 * sched.rows(3) * 5 * 2 * 4 * nw
    kw = ENS.member_arguments([{}], dict(a, phonon_rates_every=3))[0]
    assert ENS._bytes_per_member(kw, [plan]) - ENS._bytes_per_member(kw) == 8 * sched.rows(3) * 2 * 4 * nw
    rows = np.arange(2 * 2 * 4 * nw, dtype=float).reshape(2, 2, 4, nw)
    got = plan.result([0.0, 0.3], rows, E, 0.5, dE)
    assert sorted(got) == ["cells", "channels", "integrated_rates", "phonon_energy_bins", "rates", "regions", "times"]
    assert got["channels"] == list(PR.CHANNELS) and got["regions"] == ["a", "b"] and got["rates"].shape == (2, 2, 4, nw)
    assert np.array_equal(got["phonon_energy_bins"], omega)
    assert np.allclose(got["integrated_rates"], 0.25 * (rows * widths).sum(axis=-1), rtol=1e-15, atol=0)
    # without the sink the call plans exactly what it planned before
    assert S._sampling_plans(mask, None, None, 1, None, 8, 1) == []
    assert [type(p).__name__ for p, _ in S._sampling_plans(mask, None, None, 1, None, 8, 1, {}, None, 1, a)] == ["_RatesPlan"]


def test_the_reduce_is_bound_late_and_calls_the_engine_with_the_run(lib):
    """The plan's reduce reads the run's phonon planes, tables and switches at every sample, as the rate reduce does."""
    calls = []

    class Eng:
        def phonon_rates(self, *args):
            calls.append(args)

    class Run:
        ctab, phonon, dE, physics = "tables", "planes", 2.5, (True, False, True)

    reduce = S._PhononRatesReduce(Eng(), "bits", 3)

    class Sampler:
        pass
    sampler = Sampler()
    sampler.reduce = reduce
    S._bind_rates([sampler], Run)
    reduce("state", "row")
    assert calls == [("tables", "state", "planes", "bits", 3, 2.5, True, False, "row")]


# ------------------------------------------------------------------------------------------------ the library, no GPU
def test_size_query_and_workspace_formula(lib):
    """Fails on the parent commit: the symbols do not exist."""
    q = lib.qp_phonon_rates_available
    assert [q(ne, 30) for ne in (1, 2, 64, 65)] == [0, 1, 1, 0]
    assert [q(64, nw) for nw in (0, 1, 191, 192)] == [0, 1, 1, 0]
    ws = lib.qp_phonon_rates_workspace_bytes
    for nw, ncm, members, nregion in [(5, 1, 1, 1), (35, R.CHUNK, 3, 8), (149, R.CHUNK + 1, 1, 3), (191, 3 * R.CHUNK - 1, 2, 5)]:
        assert ws(nw, ncm, members, nregion) == 8 * members * ((ncm + R.CHUNK - 1) // R.CHUNK) * nregion * 4 * nw
    assert ws(192, 64, 1, 1) == 0 and ws(0, 64, 1, 1) == 0 and ws(35, 0, 1, 1) == 0 and ws(35, 64, 0, 1) == 0
    assert ws(35, 64, 1, 0) == 0 and ws(35, 64, 1, 9) == 0


def test_the_call_validates_before_any_launch(lib):
    """Fails on the parent commit: the symbol does not exist.  Every call here would fault if it launched (the pointers are
    not device memory)."""
    import ctypes as C
    from qpsim_amd import _hip
    t = _hip.CollisionTables.make(12, 35, 1, 8, 8, 8, 8, 8, 8, 0, 8, 8)
    ok = dict(t=C.byref(t), bits=8, ncm=64, members=1, nregion=1, state=8, ph=8, ws=8, out=8)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.qp_phonon_rates(a["t"], a["bits"], a["ncm"], a["members"], a["nregion"], a["state"], a["ph"], 1.0, 1, 1,
                                   a["ws"], a["out"], 0)
    for bad in (dict(bits=0), dict(state=0), dict(ph=0), dict(ws=0), dict(out=0), dict(ncm=0), dict(members=0), dict(t=None)):
        assert call(**bad) == -1, bad
    assert call(nregion=0) == -3 and call(nregion=9) == -3
    for ne, nw in ((65, 100), (1, 1), (64, 192)):
        big = _hip.CollisionTables.make(ne, nw, 1, 8, 8, 8, 8, 8, 8, 0, 8, 8)
        assert call(t=C.byref(big)) == -3 and b"qp_phonon_rates" in lib.qp_last_error()
    unstructured = _hip.CollisionTables.make(12, 35, 1, 8, 8, 8, 8, 8, 8, 0)
    assert call(t=C.byref(unstructured)) == -1 and b"diag_bin" in lib.qp_last_error()
    t.struct_size = 64
    assert call() == -1 and b"struct_size" in lib.qp_last_error()


def test_engine_refuses_unstructured_and_asymmetric_tables_before_the_library_is_called():
    """``Engine.phonon_rates`` checks the handle on the host: no ``diag_bin`` (a table set forced to "wave_unstructured")
    or no symmetry is a ``ValueError``, and neither scratch nor the library is touched."""
    from qpsim_amd.engine import Engine

    class Row:
        shape = (1, 1, 4, 35)

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError(f"touched {name}")
    eng = object.__new__(Engine)
    eng.__dict__.update(lib=Untouched(), ncell=12)
    handle = dict(ne=12, nw=35, diag_bin=None, symmetric=True)
    with pytest.raises(ValueError, match="phonon_rates.*diag_bin"):
        Engine.phonon_rates(eng, handle, None, None, None, 1, 1.0, True, True, Row())
    with pytest.raises(ValueError, match="phonon_rates.*symmetric"):
        Engine.phonon_rates(eng, dict(handle, diag_bin=object(), symmetric=False), None, None, None, 1, 1.0, True, True, Row())
