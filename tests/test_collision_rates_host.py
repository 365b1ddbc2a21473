"""Collision rate traces, host side (no GPU): the reference helper against the oracle, the soundness of the error bound on
every input the GPU tests use, number conservation of scattering, the argument checks of both public calls, the size query
and the workspace formula of the library."""
from __future__ import annotations

import inspect

import numpy as np
import pytest

import collision_exact as CE
import collision_rates_ref as R
from oracle import qp_oracle as O
from qpsim_amd import ensemble as ENS
from qpsim_amd import solver as S
from qpsim_amd.geometry import extract_edge_segments
from qpsim_amd.models import BoundaryCondition

U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


def _relax(n, gain, loss, dt):
    """The relaxation update of the collision step, restated: dn/dt = gain - loss n with frozen coefficients."""
    mu = np.maximum(loss, 0.0)
    P = np.maximum(gain + (mu - loss) * n, 0.0)
    decay = np.exp(-mu * dt)
    small = mu < 1e-14
    coeff = np.where(small, dt, (1.0 - decay) / np.where(small, 1.0, mu))
    return np.maximum(decay * n + coeff * P, 0.0)


@pytest.mark.parametrize("family", ["one", "classes"])
@pytest.mark.parametrize("ne", [12, 50])
def test_helper_reproduces_the_oracle_collision_step(ne, family):
    """gain = ch0 + ch3 and loss = the two loss sums (ch1 / n + ch2 / n, taken before the multiplication) through the
    relaxation update give the state of ``O.collision_step`` with frozen phonons, which is pinned to the reference."""
    h = CE.host_setup(ne, "regimes")
    px = h["active"]
    n, p = h["state"][family][:, px], h["ph"][:, px]
    nc = 1 if family == "one" else CE.GAPS.size
    tables = dict(kr=h["kr"][:nc], ks=h["ks"][:nc], rho=h["rho"][:nc], maps=h["maps"], dE=h["dE"])
    cls = h["cls"][px] if nc > 1 else np.zeros(int(px.sum()), dtype=int)
    idx_d, idx_s, sg = h["maps"]
    dt = 0.37
    want, _ = CE.run_oracle64(O, h, family, (True, True, False), dt)
    got = np.empty_like(n)
    for c in range(nc):
        sel = np.flatnonzero(cls == c)
        ch, loss = R.pixel_channels(n[:, sel], p[:, sel], tables["kr"][c], tables["ks"][c], tables["rho"][c], idx_d, idx_s,
                                    sg, h["dE"])
        assert np.all(ch >= 0.0)
        # ch1, ch2 are the loss sums times n (another association of the same three factors)
        assert np.allclose(ch[1], n[:, sel] * loss[0], rtol=8 * U, atol=0) and np.allclose(ch[2], n[:, sel] * loss[1],
                                                                                          rtol=8 * U, atol=0)
        got[:, sel] = _relax(n[:, sel], ch[0] + ch[3], loss[0] + loss[1], dt)
    err = np.abs(got - want)
    print(f"ne {ne} {family}: max relative difference to the oracle {np.max(err / np.maximum(want, 1e-300)):.3g}")
    assert np.all(err <= 1e-12 * want)


def _case_exact(case_key):
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case = R.case_inputs(ne, kind, ncm, members, nregion, family)
    tables = R.case_tables(case, en_r, en_s)
    flat = lambda a: a.reshape(a.shape[0], -1)  # noqa: E731
    args = (flat(case["state"]), flat(case["ph"]), tables, case["cls"].reshape(-1), en_r, en_s)
    return case, R.channels(*args, dtype=np.float64), R.channels(*args, dtype=np.longdouble)


@pytest.mark.parametrize("case_key", R.KERNEL_CASES + R.MANY_CHUNK_CASES, ids=lambda c: f"ne{c[0]}-{c[1]}-{c[2]}x{c[3]}-r{c[4]}-{c[6]}")
def test_the_bound_is_sound_on_the_inputs_of_the_gpu_tests(case_key):
    """fp64 in the kernel's association against extended precision: every pixel value within (NE + 8) u of exact, every
    region sum of c cells (added in fp64 in index order) within (NE + 8 + c - 1) u.  Scattering conserves number: the
    sums over the bins of ch0 and ch1 agree per pixel within twice the pixel bound."""
    ne, _, ncm, members, _, (en_r, en_s), _ = case_key
    case, ch64, chld = _case_exact(case_key)
    assert np.all(chld >= 0) and np.all(ch64 >= 0)
    assert np.all(np.abs(ch64 - chld) <= np.longdouble(R.bound(ne, 1)) * chld)
    if not en_r:
        assert not ch64[2:].any()
    if not en_s:
        assert not ch64[:2].any()
    ch64, chld = (a.reshape(4, ne, members, ncm) for a in (ch64, chld))
    worst = 0.0
    for m in range(members):
        for region in case["regions"]:
            cells = int(region.sum())
            exact = R.region_sums(chld[:, :, m], region)
            seq = np.zeros((4, ne))
            for c in np.flatnonzero(region):
                seq += ch64[:, :, m, c]
            limit = R.bound(ne, cells) * exact
            err = np.abs(seq - exact)
            worst = max(worst, float(np.max(err[limit > 0] / limit[limit > 0], initial=0.0)))
            assert np.all(err <= limit)
    print(f"worst error / bound of the fp64 helper: {worst:.3g}")
    if en_s:
        a, b = chld[0].sum(axis=0), chld[1].sum(axis=0)
        assert np.all(np.abs(a - b) <= 2 * np.longdouble(R.bound(ne, 1)) * np.maximum(a, b))
        a, b = ch64[0].sum(axis=0), ch64[1].sum(axis=0)
        assert np.all(np.abs(a - b) <= 2 * (R.bound(ne, 1) + ne * U) * np.maximum(a, b))


def test_the_cases_reach_every_instantiation_of_the_collision_kernel():
    """Regions rounded up to 1, 2, 4, 8: all four, each also past one chunk (the wave-order combine and the finish)."""
    nr = lambda nregion: 1 if nregion == 1 else 2 if nregion == 2 else 4 if nregion <= 4 else 8  # noqa: E731
    assert {nr(c[4]) for c in R.KERNEL_CASES} == {1, 2, 4, 8}
    assert {nr(c[4]) for c in R.KERNEL_CASES + R.MANY_CHUNK_CASES if c[2] > R.CHUNK} == {1, 2, 4, 8}


def test_the_bound_is_sound_on_the_oracle_inputs():
    for ne in (12, 50):
        h = CE.host_setup(ne, "regimes")
        tables = dict(kr=h["kr"], ks=h["ks"], rho=h["rho"], maps=h["maps"], dE=h["dE"])
        args = (h["state"]["classes"], h["ph"], tables, h["cls"])
        ch64, chld = R.channels(*args, dtype=np.float64), R.channels(*args, dtype=np.longdouble)
        assert np.all(np.abs(ch64 - chld) <= np.longdouble(R.bound(ne, 1)) * chld)


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


def test_the_three_parameters_and_their_defaults():
    """Fails on a tree without the feature: the keywords do not exist."""
    params = inspect.signature(S.run_2d_crank_nicolson).parameters
    assert [params[k].default for k in ("rates_out", "rates_regions", "rates_every")] == [None, None, 1]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("rates_out", "rates_regions", "rates_every"))
    sink = inspect.signature(ENS.run_2d_crank_nicolson_ensemble).parameters["rates_out"]
    assert sink.default is None and sink.kind is inspect.Parameter.KEYWORD_ONLY
    assert S.RATE_CHANNELS == ("scattering_in", "scattering_out", "recombination", "pair_breaking") == R.CHANNELS


ONES = np.ones((3, 4), dtype=bool)


@pytest.mark.parametrize("kw,match", [
    (dict(rates_out={}, rates_every=0), "rates_every"),
    (dict(rates_every=-1), "rates_every"),
    (dict(rates_every=True), "rates_every"),
    (dict(rates_regions={"a": ONES}), "rates_regions needs rates_out"),
    (dict(rates_out={}, rates_regions={"a": np.ones((3, 3), dtype=bool)}), r"rates_regions\['a'\].*shape"),
    (dict(rates_out={}, rates_regions={f"r{k}": ONES for k in range(9)}), "rates_regions.*1 to 8"),
    (dict(rates_out={}, rates_regions={}), "rates_regions.*1 to 8"),
    (dict(rates_out={}, energy_gap=0.0), "rates_out.*energy_gap"),
    (dict(rates_out={}, enable_recombination=False, enable_scattering=False), "rates_out.*enable_recombination"),
    (dict(rates_out={}, num_energy_bins=65), "rates_out.*num_energy_bins=65"),
    (dict(rates_out={}, num_energy_bins=100, collision_wide_bins=True), "rates_out.*num_energy_bins=100"),
    (dict(rates_out={}, num_energy_bins=1), "rates_out.*num_energy_bins=1"),
    # 100001 samples x 8 regions x 4 channels x 12 bins x 8 B = 293 MiB
    (dict(rates_out={}, rates_regions={f"r{k}": ONES for k in range(8)}, dt=1e-5, total_time=1.0, num_energy_bins=12),
     "rates_every.*256 MiB.*larger rates_every"),
])
def test_bad_rate_arguments_are_refused_before_a_sink_is_cleared_or_a_device_is_needed(lib, kw, match):
    kw = dict(kw)
    sink = kw.get("rates_out")
    if sink is not None:
        sink["stale"] = True
    other = {"stale": True}
    with pytest.raises(ValueError, match=match):
        S.run_2d_crank_nicolson(**_small(**kw), trace_out=other)
    if "larger rates_every" not in match:          # the buffer check needs the schedule: it comes after the plans
        assert other == {"stale": True} and (sink is None or sink == {"stale": True})


def test_rate_keys_are_shared_by_all_members(lib):
    common = _small()
    for key, value in (("rates_regions", {"a": ONES}), ("rates_every", 2), ("rates_out", {})):
        with pytest.raises(ValueError, match=f"member 1: '{key}' is shared by all members"):
            ENS.member_arguments([{}, {key: value}], common)
    kws = ENS.member_arguments([{}, {}], dict(common, rates_every=4))
    assert [k["rates_every"] for k in kws] == [4, 4] and kws[0]["rates_regions"] is None and kws[0]["rates_out"] is None
    with pytest.raises(ValueError, match="rates_regions needs rates_out"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], rates_regions={"a": ONES}, **common)
    with pytest.raises(ValueError, match="rates_every"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], rates_out=[], rates_every=0, **common)
    with pytest.raises(ValueError, match="rates_out.*energy_gap"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], rates_out=[], **dict(common, energy_gap=0.0))


def test_the_plan_has_the_method_set_of_the_other_plans_and_comes_third(lib):
    from qpsim_amd.timeloop import Schedule
    mask = np.ones((3, 4), dtype=bool)
    a = _small()
    sinks = [{}, {}, {}]
    plans = S._sampling_plans(mask, sinks[0], None, 1, sinks[1], 2, 1, sinks[2], {"a": ONES, "b": ~ONES}, 3, a)
    assert [type(p).__name__ for p, _ in plans] == ["_TracePlan", "_CoarsePlan", "_RatesPlan"]
    assert [sink is s for (_, sink), s in zip(plans, sinks)] == [True] * 3
    plan = plans[2][0]
    for name in ("every", "row_shape", "sampler", "result", "too_large"):
        assert hasattr(plan, name)
    assert plan.every == 3 and plan.row_shape(8) == (2, 4, 8) and plan.cells == [12, 0]
    sched = Schedule(0.75, 0.1, 1)
    assert S._sample_buffer_bytes(plan, sched, 5, 8) == 8 * sched.rows(3) * 5 * 2 * 4 * 8
    kw = ENS.member_arguments([{}], dict(a, rates_every=3))[0]
    assert ENS._bytes_per_member(kw, [plan]) - ENS._bytes_per_member(kw) == 8 * sched.rows(3) * 2 * 4 * 8
    rows = np.arange(2 * 2 * 4 * 8, dtype=float).reshape(2, 2, 4, 8)
    got = plan.result([0.0, 0.3], rows, np.linspace(180.0, 540.0, 8), 0.5, 2.0)
    assert sorted(got) == ["cells", "channels", "energy_bins", "number_rates", "rates", "regions", "times"]
    assert got["channels"] == list(R.CHANNELS) and got["regions"] == ["a", "b"] and got["rates"].shape == (2, 2, 4, 8)
    assert np.array_equal(got["number_rates"], 0.25 * 2.0 * rows.sum(axis=-1))
    # without a sink the call plans exactly what it planned before
    assert S._sampling_plans(mask, None, None, 1, None, 8, 1) == []


# ------------------------------------------------------------------------------------------------ the library, no GPU
def test_size_query_and_workspace_formula(lib):
    """Fails on a tree without the feature: the symbols do not exist."""
    q = lib.qp_collision_rates_available
    assert [q(ne, 30) for ne in (1, 2, 64, 65)] == [0, 1, 1, 0]
    assert [q(64, nw) for nw in (0, 1, 191, 192)] == [0, 1, 1, 0]
    ws = lib.qp_collision_rates_workspace_bytes
    for ne, ncm, members, nregion in [(2, 1, 1, 1), (12, R.CHUNK, 3, 8), (50, R.CHUNK + 1, 1, 3), (64, 3 * R.CHUNK - 1, 2, 5)]:
        assert ws(ne, ncm, members, nregion) == 8 * members * ((ncm + R.CHUNK - 1) // R.CHUNK) * nregion * 4 * ne
    assert ws(65, 64, 1, 1) == 0 and ws(1, 64, 1, 1) == 0 and ws(12, 0, 1, 1) == 0 and ws(12, 64, 0, 1) == 0
    assert ws(12, 64, 1, 0) == 0 and ws(12, 64, 1, 9) == 0


def test_the_call_validates_before_any_launch(lib):
    import ctypes as C
    from qpsim_amd import _hip
    t = _hip.CollisionTables.make(12, 35, 1, 8, 8, 8, 8, 8, 8, 0)
    ok = dict(t=C.byref(t), bits=8, ncm=64, members=1, nregion=1, state=8, ph=8, ws=8, out=8)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.qp_collision_rates(a["t"], a["bits"], a["ncm"], a["members"], a["nregion"], a["state"], a["ph"], 1.0, 1, 1,
                                      a["ws"], a["out"], 0)
    for bad in (dict(bits=0), dict(state=0), dict(ph=0), dict(ws=0), dict(out=0), dict(ncm=0), dict(members=0), dict(t=None)):
        assert call(**bad) == -1, bad
    assert call(nregion=0) == -3 and call(nregion=9) == -3
    for ne, nw in ((65, 100), (1, 1), (64, 192)):
        big = _hip.CollisionTables.make(ne, nw, 1, 8, 8, 8, 8, 8, 8, 0)
        assert call(t=C.byref(big)) == -3 and b"qp_collision_rates" in lib.qp_last_error()
    t.struct_size = 64
    assert call() == -1 and b"struct_size" in lib.qp_last_error()
