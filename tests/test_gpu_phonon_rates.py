"""Phonon rate traces on the GPU: ``qp_phonon_rates`` alone against the exact sums of tests/phonon_rates_ref.py within the
derived bound (NE + 8 + cells - 1) 2^-53, its determinism, its balance with ``qp_collision_rates``, and the
``phonon_rates_out`` sink of both public calls against the helper evaluated on the frames a twin run stores."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

import collision_rates_ref as R
import phonon_rates_ref as PR
from golden_utils import GoldenRun, oracle_kwargs
from test_gpu_collision_rates import _device_tables, _p, _run_arguments, _run_tables, _same_frames

pytestmark = pytest.mark.gpu
CASE_IDS = lambda c: f"ne{c[0]}-{c[1]}-{c[2]}x{c[3]}-r{c[4]}-{c[6]}"  # noqa: E731


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def lib():
    from qpsim_amd import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ the kernel alone
def _launch(torch, lib, struct, state, ph, bits, nw, ncm, members, nregion, dE, en_r, en_s, call="qp_phonon_rates"):
    """``qp_phonon_rates`` (or, with ``nw`` = ne, ``qp_collision_rates``) into a NaN-filled [members, nregion, 4, nw]."""
    import ctypes as C
    nbytes = int(getattr(lib, call + "_workspace_bytes")(nw, ncm, members, nregion))
    assert nbytes == 8 * members * ((ncm + R.CHUNK - 1) // R.CHUNK) * nregion * 4 * nw      # the formula of the header
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((members, nregion, 4, nw), float("nan"), dtype=torch.float64, device="cuda")
    rc = getattr(lib, call)(C.byref(struct), _p(bits), ncm, members, nregion, _p(state), _p(ph), float(dE), int(en_r),
                            int(en_s), _p(ws), _p(out), int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.qp_last_error()
    return out.cpu().numpy()


def _run_case(torch, lib, case_key, state=None, ph=None):
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case = R.case_inputs(ne, kind, ncm, members, nregion, family)
    struct, keep = _device_tables(torch, lib, case, ncm, members, family)
    assert struct.diag_bin and struct.anti_bin, "the case has structured bin maps"
    d_state = torch.as_tensor(np.array(case["state"] if state is None else state), device="cuda")
    d_ph = torch.as_tensor(np.array(case["ph"] if ph is None else ph), device="cuda")
    d_bits = torch.as_tensor(np.array(case["bits"]), device="cuda")
    got = _launch(torch, lib, struct, d_state, d_ph, d_bits, case["nw"], ncm, members, nregion, case["tables"]["dE"], en_r,
                  en_s)
    return case, got, (struct, keep, d_state, d_ph, d_bits)


@pytest.mark.parametrize("case_key", PR.KERNEL_CASES + PR.MANY_CHUNK_CASES, ids=CASE_IDS)
def test_phonon_rates_against_exact_sums(torch, lib, case_key):
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case, got, (struct, keep, d_state, d_ph, d_bits) = _run_case(torch, lib, case_key)
    nw = case["nw"]
    assert got.shape == (members, nregion, 4, nw) and not np.isnan(got).any(), "every entry of out is written"
    again = _launch(torch, lib, struct, d_state, d_ph, d_bits, nw, ncm, members, nregion, case["tables"]["dE"], en_r, en_s)
    assert got.tobytes() == again.tobytes(), "a second launch gives the same bits"
    exact = PR.case_exact(case_key)[2]
    worst = 0.0
    for m in range(members):
        for r, region in enumerate(case["regions"]):
            want = R.region_sums(exact[:, :, m], region)
            limit = R.bound(ne, int(region.sum())) * want
            err = np.abs(got[m, r] - want)
            worst = max(worst, float(np.max(err[limit > 0] / limit[limit > 0], initial=0.0)))
            assert np.all(err <= limit), (m, case["names"][r], float(np.max(err - limit)))
    print(f"phonon rates {case_key}: worst error / bound = {worst:.3g}")
    names = case["names"]
    assert not np.signbit(got).any()
    if not en_r:
        assert not got[:, :, 2:].any(), "a disabled process gives exact zeros"
    if not en_s:
        assert not got[:, :, :2].any()
    if "empty" in names:
        assert not got[:, names.index("empty")].any()
    if names.count("twin") == 2:
        a, b = [k for k, name in enumerate(names) if name == "twin"]
        assert got[:, a].tobytes() == got[:, b].tobytes()
    if "all" in names and en_r and en_s:
        assert np.all(got[:, names.index("all")].sum(axis=-1) > 0.0)


@pytest.mark.parametrize("case_key", [(12, "plain", 203, 3, 3, (1, 1), "classes"), (50, "plain", 64, 3, 1, (1, 1), "members")],
                         ids=["odd", "even"])
def test_a_member_of_a_batch_gives_the_bits_of_a_lone_call(torch, lib, case_key):
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case, got, _ = _run_case(torch, lib, case_key)
    t = case["tables"]
    for m in range(members):
        lone = dict(case, cls=case["cls"][m:m + 1])
        if family == "members":            # the member's own table set, as one class
            lone["tables"] = dict(t, kr=t["kr"][m:m + 1], ks=t["ks"][m:m + 1], rho=t["rho"][m:m + 1])
        struct, keep = _device_tables(torch, lib, lone, ncm, 1, "one" if family == "members" else family)
        # fresh allocations of the member's planes: whatever the parity of the member's first element was in the batch
        d_state = torch.as_tensor(np.ascontiguousarray(case["state"][:, m:m + 1]), device="cuda")
        d_ph = torch.as_tensor(np.ascontiguousarray(case["ph"][:, m:m + 1]), device="cuda")
        d_bits = torch.as_tensor(np.array(case["bits"]), device="cuda")
        one = _launch(torch, lib, struct, d_state, d_ph, d_bits, case["nw"], ncm, 1, nregion, t["dE"], en_r, en_s)
        assert one[0].tobytes() == got[m].tobytes(), m


def test_nan_outside_every_region_reaches_no_sum(torch, lib):
    """NaN in the state and the phonons of cells without a region bit - whole groups of 8 and single cells inside a group
    that is loaded - leaves ``out`` bitwise unchanged."""
    key = (12, "plain", R.CHUNK + 1, 1, 1, (1, 1), "classes")
    case, clean, _ = _run_case(torch, lib, key)
    outside = ~case["regions"][0]
    groups = outside[:R.CHUNK].reshape(-1, 8)
    assert groups.all(axis=1).any() and (groups.any(axis=1) & ~groups.all(axis=1)).any()
    state, ph = case["state"].copy(), case["ph"].copy()
    state[:, :, outside] = np.nan
    ph[:, :, outside] = np.nan
    _, got, _ = _run_case(torch, lib, key, state, ph)
    assert np.isfinite(got).all() and got.tobytes() == clean.tobytes()


@pytest.mark.parametrize("case_key", [(12, "plain", 2 * R.CHUNK + 77, 3, 8, (1, 1), "classes"),
                                      (50, "merged", 65, 3, 8, (1, 1), "members"), (64, "plain", 130, 1, 8, (1, 1), "one")],
                         ids=CASE_IDS)
def test_balance_with_the_quasiparticle_rates(torch, lib, case_key):
    """Both kernels on the same planes and regions: per region, recombination removes two quasiparticles per emitted
    phonon, pair breaking adds two per absorbed phonon, and every quasiparticle scattered out of its bin emits or absorbs
    one phonon.  Each entry of either output is within ``bound`` of its exact value and all are >= 0, so the exactly taken
    sums over the bins of the two sides agree within the sum of the two bounds."""
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case, ph, (struct, keep, d_state, d_ph, d_bits) = _run_case(torch, lib, case_key)
    qp = _launch(torch, lib, struct, d_state, d_ph, d_bits, ne, ncm, members, nregion, case["tables"]["dE"], en_r, en_s,
                 call="qp_collision_rates")
    worst = 0.0
    for m in range(members):
        for r, region in enumerate(case["regions"]):
            tol = 2 * R.bound(ne, int(region.sum()))
            s = lambda a: R.exact_sum(a.astype(np.longdouble))  # noqa: E731
            for a, b in ((s(qp[m, r, 2]), 2 * s(ph[m, r, 2])), (s(qp[m, r, 3]), 2 * s(ph[m, r, 3])),
                         (s(qp[m, r, 1]), R.exact_sum(np.concatenate([ph[m, r, 0], ph[m, r, 1]]).astype(np.longdouble)))):
                assert (a > 0) == bool(region.any()) and (b > 0) == bool(region.any())
                if a > 0:
                    worst = max(worst, abs(a - b) / (tol * max(a, b)))
                assert abs(a - b) <= tol * max(a, b), (m, case["names"][r], a, b)
    print(f"balance {case_key}: worst difference / (sum of the two bounds) = {worst:.3g}")


def test_unstructured_tables_are_refused_without_a_launch(torch, lib):
    """A table set forced to "wave_unstructured" carries no ``diag_bin``: ``Engine.phonon_rates`` raises before it takes
    scratch or calls the library, and the library refuses the struct as well."""
    import ctypes as C
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((4, 8), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    case = R.case_inputs(12, "plain", 32, 1, 1, "one")
    t = case["tables"]
    handle = eng.make_collision_tables(t["kr"], t["ks"], t["rho"], *t["maps"], kernel="wave_unstructured")
    assert handle["diag_bin"] is None and handle["symmetric"]
    state = torch.as_tensor(np.array(case["state"]), device="cuda")
    ph = torch.as_tensor(np.array(case["ph"]), device="cuda")
    bits = torch.as_tensor(np.array(case["bits"]), device="cuda")
    out = torch.full((1, 1, 4, case["nw"]), float("nan"), dtype=torch.float64, device="cuda")
    before = set(eng._scratch)
    with pytest.raises(ValueError, match="phonon_rates.*diag_bin"):
        eng.phonon_rates(handle, state, ph, bits, 1, t["dE"], True, True, out)
    assert set(eng._scratch) == before and torch.isnan(out).all().item(), "nothing was allocated or written"
    ws = torch.empty(8 * 4 * case["nw"], dtype=torch.uint8, device="cuda")
    rc = lib.qp_phonon_rates(C.byref(handle["struct"]), _p(bits), 32, 1, 1, _p(state), _p(ph), t["dE"], 1, 1, _p(ws), _p(out),
                             int(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"diag_bin" in lib.qp_last_error() and torch.isnan(out).all().item()
    # the same tables with their structure are served, through the engine, and agree with the helper
    handle = eng.make_collision_tables(t["kr"], t["ks"], t["rho"], *t["maps"])
    eng.phonon_rates(handle, state, ph, bits, 1, t["dE"], True, True, out)
    exact = PR.case_exact((12, "plain", 32, 1, 1, (1, 1), "one"))[2]
    want = R.region_sums(exact[:, :, 0], case["regions"][0])
    assert np.all(np.abs(out.cpu().numpy()[0, 0] - want) <= R.bound(12, int(case["regions"][0].sum())) * want)


# ------------------------------------------------------------------------------------------------ whole runs
def _check_against_stored_frames(sink, stored, history, kw, regions, gap_values=None, label=""):
    """``rates`` [S, R, 4, NW] against the helper on the energy frames and phonon frames of the store points of a twin run
    that stores every sampled step; ``integrated_rates`` against its definition."""
    from qpsim_amd import tables as T
    mask, ne = kw["mask"], kw["num_energy_bins"]
    tables, cls = _run_tables(kw, gap_values)
    en_r, en_s = kw["enable_recombination"], kw["enable_scattering"]
    assert sink["times"] == list(stored[0])
    worst = 0.0
    for s in range(len(stored[0])):
        n = np.stack(stored[4][s])[:, mask]
        p = np.stack(history["phonon_energy_frames"][s])[:, mask]
        exact = PR.channels(n, p, R.case_tables(dict(tables=tables), en_r, en_s), cls, en_r, en_s, dtype=np.longdouble)[0]
        for r, region in enumerate(regions.values()):
            inside = (region & mask)[mask]
            want = R.region_sums(exact, inside)
            limit = R.bound(ne, int(inside.sum())) * want
            err = np.abs(sink["rates"][s, r] - want)
            worst = max(worst, float(np.max(err[limit > 0] / limit[limit > 0], initial=0.0)))
            assert np.all(err <= limit), (s, r, float(np.max(err - limit)))
    print(f"{label}: phonon rates worst error / bound = {worst:.3g}")
    omega = np.asarray(history["phonon_energy_bins"])
    assert np.array_equal(sink["phonon_energy_bins"], omega)
    widths = T.integration_widths_from_centers(omega, fallback_width=tables["dE"])
    assert np.allclose(sink["integrated_rates"], kw["dx"] ** 2 * (widths * sink["rates"]).sum(axis=-1), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", ["ne12_dynamic_phonons", "ne50_16x16", "nonuniform_gap_4x4"])
def test_rates_of_a_run_against_the_helper_on_the_frames_of_its_twin(name):
    """``phonon_rates_every = 1`` beside a twin with ``store_every = 1`` and a phonon history: every sample is the helper on
    the twin's frames of that step, and what the sampled run stores (``store_every = 3``) is bit for bit what the twin - a
    run with ``store_every`` = the sampling cadence and no sink - stores at those steps."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    gap_values = None
    if name == "nonuniform_gap_4x4":
        run = GoldenRun("regress_nonuniform_gap_collisions_4x4")
        kw = dict(run.kwargs)
        kw.pop("store_every")
        gap_values = oracle_kwargs(run)["gap_values"]
        assert np.unique(gap_values).size > 1
        regions = {"all": kw["mask"].copy(), "row0": np.arange(16).reshape(4, 4) < 4}
    elif name == "ne50_16x16":
        kw, regions = _run_arguments(50, 16, 16)
    else:
        kw, regions = _run_arguments(12)
    hist_a, hist_b, sink = {}, {}, {"stale": True}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        twin = run_2d_crank_nicolson(**kw, store_every=1, phonon_history_out=hist_a)
        rated = run_2d_crank_nicolson(**kw, store_every=3, phonon_history_out=hist_b, phonon_rates_out=sink,
                                      phonon_rates_regions=regions, phonon_rates_every=1)
    assert sorted(sink) == ["cells", "channels", "integrated_rates", "phonon_energy_bins", "rates", "regions", "times"]
    steps = [list(twin[0]).index(t) for t in rated[0]]
    assert len(steps) >= 3 and len(twin[0]) > len(rated[0])
    for k, s in enumerate(steps):
        assert np.array_equal(rated[1][k], twin[1][s], equal_nan=True)
        assert np.array_equal(np.stack(rated[4][k]), np.stack(twin[4][s]), equal_nan=True)
        assert np.array_equal(np.stack(hist_b["phonon_energy_frames"][k]), np.stack(hist_a["phonon_energy_frames"][s]),
                              equal_nan=True)
    mask = kw["mask"]
    nw = len(hist_a["phonon_energy_bins"])
    assert sink["channels"] == list(PR.CHANNELS) and sink["regions"] == list(regions)
    assert sink["cells"] == [int((r & mask).sum()) for r in regions.values()]
    assert sink["rates"].shape == (len(twin[0]), len(regions), 4, nw)
    assert sink["integrated_rates"].shape == sink["rates"].shape[:3]
    _check_against_stored_frames(sink, twin, hist_a, kw, regions, gap_values, name)
    if "none" in regions:
        assert not sink["rates"][:, list(regions).index("none")].any()
    assert np.all(sink["rates"][:, 0].sum(axis=-1) > 0.0)


def test_all_four_sinks_at_once_leave_each_sink_as_its_solo_run():
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw, regions = _run_arguments(12)
    solo = [{}, {}, {}, {}]
    t, c, r, p = {}, {}, {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run_2d_crank_nicolson(**kw, store_every=100, trace_out=solo[0], trace_regions=regions, trace_every=2)
        run_2d_crank_nicolson(**kw, store_every=100, coarse_out=solo[1], coarse_bin=4, coarse_every=3)
        run_2d_crank_nicolson(**kw, store_every=100, rates_out=solo[2], rates_regions=regions, rates_every=4)
        run_2d_crank_nicolson(**kw, store_every=100, phonon_rates_out=solo[3], phonon_rates_regions=regions,
                              phonon_rates_every=5)
        run_2d_crank_nicolson(**kw, store_every=100, trace_out=t, trace_regions=regions, trace_every=2, coarse_out=c,
                              coarse_bin=4, coarse_every=3, rates_out=r, rates_regions=regions, rates_every=4,
                              phonon_rates_out=p, phonon_rates_regions=regions, phonon_rates_every=5)
    for got, alone, keys in ((t, solo[0], ("density", "number")), (c, solo[1], ("energy_sums", "frames")),
                             (r, solo[2], ("rates", "number_rates")), (p, solo[3], ("rates", "integrated_rates"))):
        assert got["times"] == alone["times"] and sorted(got) == sorted(alone)
        for key in keys:
            assert got[key].tobytes() == alone[key].tobytes(), key
    assert len(p["times"]) == 3 and len(r["times"]) == 3 and len(t["times"]) == 5


def _ensemble_arguments(sweep: bool):
    from qpsim_amd.models import ExternalGenerationSpec
    kw, regions = _run_arguments(12)
    rng = np.random.default_rng(11)
    gen = [2e-5, 2e-5, 2e-5] if sweep else [1e-5, 3e-5, 0.0]
    members = [dict(initial_field=1e-4 * (1.0 + rng.random(kw["mask"].shape)),
                    external_generation=ExternalGenerationSpec(mode="constant", rate=rate)) for rate in gen]
    kw.pop("initial_field")
    kw.pop("external_generation")
    kw.update(store_every=3, phonon_rates_regions=regions, phonon_rates_every=3)
    return kw, members, regions, ({"tau_0": [440.0, 300.0, 600.0]} if sweep else None)


def test_ensemble_members_give_the_phonon_rates_of_their_lone_runs():
    """Three members on the 20 x 28 masked grid, ADI in both calls (the ensemble module's bit-equality conditions): each
    member's state and phonons are those of its lone run bit for bit, and so is its dict."""
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from qpsim_amd.solver import run_2d_crank_nicolson
    common, members, _, _ = _ensemble_arguments(False)
    sinks: list = ["stale"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, phonon_rates_out=sinks, **common)
        assert len(sinks) == 3 and len(got) == 3
        for m, member in enumerate(members):
            lone: dict = {}
            alone = run_2d_crank_nicolson(**dict(common, **member), phonon_rates_out=lone)
            _same_frames(got[m], alone)
            assert sorted(sinks[m]) == sorted(lone)
            for key in ("times", "regions", "cells", "channels"):
                assert sinks[m][key] == lone[key]
            for key in ("phonon_energy_bins", "rates", "integrated_rates"):
                assert sinks[m][key].tobytes() == lone[key].tobytes(), key
    assert sinks[0]["rates"].tobytes() != sinks[1]["rates"].tobytes()


def test_swept_ensemble_members_against_the_helper_with_their_own_tables():
    """With ``sweep=`` a member runs other collision kernels than its lone run (member tables through the class map), so
    its state agrees with the lone run's to rounding only; what is held to the bound is each member's rates against the
    helper with that member's own tables on that member's own stored frames."""
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    common, members, regions, swept = _ensemble_arguments(True)
    histories = [{} for _ in members]
    members = [dict(member, phonon_history_out=h) for member, h in zip(members, histories)]
    sinks: list = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=swept, phonon_rates_out=sinks, **common)
    assert len(sinks) == 3
    for m in range(3):
        kw = dict(common, tau_0=swept["tau_0"][m])
        _check_against_stored_frames(sinks[m], got[m], histories[m], kw, regions, None, f"swept member {m}")
    assert sinks[0]["rates"].tobytes() != sinks[1]["rates"].tobytes() != sinks[2]["rates"].tobytes()
