"""Collision rate traces on the GPU: ``qp_collision_rates`` alone against the exact sums of tests/collision_rates_ref.py
within the derived bound (NE + 8 + cells - 1) 2^-53, its determinism, and the ``rates_out`` sink of both public calls
against the helper evaluated on the frames a run stores at the same steps."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

import collision_rates_ref as R
from golden_utils import GoldenRun, oracle_kwargs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def lib():
    from qpsim_amd import _hip
    return _hip.load()


def _p(t):
    return int(t.data_ptr())


# ------------------------------------------------------------------------------------------------ the kernel alone
def _device_tables(torch, lib, case, ncm, members, family):
    """The device tables of a case as ``Engine.make_collision_tables`` uploads them: (struct, tensors kept alive)."""
    from qpsim_amd import collision_tables as CT
    t = case["tables"]
    idx_d, idx_s, sg = t["maps"]
    plan = CT.plan_collision_tables(lib, ncm, np.ones(ncm, dtype=bool), t["kr"], t["ks"], t["rho"], idx_d, idx_s, sg,
                                    case["cls"][0] if family == "classes" else None, members=members,
                                    member_classes=family == "members")
    assert plan.symmetric and plan.nw == case["nw"]
    dev = {name: None if a is None else torch.as_tensor(a, device="cuda") for name, a in plan.arrays.items()}
    return plan.struct({name: 0 if a is None else _p(a) for name, a in dev.items()}), dev


def _launch(torch, lib, struct, state, ph, bits, ne, ncm, members, nregion, dE, en_r, en_s):
    import ctypes as C
    nbytes = int(lib.qp_collision_rates_workspace_bytes(ne, ncm, members, nregion))
    assert nbytes == 8 * members * ((ncm + R.CHUNK - 1) // R.CHUNK) * nregion * 4 * ne      # the formula of the header
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((members, nregion, 4, ne), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.qp_collision_rates(C.byref(struct), _p(bits), ncm, members, nregion, _p(state), _p(ph), float(dE), int(en_r),
                                int(en_s), _p(ws), _p(out), int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.qp_last_error()
    return out.cpu().numpy()


def _run_case(torch, lib, case_key, state=None, ph=None):
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case = R.case_inputs(ne, kind, ncm, members, nregion, family)
    struct, keep = _device_tables(torch, lib, case, ncm, members, family)
    d_state = torch.as_tensor(np.array(case["state"] if state is None else state), device="cuda")
    d_ph = torch.as_tensor(np.array(case["ph"] if ph is None else ph), device="cuda")
    d_bits = torch.as_tensor(np.array(case["bits"]), device="cuda")
    got = _launch(torch, lib, struct, d_state, d_ph, d_bits, ne, ncm, members, nregion, case["tables"]["dE"], en_r, en_s)
    return case, got, (struct, keep, d_state, d_ph, d_bits)


@pytest.mark.parametrize("case_key", R.KERNEL_CASES + R.MANY_CHUNK_CASES, ids=lambda c: f"ne{c[0]}-{c[1]}-{c[2]}x{c[3]}-r{c[4]}-{c[6]}")
def test_rates_against_exact_sums(torch, lib, case_key):
    ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
    case, got, (struct, keep, d_state, d_ph, d_bits) = _run_case(torch, lib, case_key)
    assert got.shape == (members, nregion, 4, ne) and not np.isnan(got).any(), "every entry of out is written"
    again = _launch(torch, lib, struct, d_state, d_ph, d_bits, ne, ncm, members, nregion, case["tables"]["dE"], en_r, en_s)
    assert got.tobytes() == again.tobytes(), "a second launch gives the same bits"
    flat = lambda a: a.reshape(a.shape[0], -1)  # noqa: E731
    exact = R.channels(flat(case["state"]), flat(case["ph"]), R.case_tables(case, en_r, en_s), case["cls"].reshape(-1),
                       en_r, en_s, dtype=np.longdouble).reshape(4, ne, members, ncm)
    worst = 0.0
    for m in range(members):
        for r, region in enumerate(case["regions"]):
            want = R.region_sums(exact[:, :, m], region)
            limit = R.bound(ne, int(region.sum())) * want
            err = np.abs(got[m, r] - want)
            worst = max(worst, float(np.max(err[limit > 0] / limit[limit > 0], initial=0.0)))
            assert np.all(err <= limit), (m, case["names"][r], float(np.max(err - limit)))
    print(f"rates {case_key}: worst error / bound = {worst:.3g}")
    names = case["names"]
    if not en_r:
        assert not got[:, :, 2:].any() and not np.signbit(got[:, :, 2:]).any(), "a disabled process gives exact zeros"
    if not en_s:
        assert not got[:, :, :2].any() and not np.signbit(got[:, :, :2]).any()
    if "empty" in names:
        k = names.index("empty")
        assert not got[:, k].any() and not np.signbit(got[:, k]).any()
    if names.count("twin") == 2:
        a, b = [k for k, name in enumerate(names) if name == "twin"]
        assert got[:, a].tobytes() == got[:, b].tobytes()
    if "all" in names and en_r and en_s:
        assert np.all(got[:, names.index("all")] > 0.0)


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
        one = _launch(torch, lib, struct, d_state, d_ph, d_bits, ne, ncm, 1, nregion, t["dE"], en_r, en_s)
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


# ------------------------------------------------------------------------------------------------ whole runs
def _masked_geometry(ny=20, nx=28):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((ny, nx), dtype=bool)
    mask[ny // 4:ny // 4 + 3, nx // 3:nx // 3 + 4] = False
    mask[ny - 3, nx - 5] = False
    mask[0, 0] = False
    edges = extract_edge_segments(mask)
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 1e-5), BoundaryCondition("absorbing"),
             BoundaryCondition("robin", 0.3, 1e-6)]
    bcs = {e.edge_id: kinds[i % 4] for i, e in enumerate(edges)}
    left = np.zeros_like(mask)
    left[:, :nx // 2] = True
    band = np.zeros_like(mask)
    band[3:7, :] = True
    regions = {"all": mask.copy(), "left": left, "band": band, "none": np.zeros_like(mask)}
    return mask, edges, bcs, regions


def _run_arguments(ne, ny=20, nx=28, scheme="adi"):
    from qpsim_amd.models import ExternalGenerationSpec
    mask, edges, bcs, regions = _masked_geometry(ny, nx)
    init = 1e-4 * (1.0 + np.random.default_rng(3).random(mask.shape))
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1,
              total_time=0.75, dx=0.5, diffusion_scheme=scheme, energy_gap=180.0, energy_min_factor=1.0,
              energy_max_factor=3.0, num_energy_bins=ne, enable_recombination=True, enable_scattering=True, T_c=1.2,
              external_generation=ExternalGenerationSpec(mode="constant", rate=2e-5))
    return kw, regions


def _run_tables(kw, gap_values=None):
    """The collision tables of a run as the helper takes them, and the class of every interior cell (packed order)."""
    from qpsim_amd import tables as T
    gap = kw["energy_gap"]
    E, dE = T.build_energy_grid(gap, kw.get("energy_min_factor", 1.0), kw.get("energy_max_factor", 10.0), kw["num_energy_bins"])
    tau0 = kw.get("tau_0", 440.0)
    tau_r, tau_s, T_c, gamma = kw.get("tau_r") or tau0, kw.get("tau_s") or tau0, kw.get("T_c", 1.2), kw.get("dynes_gamma", 0.0)
    n = int(kw["mask"].sum())
    gaps, cls = (np.array([gap]), np.zeros(n, dtype=int)) if gap_values is None else np.unique(gap_values, return_inverse=True)
    tables = dict(kr=np.stack([T.recombination_kernel_base(E, float(g), tau_r, T_c) for g in gaps]),
                  ks=np.stack([T.scattering_kernel_base(E, float(g), tau_s, T_c) for g in gaps]),
                  rho=np.stack([T.dynes_density_of_states(E, float(g), gamma) for g in gaps]),
                  maps=T.build_phonon_frequency_map(E)[1:], dE=float(dE))
    return tables, cls


def _check_rates_against_stored_frames(sink, stored, history, kw, regions, gap_values=None, label=""):
    """``rates`` [S, R, 4, NE] against the helper on the energy frames and phonon frames of the store points."""
    mask, ne = kw["mask"], kw["num_energy_bins"]
    tables, cls = _run_tables(kw, gap_values)
    en_r, en_s = kw["enable_recombination"], kw["enable_scattering"]
    worst = 0.0
    for s in range(len(stored[0])):
        n = np.stack(stored[4][s])[:, mask]
        p = np.stack(history["phonon_energy_frames"][s])[:, mask]
        exact = R.channels(n, p, R.case_tables(dict(tables=tables), en_r, en_s), cls, en_r, en_s, dtype=np.longdouble)
        for r, region in enumerate(regions.values()):
            inside = (region & mask)[mask]
            want = R.region_sums(exact, inside)
            limit = R.bound(ne, int(inside.sum())) * want
            err = np.abs(sink["rates"][s, r] - want)
            worst = max(worst, float(np.max(err[limit > 0] / limit[limit > 0], initial=0.0)))
            assert np.all(err <= limit), (s, r, float(np.max(err - limit)))
    print(f"{label}: rates worst error / bound = {worst:.3g}")
    dE = tables["dE"]
    assert np.allclose(sink["number_rates"], kw["dx"] ** 2 * dE * sink["rates"].sum(axis=-1), rtol=1e-14, atol=0)


def _same_frames(a, b):
    assert list(a[0]) == list(b[0])
    for k in range(len(a[0])):
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True)
        assert np.array_equal(np.stack(a[4][k]), np.stack(b[4][k]), equal_nan=True)


@pytest.mark.parametrize("name", ["ne12_dynamic_phonons", "ne50_16x16", "nonuniform_gap_4x4"])
def test_rates_of_a_run_against_the_helper_on_its_stored_frames(name):
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
        plain = run_2d_crank_nicolson(**kw, store_every=3, phonon_history_out=hist_a)
        rated = run_2d_crank_nicolson(**kw, store_every=3, phonon_history_out=hist_b, rates_out=sink, rates_regions=regions,
                                      rates_every=3)
    assert sorted(sink) == ["cells", "channels", "energy_bins", "number_rates", "rates", "regions", "times"]
    _same_frames(plain, rated)
    for s in range(len(plain[0])):
        assert np.array_equal(np.stack(hist_a["phonon_energy_frames"][s]), np.stack(hist_b["phonon_energy_frames"][s]),
                              equal_nan=True)
    ne, mask = kw["num_energy_bins"], kw["mask"]
    assert sink["times"] == list(plain[0]) and len(sink["times"]) >= 3
    assert sink["channels"] == list(R.CHANNELS) and sink["regions"] == list(regions)
    assert sink["cells"] == [int((r & mask).sum()) for r in regions.values()]
    assert np.array_equal(sink["energy_bins"], plain[5])
    assert sink["rates"].shape == (len(plain[0]), len(regions), 4, ne) and sink["number_rates"].shape == sink["rates"].shape[:3]
    _check_rates_against_stored_frames(sink, plain, hist_a, kw, regions, gap_values, name)
    if "none" in regions:
        assert not sink["rates"][:, list(regions).index("none")].any()
    assert np.all(sink["rates"][:, 0].sum(axis=-1) > 0.0)


def test_rates_beside_a_trace_and_coarse_frames_leave_each_sink_as_its_solo_run():
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw, regions = _run_arguments(12)
    solo_t, solo_c, solo_r, t, c, r = {}, {}, {}, {}, {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run_2d_crank_nicolson(**kw, store_every=100, trace_out=solo_t, trace_regions=regions, trace_every=2)
        run_2d_crank_nicolson(**kw, store_every=100, coarse_out=solo_c, coarse_bin=4, coarse_every=3)
        run_2d_crank_nicolson(**kw, store_every=100, rates_out=solo_r, rates_regions=regions, rates_every=4)
        run_2d_crank_nicolson(**kw, store_every=100, trace_out=t, trace_regions=regions, trace_every=2, coarse_out=c,
                              coarse_bin=4, coarse_every=3, rates_out=r, rates_regions=regions, rates_every=4)
    for got, solo, keys in ((t, solo_t, ("density", "number")), (c, solo_c, ("energy_sums", "frames")),
                            (r, solo_r, ("rates", "number_rates"))):
        assert got["times"] == solo["times"] and sorted(got) == sorted(solo)
        for key in keys:
            assert got[key].tobytes() == solo[key].tobytes(), key
    assert len(r["times"]) == 3 and len(t["times"]) == 5


def _ensemble_arguments(sweep: bool):
    from qpsim_amd.models import ExternalGenerationSpec
    kw, regions = _run_arguments(12)
    rng = np.random.default_rng(11)
    gen = [2e-5, 2e-5, 2e-5] if sweep else [1e-5, 3e-5, 0.0]
    members = [dict(initial_field=1e-4 * (1.0 + rng.random(kw["mask"].shape)),
                    external_generation=ExternalGenerationSpec(mode="constant", rate=rate)) for rate in gen]
    kw.pop("initial_field")
    kw.pop("external_generation")
    kw.update(store_every=3, rates_regions=regions, rates_every=3)
    return kw, members, regions, ({"tau_0": [440.0, 300.0, 600.0]} if sweep else None)


def test_ensemble_members_give_the_rates_of_their_lone_runs():
    """Three members on the 20 x 28 masked grid, ADI in both calls (the ensemble module's bit-equality conditions): each
    member's state is the state of its lone run bit for bit, and so is its dict."""
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from qpsim_amd.solver import run_2d_crank_nicolson
    common, members, _, _ = _ensemble_arguments(False)
    sinks: list = ["stale"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, rates_out=sinks, **common)
        assert len(sinks) == 3 and len(got) == 3
        for m, member in enumerate(members):
            lone: dict = {}
            alone = run_2d_crank_nicolson(**dict(common, **member), rates_out=lone)
            _same_frames(got[m], alone)
            assert sorted(sinks[m]) == sorted(lone)
            for key in ("times", "regions", "cells", "channels"):
                assert sinks[m][key] == lone[key]
            assert sinks[m]["rates"].tobytes() == lone["rates"].tobytes()
            assert sinks[m]["number_rates"].tobytes() == lone["number_rates"].tobytes()
    assert sinks[0]["rates"].tobytes() != sinks[1]["rates"].tobytes()


def test_swept_ensemble_members_against_the_helper_with_their_own_tables():
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    common, members, regions, swept = _ensemble_arguments(True)
    histories = [{} for _ in members]
    members = [dict(member, phonon_history_out=h) for member, h in zip(members, histories)]
    sinks: list = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=swept, rates_out=sinks, **common)
    assert len(sinks) == 3
    for m in range(3):
        kw = dict(common, tau_0=swept["tau_0"][m])
        assert sinks[m]["times"] == list(got[m][0])
        _check_rates_against_stored_frames(sinks[m], got[m], histories[m], kw, regions, None, f"swept member {m}")
    assert sinks[0]["rates"].tobytes() != sinks[1]["rates"].tobytes() != sinks[2]["rates"].tobytes()
