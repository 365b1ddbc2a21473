"""Time traces on the GPU: ``qp_region_sums`` against exact sums, traced runs against the untraced path, ensembles against
lone runs, and a recorded reference run.

The error bound of a sum is derived, not measured: whatever the order, a floating-point sum of n non-negative doubles lies
within (n - 1) 2^-53 sum(x) of the exact sum (every partial sum is at most sum(x), each of the n - 1 additions rounds once).
The exact sum is ``math.fsum``; n is the cell count of the region (cells outside a region enter the kernel as exact + 0.0).

Bitwise equality of an ensemble member's trace with its lone run holds under the conditions ``qpsim_amd.ensemble`` gives
for bit-equal states (``diffusion_scheme="adi"``, same tile family, same step form) and an even cell count of the device
grid: with an odd count every second member plane starts on an odd element and pairs its cells differently.
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import pytest

from golden_utils import GoldenRun

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CHUNK = 8192      # kRegionChunk of csrc/qp_misc.hip: the cells of a plane one stage-1 block reduces


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
def _region_bits(rng, ncm, nregion):
    """Regions of a case: everything, nothing, two identical random ones, another random one, the first cell only (the
    scalar head of a plane that starts on an odd element), the last cell only (the scalar tail), a sparse one."""
    twin = rng.random(ncm) < 0.5
    kinds = {"all": np.ones(ncm, dtype=bool), "empty": np.zeros(ncm, dtype=bool), "twin": twin,
             "other": rng.random(ncm) < 0.3, "first": np.arange(ncm) == 0, "last": np.arange(ncm) == ncm - 1,
             "sparse": rng.random(ncm) < 0.01}
    order = {1: ["other"], 2: ["all", "empty"]}.get(nregion,
                                                    ["all", "empty", "twin", "twin", "other", "first", "last", "sparse"][:nregion])
    regions = [kinds[k] for k in order]
    bits = np.zeros(ncm, dtype=np.uint8)
    for r, region in enumerate(regions):
        bits |= region.astype(np.uint8) << r
    return order, regions, bits


def _launch(torch, lib, state, bits, nfield, ncm, members, nregion):
    nbytes = int(lib.qp_region_sums_workspace_bytes(nfield, ncm, members, nregion))
    assert nbytes == 8 * nfield * members * nregion * ((ncm + CHUNK - 1) // CHUNK)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((members, nregion, nfield), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.qp_region_sums(_p(state), _p(bits), nfield, ncm, members, nregion, _p(ws), _p(out),
                              int(torch.cuda.current_stream().cuda_stream)) == 0
    return out.cpu().numpy()


# ncell_member: 1; around a wave; odd with three members (misaligned member planes); chunk edges; three chunks with a ragged
# last one (odd again).  nregion 1 and 8 and the sizes in between that round up to 4 and 8; nfield 1 and 50.
KERNEL_CASES = [(1, 1, 1, 1), (1, 3, 8, 2), (63, 1, 8, 1), (64, 1, 8, 50), (65, 3, 8, 2), (65, 2, 1, 50), (130, 2, 5, 3),
                (CHUNK, 1, 2, 1), (CHUNK + 1, 2, 3, 1), (2 * CHUNK + 777, 3, 8, 2), (3 * CHUNK + 100, 1, 1, 1)]


@pytest.mark.parametrize("ncm,members,nregion,nfield", KERNEL_CASES)
def test_region_sums_against_exact_sums(torch, lib, ncm, members, nregion, nfield):
    rng = np.random.default_rng(ncm * 131 + members * 17 + nregion)
    host = rng.random((nfield, members, ncm)) ** 4 * 1e3
    order, regions, bits_host = _region_bits(rng, ncm, nregion)
    state = torch.as_tensor(host, device="cuda")
    bits = torch.as_tensor(bits_host, device="cuda")
    got = _launch(torch, lib, state, bits, nfield, ncm, members, nregion)
    assert not np.isnan(got).any(), "every entry of out is written"
    again = _launch(torch, lib, state, bits, nfield, ncm, members, nregion)
    assert got.tobytes() == again.tobytes(), "the reduction is reproducible bit for bit"
    worst = 0.0
    for m in range(members):
        for r, region in enumerate(regions):
            n = int(region.sum())
            for f in range(nfield):
                exact = math.fsum(host[f, m][region])
                bound = max(n - 1, 0) * U * exact
                err = abs(got[m, r, f] - exact)
                worst = max(worst, err / bound if bound else err)
                assert err <= bound, (m, order[r], f, got[m, r, f], exact, bound)
    print(f"region sums {ncm} x {members} x {nregion} x {nfield}: worst error / bound = {worst:.3g}")
    if "empty" in order:
        assert np.all(got[:, order.index("empty")] == 0.0) and not np.signbit(got[:, order.index("empty")]).any()
    if order.count("twin") == 2:
        a, b = [k for k, name in enumerate(order) if name == "twin"]
        assert got[:, a].tobytes() == got[:, b].tobytes()
    if "first" in order:
        assert np.array_equal(got[:, order.index("first")], host[:, :, 0].T)
        assert np.array_equal(got[:, order.index("last")], host[:, :, -1].T)
    # a state that is only 8-byte aligned takes the 8-byte loads and adds the same pairs: same bits
    shifted = torch.empty(host.size + 1, dtype=torch.float64, device="cuda")[1:]
    shifted.copy_(state.reshape(-1))
    assert _p(shifted) % 16 == 8
    assert _launch(torch, lib, shifted, bits, nfield, ncm, members, nregion).tobytes() == got.tobytes()


def test_region_sums_ignore_what_lies_outside_a_region(torch, lib):
    """NaN and infinities in cells of no region do not reach any sum (the bits are read instead of flags)."""
    ncm, members, nfield = 200, 2, 3
    rng = np.random.default_rng(5)
    host = rng.random((nfield, members, ncm))
    inside = rng.random(ncm) < 0.6
    poisoned = host.copy()
    poisoned[:, :, ~inside] = np.where(rng.random((nfield, members, int((~inside).sum()))) < 0.5, np.nan, np.inf)
    bits = torch.as_tensor(inside.astype(np.uint8) * 3, device="cuda")
    clean = _launch(torch, lib, torch.as_tensor(host * inside, device="cuda"), bits, nfield, ncm, members, 2)
    got = _launch(torch, lib, torch.as_tensor(poisoned, device="cuda"), bits, nfield, ncm, members, 2)
    assert np.isfinite(got).all() and got.tobytes() == clean.tobytes()


def test_region_sums_refuse_bad_arguments(torch, lib):
    state = torch.zeros(64, dtype=torch.float64, device="cuda")
    bits = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ok = dict(state=_p(state), bits=_p(bits), nfield=1, ncm=64, members=1, nregion=1, ws=_p(state), out=_p(state))
    for bad in (dict(nregion=0), dict(nregion=9), dict(state=0), dict(bits=0), dict(ws=0), dict(out=0), dict(nfield=0),
                dict(ncm=0), dict(members=-1)):
        a = dict(ok, **bad)
        assert lib.qp_region_sums(a["state"], a["bits"], a["nfield"], a["ncm"], a["members"], a["nregion"], a["ws"], a["out"],
                                  0) == -1, bad
    assert lib.qp_region_sums_workspace_bytes(0, 64, 1, 1) == 0 and lib.qp_region_sums_workspace_bytes(1, 64, 1, 0) == 0


# ------------------------------------------------------------------------------------------------ whole runs
def _geometry(kind: str):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    if kind == "rect":
        mask = np.ones((24, 40), dtype=bool)
    else:                                  # a 9 x 11 grid with holes inside a padded frame: the device grid is cropped
        mask = np.zeros((12, 15), dtype=bool)
        mask[2:11, 3:14] = True
        mask[4:6, 6:8] = False
        mask[8, 10] = False
        mask[2, 3] = False
    edges = extract_edge_segments(mask)
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 1e-5), BoundaryCondition("absorbing"),
             BoundaryCondition("robin", 0.3, 1e-6)]
    bcs = {e.edge_id: (kinds[i % 4] if kind != "rect" else kinds[1]) for i, e in enumerate(edges)}
    left = np.zeros_like(mask)
    left[:, :mask.shape[1] // 2] = True
    band = np.zeros_like(mask)
    band[3:7, :] = True
    regions = {"all": mask.copy(), "left": left, "band": band, "none": np.zeros_like(mask)}
    return mask, edges, bcs, regions


def _run_arguments(kind: str, mode: str):
    from qpsim_amd.models import ExternalGenerationSpec
    mask, edges, bcs, regions = _geometry(kind)
    init = 1e-4 * (1.0 + np.random.default_rng(3).random(mask.shape))
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1,
              total_time=0.75, dx=0.5, diffusion_scheme="cn_exact" if mode == "cn_exact" else "adi")
    if mode != "scalar":
        kw.update(energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=8, enable_recombination=True,
                  enable_scattering=True, T_c=1.2, external_generation=ExternalGenerationSpec(mode="constant", rate=2e-5))
    return kw, regions


def _exact_region_sums(frames_per_point, mask, regions):
    """(exact sums [S, R, planes], their error bounds) from the frames of the store points."""
    sums = np.array([[[math.fsum(frame[region & mask]) for frame in frames] for region in regions.values()]
                     for frames in frames_per_point])
    cells = np.array([int((region & mask).sum()) for region in regions.values()])
    return sums, np.maximum(cells - 1, 0)[None, :, None] * U * sums


@pytest.mark.parametrize("mode", ["adi", "cn_exact", "scalar"])
@pytest.mark.parametrize("kind", ["rect", "holes"])
def test_traced_run_against_the_untraced_path(kind, mode):
    """8 steps with a remainder, sampled every 2 without stores in between, against the run that stores every 2.  The
    ``number`` bound is the bound of the sums scaled by dx^2 dE NE (both sides sum the same non-negative values in other
    orders; the observed difference is printed)."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw, regions = _run_arguments(kind, mode)
    mask, dx = kw["mask"], kw["dx"]
    trace: dict = {"stale": True}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        traced = run_2d_crank_nicolson(**kw, store_every=100, trace_out=trace, trace_regions=regions, trace_every=2)
        stored = run_2d_crank_nicolson(**kw, store_every=2)
    assert sorted(trace) == ["cells", "density", "energy_bins", "number", "regions", "times"]
    assert trace["times"] == list(stored[0]) and len(trace["times"]) == 5 and list(traced[0]) == [stored[0][0], stored[0][-1]]
    assert trace["regions"] == list(regions) and trace["cells"] == [int((r & mask).sum()) for r in regions.values()]
    # same kernel sequence up to every sampled step: the frames both runs store are the same bits
    for k in (0, -1):
        assert np.array_equal(traced[1][k], stored[1][k], equal_nan=True)
        assert traced[2][k] == stored[2][k]
        if mode != "scalar":
            assert np.array_equal(np.stack(traced[4][k]), np.stack(stored[4][k]), equal_nan=True)
    if mode == "scalar":
        assert trace["energy_bins"] is None and traced[4] is None
        planes, dE, ne = [[frame] for frame in stored[1]], 1.0, 1
    else:
        assert np.array_equal(trace["energy_bins"], stored[5])
        planes, dE, ne = stored[4], float(stored[5][1] - stored[5][0]), 8
    exact, bound = _exact_region_sums(planes, mask, regions)
    assert trace["density"].shape == exact.shape == (5, 4, ne)
    err = np.abs(trace["density"] - exact)
    print(f"{kind} {mode}: density worst error / bound = {np.max(err[bound > 0] / bound[bound > 0]):.3g}")
    assert np.all(err <= bound)
    assert np.all(trace["density"][:, 3] == 0.0) and np.all(trace["density"][:, 0] > 0.0)
    mass = np.asarray(stored[2])
    number_bound = dx * dx * dE * ne * bound[:, 0].sum(axis=-1)
    diff = np.abs(trace["number"][:, 0] - mass)
    print(f"{kind} {mode}: |number - mass| / bound = {np.max(diff / number_bound):.3g}")
    assert trace["number"].shape == (5, 4) and np.all(diff <= number_bound)


def _ensemble_arguments(sweep: bool):
    from qpsim_amd.models import ExternalGenerationSpec
    kw, regions = _run_arguments("rect", "adi")
    rng = np.random.default_rng(11)
    rates = [2e-5, 2e-5, 2e-5] if sweep else [1e-5, 3e-5, 0.0]
    members = [dict(initial_field=1e-4 * (1.0 + rng.random(kw["mask"].shape)),
                    external_generation=ExternalGenerationSpec(mode="constant", rate=rate)) for rate in rates]
    kw.pop("initial_field")
    kw.pop("external_generation")
    kw.update(store_every=100, trace_regions=regions, trace_every=2)
    return kw, members, ({"tau_0": [440.0, 300.0, 600.0]} if sweep else None)


@pytest.mark.parametrize("sweep", [False, True], ids=["rates", "swept_tau_0"])
def test_ensemble_members_trace_what_their_lone_runs_trace(sweep):
    """Three members (other initial fields; other generation rates or a swept tau_0) on the 24 x 40 rectangle: ADI on the
    64 x 64 tile family in both calls, 960 cells per member (even, a multiple of 64)."""
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from qpsim_amd.solver import run_2d_crank_nicolson
    common, members, swept = _ensemble_arguments(sweep)
    sinks: list = ["stale"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, sweep=swept, trace_out=sinks, **common)
        assert len(sinks) == 3 and len(got) == 3
        for m, member in enumerate(members):
            lone: dict = {}
            extra = {} if swept is None else {key: values[m] for key, values in swept.items()}
            run_2d_crank_nicolson(**dict(common, **member, **extra), trace_out=lone)
            rel = np.max(np.abs(sinks[m]["density"] - lone["density"])) / np.max(lone["density"])
            print(f"member {m}: max |ensemble - lone| / max = {rel:.3g}")
            assert sinks[m]["times"] == lone["times"] and sinks[m]["regions"] == lone["regions"]
            assert sinks[m]["cells"] == lone["cells"] and np.array_equal(sinks[m]["energy_bins"], lone["energy_bins"])
            assert sinks[m]["density"].tobytes() == lone["density"].tobytes()
            assert sinks[m]["number"].tobytes() == lone["number"].tobytes()
    assert sinks[0]["density"].tobytes() != sinks[1]["density"].tobytes()


def test_trace_of_a_recorded_reference_run():
    """``full_physics_16x16_ne8_mixed_bc`` stores every 5 steps and all energy frames.  Each cell agrees with the reference
    within tol max|frame| (the existing parity), so a sum over the cells of a region agrees within cells tol max|frame|."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    run = GoldenRun("full_physics_16x16_ne8_mixed_bc")
    kw = dict(run.kwargs)
    mask = kw["mask"]
    corner = np.zeros_like(mask)
    corner[:7, 5:] = True
    regions = {"all": mask.copy(), "corner": corner}
    trace: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run_2d_crank_nicolson(**kw, trace_out=trace, trace_regions=regions, trace_every=int(kw["store_every"]))
    golden = run.expected("energy_frames")                                  # [S, NE, ny, nx]
    assert np.allclose(trace["times"], run.expected("times"), rtol=0, atol=1e-12)
    want = np.array([[[math.fsum(frame[region & mask]) for frame in frames] for region in regions.values()] for frames in golden])
    cells = np.array(trace["cells"], dtype=float)
    bound = cells[None, :, None] * run.tol * float(np.nanmax(np.abs(golden)))
    err = np.abs(trace["density"] - want)
    print(f"reference run: worst error / bound = {np.max(err / bound):.3g}")
    assert trace["density"].shape == want.shape and np.all(err <= bound)
