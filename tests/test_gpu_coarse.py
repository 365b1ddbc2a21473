"""Coarse frames on the GPU: ``qp_block_sums`` against exact sums, runs with coarse frames against the plain path, ensembles
against lone runs, and a recorded reference run.

The error bound of a sum is derived, not measured: whatever the order, a floating-point sum of n non-negative doubles lies
within (n - 1) 2^-53 sum(x) of the exact sum (every partial sum is at most sum(x), each of the n - 1 additions rounds once;
a cell outside the mask or the grid enters as an exact + 0.0).  The exact sum is ``math.fsum``; n is the number of active
cells of the block.

Measured on an MI355X (each test prints its figure): worst error / bound 0.999 over the kernel cases (b = 4, 50 planes),
0.10 - 0.83 over the runs; the recorded reference run agrees to 8.8e-15 of its largest block sum.
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import pytest

from golden_utils import GoldenRun

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ACTIVE = 16       # QP_FLAG_ACTIVE of include/qpsim_hip.h


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


def _coarse_shape(ny, nx, oy, ox, b):
    return -(-(oy + ny) // b), -(-(ox + nx) // b)


def _launch(torch, lib, state, flags, nfield, ny, nx, members, b, oy, ox):
    cny, cnx = _coarse_shape(ny, nx, oy, ox, b)
    out = torch.full((members, nfield, cny, cnx), float("nan"), dtype=torch.float64, device="cuda")
    assert lib.qp_block_sums(_p(state), _p(flags), nfield, ny, nx, members, b, oy, ox, _p(out),
                             int(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _block_cells(active, oy, ox, b):
    """{(cy, cx): flat indices of the active cells of the block}, every block of the output included."""
    ny, nx = active.shape
    cny, cnx = _coarse_shape(ny, nx, oy, ox, b)
    cells = {(cy, cx): [] for cy in range(cny) for cx in range(cnx)}
    for j, i in zip(*np.nonzero(active)):
        cells[(oy + j) // b, (ox + i) // b].append(j * nx + i)
    return cells


# ------------------------------------------------------------------------------------------------ the kernel alone
# (ny, nx, oy, ox, b, members, nfield): one cell; one block larger than the grid; just below, at and just above a wave of
# columns with the smallest blocks and offsets; 50 planes; several waves across and several row groups down with offsets in
# both directions; b = 64 with ox = 63 (one column in the first wave); b = 32 with two rounds of rows; a single column
# with an odd cell count and three members (member planes start on odd elements).
KERNEL_CASES = [(1, 1, 0, 0, 2, 1, 1), (5, 7, 0, 0, 64, 1, 2), (9, 63, 1, 1, 2, 3, 1), (9, 64, 0, 0, 4, 1, 50),
                (9, 65, 3, 5, 8, 3, 2), (33, 129, 7, 15, 16, 2, 3), (70, 130, 5, 63, 64, 1, 2), (40, 200, 31, 0, 32, 2, 1),
                (65, 1, 0, 0, 8, 3, 1)]


def _case_inputs(ny, nx, oy, ox, b, members, nfield, empty_block=False):
    rng = np.random.default_rng(ny * 1009 + nx * 31 + b)
    host = rng.random((nfield, members, ny, nx)) ** 4 * 1e3
    active = rng.random((ny, nx)) < 0.7
    if empty_block:                                        # the block of device cell (ny / 2, nx / 2) loses all its cells
        cy, cx = (oy + ny // 2) // b, (ox + nx // 2) // b
        jj, ii = np.indices((ny, nx))
        active[((oy + jj) // b == cy) & ((ox + ii) // b == cx)] = False
    # the other flag bits are set at random: only QP_FLAG_ACTIVE may matter
    flags = (rng.integers(0, 16, (ny, nx)) | np.where(active, ACTIVE, 0) | rng.integers(0, 4, (ny, nx)) * 32).astype(np.uint8)
    return host, active, flags


def _check_against_exact(got, host, active, oy, ox, b, label):
    nfield, members = host.shape[:2]
    cells = _block_cells(active, oy, ox, b)
    worst, singles, empties = 0.0, 0, 0
    for (cy, cx), idx in cells.items():
        n = len(idx)
        for m in range(members):
            for f in range(nfield):
                values = host[f, m].reshape(-1)[idx]
                exact = math.fsum(values)
                bound = max(n - 1, 0) * U * exact
                err = abs(got[m, f, cy, cx] - exact)
                worst = max(worst, err / bound if bound else err)
                assert err <= bound, (label, m, f, cy, cx, n, got[m, f, cy, cx], exact, bound)
                if n == 0:
                    assert got[m, f, cy, cx] == 0.0 and not np.signbit(got[m, f, cy, cx]), "an empty block gives +0.0"
                if n == 1:
                    assert got[m, f, cy, cx] == values[0], "a block with one active cell returns that cell"
        singles += n == 1
        empties += n == 0
    print(f"block sums {label}: worst error / bound = {worst:.3g}; {len(cells)} blocks, {singles} with one cell, "
          f"{empties} empty")
    return singles, empties


@pytest.mark.parametrize("ny,nx,oy,ox,b,members,nfield", KERNEL_CASES)
def test_block_sums_against_exact_sums(torch, lib, ny, nx, oy, ox, b, members, nfield):
    host, active, flags_host = _case_inputs(ny, nx, oy, ox, b, members, nfield)
    state = torch.as_tensor(host, device="cuda")
    flags = torch.as_tensor(flags_host, device="cuda")
    got = _launch(torch, lib, state, flags, nfield, ny, nx, members, b, oy, ox)
    assert got.shape == (members, nfield) + _coarse_shape(ny, nx, oy, ox, b)
    assert not np.isnan(got).any(), "every entry of out is written"
    _check_against_exact(got, host, active, oy, ox, b, (ny, nx, oy, ox, b, members, nfield))
    again = _launch(torch, lib, state, flags, nfield, ny, nx, members, b, oy, ox)
    assert got.tobytes() == again.tobytes(), "the reduction is reproducible bit for bit"
    assert np.array_equal(state.cpu().numpy(), host) and np.array_equal(flags.cpu().numpy(), flags_host), "inputs are only read"
    # member m of a batch gives the bytes of a lone launch on its slice (odd member planes included)
    for m in range(members):
        lone = _launch(torch, lib, state[:, m].contiguous(), flags, nfield, ny, nx, 1, b, oy, ox)
        assert lone[0].tobytes() == got[m].tobytes(), f"member {m}"
    # a plane of the batch gives the bytes of a launch on that plane alone
    alone = _launch(torch, lib, state[nfield - 1, members - 1].contiguous(), flags, 1, ny, nx, 1, b, oy, ox)
    assert alone[0, 0].tobytes() == got[members - 1, nfield - 1].tobytes()
    # a state that is only 8-byte aligned gives the same bytes
    shifted = torch.empty(host.size + 1, dtype=torch.float64, device="cuda")[1:]
    shifted.copy_(state.reshape(-1))
    assert _p(shifted) % 16 == 8
    assert _launch(torch, lib, shifted, flags, nfield, ny, nx, members, b, oy, ox).tobytes() == got.tobytes()
    # NaN and infinities planted in inactive cells change no output bit
    poisoned = host.copy()
    junk = np.array([np.nan, np.inf, -np.inf])[np.random.default_rng(1).integers(0, 3, host.shape)]
    poisoned[:, :, ~active] = junk[:, :, ~active]
    dirty = _launch(torch, lib, torch.as_tensor(poisoned, device="cuda"), flags, nfield, ny, nx, members, b, oy, ox)
    assert np.isfinite(dirty).all() and dirty.tobytes() == got.tobytes()


def test_block_sums_with_an_empty_block_and_single_cells(torch, lib):
    """33 x 129 at b = 16 with one block emptied, and 9 x 65 at b = 2 (random mask at 70 %: many blocks of one cell)."""
    seen = [0, 0]
    for ny, nx, oy, ox, b, members, nfield in ((33, 129, 7, 15, 16, 2, 3), (9, 65, 1, 0, 2, 2, 2)):
        host, active, flags_host = _case_inputs(ny, nx, oy, ox, b, members, nfield, empty_block=b == 16)
        got = _launch(torch, lib, torch.as_tensor(host, device="cuda"), torch.as_tensor(flags_host, device="cuda"), nfield, ny,
                      nx, members, b, oy, ox)
        assert not np.isnan(got).any()
        singles, empties = _check_against_exact(got, host, active, oy, ox, b, (ny, nx, oy, ox, b, "emptied" if b == 16 else ""))
        seen[0] += singles
        seen[1] += empties
    assert seen[0] > 0 and seen[1] > 0


def test_block_sums_refuse_bad_arguments(torch, lib):
    state = torch.zeros(64, dtype=torch.float64, device="cuda")
    flags = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ok = dict(state=_p(state), flags=_p(flags), nfield=1, ny=8, nx=8, members=1, b=8, oy=0, ox=0, out=_p(state))
    for bad in (dict(b=3), dict(ox=8), dict(out=0), dict(state=0), dict(flags=0), dict(b=128), dict(oy=-1), dict(ny=0),
                dict(members=0), dict(nfield=0)):
        a = dict(ok, **bad)
        assert lib.qp_block_sums(a["state"], a["flags"], a["nfield"], a["ny"], a["nx"], a["members"], a["b"], a["oy"], a["ox"],
                                 a["out"], 0) == -1, bad
        assert b"qp_block_sums" in lib.qp_last_error()


# ------------------------------------------------------------------------------------------------ whole runs
def _geometry(kind: str):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    if kind == "rect":
        mask = np.ones((20, 28), dtype=bool)
    else:                                  # 37 x 44: a margin on all sides (origin inside a block) and a hole with a whole block
        mask = np.zeros((37, 44), dtype=bool)
        mask[3:35, 5:42] = True
        mask[15:25, 15:26] = False
    edges = extract_edge_segments(mask)
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 1e-5), BoundaryCondition("absorbing"),
             BoundaryCondition("robin", 0.3, 1e-6)]
    bcs = {e.edge_id: (kinds[i % 4] if kind != "rect" else kinds[1]) for i, e in enumerate(edges)}
    return mask, edges, bcs


def _run_arguments(kind: str, scalar: bool = False):
    from qpsim_amd.models import ExternalGenerationSpec
    mask, edges, bcs = _geometry(kind)
    init = 1e-4 * (1.0 + np.random.default_rng(3).random(mask.shape))
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1,
              total_time=1.25, dx=0.5, diffusion_scheme="adi")             # 12 steps of 0.1 and one of 0.05
    if not scalar:
        kw.update(energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=6, enable_recombination=True,
                  enable_scattering=True, T_c=1.2, external_generation=ExternalGenerationSpec(mode="constant", rate=2e-5))
    return kw


def _same(a, b) -> bool:
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and (
            a.tobytes() == b.tobytes() if a.dtype.kind == "f" else np.array_equal(a, b))
    return a == b


def _exact_block_sums(frames, mask, b):
    """(exact sums [cy, cx] of a full frame over the in-mask cells of each block, active cells per block)."""
    cells = _block_cells(mask, 0, 0, b)
    cy, cx = _coarse_shape(mask.shape[0], mask.shape[1], 0, 0, b)
    flat = np.asarray(frames).reshape(-1)
    sums, count = np.zeros((cy, cx)), np.zeros((cy, cx), dtype=int)
    for (y, x), idx in cells.items():
        sums[y, x], count[y, x] = math.fsum(flat[idx]), len(idx)
    return sums, count


@pytest.mark.parametrize("kind,scalar,b", [("rect", False, 8), ("holes", False, 4), ("holes", True, 8)],
                         ids=["rect", "holes", "holes_scalar"])
def test_run_with_coarse_frames_against_the_plain_path(kind, scalar, b):
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw = _run_arguments(kind, scalar)
    mask = kw["mask"]
    ne = 1 if scalar else 6
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain_history: dict = {}
        plain = run_2d_crank_nicolson(**kw, store_every=3, phonon_history_out=plain_history)
        one: dict = {"stale": True}
        one_history: dict = {}
        stored = run_2d_crank_nicolson(**kw, store_every=3, phonon_history_out=one_history, coarse_out=one, coarse_bin=b,
                                       coarse_every=3)
        two: dict = {}
        sparse = run_2d_crank_nicolson(**kw, store_every=13, coarse_out=two, coarse_bin=b, coarse_every=3)
    # 1. the run itself is untouched by the sampling
    assert _same(list(stored), list(plain)) and _same(one_history, plain_history)
    assert sorted(one) == ["bin", "cells", "energy_bins", "energy_frames", "energy_sums", "frames", "times"]
    assert one["times"] == list(plain[0]) and len(one["times"]) == 6 and one["bin"] == b
    # 2. a sampled step is sequenced like a stored one
    assert two["energy_sums"].tobytes() == one["energy_sums"].tobytes() and two["times"] == one["times"]
    assert list(sparse[0]) == [plain[0][0], plain[0][-1]]
    for k in (0, -1):
        assert _same(sparse[1][k], plain[1][k]) and sparse[2][k] == plain[2][k]
        if not scalar:
            assert _same(list(sparse[4][k]), list(plain[4][k]))
    # 3. against exact block sums of the frames this run stored at the same steps
    planes = [[frame] for frame in plain[1]] if scalar else plain[4]
    from qpsim_amd.engine import coarse_layout
    lay = coarse_layout(mask, b)
    assert np.array_equal(one["cells"], lay.cells) and one["energy_sums"].shape == (6, ne) + lay.shape
    worst = 0.0
    for s, frames in enumerate(planes):
        for i, frame in enumerate(frames):
            exact, count = _exact_block_sums(np.nan_to_num(frame), mask, b)
            assert np.array_equal(count, lay.cells)
            bound = np.maximum(count - 1, 0) * U * exact
            err = np.abs(one["energy_sums"][s, i] - exact)
            assert np.all(err <= bound), (s, i, float(np.max(err - bound)))
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    print(f"{kind} scalar={scalar} b={b}: energy_sums worst error / bound = {worst:.3g}")
    # 4. the derived keys
    empty = lay.cells == 0
    if kind == "holes":
        assert empty.any() and (lay.cells[~empty] < b * b).any()
    assert np.all(one["energy_sums"][:, :, empty] == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        want_frames = one["energy_sums"] / lay.cells
    assert np.array_equal(np.isnan(one["energy_frames"]), np.broadcast_to(empty, one["energy_frames"].shape))
    assert np.array_equal(one["energy_frames"][:, :, ~empty], want_frames[:, :, ~empty])
    assert np.array_equal(np.isnan(one["frames"]), np.broadcast_to(empty, one["frames"].shape))
    if scalar:
        assert one["energy_bins"] is None and np.array_equal(one["frames"], one["energy_frames"][:, 0], equal_nan=True)
    else:
        assert np.array_equal(one["energy_bins"], plain[5])
        dE = float(plain[5][1] - plain[5][0])
        total = one["energy_sums"][:, 0].copy()
        for i in range(1, ne):
            total += one["energy_sums"][:, i]
        # dE sum_i sums / cells: ne - 1 additions, one product, one division
        with np.errstate(invalid="ignore"):                  # 0 / 0 in the blocks that are left out
            want = total * dE / lay.cells
        np.testing.assert_allclose(one["frames"][:, ~empty], want[:, ~empty], rtol=(ne + 1) * 2 * U, atol=0)


def test_trace_and_coarse_frames_in_one_call():
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw = _run_arguments("holes")
    mask = kw["mask"]
    trace: dict = {}
    coarse: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run_2d_crank_nicolson(**kw, store_every=13, trace_out=trace, trace_every=4, coarse_out=coarse, coarse_bin=8, coarse_every=3)
    assert len(trace["times"]) == 5 and len(coarse["times"]) == 6                  # steps 0 4 8 12 13 and 0 3 6 9 12 13
    common = [(trace["times"].index(t), coarse["times"].index(t)) for t in trace["times"] if t in coarse["times"]]
    assert len(common) == 3                                                        # t = 0, step 12, step 13
    n = int(mask.sum())
    for ts, cs in common:
        total = coarse["energy_sums"][cs].sum(axis=(-2, -1))
        density = trace["density"][ts, 0]
        # both are sums of the same n non-negative cells: each within (n - 1) u of the exact sum
        bound = 2 * (n - 1) * U * np.maximum(total, density)
        print(f"sample {ts}/{cs}: |coarse total - trace density| / bound = {np.max(np.abs(total - density) / bound):.3g}")
        assert np.all(np.abs(total - density) <= bound)


def test_ensemble_members_get_the_coarse_frames_of_their_lone_runs():
    """Three members (other initial fields, other diffusion coefficients) on the 20 x 28 rectangle: ADI on the same tile
    family in both calls, so the states are bit-equal and the coarse frames with them."""
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw = _run_arguments("rect")
    rng = np.random.default_rng(11)
    members = [dict(initial_field=1e-4 * (1.0 + rng.random(kw["mask"].shape)), diffusion_coefficient=d) for d in (6.0, 4.0, 8.0)]
    kw.pop("initial_field")
    kw.pop("diffusion_coefficient")
    kw.update(store_every=13, coarse_bin=8, coarse_every=3)
    sinks: list = ["stale"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, coarse_out=sinks, **kw)
        assert len(sinks) == 3 and len(got) == 3
        for m, member in enumerate(members):
            lone: dict = {}
            run_2d_crank_nicolson(**dict(kw, **member), coarse_out=lone)
            assert _same(sinks[m], lone), f"member {m}"
    assert sinks[0]["energy_sums"].tobytes() != sinks[1]["energy_sums"].tobytes()


def test_a_failed_member_gets_none():
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    kw = _run_arguments("rect")
    base = kw.pop("initial_field")
    members = [dict(initial_field=base), dict(initial_field=base * 1e9), dict(initial_field=base * 0.5)]
    kw.update(store_every=13, coarse_bin=4, coarse_every=3, pauli_error_threshold=1.0, enforce_pauli=True)
    sinks: list = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = run_2d_crank_nicolson_ensemble(members, errors="return", coarse_out=sinks, **kw)
    kinds = ["error" if isinstance(r, Exception) else "ok" for r in got]
    assert kinds == ["ok", "error", "ok"], got
    assert sinks[1] is None and sinks[0]["bin"] == 4 and len(sinks[2]["times"]) == 6


def test_coarse_frames_of_a_recorded_reference_run():
    """``masked_holes_mixed_bc_9x11`` (scalar mode, the plane is u) stores every 5 steps; with ``coarse_every = store_every``
    the block sums at the store points agree with the block sums of the golden frames to the 2-D parity tolerance of
    ``test_gpu_parity.py``: 1e-9 relative to the largest block sum of the plane."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    run = GoldenRun("masked_holes_mixed_bc_9x11")
    kw = dict(run.kwargs)
    mask = kw["mask"]
    coarse: dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = run_2d_crank_nicolson(**kw, coarse_out=coarse, coarse_bin=2, coarse_every=int(kw["store_every"]))
    from golden_utils import rel_err
    assert np.allclose(res[0], run.expected("times"), rtol=0, atol=1e-12)
    assert rel_err(np.stack(res[1]), run.expected("frames")) < run.tol
    scale = max(float(np.max(np.abs(run.expected("mass")))), 1e-300)
    assert np.max(np.abs(np.asarray(res[2]) - run.expected("mass"))) <= run.tol * scale
    assert res[4] is None and res[5] is None and coarse["energy_bins"] is None
    assert np.allclose(coarse["times"], run.expected("times"), rtol=0, atol=1e-12)
    golden = run.expected("frames")                                         # [S, ny, nx]
    assert coarse["energy_sums"].shape == (golden.shape[0], 1, 5, 6)
    worst = 0.0
    for s, frame in enumerate(golden):
        want, count = _exact_block_sums(np.nan_to_num(frame), mask, 2)
        assert np.array_equal(count, coarse["cells"])
        err = float(np.max(np.abs(coarse["energy_sums"][s, 0] - want))) / float(np.max(want))
        worst = max(worst, err)
        assert err <= 1e-9, (s, err)
    print(f"reference run: worst block-sum error relative to the largest block sum = {worst:.3g}")
