"""The reductions and the elementwise kernels of csrc/qp_misc.hip past their first round, each against NumPy.

Every launch geometry of that file has a cap; past it a thread takes a second trip of its grid-stride loop, a merge stage
sees more than one partial per block, or a finish holds a second tile.  The production sizes all run there.  Next to each
case list stands a restatement of the launch geometry in plain Python, and every case asserts the regime it claims from it;
tests/test_reduction_rounds_host.py reads the mirrored constants out of the sources, so a changed constant fails loudly.

  kernel                                   regime                                      begins at
  qp_pauli_stats                           lane u >= 1 holds a cell (cap on bx binds)  NE 12: 21 761 cells, NE 50: 5 121
                                           second trip of a thread                     NE 12: 87 041 cells
  qp_pauli_stats_members                   second trip inside a member                 5 members, ne 7: 14 849 cells a member
                                           a block strides over bins (budget < ne)     ne 7: 293 members
                                           one block per member (budget 1)             1 025 members
  fused guard, lone (pauli_merge_kernel)   two partials per merge block                32 769 cells
  fused guard, members (..._final_kernel)  second trip over a member's partials        16 448 cells a member
  qp_region_sums (region_final_kernel)     second LDS tile                             4 194 305 cells a member
  per-field norms (absmax_fields_kernel)   second trip over a field's partials         257 rows (general, row-wise rectangle),
                                                                                       1 025 rows (banded rectangle), <= 3 fields
  qp_absmax                                second trip                                 262 145 elements
  kernels behind grid_for                  second trip                                 2 097 153 elements

(The batched finish of qp_collision_rates / qp_phonon_rates, from 32 chunks of 1024 cells, is in the case lists of
tests/collision_rates_ref.py.)  Not reached: the `k += 256` trip of the third guard stage (pauli_final_kernel reads the 512
merge partials in two trips at any size, but a second trip of the merge stage's own loop needs more than 256 partials per
merge block: 8.39 M cells).

No tolerance here is tuned to a kernel: a result is either equal to NumPy bit for bit, or within a bound counted from the
roundings of the operation (u = 2^-53), stated where it is used.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import collision_rates_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ACTIVE = 16                   # QP_FLAG_ACTIVE of include/qpsim_hip.h
THREADS = 256                 # threads of a block in every kernel here
# the constants of the sources that the geometry below mirrors (tests/test_reduction_rounds_host.py compares them)
RED_BLOCKS = 1024             # kRedBlocks, csrc/qp_misc.hip
GUARD_MERGE_BLOCKS = 512      # kGuardMergeBlocks, csrc/qp_common.h
REGION_CHUNK = 8192           # kRegionChunk, csrc/qp_misc.hip
REGION_TILE = 512             # kRegionTile, csrc/qp_misc.hip
RATES_CHUNK = R.CHUNK         # QP_RATES_CHUNK, include/qpsim_hip.h
RATES_BATCH = R.FINAL_BATCH   # B of rates_final_kernel (the finish of both rate kernels)
MEMBER_GUARD_BUDGET = 2048    # blocks in all of pauli_members_partial_kernel (pauli_member_budget)
GRID_FOR_BLOCKS = 8192        # cap of grid_for, csrc/qp_misc.hip
NORM_SLOTS = 1024             # partial slots of the per-field norms (stencil_combine_launch, rect_combine_launch)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def lib():
    from qpsim_amd import _hip
    return _hip.load()


def _p(t):
    return 0 if t is None else int(t.data_ptr())


def _stream(torch):
    return int(torch.cuda.current_stream().cuda_stream)


def _ceil(a, b):
    return -(-a // b)


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ================================================================================================ the Pauli guard, standalone
def pauli_reference(n, rho, cls, flags, members, floor):
    """NumPy per member slice of n [ne, members * ncm]: f = where(rho > 1e-30, n / max(rho, 1e-30), 0) over the active
    cells, np.argmax in C order of the member's [ne, ncm] (NaN is the maximum, the first NaN wins), the first index with
    rho <= 1e-30 and n > floor or -1.  Returns (values [members], argmax [members], forbidden [members]), member-local."""
    ne = n.shape[0]
    ncm = n.shape[1] // members
    rho_c = rho[0][:, None] if cls is None else rho[cls].T
    with np.errstate(invalid="ignore"):
        f = np.where(rho_c > 1e-30, n / np.maximum(rho_c, 1e-30), 0.0)
        active = (flags & ACTIVE) != 0
        bad = (rho_c <= 1e-30) & (n > floor) & active[None, :]
    f = np.where(active[None, :], f, -np.inf)
    per_member = lambda a: a.reshape(ne, members, ncm).transpose(1, 0, 2).reshape(members, ne * ncm)  # noqa: E731
    f, bad = per_member(f), per_member(bad)
    k = np.argmax(f, axis=1)
    return f[np.arange(members), k], k, np.where(bad.any(axis=1), np.argmax(bad, axis=1), -1)


def pauli_geometry(ne, ncell):
    """qp_pauli_stats: grid (bx, by) of 256 threads; a thread handles cells p0 + u stride, u = 0 ... 3, per trip."""
    by = min(ne, RED_BLOCKS)
    bx = max(1, min(_ceil(ncell, THREADS), RED_BLOCKS // by))
    stride = THREADS * bx
    return dict(bx=bx, by=by, stride=stride, trips=_ceil(ncell, 4 * stride), bins_per_block=_ceil(ne, by))


def pauli_cell(geo, p):
    """(trip, lane u, blockIdx.x) of cell p."""
    return p // (4 * geo["stride"]), p % (4 * geo["stride"]) // geo["stride"], p % geo["stride"] // THREADS


def _guard_tables(ne, nclass):
    """rho [nclass, ne] of test_gpu_ensemble._guard_inputs (its two classes; the first alone for one class); the last
    class has no states in bins 2 and ne - 2 (there: bin 2), so that two forbidden bins exist for the C-order placement."""
    rho = np.stack([np.linspace(1.0, 2.0, ne), np.linspace(1.5, 0.5, ne)])[:nclass]
    rho[-1, 2] = 0.0
    rho[-1, ne - 2] = 0.0
    return rho


def _guard_state(rng, ne, ncm, members, rho, nclass, forced):
    """Occupations below 0.8, ~15 % of the cells inactive (the cells of `forced` active), nothing in a forbidden bin."""
    n = members * ncm
    flags = np.where(rng.random(n) < 0.85, ACTIVE, 0).astype(np.uint8) | rng.integers(0, 16, size=n).astype(np.uint8)
    flags[np.asarray(forced)] |= ACTIVE
    cls = None if nclass == 1 else (rng.random(n) < 0.5).astype(np.int32)
    rho_c = np.broadcast_to(rho[0][:, None], (ne, n)) if cls is None else rho[cls].T
    return rng.random((ne, n)) * 0.8 * rho_c, flags, cls, rho_c


def _lone_stats(torch, lib, ws, d_state, d_rho, d_cls, d_flags, ne, nclass, ncell):
    vals = torch.zeros(2, dtype=torch.float64, device="cuda")
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.qp_pauli_stats(_p(d_state), _p(d_rho), _p(d_cls), _p(d_flags), ne, nclass, ncell, 1e-18, _p(ws), _p(vals),
                              _p(idx), _stream(torch)) == 0
    i = idx.cpu().numpy()
    return vals.cpu().numpy()[0], int(i[0]), int(i[1])


# (ne, classes, cells, what the case is there for)
PAULI_CASES = [(12, 1, 21761, "first cell of lane 1"), (12, 1, 87041, "first cell of a second trip"),
               (12, 1, 100003, "ragged second trip"), (50, 1, 30011, "two trips at bx = 20"),
               (7, 2, 150001, "two classes, two trips"), (600, 1, 3001, "bx = 1: one block per bin, three trips")]
PAULI_REGIMES = {21761: dict(bx=85, trips=1, last=(0, 1, 0)), 87041: dict(bx=85, trips=2, last=(1, 0, 0)),
                 100003: dict(bx=85, trips=2, last=(1, 0, 50)), 30011: dict(bx=20, trips=2, last=(1, 1, 17)),
                 150001: dict(bx=146, trips=2, last=(1, 0, 1)), 3001: dict(bx=1, trips=3, last=(2, 3, 0))}


@pytest.mark.parametrize("ne,nclass,ncell,what", PAULI_CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_pauli_stats_past_the_first_lane_and_trip(torch, lib, ne, nclass, ncell, what):
    """Value, argmax and forbidden index equal NumPy exactly, with the winner planted in turn (one launch each)."""
    geo = pauli_geometry(ne, ncell)
    want_regime = PAULI_REGIMES[ncell]
    assert (geo["bx"], geo["trips"]) == (want_regime["bx"], want_regime["trips"]), geo
    assert geo["bx"] * THREADS < ncell, "the cap binds: lanes u >= 1 hold real cells"
    assert pauli_cell(geo, ncell - 1) == want_regime["last"], (what, pauli_cell(geo, ncell - 1))
    assert geo["bins_per_block"] == 1
    cells = np.arange(ncell)
    trip, lane, block = pauli_cell(geo, cells)
    top_lane = int(lane.max())
    assert top_lane == (1 if ncell == 21761 else 3)
    lane3 = int(cells[lane == top_lane][-1])            # the last cell of the highest lane (3 but for 21 761 cells)
    first_of_last_trip = (geo["trips"] - 1) * 4 * geo["stride"]
    early, mid = 300, ncell // 3                        # block 1 of trip 0; somewhere in between
    assert block[early] != block[lane3] or geo["bx"] == 1
    forced = [0, early, mid, lane3, first_of_last_trip, ncell - 1]
    rng = np.random.default_rng(ne * 1000003 + ncell)
    rho = _guard_tables(ne, nclass)
    base, flags, cls, rho_c = _guard_state(rng, ne, ncell, 1, rho, nclass, forced)
    zero_bins = (2, ne - 2)
    if cls is None:
        base[list(zero_bins), :] = 0.0
    else:
        base[np.ix_(list(zero_bins), np.flatnonzero(cls == nclass - 1))] = 0.0
    good = [b for b in range(ne) if np.all(rho[:, b] > 0)]
    lo_bin, hi_bin = good[0], good[-1]
    assert lo_bin == 0 and hi_bin == ne - 1
    forb_cells = np.flatnonzero(((flags & ACTIVE) != 0) & (True if cls is None else cls == nclass - 1))
    f_late = int(forb_cells[forb_cells >= first_of_last_trip][-1])       # in the last trip
    f_early = int(forb_cells[forb_cells < f_late][5])
    nan = float("nan")
    # name -> ([(bin, cell, occupation or None for a density in a forbidden bin)], the (bin, cell) that must win, forbidden)
    placements = {
        "last active cell": ([(hi_bin, ncell - 1, 2.0)], (hi_bin, ncell - 1), None),
        "highest lane": ([(lo_bin + 1, lane3, 2.0)], (lo_bin + 1, lane3), None),
        "cell 0": ([(lo_bin, 0, 2.0)], (lo_bin, 0), None),
        "tie of two blocks in one bin": ([(hi_bin, lane3, 2.0), (hi_bin, early, 2.0)], (hi_bin, early), None),
        "tie of two bins": ([(hi_bin, early, 2.0), (lo_bin + 1, lane3, 2.0)], (lo_bin + 1, lane3), None),
        "NaN behind a larger value": ([(lo_bin, early, 4.0), (hi_bin, ncell - 1, nan)], (hi_bin, ncell - 1), None),
        "two NaNs": ([(hi_bin, early, nan), (lo_bin + 1, lane3, nan), (lo_bin, mid, 4.0)], (lo_bin + 1, lane3), None),
        "forbidden cells": ([(zero_bins[0], f_late, None), (zero_bins[1], f_early, None), (lo_bin, mid, 2.0)], (lo_bin, mid),
                            (zero_bins[0], f_late)),
    }
    d = lambda a: None if a is None else torch.as_tensor(a, device="cuda")  # noqa: E731
    d_rho, d_cls, d_flags, d_base = d(rho), d(cls), d(flags), d(base)
    ws = torch.empty(int(lib.qp_pauli_workspace_bytes()), dtype=torch.uint8, device="cuda")
    assert int(lib.qp_pauli_workspace_bytes()) >= 24 * geo["bx"] * geo["by"]
    want = pauli_reference(base, rho, cls, flags, 1, 1e-18)
    got = _lone_stats(torch, lib, ws, d_base, d_rho, d_cls, d_flags, ne, nclass, ncell)
    assert _same_bits(got[0], want[0][0]) and got[1:] == (int(want[1][0]), -1), ("unplanted", got, want)
    for name, (plants, winner, forbidden) in placements.items():
        host, dev = base.copy(), d_base.clone()
        for b, c, occ in plants:
            value = 1e-6 if occ is None else occ * rho_c[b, c]
            assert occ is None or rho_c[b, c] > 0
            host[b, c] = value
            dev[b, c] = value
        v, k, fb = (a[0] for a in pauli_reference(host, rho, cls, flags, 1, 1e-18))
        assert int(k) == winner[0] * ncell + winner[1], (name, "the planted cell is what NumPy picks")
        assert int(fb) == (-1 if forbidden is None else forbidden[0] * ncell + forbidden[1]), name
        got = _lone_stats(torch, lib, ws, dev, d_rho, d_cls, d_flags, ne, nclass, ncell)
        print(f"pauli_stats ne {ne} cells {ncell} [{name}]: got {got}, NumPy {(float(v), int(k), int(fb))}")
        assert _same_bits(got[0], v) and got[1:] == (int(k), int(fb)), (name, got, (v, k, fb))


def members_geometry(ne, ncm, members):
    """qp_pauli_stats_members: grid (bxm * members, by); the finish of a member loops `k += 256` over bxm * by partials."""
    budget = min(max(MEMBER_GUARD_BUDGET // members, 1), RED_BLOCKS)
    by = min(ne, budget)
    bxm = max(1, min(_ceil(ncm, THREADS), budget // by))
    return dict(budget=budget, by=by, bxm=bxm, stride=THREADS * bxm, trips=_ceil(ncm, THREADS * bxm),
                bins_per_block=_ceil(ne, by), partials=bxm * by)


MEMBERS_CASES = [(5, 7, 14849), (5, 7, 40001), (1000, 7, 300), (3000, 5, 130)]
MEMBERS_REGIMES = {(5, 14849): dict(budget=409, by=7, bxm=58, trips=2, bins_per_block=1, partials=406),
                   (5, 40001): dict(budget=409, by=7, bxm=58, trips=3, bins_per_block=1, partials=406),
                   (1000, 300): dict(budget=2, by=2, bxm=1, trips=2, bins_per_block=4, partials=2),
                   (3000, 130): dict(budget=1, by=1, bxm=1, trips=1, bins_per_block=5, partials=1)}


@pytest.mark.parametrize("members,ne,ncm", MEMBERS_CASES)
def test_pauli_stats_members_against_numpy_per_member(torch, lib, members, ne, ncm):
    """Every member against NumPy on its own slice, with NaN, ties and forbidden cells planted in the first member, the
    last member and one in between; 406 partials per member also take the member finish through a second trip."""
    geo = members_geometry(ne, ncm, members)
    regime = MEMBERS_REGIMES[(members, ncm)]
    assert {k: geo[k] for k in regime} == regime, geo
    assert members != 5 or (geo["bxm"] * THREADS < ncm and geo["partials"] > THREADS), "cap binds; the finish takes 2 trips"
    nclass = 2
    rng = np.random.default_rng(members * 7919 + ncm)
    rho = _guard_tables(ne, nclass)
    planted = [0, members // 2, members - 1]
    last, early, late = ncm - 1, 3, min(ncm - 2, geo["stride"] + 1 if geo["trips"] > 1 else ncm - 2)
    third = ncm // 3
    forced = [m * ncm + c for m in planted for c in (early, third, late, last)]
    base, flags, cls, rho_c = _guard_state(rng, ne, ncm, members, rho, nclass, forced)
    zero_bins = (2, ne - 2)
    base[np.ix_(list(zero_bins), np.flatnonzero(cls == 1))] = 0.0
    for m in planted:                                   # the forbidden placement needs class 1 in two cells
        cls[m * ncm + last] = 1
        cls[m * ncm + third] = 1
        base[list(zero_bins), m * ncm + last] = 0.0
        base[list(zero_bins), m * ncm + third] = 0.0
    rho_c = rho[cls].T
    for m in planted:                                   # ... and occupations below 0.8 under the new class
        for c in (last, third):
            base[:, m * ncm + c] = 0.1 * rho_c[:, m * ncm + c]
    hi_bin, nan = ne - 1, float("nan")
    placements = {
        "last cell of the member": ([(hi_bin, last, 2.0)], (hi_bin, last), None),
        "tie in one bin": ([(hi_bin, last, 2.0), (hi_bin, early, 2.0)], (hi_bin, early), None),
        "tie of two bins": ([(hi_bin, early, 2.0), (1, last, 2.0)], (1, last), None),
        "NaN behind a larger value": ([(0, early, 4.0), (hi_bin, last, nan)], (hi_bin, last), None),
        "two NaNs": ([(hi_bin, early, nan), (1, late, nan), (0, third, 4.0)], (1, late), None),
        "forbidden cells": ([(zero_bins[0], last, None), (zero_bins[1], third, None), (0, early, 2.0)], (0, early),
                            (zero_bins[0], last)),
    }
    d = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    d_rho, d_cls, d_flags, d_base = d(rho), d(cls), d(flags), d(base)
    nbytes = int(lib.qp_pauli_members_workspace_bytes(ncm, members))
    assert nbytes >= 24 * members * geo["partials"]
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    vals = torch.zeros(members, dtype=torch.float64, device="cuda")
    idx = torch.zeros(2 * members, dtype=torch.int64, device="cuda")
    for name, (plants, winner, forbidden) in placements.items():
        host, dev = base.copy(), d_base.clone()
        for m in planted:
            for b, c, occ in plants:
                value = 1e-6 if occ is None else occ * rho_c[b, m * ncm + c]
                assert occ is None or rho_c[b, m * ncm + c] > 0
                host[b, m * ncm + c] = value
                dev[b, m * ncm + c] = value
        v, k, fb = pauli_reference(host, rho, cls, flags, members, 1e-18)
        for m in planted:
            assert k[m] == winner[0] * ncm + winner[1], (name, m, "the planted cell is what NumPy picks")
            assert fb[m] == (-1 if forbidden is None else forbidden[0] * ncm + forbidden[1]), (name, m)
        vals.fill_(-7.0)
        idx.fill_(-7)
        assert lib.qp_pauli_stats_members(_p(dev), _p(d_rho), _p(d_cls), _p(d_flags), ne, nclass, ncm, members, 1e-18, _p(ws),
                                          _p(vals), _p(idx), _stream(torch)) == 0
        got_v, got_i = vals.cpu().numpy(), idx.cpu().numpy().reshape(members, 2)
        wrong = np.flatnonzero((got_i[:, 0] != k) | (got_i[:, 1] != fb) | (got_v.view(np.int64) != v.view(np.int64)))
        print(f"pauli_stats_members {members} x {ncm}, ne {ne} [{name}]: {wrong.size} members differ from NumPy")
        assert wrong.size == 0, (name, wrong[:5], got_v[wrong[:5]], got_i[wrong[:5]], v[wrong[:5]], k[wrong[:5]], fb[wrong[:5]])


# ================================================================================================ the fused guard
def merge_geometry(ncell):
    """Per-wave partials of the register and pair kernels (wave w: cells [64 w, 64 w + 64)) and their merge stage."""
    nparts = 2 * _ceil(ncell, 128)
    per = _ceil(nparts, GUARD_MERGE_BLOCKS)
    return dict(nparts=nparts, per=per, full=nparts // per, ragged=nparts % per, empty=GUARD_MERGE_BLOCKS - _ceil(nparts, per))


GUARD_GRIDS = {"66203": (239, 277), "32897": (67, 491)}
GUARD_REGIMES = {"66203": dict(nparts=1036, per=3, full=345, ragged=1, empty=166),
                 "32897": dict(nparts=516, per=2, full=258, ragged=0, empty=254)}


def _guard_engine(shape, waves):
    """A masked grid (~15 % inactive) whose cells 5 of the listed waves are active, its engine and the NE = 12 tables."""
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    rng = np.random.default_rng(shape[0])
    mask = rng.random(shape) > 0.15
    flat = mask.reshape(-1)
    for w in waves:
        flat[min(64 * w + 5, flat.size - 1)] = True
    flat[-1] = True
    z = np.zeros(shape)
    return Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z)), mask


@pytest.mark.parametrize("mode", ["plain", "ties_first_last", "ties_two_merge_blocks", "forbidden"])
@pytest.mark.parametrize("call", ["single_pair", "gap_classes_step"])
@pytest.mark.parametrize("grid", sorted(GUARD_GRIDS))
def test_fused_guard_with_several_partials_per_merge_block(torch, grid, call, mode):
    """`collide_pair_guarded` (one class) and `collide_guarded` (gap classes) at NE = 12 on the register route: the ticket
    equals NumPy on the downloaded state it describes and `Engine.pauli_stats` on the same device state.  Tied pixels are
    identical pixels (near-full occupation, copied state and phonons), the first of them must win."""
    from qpsim_amd import _hip
    from qpsim_amd import tables as T
    ne = 12
    shape = GUARD_GRIDS[grid]
    ncell = shape[0] * shape[1]
    geo = merge_geometry(ncell)
    assert ncell == int(grid) and geo == GUARD_REGIMES[grid], geo
    assert geo["per"] >= 2 and geo["empty"] > 0, "several partials per merge block; the last blocks are ragged or empty"
    last_wave = (ncell - 1) // 64
    first_of_block, last_of_block = geo["per"] * 100, geo["per"] * 200 + geo["per"] - 1
    tied_waves = {"ties_first_last": [0, last_wave], "ties_two_merge_blocks": [first_of_block, last_of_block]}.get(mode, [])
    assert [w // geo["per"] for w in tied_waves] in ([], [0, last_wave // geo["per"]], [100, 200])
    eng, mask = _guard_engine(shape, [0, last_wave, first_of_block, last_of_block])
    cell_of_px = np.flatnonzero(mask.reshape(-1))
    px_of_cell = {int(c): k for k, c in enumerate(cell_of_px)}
    n = cell_of_px.size
    nclass = 1 if call == "single_pair" else 3
    rng = np.random.default_rng(ncell + nclass)
    gaps = np.array([180.0, 171.0, 165.5])[:nclass]
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in gaps])
    kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in gaps])
    ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in gaps])
    cls = rng.integers(0, nclass, size=n)
    wave_cell = lambda w: min(64 * w + 5, ncell - 1)  # noqa: E731  (the last wave of 32 897 cells holds one cell)
    tied = [px_of_cell[wave_cell(w)] for w in tied_waves]
    assert [wave_cell(w) // 64 for w in tied_waves] == tied_waves
    for px in tied[1:]:
        cls[px] = cls[tied[0]]
    state = rng.random((ne, n)) * rho[cls].T * rng.choice([1e-5, 1e-2, 0.3, 0.5], size=n)[None, :]
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    forb_px = [n - 1, n // 2]                    # the last cell (the last wave that holds cells), and the middle
    if mode == "forbidden":                     # a bin without states that nevertheless holds density
        rho[:, 2] = 0.0
        state[2, :] = 0.0
        state[2, forb_px] = 1e-6
    if tied:                                    # near-full occupation (the others: at most half): the maximum after the update too
        state[:, tied[0]] *= 0.97 / np.max(state[:, tied[0]] / rho[cls[tied[0]]])
        for px in tied[1:]:
            state[:, px] = state[:, tied[0]]
            ph[:, px] = ph[:, tied[0]]
    tab = eng.make_collision_tables(kr, ks, rho, idx_d, idx_s, sg, cls if nclass > 1 else None,
                                    gap_params=dict(E=E, gaps=gaps, tau_r=500.0, tau_s=400.0, T_c=1.2))
    route = eng.lib.qp_collision_route(C.byref(tab["struct"]), eng.ncell, 1, 1, 1, 0)
    assert tab["kernel"] == "register" and route == (_hip.ROUTE_REGISTER if nclass == 1 else _hip.ROUTE_REGISTER_CLASSES)
    # the state the guard describes, from the unguarded call
    s_ref, p_ref = eng.upload_packed(state), eng.upload_packed(ph)
    out_ref = eng.empty(ne, eng.ncell)
    eng.collide(tab, s_ref, out_ref, p_ref, dE, 0.2, True, True, True)
    s_in, p_dev = eng.upload_packed(state), eng.upload_packed(ph)
    s_out = eng.empty(ne, eng.ncell)
    if call == "single_pair":                   # its guard describes the state after the first half-step
        assert tab["pair"]
        ticket = eng.collide_pair_guarded(tab, s_in, s_out, p_dev, dE, 0.2, 0.03, 0.0, True, True, True, 1e-18)
    else:
        ticket = eng.collide_guarded(tab, s_in, s_out, p_dev, dE, 0.2, True, True, True, 1e-18)
        assert np.array_equal(s_out.cpu().numpy(), out_ref.cpu().numpy())
    got = eng.pauli_stats_result(ticket)
    out = eng.download_packed(out_ref)
    rho_c = rho[cls].T
    f = np.where(rho_c > 1e-30, out / np.maximum(rho_c, 1e-30), 0.0)
    k = int(np.argmax(f))
    bad = np.flatnonzero(((rho_c <= 1e-30) & (out > 1e-18)).reshape(-1))
    want = (float(f.reshape(-1)[k]), (k // n, int(cell_of_px[k % n])),
            None if bad.size == 0 else (int(bad[0]) // n, int(cell_of_px[int(bad[0]) % n])))
    print(f"fused guard {grid} {call} {mode}: ticket {got}, NumPy {want}")
    assert got == want
    assert got == eng.pauli_stats(out_ref, tab, 1e-18)
    if mode == "forbidden":
        assert want[2] == (2, int(cell_of_px[n // 2])) and int(cell_of_px[n - 1]) == ncell - 1
    else:
        assert want[2] is None
    if tied:
        assert all(np.array_equal(out[:, tied[0]], out[:, px]) for px in tied[1:])
        assert want[1][1] == int(cell_of_px[tied[0]]) == wave_cell(tied_waves[0]), "the identical pixels carry the maximum"


def test_fused_member_guard_with_a_second_trip_over_a_members_partials(torch):
    """3 members of 16 448 = 257 x 64 cells: partial 256 of a member is thread 0's second trip in the member finish.  The
    tie and the forbidden cell of member 1 lie in its last wave; member-local indices against NumPy per member slice."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    ne, members, ny, nx = 12, 3, 64, 257
    ncm = ny * nx
    assert ncm == 16448 and ncm % 64 == 0 and ncm // 64 == THREADS + 1, "257 partials per member: 256 + 1"
    mask = np.ones((ny, nx), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = T.dynes_density_of_states(E, 180.0, 0.1)
    rho[2] = 0.0
    tab = eng.make_collision_tables(T.recombination_kernel_base(E, 180.0, 500.0, 1.2)[None],
                                    T.scattering_kernel_base(E, 180.0, 400.0, 1.2)[None], rho[None], idx_d, idx_s, sg)
    assert tab["kernel"] == "register" and tab["pair"] and eng.pair_members_supported(tab, ncm, members)
    rng = np.random.default_rng(41)
    n = members * ncm
    state = rng.random((ne, n)) * rho[:, None] * rng.choice([1e-5, 1e-2, 0.3, 0.5], size=n)[None, :]
    state[2, :] = 0.0
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    last_wave = ncm - 64
    tie_a, tie_b = ncm + last_wave + 3, ncm + last_wave + 40            # member 1, both in its partial 256
    forb = {1: last_wave + 17, 2: 100}                                  # member-local; member 0 has none
    for m, c in forb.items():
        state[2, m * ncm + c] = 1e-6
    live = np.arange(ne) != 2
    state[:, tie_a] *= 0.97 / np.max(state[live, tie_a] / rho[live])
    state[:, tie_b], ph[:, tie_b] = state[:, tie_a], ph[:, tie_a]
    flags = eng.d_flags.reshape(-1).repeat(members)
    results = {}
    for name in ("step", "pair"):
        s_in = torch.as_tensor(state, device="cuda")
        p_dev = torch.as_tensor(ph, device="cuda")
        s_out = torch.empty_like(s_in)
        if name == "step":
            ticket = eng.collide_guarded_members(tab, s_in, s_out, p_dev, dE, 0.2, True, True, True, 1e-18, ncm, members, flags)
            out = s_out.cpu().numpy()           # the pair's guard describes this state too: its first half-step
        else:
            ticket = eng.collide_pair_guarded_members(tab, s_in, s_out, p_dev, dE, 0.2, 0.03, 0.0, True, True, True, 1e-18,
                                                      ncm, members, flags)
        results[name] = eng.pauli_stats_members_result(ticket)
    v, k, fb = pauli_reference(out, rho[None], None, np.full(n, ACTIVE, dtype=np.uint8), members, 1e-18)
    want = [(float(v[m]), (int(k[m]) // ncm, int(k[m]) % ncm), None if fb[m] < 0 else (int(fb[m]) // ncm, int(fb[m]) % ncm))
            for m in range(members)]
    print(f"fused member guard: step {results['step']}, NumPy {want}")
    assert want[1][1][1] == tie_a - ncm and want[1][1][1] // 64 == THREADS, "member 1's maximum is the first tied pixel"
    assert np.array_equal(out[:, tie_a], out[:, tie_b])
    assert [w[2] for w in want] == [None, (2, forb[1]), (2, forb[2])]
    assert results["step"] == want and results["pair"] == want


# ================================================================================================ region sums
REGION_NCM = (REGION_TILE + 1) * REGION_CHUNK + 5


@pytest.fixture(scope="module")
def region_case():
    """One plane of 513 x 8192 + 5 cells with the eight regions of test_gpu_trace._region_bits and their exact sums."""
    from test_gpu_trace import _region_bits
    rng = np.random.default_rng(2024)
    host = rng.random(REGION_NCM) ** 4 * 1e3
    order, regions, bits = _region_bits(rng, REGION_NCM, 8)
    exact = [math.fsum(host[region]) for region in regions]
    for a in (host, bits):
        a.setflags(write=False)
    return host, order, regions, bits, exact


@pytest.mark.parametrize("nregion", [8, 3])
def test_region_sums_past_one_tile_of_chunk_partials(torch, lib, region_case, nregion):
    """514 chunk partials: the finish holds 512 in LDS, then 2 (the last of 5 cells).  Bound as in tests/test_gpu_trace.py:
    (n - 1) 2^-53 times the exact sum, for n non-negative terms in any order."""
    from test_gpu_trace import _launch
    host, order, regions, bits_host, exact = region_case
    nchunk = _ceil(REGION_NCM, REGION_CHUNK)
    assert (nchunk, _ceil(nchunk, REGION_TILE), nchunk - REGION_TILE, REGION_NCM - (nchunk - 1) * REGION_CHUNK) == (514, 2, 2, 5)
    assert order[:3] == ["all", "empty", "twin"] and order[3] == "twin"
    bits_case = bits_host & np.uint8((1 << nregion) - 1)
    state = torch.as_tensor(np.array(host), device="cuda")
    bits = torch.as_tensor(bits_case, device="cuda")
    got = _launch(torch, lib, state, bits, 1, REGION_NCM, 1, nregion)
    assert got.shape == (1, nregion, 1) and not np.isnan(got).any()
    assert _launch(torch, lib, state, bits, 1, REGION_NCM, 1, nregion).tobytes() == got.tobytes(), "a second launch: same bits"
    worst = 0.0
    for r in range(nregion):
        n = int(regions[r].sum())
        bound = max(n - 1, 0) * U * exact[r]
        err = abs(got[0, r, 0] - exact[r])
        worst = max(worst, err / bound if bound else err)
        assert err <= bound, (order[r], got[0, r, 0], exact[r], bound)
    print(f"region sums {REGION_NCM} cells, {nregion} regions: worst error / bound = {worst:.3g}")
    assert got[0, 1, 0] == 0.0 and not np.signbit(got[0, 1, 0])
    if nregion == 8:
        assert got[0, 2, 0] == got[0, 3, 0] and got[0, 5, 0] == host[0] and got[0, 6, 0] == host[-1]
    shifted = torch.empty(host.size + 1, dtype=torch.float64, device="cuda")[1:]
    shifted.copy_(state)
    assert _p(shifted) % 16 == 8
    assert _launch(torch, lib, shifted, bits, 1, REGION_NCM, 1, nregion).tobytes() == got.tobytes()


# ================================================================================================ per-field norms
def norms_geometry(kind, ny, nx, nfield):
    """Blocks per field (`per`) of the combine kernels with per-field norms and the block (within its field) of row j.
    general / rows: one row per block and trip; bands: bands of 4 rows (fewer than 2^22 cells) when nx % 4 == 0."""
    lanes = min(nfield, NORM_SLOTS)
    if kind == "bands":
        assert nx % 4 == 0 and nx <= 1024 and nfield * ny * nx < (1 << 22)
        items, rows_per_item = _ceil(ny, 4), 4
    else:
        assert kind == "general" or nx % 4 != 0
        items, rows_per_item = ny, 1
    per = min(NORM_SLOTS // lanes, items)
    return per, (lambda j: (j // rows_per_item) % per)


@pytest.mark.parametrize("nfield", [1, 3])
@pytest.mark.parametrize("kind,ny,nx", [("general", 300, 40), ("rows", 300, 41), ("bands", 1028, 40)])
def test_per_field_norms_past_256_partials_per_field(torch, kind, ny, nx, nfield):
    """The largest |out| of every field lies in a row whose block has index >= 256 within its field: the finish of that
    field reaches it in its second trip.  The norm equals the maximum of the plane the same call stored, exactly."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    per, block_of_row = norms_geometry(kind, ny, nx, nfield)
    assert per > THREADS, "a second trip of absmax_fields_kernel"
    mask = np.ones((ny, nx), dtype=bool)
    if kind == "general":
        mask[5:9, 7:11] = False
        mask[270:280, 20:25] = False
        mask[299, 0] = False
    edges = extract_edge_segments(mask)
    kinds = [BoundaryCondition("reflective"), BoundaryCondition("dirichlet", 1e-5), BoundaryCondition("absorbing"),
             BoundaryCondition("robin", 0.3, 1e-6)]
    bcs = {e.edge_id: (kinds[i % 4] if kind == "general" else kinds[1]) for i, e in enumerate(edges)}
    eng = Engine(compile_geometry(mask, edges, bcs, 0.9))
    op = DiffusionOperator(eng, nfield, 0.11, dcoef=[6.0, 0.35, 1.5][:nfield])
    assert (op.rect is None) == (kind == "general")
    rows = [(1024 + f) if kind == "bands" else (257 + 11 * f) for f in range(nfield)]
    assert all(block_of_row(j) >= THREADS for j in rows) and max(rows) < ny
    rng = np.random.default_rng(ny + nx + nfield)
    flat = mask.reshape(-1)
    u = rng.random((nfield, ny * nx)) * flat
    rin = rng.random((nfield, ny * nx)) * flat
    for f, j in enumerate(rows):
        assert mask[j, 13]
        rin[f, j * nx + 13] = -1e6 * (f + 1)
    d_u, d_rin = torch.as_tensor(u, device=eng.device), torch.as_tensor(rin, device=eng.device)
    out, norms = eng.empty(nfield, eng.ncell), eng.empty(nfield)
    norms.fill_(-1.0)
    eng.stencil(op, d_u, out, -1.0, 1.0, 1.0, 0.5, rin=d_rin, cr=1.0, norms_out=norms)
    plane = np.abs(out.cpu().numpy())
    assert [int(np.argmax(plane[f])) // nx for f in range(nfield)] == rows, "the maximum lies in the planted row"
    print(f"norms {kind} {ny} x {nx} x {nfield}: per = {per}, got {norms.cpu().numpy()}, NumPy {plane.max(axis=1)}")
    assert np.array_equal(norms.cpu().numpy(), plane.max(axis=1))
    if op.rect is not None:                      # norms only, no plane stored
        norms.fill_(-1.0)
        eng.stencil(op, d_u, None, -1.0, 1.0, 1.0, 0.5, rin=d_rin, cr=1.0, norms_out=norms)
        assert np.array_equal(norms.cpu().numpy(), plane.max(axis=1))


# ================================================================================================ qp_absmax
def absmax_geometry(n):
    blocks = min(_ceil(n, THREADS), RED_BLOCKS)
    return blocks, _ceil(n, THREADS * blocks)


ABSMAX_SIZES = {1: (1, 1), 255: (1, 1), 256: (1, 1), 257: (2, 1), 262144: (1024, 1), 262145: (1024, 2), 1000003: (1024, 4)}


@pytest.mark.parametrize("n", sorted(ABSMAX_SIZES))
def test_absmax_against_numpy(torch, lib, n):
    """Mixed signs over 100 decades; the maximum at element 0, at element n - 1, negative, -0.0 only (+0.0 comes back), a
    subnormal; a single NaN anywhere gives +inf (also from the second trip, also beside an infinity)."""
    assert absmax_geometry(n) == ABSMAX_SIZES[n]
    blocks, trips = absmax_geometry(n)
    rng = np.random.default_rng(n)
    base = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-50.0, 50.0, size=n)
    ws = torch.empty(RED_BLOCKS, dtype=torch.float64, device="cuda")
    out = torch.empty(1, dtype=torch.float64, device="cuda")

    def run(host):
        out.fill_(-1.0)
        dev = torch.as_tensor(host, device="cuda")
        assert lib.qp_absmax(_p(dev), n, _p(ws), _p(out), _stream(torch)) == 0
        return out.cpu().numpy()[0]

    def planted(index, value, background=None):
        host = base.copy() if background is None else np.full(n, background)
        host[index] = value
        return host

    second_trip = THREADS * blocks if trips > 1 else n - 1       # the first element any thread reads in its second trip
    assert second_trip < n and (trips == 1 or second_trip // (THREADS * blocks) == 1)
    cases = {"random": base, "maximum at 0": planted(0, 1e60), "maximum at n - 1": planted(n - 1, -1e60),
             "negative maximum in the last trip": planted(max(second_trip, n // 2), -3e70),
             "-0.0 only": np.full(n, -0.0), "a subnormal": planted(n - 1, -5e-324 * 7, 0.0),
             "subnormals": planted(n // 2, 2e-310, 5e-324)}
    for name, host in cases.items():
        got, want = run(host), np.max(np.abs(host))
        print(f"absmax n {n} [{name}]: got {got!r}, NumPy {want!r}")
        assert _same_bits(got, want), name
    assert not np.signbit(run(np.full(n, -0.0)))
    nan = float("nan")
    for name, host in {"NaN at 0": planted(0, nan), "NaN at n - 1": planted(n - 1, nan),
                       "NaN in the second trip": planted(second_trip, nan)}.items():
        assert run(host) == np.inf, name
    if n > 1:
        for inf_at, value, nan_at in ((n - 1, -np.inf, 0), (0, np.inf, n - 1), (0, -np.inf, second_trip)):
            host = planted(inf_at, value)
            assert run(host) == np.inf
            if nan_at != inf_at:
                host[nan_at] = nan
                assert np.isnan(host).any() and run(host) == np.inf, "a NaN beside an infinity"


# ================================================================================================ qp_cheb_update, qp_axpy
def grid_for_trips(n):
    return _ceil(n, THREADS * min(max(_ceil(n, THREADS), 1), GRID_FOR_BLOCKS))


PAST_ONE_TRIP = GRID_FOR_BLOCKS * THREADS + 300
assert PAST_ONE_TRIP == 2097152 + 300 and grid_for_trips(PAST_ONE_TRIP) == 2 and grid_for_trips(PAST_ONE_TRIP - 300) == 1
LD = np.longdouble
TWO_ROUNDINGS = LD(2.0) * LD(U) * (LD(1.0) + LD(U))        # (1 + u)^2 - 1 rounded up: a product and a sum, or one fma


def _mixed(rng, n):
    return rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-3.0, 3.0, size=n)


@pytest.mark.parametrize("n", [1, 257, PAST_ONE_TRIP])
def test_cheb_update_and_axpy(torch, lib, n):
    """c2 == 0: d is not read (it holds NaN), d = c1 z bit for bit.  c2 != 0: d within two roundings of the extended-precision
    c1 z + c2 d (the kernel's fma rounds once, after an exact product of c1 z with the rounded c2 d).  v = fl(v + d) of the d
    that was stored, bit for bit.  qp_axpy within two roundings of y + alpha x (the compiler may fuse)."""
    assert grid_for_trips(n) == (2 if n == PAST_ONE_TRIP else 1)
    rng = np.random.default_rng(n + 1)
    z, d0, v0 = _mixed(rng, n), _mixed(rng, n), _mixed(rng, n)
    up = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    c1, c2 = 0.7853981633974483, -0.31830988618379067
    d_z, d_d, d_v = up(z), up(np.full(n, np.nan)), up(v0)
    assert lib.qp_cheb_update(n, c1, _p(d_z), 0.0, _p(d_d), _p(d_v), _stream(torch)) == 0
    d_got, v_got = d_d.cpu().numpy(), d_v.cpu().numpy()
    assert _same_bits(d_got, c1 * z), "c2 == 0: d = c1 z, and the NaN in d was not read"
    assert np.isfinite(v_got).all() and _same_bits(v_got, v0 + d_got)
    d_d, d_v = up(d0), up(v0)
    assert lib.qp_cheb_update(n, c1, _p(d_z), c2, _p(d_d), _p(d_v), _stream(torch)) == 0
    d_got, v_got = d_d.cpu().numpy(), d_v.cpu().numpy()
    exact = LD(c1) * z.astype(LD) + LD(c2) * d0.astype(LD)
    bound = TWO_ROUNDINGS * (np.abs(LD(c1) * z.astype(LD)) + np.abs(LD(c2) * d0.astype(LD)))
    err = np.abs(d_got.astype(LD) - exact)
    print(f"cheb_update n {n}: worst error / bound of d = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)
    assert _same_bits(v_got, v0 + d_got)
    alpha = -2.718281828459045
    d_y = up(v0)
    assert lib.qp_axpy(n, alpha, _p(d_z), _p(d_y), _stream(torch)) == 0
    exact = v0.astype(LD) + LD(alpha) * z.astype(LD)
    bound = TWO_ROUNDINGS * (np.abs(v0.astype(LD)) + np.abs(LD(alpha) * z.astype(LD)))
    err = np.abs(d_y.cpu().numpy().astype(LD) - exact)
    print(f"axpy n {n}: worst error / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)


# ================================================================================================ behind grid_for
def _flags(rng, n):
    """~15 % inactive; the other flag bits at random (only QP_FLAG_ACTIVE may matter); the last cell active."""
    flags = np.where(rng.random(n) < 0.85, ACTIVE, 0).astype(np.uint8) | rng.integers(0, 16, size=n).astype(np.uint8)
    flags[-1] |= ACTIVE
    return flags, (flags & ACTIVE) != 0


def test_add_constant_past_one_trip(torch, lib):
    ncell, nfield, amount = 700001, 4, 1e-3
    assert grid_for_trips(ncell * nfield) == 2
    rng = np.random.default_rng(1)
    flags, active = _flags(rng, ncell)
    host = _mixed(rng, nfield * ncell).reshape(nfield, ncell)
    s, d_flags = torch.as_tensor(host, device="cuda"), torch.as_tensor(flags, device="cuda")
    assert lib.qp_add_constant(_p(d_flags), ncell, nfield, _p(s), amount, _stream(torch)) == 0
    assert _same_bits(s.cpu().numpy(), np.where(active[None, :], host + amount, host)), "one rounding; inactive cells untouched"


def test_add_constant_members_past_one_trip(torch, lib):
    members, ncm, nfield = 3, 233337, 3
    assert grid_for_trips(members * ncm * nfield) == 2
    rng = np.random.default_rng(2)
    flags, active = _flags(rng, members * ncm)
    amounts = np.array([1e-3, 0.37, 1e-17])
    host = _mixed(rng, nfield * members * ncm).reshape(nfield, members * ncm)
    s, d_flags, d_amounts = (torch.as_tensor(a, device="cuda") for a in (host, flags, amounts))
    assert lib.qp_add_constant_members(_p(d_flags), ncm, members, nfield, _p(s), _p(d_amounts), _stream(torch)) == 0
    want = np.where(active[None, :], host + np.repeat(amounts, ncm)[None, :], host)
    assert _same_bits(s.cpu().numpy(), want)


def test_add_scaled_past_one_trip(torch, lib):
    """s + scale g: a product that feeds a sum, two roundings or one (fused)."""
    n, scale = PAST_ONE_TRIP, 0.1
    rng = np.random.default_rng(3)
    host, g = _mixed(rng, n), _mixed(rng, n)
    s, d_g = torch.as_tensor(host, device="cuda"), torch.as_tensor(g, device="cuda")
    assert lib.qp_add_scaled(n, _p(s), _p(d_g), scale, _stream(torch)) == 0
    exact = host.astype(LD) + LD(scale) * g.astype(LD)
    bound = TWO_ROUNDINGS * (np.abs(host.astype(LD)) + np.abs(LD(scale) * g.astype(LD)))
    err = np.abs(s.cpu().numpy().astype(LD) - exact)
    print(f"add_scaled: worst error / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)


def test_nan_pad_past_one_trip(torch, lib):
    ncell, nfield, scale = PAST_ONE_TRIP, 2, 0.3
    assert grid_for_trips(ncell) == 2
    rng = np.random.default_rng(4)
    flags, active = _flags(rng, ncell)
    host = _mixed(rng, nfield * ncell).reshape(nfield, ncell)
    out = torch.zeros((nfield, ncell), dtype=torch.float64, device="cuda")
    d_flags, d_in = torch.as_tensor(flags, device="cuda"), torch.as_tensor(host, device="cuda")
    assert lib.qp_nan_pad(_p(d_flags), ncell, nfield, _p(d_in), scale, _p(out), _stream(torch)) == 0
    got = out.cpu().numpy()
    assert np.isnan(got[:, ~active]).all() and _same_bits(got[:, active], (scale * host)[:, active])


def test_energy_integrate_and_weighted_sum_past_one_trip(torch, lib):
    """energy_integrate: ((s0 + s1) + s2) dE, additions and one product that nothing can fuse: equal to NumPy.  weighted_sum:
    acc = fl(acc + s_i w_i) from 0: term i passes one product rounding and the additions i ... n - 1 (the first addition, to
    0, is exact), fused or not: r_i = 1 + n - max(i, 1) roundings, so the error is at most sum_i ((1 + u)^r_i - 1) |s_i w_i|."""
    ne, ncell, dE = 3, PAST_ONE_TRIP, 0.137
    assert grid_for_trips(ncell) == 2
    rng = np.random.default_rng(5)
    host = _mixed(rng, ne * ncell).reshape(ne, ncell)
    w = np.array([0.3, -1.7, 2.9e-3])
    s = torch.as_tensor(host, device="cuda")
    out = torch.zeros(ncell, dtype=torch.float64, device="cuda")
    assert lib.qp_energy_integrate(_p(s), ne, ncell, dE, _p(out), _stream(torch)) == 0
    assert _same_bits(out.cpu().numpy(), ((host[0] + host[1]) + host[2]) * dE)
    out.zero_()
    d_w = torch.as_tensor(w, device="cuda")
    assert lib.qp_weighted_sum(_p(s), _p(d_w), ne, ncell, _p(out), _stream(torch)) == 0
    terms = host.astype(LD) * w.astype(LD)[:, None]
    growth = np.array([(LD(1.0) + LD(U)) ** (1 + ne - max(i, 1)) - LD(1.0) for i in range(ne)])
    bound = (growth[:, None] * np.abs(terms)).sum(axis=0)
    err = np.abs(out.cpu().numpy().astype(LD) - terms.sum(axis=0))
    print(f"weighted_sum: worst error / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)
