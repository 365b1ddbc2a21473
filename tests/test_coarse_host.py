"""Coarse frames, host side (no GPU): the block layout, argument checks, the two sample cadences and the sequencing of a run
with coarse frames.

The sequencing tests run the public functions over the recording fake of ``test_timeloop_trace.py``, extended in THIS file
by the engine calls of a trace (``region_bits``, ``region_sums``) and of the coarse frames (``block_sums``).  The fake's
block sums are ``math.fsum`` over the active cells of a block, exact in any order, so "the coarse frames are the block sums
of the frames a run with ``store_every = coarse_every`` returns" is a bitwise statement about the state the loop samples.
"""
from __future__ import annotations

import inspect
import json
import math

import numpy as np
import pytest
import torch

import test_timeloop_trace as TT
from golden_utils import GoldenRun
from qpsim_amd import engine as ENG
from qpsim_amd import ensemble as ENS
from qpsim_amd import solver as S
from qpsim_amd.geometry import extract_edge_segments
from qpsim_amd.models import BoundaryCondition
from qpsim_amd.timeloop import Schedule

SAMPLING = ("region_bits", "region_sums", "block_sums")      # the calls only a sampler issues


class CoarseFake(TT.FakeEngine):
    """``FakeEngine`` plus the calls of a trace and of the coarse frames."""

    def region_bits(self, regions, offset=(0, 0)):
        self.log.append(["region_bits", len(regions), [int(v) for v in offset]])
        return torch.as_tensor(ENG.pack_region_bits(regions, self.geom.mask, offset).reshape(-1))

    def region_sums(self, state, bits, members, out_row):
        nregion, nfield = int(out_row.shape[-2]), int(out_row.shape[-1])
        self.log.append(["region_sums", int(members), nregion, nfield])
        planes = state.reshape(nfield, members, self.ncell).numpy()
        for r in range(nregion):
            inside = ((bits.numpy() >> r) & 1).astype(bool)
            for m in range(members):
                for f in range(nfield):
                    out_row[m, r, f] = math.fsum(planes[f, m][inside])

    def block_sums(self, state, members, bin, oy, ox, out_row):
        nfield, cny, cnx = (int(v) for v in out_row.shape[1:])
        self.log.append(["block_sums", int(members), int(bin), int(oy), int(ox), nfield, cny, cnx])
        planes = state.reshape(nfield, members, self.ny, self.nx).numpy()
        for m in range(members):
            for f in range(nfield):
                out_row[m, f] = torch.as_tensor(_naive_block_sums(planes[f, m], self.geom.mask, bin, oy, ox))


def _naive_block_sums(plane, mask, b, oy, ox):
    """[cny, cnx] exact sums of ``plane`` over the in-mask cells of every block, device cell (0, 0) at (oy, ox) of its block."""
    ny, nx = mask.shape
    sums = [[[] for _ in range(-(-(ox + nx) // b))] for _ in range(-(-(oy + ny) // b))]
    for j in range(ny):
        for i in range(nx):
            if mask[j, i]:
                sums[(oy + j) // b][(ox + i) // b].append(plane[j, i])
    return np.array([[math.fsum(cell) for cell in row] for row in sums])


def _naive_layout(mask, b):
    """``coarse_layout`` by a double loop over the cells of the full frame."""
    H, W = mask.shape
    cells = np.zeros((-(-H // b), -(-W // b)), dtype=int)
    rows, cols = [], []
    for r in range(H):
        for c in range(W):
            if mask[r, c]:
                cells[r // b, c // b] += 1
                rows.append(r)
                cols.append(c)
    r0, r1, c0, c1 = min(rows), max(rows), min(cols), max(cols)
    oy, ox = r0 % b, c0 % b
    window = (r0 // b, c0 // b, (oy + r1 - r0 + 1 + b - 1) // b, (ox + c1 - c0 + 1 + b - 1) // b)
    return cells.shape, cells, (r0, c0), (oy, ox), window


def _layout_masks():
    full = np.ones((16, 24), dtype=bool)
    inset = np.zeros((37, 150), dtype=bool)
    inset[3:34, 5:141] = True
    golden = GoldenRun("masked_holes_mixed_bc_9x11").kwargs["mask"]
    holed = np.ones((40, 48), dtype=bool)
    holed[16:32, 16:32] = False
    return {"full": full, "inset": inset, "golden": golden, "holed": holed}


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("name,b", [("full", 8), ("inset", 2), ("inset", 8), ("inset", 64), ("golden", 2), ("golden", 4),
                                    ("holed", 16), ("holed", 4)])
def test_coarse_layout_against_a_double_loop(name, b):
    mask = _layout_masks()[name]
    lay = ENG.coarse_layout(mask, b)
    shape, cells, origin, offset, window = _naive_layout(mask, b)
    assert lay.bin == b and lay.shape == shape and lay.origin == origin and lay.offset == offset and lay.window == window
    assert lay.cells.shape == shape and np.array_equal(lay.cells, cells) and lay.cells.dtype.kind == "i"
    assert lay.cells.sum() == mask.sum()
    wy, wx, cny, cnx = lay.window
    outside = np.ones(shape, dtype=bool)
    outside[wy:wy + cny, wx:wx + cnx] = False
    assert not lay.cells[outside].any(), "every in-mask cell lies in the window of the device output"
    if name == "full":
        assert np.all(lay.cells == 64) and lay.offset == (0, 0) and lay.window == (0, 0, 2, 3)
    if name == "inset":
        assert lay.origin == (3, 5) and lay.offset == (3 % b, 5 % b)
    if name == "golden":
        assert np.any((lay.cells > 0) & (lay.cells < b * b)), "a block that the mask fills only partly"
    if name == "holed":
        assert np.any(lay.cells == 0), "a block inside the hole"
        if b == 16:
            assert lay.cells[1, 1] == 0 and lay.cells[0, 0] == 256 and lay.cells[2, 2] == 8 * 16


def test_coarse_layout_needs_an_interior():
    with pytest.raises(ValueError, match="interior"):
        ENG.coarse_layout(np.zeros((4, 4), dtype=bool), 2)


# ------------------------------------------------------------------------------------------------ arguments
def _small():
    mask = np.ones((3, 4), dtype=bool)
    edges = extract_edge_segments(mask)
    return dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BoundaryCondition("reflective") for e in edges},
                initial_field=np.ones(mask.shape), diffusion_coefficient=1.0, dt=0.1, total_time=0.75, dx=1.0)


def _large(n=2048):
    mask = np.ones((n, n), dtype=bool)
    edges = extract_edge_segments(mask)
    return dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BoundaryCondition("reflective") for e in edges},
                initial_field=np.ones(mask.shape), diffusion_coefficient=1.0, dt=0.1, total_time=1.0, dx=1.0)


def test_the_three_parameters_and_their_defaults():
    params = list(inspect.signature(S.run_2d_crank_nicolson).parameters.values())
    names = [p.name for p in params]
    at = names.index("trace_every")
    assert names[at + 1:at + 4] == ["coarse_out", "coarse_bin", "coarse_every"]
    assert [p.default for p in params[at + 1:at + 4]] == [None, 8, 1]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[at + 1:at + 4])
    sink = inspect.signature(ENS.run_2d_crank_nicolson_ensemble).parameters["coarse_out"]
    assert sink.default is None and sink.kind is inspect.Parameter.KEYWORD_ONLY
    assert "coarse_bin" not in ENS.PER_MEMBER_KEYS and "coarse_every" not in ENS.PER_MEMBER_KEYS


@pytest.mark.parametrize("kw,match", [
    (dict(coarse_out={}, coarse_bin=3), "coarse_bin must be one of 2, 4, 8, 16, 32, 64"),
    (dict(coarse_out={}, coarse_bin=128), "coarse_bin must be one of"),
    (dict(coarse_out={}, coarse_bin=8.0), "coarse_bin must be one of"),
    (dict(coarse_bin=0), "coarse_bin must be one of"),
    (dict(coarse_out={}, coarse_every=0), "coarse_every must be an integer >= 1"),
    (dict(coarse_out={}, coarse_every=2.5), "coarse_every must be an integer >= 1"),
    (dict(coarse_every=-1), "coarse_every must be an integer >= 1"),
    (dict(coarse_bin=4), "coarse_bin needs coarse_out"),
    (dict(coarse_every=3), "coarse_every needs coarse_out"),
])
def test_bad_coarse_arguments_are_refused_before_a_device_is_needed(kw, match):
    with pytest.raises(ValueError, match=match):
        S.run_2d_crank_nicolson(**dict(_small(), **kw))


def test_a_buffer_above_the_limit_is_refused_before_a_device_is_needed():
    # 11 samples x 12 planes x 1024 x 1024 blocks x 8 B = 1056 MiB
    with pytest.raises(ValueError, match="coarse_every=1, coarse_bin=2.*256 MiB.*larger coarse_every or coarse_bin"):
        S.run_2d_crank_nicolson(**_large(), coarse_out={}, coarse_bin=2, energy_gap=180.0, num_energy_bins=12)


def test_the_buffer_limit_counts_samples_members_planes_and_blocks():
    mask = np.ones((1024, 1024), dtype=bool)
    plan = S._coarse_plan(mask, True, 8, 1)                            # 128 x 128 blocks
    sched = Schedule(1.0, 1e-2, 1)
    assert sched.rows(plan.every) == 101 and plan.row_shape(20) == (20, 128, 128)
    S._check_sample_buffer(plan, sched, 1, 20)                         # 101 * 20 * 16384 * 8 B = 252.5 MiB
    with pytest.raises(ValueError, match="larger coarse_every or coarse_bin"):
        S._check_sample_buffer(plan, sched, 1, 21)                     # 265 MiB
    with pytest.raises(ValueError, match="2 members"):
        S._check_sample_buffer(plan, sched, 2, 11)
    S._check_sample_buffer(None, Schedule(1.0, 1e-3, 1), 10 ** 6, 50)  # off: nothing to check
    assert S._coarse_plan(mask, False, 8, 1) is None


def test_coarse_keys_are_shared_by_all_members():
    common = _small()
    for key, value in (("coarse_bin", 4), ("coarse_every", 2), ("coarse_out", {})):
        with pytest.raises(ValueError, match=f"member 1: '{key}' is shared by all members"):
            ENS.member_arguments([{}, {key: value}], common)
    kws = ENS.member_arguments([{}, {}], dict(common, coarse_every=4))
    assert [k["coarse_every"] for k in kws] == [4, 4] and kws[0]["coarse_bin"] == 8 and kws[0]["coarse_out"] is None
    with pytest.raises(ValueError, match="coarse_bin needs coarse_out"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], coarse_bin=16, **common)
    with pytest.raises(ValueError, match="coarse_every must be"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], coarse_out=[], coarse_every=0, **common)
    with pytest.raises(ValueError, match="coarse_bin must be one of"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], coarse_out=[], coarse_bin=5, **common)


def test_bytes_per_member_include_the_coarse_buffer():
    kw = ENS.member_arguments([{}], dict(_small(), energy_gap=180.0, num_energy_bins=8, coarse_every=3, coarse_bin=2))[0]
    # 4 samples, NE 8, 2 x 2 blocks on the 3 x 4 grid
    plan = S._coarse_plan(kw["mask"], True, kw["coarse_bin"], kw["coarse_every"])
    assert ENS._bytes_per_member(kw, [plan]) - ENS._bytes_per_member(kw) == 8 * 4 * 8 * 2 * 2
    assert ENS._bytes_per_member(kw) == ENS._bytes_per_member(kw, [])
    # the share is the figure the buffer check counts for one member, and both kinds add up
    assert S._sample_buffer_bytes(plan, Schedule(kw["total_time"], kw["dt"], 1), 1, 8) == 8 * 4 * 8 * 2 * 2
    trace = S._trace_plan(kw["mask"], True, None, 3)
    assert ENS._bytes_per_member(kw, [trace, plan]) - ENS._bytes_per_member(kw) == 8 * 4 * 8 * (1 + 2 * 2)


# ------------------------------------------------------------------------------------------------ schedule
def test_the_two_cadences_of_a_schedule():
    steps = range(1, 24)
    sched = Schedule(2.25, 0.1, 100)                            # 22 steps of 0.1 and one of 0.05
    assert sched.total_steps == 23 and sched.rem > 0.0
    assert [k for k in steps if sched.due(5, k)] == [5, 10, 15, 20, 23] and sched.rows(5) == 6
    assert [k for k in steps if sched.due(4, k)] == [4, 8, 12, 16, 20, 23] and sched.rows(4) == 7
    assert [k for k in steps if sched.stored(k)] == [23]
    # a cadence that is off has no row and no step, whatever the other one is
    assert sched.rows(None) == 0 and not any(sched.due(None, k) for k in steps)
    off = Schedule(2.25, 0.1, 3)
    assert off.rows(None) == 0 and not any(off.due(None, k) for k in steps)
    # the last step is sampled once when the cadence divides the step count
    assert Schedule(0.8, 0.1, 1).rows(4) == 3 and Schedule(0.8, 0.1, 1).rows(1) == 9


# ------------------------------------------------------------------------------------------------ sequencing
def _run(case, ensemble: bool, *, trace=False, coarse=False, **kw):
    """Runs a case of ``test_timeloop_trace`` over ``CoarseFake``; ``kw`` overrides its common arguments.  Returns (outcome,
    trace sink, coarse sink): dicts for the lone run of member 0, lists for the ensemble, None for a sink not asked for."""
    common, members = TT._arguments(case)
    common.update(kw)
    tsink = ([] if ensemble else {}) if trace else None
    csink = ([] if ensemble else {}) if coarse else None
    if ensemble:
        common.update(sweep=case.get("sweep"), errors=case.get("errors", "raise"))
    with TT._fakes(case, ensemble=ensemble) as log:
        S.Engine = ENS.Engine = CoarseFake          # restored by _fakes together with the rest

        def call():
            if ensemble:
                return ENS.run_2d_crank_nicolson_ensemble(members, trace_out=tsink, coarse_out=csink, **common)
            return S.run_2d_crank_nicolson(trace_out=tsink, coarse_out=csink, **dict(common, **members[0]))
        out = TT._outcome(call, log)
        if ensemble:
            out["stats"] = ENS.last_run_stats()
    assert out["error"] is None, out["error"]
    return out, tsink, csink


def _without_sampling(trace):
    return [call for call in trace if call[0] not in SAMPLING]


@pytest.mark.parametrize("ensemble", [False, True], ids=["lone", "ensemble"])
@pytest.mark.parametrize("name", ["full_adi_constant_pair", "scalar_adi", "diffusion_only_one_call", "padded_mask"])
def test_a_coarse_sampler_sequences_a_run_as_a_tracer_of_the_same_cadence_does(name, ensemble):
    """``energy_loop`` (coupled, batched diffusion) and ``scalar_loop``: the same calls in the same order but for the sampling
    call itself, which stands at the same places."""
    case = TT.CASES[name]
    coarse, _, csink = _run(case, ensemble, coarse=True, store_every=100, coarse_every=2, coarse_bin=2)
    traced, tsink, _ = _run(case, ensemble, trace=True, store_every=100, trace_every=2)
    assert _without_sampling(coarse["trace"]) == _without_sampling(traced["trace"])
    place = lambda out, name: [k for k, call in enumerate(_without_sampling_index(out["trace"])) if call == name]   # noqa: E731
    assert place(coarse, "block_sums") == place(traced, "region_sums") and len(place(coarse, "block_sums")) == 5
    assert not any(call[0] in ("region_bits", "region_sums") for call in coarse["trace"])
    assert not any(call[0] == "block_sums" for call in traced["trace"])
    first = csink[0] if ensemble else csink
    assert first["times"] == (tsink[0] if ensemble else tsink)["times"]


def _without_sampling_index(trace):
    """The log with ``region_bits`` dropped, so that the places of the sampling calls of two logs can be compared."""
    return [call[0] for call in trace if call[0] != "region_bits"]


@pytest.mark.parametrize("name", ["full_adi_constant_pair", "padded_mask", "scalar_cn_exact_callback", "members_sweep",
                                  "diffusion_only_one_call"])
def test_without_a_sink_the_recorded_calls_are_issued(name):
    """The engine with the new methods, both sinks left at None: the log is the one recorded before the loops were merged."""
    recorded = json.loads(TT.TRACE_FILE.read_text())[name]
    case = TT.CASES[name]
    common, members = TT._arguments(case)
    histories = [{} if case.get("history") else None for _ in members]
    with TT._fakes(case, ensemble=False) as log:
        S.Engine = ENS.Engine = CoarseFake
        kw = dict(common, **members[0])
        if case.get("callbacks"):
            kw["progress_callback"] = TT._callback(log, 0)

        def call():
            return S.run_2d_crank_nicolson(phonon_history_out=histories[0], trace_out=None, coarse_out=None, **kw)
        lone = TT._outcome(call, log)
    assert TT._record_of(lone, ensemble=False) == recorded["lone"]
    with TT._fakes(case, ensemble=True) as log:
        S.Engine = ENS.Engine = CoarseFake
        for m, over in enumerate(members):
            over["phonon_history_out"] = histories[m]
            if case.get("callbacks"):
                over["progress_callback"] = TT._callback(log, m)
        common.update(sweep=case.get("sweep"), errors=case.get("errors", "raise"))

        def call():      # noqa: F811
            return ENS.run_2d_crank_nicolson_ensemble(members, trace_out=None, coarse_out=None, **common)
        ens = TT._outcome(call, log)
        ens["stats"] = ENS.last_run_stats()
    assert TT._record_of(ens, ensemble=True) == recorded["ensemble"]


PAIR_CASE = dict(kw=dict(TT.FULL, external_generation=TT.CONSTANT), pair=True, pad=1)


def _steps_of(trace, names) -> list[int]:
    """The steps (1-based; one diffusion step each) at which the calls ``names`` appear in a log."""
    step, found = 0, []
    for call in trace:
        if call[0] == "adi_step":
            step += 1
        elif call[0] in names:
            found.append(step)
    return found


@pytest.mark.parametrize("ensemble", [False, True], ids=["lone", "ensemble"])
def test_a_coarse_step_is_sequenced_like_a_stored_one_and_sums_the_state_stored_there(ensemble):
    mask = TT._geometry(1)[0]
    pair = ("collide_pair_guarded_members",) if ensemble else ("collide_pair_guarded",)
    coarse, _, sink = _run(PAIR_CASE, ensemble, coarse=True, store_every=100, coarse_every=2, coarse_bin=2)
    stored, _, _ = _run(PAIR_CASE, ensemble, store_every=2)
    plain, _, _ = _run(PAIR_CASE, ensemble, store_every=100)
    assert _steps_of(coarse["trace"], pair) == [1, 3, 5, 7] == _steps_of(stored["trace"], pair)
    assert _steps_of(plain["trace"], pair) == [1, 2, 3, 4, 5, 6, 7]
    assert _steps_of(coarse["trace"], ("block_sums",)) == [0, 2, 4, 6, 8]
    count = lambda out, name: sum(1 for call in out["trace"] if call[0] == name)      # noqa: E731
    assert count(coarse, "download_frames_async") == count(plain, "download_frames_async")
    results = ("pauli_stats_members_result",) if ensemble else ("pauli_stats_result",)
    assert [c for c in coarse["trace"] if c[0] in results] == [c for c in stored["trace"] if c[0] in results]
    lay = ENG.coarse_layout(mask, 2)
    assert lay.origin != (0, 0), "the case is a padded frame: the device grid is cropped"
    call = next(c for c in coarse["trace"] if c[0] == "block_sums")
    assert call[1:] == [3 if ensemble else 1, 2, lay.offset[0], lay.offset[1], 8, lay.window[2], lay.window[3]]
    sinks = sink if ensemble else [sink]
    raws = stored["raw"] if ensemble else [stored["raw"]]
    assert len(sinks) == len(raws)
    for got, raw in zip(sinks, raws):
        assert sorted(got) == ["bin", "cells", "energy_bins", "energy_frames", "energy_sums", "frames", "times"]
        assert got["times"] == list(raw[0]) and got["bin"] == 2 and np.array_equal(got["cells"], lay.cells)
        assert np.array_equal(got["energy_bins"], raw[5])
        want = np.array([[_naive_block_sums(np.nan_to_num(frame), mask, 2, 0, 0) for frame in frames] for frames in raw[4]])
        assert got["energy_sums"].shape == (5, 8) + lay.shape and np.array_equal(got["energy_sums"], want)
        empty = lay.cells == 0
        assert np.any(lay.cells < 4) and np.all(got["energy_sums"][:, :, empty] == 0.0)
        assert np.isnan(got["energy_frames"][:, :, empty]).all() and np.isnan(got["frames"][:, empty]).all()
        assert np.array_equal(got["energy_frames"][:, :, ~empty], (want / lay.cells)[:, :, ~empty])
        dE = raw[5][1] - raw[5][0]
        np.testing.assert_allclose(got["frames"][:, ~empty], (dE * want.sum(axis=1) / lay.cells)[:, ~empty], rtol=1e-14)


def test_the_result_embeds_the_window_and_marks_blocks_without_cells():
    """``_CoarsePlan.result`` on a 40 x 48 frame whose mask starts at (5, 9) and has a 16 x 16 hole, b = 8: the device sums land
    in their window of the full coarse frame with their bits, 0.0 around it, NaN means exactly where ``cells == 0``."""
    mask = np.zeros((40, 48), dtype=bool)
    mask[5:38, 9:47] = True
    mask[16:32, 16:32] = False
    plan = S._coarse_plan(mask, True, 8, 1)
    lay = plan.layout
    assert lay.shape == (5, 6) and lay.window == (0, 1, 5, 5) and lay.offset == (5, 1)
    rng = np.random.default_rng(2)
    sums = rng.random((3, 4, 5, 5)) * (lay.cells[:, 1:] > 0)
    E_bins, dE = np.linspace(180.0, 540.0, 4), 120.0
    got = plan.result([0.0, 0.1, 0.2], sums, E_bins, 1.0, dE)
    assert got["energy_sums"].shape == (3, 4, 5, 6) and got["energy_sums"][..., 1:].tobytes() == sums.tobytes()
    assert np.all(got["energy_sums"][..., 0] == 0.0) and not np.signbit(got["energy_sums"]).any()
    empty = lay.cells == 0
    assert empty[2, 2] and empty[:, 0].all() and empty.sum() == 5 + 4
    assert np.array_equal(np.isnan(got["energy_frames"]), np.broadcast_to(empty, (3, 4, 5, 6)))
    assert np.array_equal(np.isnan(got["frames"]), np.broadcast_to(empty, (3, 5, 6)))
    with np.errstate(invalid="ignore"):                      # 0 / 0 in the blocks that are left out below
        assert np.array_equal(got["energy_frames"][..., ~empty], (got["energy_sums"] / lay.cells)[..., ~empty])
        np.testing.assert_allclose(got["frames"][:, ~empty], (dE * got["energy_sums"].sum(axis=1) / lay.cells)[:, ~empty],
                                   rtol=1e-15)
        scalar = plan.result([0.0], sums[:1, :1], None, 1.0, None)
        assert scalar["energy_bins"] is None
        assert np.array_equal(scalar["frames"], scalar["energy_frames"][:, 0], equal_nan=True)
        assert np.array_equal(scalar["frames"][:, ~empty], (scalar["energy_sums"][:, 0] / lay.cells)[:, ~empty])


def test_trace_and_coarse_frames_sample_at_their_own_steps():
    out, tsink, csink = _run(PAIR_CASE, False, trace=True, coarse=True, store_every=100, trace_every=3, coarse_every=2,
                             coarse_bin=4)
    assert _steps_of(out["trace"], ("region_sums",)) == [0, 3, 6, 8]
    assert _steps_of(out["trace"], ("block_sums",)) == [0, 2, 4, 6, 8]
    pair = _steps_of(out["trace"], ("collide_pair_guarded",))
    assert pair == [1, 5, 7], "a pair pass closes the steps that neither cadence samples"
    assert len(tsink["times"]) == 4 and len(csink["times"]) == 5 and tsink["times"][-1] == csink["times"][-1]
    # both saw the same state at step 6: the sum over all blocks is the sum over the region "all" (exact in the fake)
    total = np.array([math.fsum(plane.reshape(-1)) for plane in csink["energy_sums"][3]])
    np.testing.assert_allclose(total, tsink["density"][2, 0], rtol=1e-15)


def test_a_member_gets_the_coarse_frames_of_its_lone_run():
    kw = dict(store_every=100, coarse_every=2, coarse_bin=2)
    _, _, sinks = _run(PAIR_CASE, True, coarse=True, **kw)
    assert len(sinks) == 3
    common, members = TT._arguments(PAIR_CASE)
    for m, got in enumerate(sinks):
        with TT._fakes(PAIR_CASE, ensemble=False):
            S.Engine = ENS.Engine = CoarseFake
            lone: dict = {"stale": 1}
            S.run_2d_crank_nicolson(coarse_out=lone, **dict(common, **members[m], **kw))
        assert "stale" not in lone and TT._same(got, lone), f"member {m}"
    assert not TT._same(sinks[0]["energy_sums"], sinks[1]["energy_sums"])


def test_scalar_mode_sums_the_one_plane():
    case = TT.CASES["scalar_adi"]
    mask = TT._geometry(0)[0]
    coarse, _, sink = _run(case, False, coarse=True, store_every=100, coarse_every=2, coarse_bin=2)
    stored, _, _ = _run(case, False, store_every=2)
    lay = ENG.coarse_layout(mask, 2)
    assert sink["energy_bins"] is None and sink["energy_sums"].shape == (5, 1) + lay.shape
    assert sink["times"] == list(stored["raw"][0])
    want = np.array([_naive_block_sums(np.nan_to_num(frame), mask, 2, 0, 0) for frame in stored["raw"][1]])
    assert np.array_equal(sink["energy_sums"][:, 0], want)
    assert np.array_equal(sink["frames"], want / lay.cells) and np.array_equal(sink["energy_frames"][:, 0], sink["frames"])
    assert [c[2] for c in coarse["trace"] if c[0] == "adi_steps"] == [c[2] for c in stored["trace"] if c[0] == "adi_steps"]
    _, _, sinks = _run(case, True, coarse=True, store_every=100, coarse_every=2, coarse_bin=2)
    assert TT._same(sinks[0], sink) and len(sinks) == 3


def test_a_failed_member_gets_no_coarse_frames():
    case = dict(TT.CASES["guard_return"])
    out, _, sinks = _run(case, True, coarse=True, coarse_every=3)
    kinds = ["error" if isinstance(r, Exception) else "ok" for r in out["raw"]]
    assert kinds == ["ok", "error", "ok"]
    assert sinks[1] is None and sinks[0]["bin"] == 8 and len(sinks[2]["times"]) == 4


# ------------------------------------------------------------------------------------------------ C ABI
def test_block_sums_entry_point_validates_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    lib = _hip.load()
    assert hasattr(lib, "qp_block_sums") and "qp_block_sums" in _hip.SIGNATURES
    ok = [8, 8, 1, 8, 8, 1, 8, 0, 0, 8, 0]       # state, flags, nfield, ny, nx, members, bin, oy, ox, out, stream
    bad = [(6, 3), (8, 8), (9, 0),               # the three of the issue: bin = 3, ox = bin, a null out
           (0, 0), (1, 0), (2, 0), (3, 0), (4, -1), (5, 0), (6, 0), (6, 128), (6, 1), (7, 8), (7, -1), (8, -1)]
    for at, value in bad:
        args = list(ok)
        args[at] = value
        assert lib.qp_block_sums(*args) == -1, (at, value)
        assert b"qp_block_sums" in lib.qp_last_error()
