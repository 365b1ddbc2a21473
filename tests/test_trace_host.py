"""Time traces, host side (no GPU): argument checks, the sample schedule, region packing and the sequencing of a traced run.

The sequencing tests run the public functions over the recording fake of ``test_timeloop_trace.py``, extended by the two
engine calls a trace adds (``region_bits``, ``region_sums``).  The fake's region sums are ``math.fsum`` over the cells of a
region, which is exact to the last bit in any order, so "the trace equals the region sums of the frames a run with
``store_every = trace_every`` returns" is a bitwise statement about the state the time loop samples.
"""
from __future__ import annotations

import inspect
import json
import math

import numpy as np
import pytest
import torch

import test_timeloop_trace as TT
from qpsim_amd import engine as ENG
from qpsim_amd import ensemble as ENS
from qpsim_amd import solver as S
from qpsim_amd.geometry import extract_edge_segments
from qpsim_amd.models import BoundaryCondition
from qpsim_amd.timeloop import Schedule


class TraceFake(TT.FakeEngine):
    """``FakeEngine`` plus the two calls of a trace."""

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


def _traced(case, ensemble: bool, **kw):
    """Runs a case of ``test_timeloop_trace`` over ``TraceFake``; ``kw`` overrides its common arguments.  Returns
    (outcome, trace sink: a dict for the lone run of member 0, a list for the ensemble)."""
    common, members = TT._arguments(case)
    tracing = kw.pop("tracing", True)
    common.update(kw)
    sink = ([] if ensemble else {}) if tracing else None
    if ensemble:
        common.update(sweep=case.get("sweep"), errors=case.get("errors", "raise"))
    with TT._fakes(case, ensemble=ensemble) as log:
        S.Engine = ENS.Engine = TraceFake          # restored by _fakes together with the rest

        def call():
            if ensemble:
                return ENS.run_2d_crank_nicolson_ensemble(members, trace_out=sink, **common)
            return S.run_2d_crank_nicolson(trace_out=sink, **dict(common, **members[0]))
        out = TT._outcome(call, log)
        if ensemble:
            out["stats"] = ENS.last_run_stats()
    assert out["error"] is None, out["error"]
    return out, sink


def _small():
    mask = np.ones((3, 4), dtype=bool)
    edges = extract_edge_segments(mask)
    return dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BoundaryCondition("reflective") for e in edges},
                initial_field=np.ones(mask.shape), diffusion_coefficient=1.0, dt=0.1, total_time=0.75, dx=1.0)


# ------------------------------------------------------------------------------------------------ arguments
def test_the_three_parameters_and_their_defaults():
    params = list(inspect.signature(S.run_2d_crank_nicolson).parameters.values())
    names = [p.name for p in params]
    at = names.index("collision_padded_bins")
    assert names[at + 1:at + 4] == ["trace_out", "trace_regions", "trace_every"]
    assert [p.default for p in params[at + 1:at + 4]] == [None, None, 1]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[at + 1:at + 4])
    sink = inspect.signature(ENS.run_2d_crank_nicolson_ensemble).parameters["trace_out"]
    assert sink.default is None and sink.kind is inspect.Parameter.KEYWORD_ONLY
    assert ENS.PER_MEMBER_KEYS == ("initial_field", "energy_weights", "initial_condition_spec", "external_generation",
                                   "bath_temperature", "diffusion_coefficient", "phonon_history_out", "progress_callback")


@pytest.mark.parametrize("kw,match", [
    (dict(trace_out={}, trace_regions={"a": np.ones((3, 3), dtype=bool)}), r"trace_regions\['a'\].*shape"),
    (dict(trace_out={}, trace_regions={f"r{k}": np.ones((3, 4), dtype=bool) for k in range(9)}), "trace_regions.*1 to 8"),
    (dict(trace_out={}, trace_regions={}), "trace_regions.*1 to 8"),
    (dict(trace_out={}, trace_every=0), "trace_every"),
    (dict(trace_every=-2), "trace_every"),
    (dict(trace_regions={"a": np.ones((3, 4), dtype=bool)}), "trace_regions needs trace_out"),
    # 100001 samples x 8 regions x 50 planes x 8 B = 305 MiB
    (dict(trace_out={}, trace_regions={f"r{k}": np.ones((3, 4), dtype=bool) for k in range(8)}, dt=1e-5, total_time=1.0,
          energy_gap=180.0, num_energy_bins=50), "trace_every.*256 MiB.*larger trace_every"),
])
def test_bad_trace_arguments_are_refused_before_a_device_is_needed(kw, match):
    with pytest.raises(ValueError, match=match):
        S.run_2d_crank_nicolson(**dict(_small(), **kw))


def test_the_buffer_limit_counts_members_regions_planes_and_samples():
    plan = S._trace_plan(np.ones((3, 4), dtype=bool), True, None, 1)
    sched = Schedule(1.0, 1e-3, 1)
    assert sched.rows(plan.every) == 1001 and plan.row_shape(50) == (1, 50)
    S._check_sample_buffer(plan, sched, 640, 50)                      # 1001 * 640 * 1 * 50 * 8 B = 244 MiB
    with pytest.raises(ValueError, match="larger trace_every"):
        S._check_sample_buffer(plan, sched, 700, 50)                  # 267 MiB
    S._check_sample_buffer(None, sched, 10 ** 6, 50)                  # off: nothing to check


def test_trace_keys_are_shared_by_all_members():
    common = _small()
    for key, value in (("trace_regions", {"a": np.ones((3, 4), dtype=bool)}), ("trace_every", 2), ("trace_out", {})):
        with pytest.raises(ValueError, match=f"member 1: '{key}' is shared by all members"):
            ENS.member_arguments([{}, {key: value}], common)
    kws = ENS.member_arguments([{}, {}], dict(common, trace_every=4))
    assert [k["trace_every"] for k in kws] == [4, 4] and kws[0]["trace_regions"] is None and kws[0]["trace_out"] is None
    with pytest.raises(ValueError, match="trace_regions needs trace_out"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], trace_regions={"a": np.ones((3, 4), dtype=bool)}, **common)
    with pytest.raises(ValueError, match="trace_every"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], trace_out=[], trace_every=0, **common)


def test_bytes_per_member_include_the_trace_buffer():
    kw = ENS.member_arguments([{}], dict(_small(), energy_gap=180.0, num_energy_bins=8, trace_every=3,
                                         trace_regions={"a": np.ones((3, 4), dtype=bool), "b": np.zeros((3, 4), dtype=bool)}))[0]
    plan = S._trace_plan(kw["mask"], True, kw["trace_regions"], kw["trace_every"])
    assert ENS._bytes_per_member(kw, [plan]) - ENS._bytes_per_member(kw) == 8 * 4 * 2 * 8   # 4 samples, 2 regions, NE 8
    assert ENS._bytes_per_member(kw) == ENS._bytes_per_member(kw, [])
    # the share is the figure the buffer check counts for one member
    assert S._sample_buffer_bytes(plan, Schedule(kw["total_time"], kw["dt"], 1), 1, 8) == 8 * 4 * 2 * 8


# ------------------------------------------------------------------------------------------------ schedule
def test_sample_schedule_with_a_remainder_step():
    sched = Schedule(0.75, 0.1, 100)                       # 7 steps of 0.1 and one of 0.05
    assert sched.total_steps == 8 and sched.rem > 0.0
    assert [k for k in range(1, 9) if sched.due(3, k)] == [3, 6, 8]
    assert sched.rows(3) == 4                              # with t = 0
    assert [k for k in range(1, 9) if sched.stored(k)] == [8]
    assert sched.rows(None) == 0 and not any(sched.due(None, k) for k in range(1, 9))      # no cadence
    assert Schedule(0.8, 0.1, 1).rows(4) == 3 and Schedule(0.8, 0.1, 1).rows(1) == 9


@pytest.mark.parametrize("name", ["full_adi_constant_pair", "scalar_adi", "diffusion_only_one_call"])
def test_sample_times_are_the_times_a_run_storing_there_returns(name):
    case = TT.CASES[name]
    traced, sink = _traced(case, False, store_every=100, trace_every=3)
    stored, _ = _traced(case, False, store_every=3, tracing=False)
    assert sink["times"] == list(stored["raw"][0]) and len(sink["times"]) == 4
    assert list(traced["raw"][0]) == [sink["times"][0], sink["times"][-1]]


# ------------------------------------------------------------------------------------------------ region packing
def _padded_geometry():
    """A 5 x 7 interior with a hole inside a frame padded by 2 rows above, 1 below, 3 columns left and 2 right."""
    mask = np.zeros((8, 12), dtype=bool)
    mask[2:7, 3:10] = True
    mask[4, 5:7] = False
    left = np.zeros_like(mask)
    left[:, :6] = True                                      # reaches into the padding and across the hole
    middle = np.zeros_like(mask)
    middle[3:6, 4:8] = True                                 # overlaps `left`, contains the hole
    return mask, {"left": left, "middle": middle, "all": mask, "padding": ~mask}


def test_region_bits_land_on_the_cropped_grid_and_keep_out_of_holes():
    mask, regions = _padded_geometry()
    grid_mask = mask[2:7, 3:10]
    bits = ENG.pack_region_bits(list(regions.values()), grid_mask, offset=(2, 3))
    assert bits.shape == (5, 7) and bits.dtype == np.uint8
    for r, region in enumerate(regions.values()):
        assert np.array_equal(((bits >> r) & 1).astype(bool), (region & mask)[2:7, 3:10])
    assert not bits[~grid_mask].any() and not (bits >> 4).any()
    assert bits[0, 0] == 0b0101 and bits[1, 1] == 0b0111 and bits[2, 2] == 0     # left+all, left+middle+all, the hole
    plan = S._trace_plan(mask, True, regions, 2)
    assert plan.names == ["left", "middle", "all", "padding"]
    assert plan.cells == [5 * 3 - 1, 3 * 4 - 2, 5 * 7 - 2, 0]
    assert S._trace_plan(mask, True, None, 1).names == ["all"] and S._trace_plan(mask, False, None, 1) is None
    with pytest.raises(ValueError, match="does not cover"):
        ENG.pack_region_bits([np.ones((4, 4), dtype=bool)], grid_mask, offset=(2, 3))
    with pytest.raises(ValueError, match="1 to 8"):
        ENG.pack_region_bits([mask] * 9, mask)


# ------------------------------------------------------------------------------------------------ sequencing
@pytest.mark.parametrize("name", ["full_adi_constant_pair", "padded_mask", "scalar_cn_exact_callback", "members_sweep",
                                  "diffusion_only_one_call"])
def test_without_a_sink_the_recorded_calls_are_issued(name):
    """The engine with the two new methods, the sink left at None: the log is the one recorded before the loops were merged
    (``test_timeloop_trace`` guards the same for its own fake)."""
    recorded = json.loads(TT.TRACE_FILE.read_text())[name]
    case = TT.CASES[name]
    common, members = TT._arguments(case)
    histories = [{} if case.get("history") else None for _ in members]
    with TT._fakes(case, ensemble=False) as log:
        S.Engine = ENS.Engine = TraceFake
        kw = dict(common, **members[0])
        if case.get("callbacks"):
            kw["progress_callback"] = TT._callback(log, 0)

        def call():
            return S.run_2d_crank_nicolson(phonon_history_out=histories[0], trace_out=None, **kw)
        lone = TT._outcome(call, log)
    assert TT._record_of(lone, ensemble=False) == recorded["lone"]
    with TT._fakes(case, ensemble=True) as log:
        S.Engine = ENS.Engine = TraceFake
        for m, over in enumerate(members):
            over["phonon_history_out"] = histories[m]
            if case.get("callbacks"):
                over["progress_callback"] = TT._callback(log, m)
        common.update(sweep=case.get("sweep"), errors=case.get("errors", "raise"))

        def call():      # noqa: F811
            return ENS.run_2d_crank_nicolson_ensemble(members, trace_out=None, **common)
        ens = TT._outcome(call, log)
        ens["stats"] = ENS.last_run_stats()
    assert TT._record_of(ens, ensemble=True) == recorded["ensemble"]


def _steps_of(trace, names) -> list[int]:
    """The steps (1-based; one diffusion step each) at which the calls ``names`` appear in a log."""
    step, found = 0, []
    for call in trace:
        if call[0] == "adi_step":
            step += 1
        elif call[0] in names:
            found.append(step)
    return found


def _region_sums_of_frames(energy_frames, mask, regions):
    """[S, R, NE] from the per-bin frames of the store points, exact (fsum)."""
    return np.array([[[math.fsum(frame[region & mask]) for frame in frames] for region in regions.values()]
                     for frames in energy_frames])


PAIR_CASE = dict(kw=dict(TT.FULL, external_generation=TT.CONSTANT), pair=True, pad=1)


def _pair_case_regions():
    mask = TT._geometry(1)[0]
    left = np.zeros_like(mask)
    left[:, :4] = True
    rows = np.zeros_like(mask)
    rows[2:4, :] = True
    return mask, {"all": mask, "left": left, "rows": rows, "none": np.zeros_like(mask)}


@pytest.mark.parametrize("ensemble", [False, True], ids=["lone", "ensemble"])
def test_a_sampled_step_is_sequenced_like_a_stored_one(ensemble):
    mask, regions = _pair_case_regions()
    pair = ("collide_pair_guarded_members",) if ensemble else ("collide_pair_guarded",)
    traced, sink = _traced(PAIR_CASE, ensemble, store_every=100, trace_every=2, trace_regions=regions)
    stored, _ = _traced(PAIR_CASE, ensemble, store_every=2, tracing=False)
    plain, _ = _traced(PAIR_CASE, ensemble, store_every=100, tracing=False)
    # 8 steps, sampled after 2, 4, 6 and 8: a pair pass closes exactly the steps that are neither sampled nor the last
    assert _steps_of(traced["trace"], pair) == [1, 3, 5, 7] == _steps_of(stored["trace"], pair)
    assert _steps_of(plain["trace"], pair) == [1, 2, 3, 4, 5, 6, 7]
    assert _steps_of(traced["trace"], ("region_sums",)) == [0, 2, 4, 6, 8]
    # a sample enqueues the reduction and nothing else: the downloads are those of t = 0 and the end
    count = lambda out, name: sum(1 for call in out["trace"] if call[0] == name)      # noqa: E731
    assert count(traced, "download_frames_async") == count(plain, "download_frames_async")
    assert count(traced, "region_bits") == 1 and count(traced, "region_sums") == 5
    # the guard is read at a sampled step as at a stored one
    results = ("pauli_stats_members_result",) if ensemble else ("pauli_stats_result",)
    assert [c for c in traced["trace"] if c[0] in results] == [c for c in stored["trace"] if c[0] in results]
    sinks = sink if ensemble else [sink]
    raws = stored["raw"] if ensemble else [stored["raw"]]
    assert len(sinks) == len(raws)
    for got, raw in zip(sinks, raws):
        assert got["times"] == list(raw[0]) and got["regions"] == list(regions)
        assert got["cells"] == [24, 12, 12, 0]
        assert np.array_equal(got["energy_bins"], raw[5])
        want = _region_sums_of_frames(raw[4], mask, regions)
        assert got["density"].shape == (5, 4, 8) and np.array_equal(got["density"], want)
        dE = raw[5][1] - raw[5][0]
        assert got["number"].shape == (5, 4)
        np.testing.assert_allclose(got["number"], dE * want.sum(axis=-1), rtol=1e-14)
        assert np.all(got["density"][:, 3] == 0.0) and np.all(got["density"][:, 0] > 0.0)


def test_a_member_traces_what_its_lone_run_traces():
    mask, regions = _pair_case_regions()
    kw = dict(store_every=100, trace_every=2, trace_regions=regions)
    _, sinks = _traced(PAIR_CASE, True, **kw)
    assert len(sinks) == 3
    common, members = TT._arguments(PAIR_CASE)
    for m, got in enumerate(sinks):
        with TT._fakes(PAIR_CASE, ensemble=False):
            S.Engine = ENS.Engine = TraceFake
            lone: dict = {"stale": 1}
            S.run_2d_crank_nicolson(trace_out=lone, **dict(common, **members[m], **kw))
        assert "stale" not in lone and sorted(lone) == ["cells", "density", "energy_bins", "number", "regions", "times"]
        assert TT._same(got, lone), f"member {m}"
    assert not TT._same(sinks[0]["density"], sinks[1]["density"])


def test_scalar_mode_traces_the_one_plane():
    case = TT.CASES["scalar_adi"]
    mask = TT._geometry(0)[0]
    half = np.zeros_like(mask)
    half[:, 3:] = True
    traced, sink = _traced(case, False, store_every=100, trace_every=2, trace_regions={"all": mask, "half": half})
    stored, _ = _traced(case, False, store_every=2, tracing=False)
    assert sink["energy_bins"] is None and sink["density"].shape == (5, 2, 1) and sink["times"] == list(stored["raw"][0])
    want = np.array([[math.fsum(frame[mask]), math.fsum(frame[half & mask])] for frame in stored["raw"][1]])
    assert np.array_equal(sink["density"][..., 0], want)
    assert np.array_equal(sink["number"], want)            # dx = 1
    # the stretches of diffusion steps end at the sampled steps
    assert [c[2] for c in traced["trace"] if c[0] == "adi_steps"] == [c[2] for c in stored["trace"] if c[0] == "adi_steps"]
    _, sinks = _traced(case, True, store_every=100, trace_every=2, trace_regions={"all": mask, "half": half})
    assert TT._same(sinks[0], sink) and len(sinks) == 3


def test_a_failed_member_gets_no_trace():
    case = dict(TT.CASES["guard_return"])
    out, sinks = _traced(case, True, trace_every=3)
    kinds = ["error" if isinstance(r, Exception) else "ok" for r in out["raw"]]
    assert kinds == ["ok", "error", "ok"]
    assert sinks[1] is None and sinks[0]["regions"] == ["all"] and len(sinks[2]["times"]) == 4


# ------------------------------------------------------------------------------------------------ C ABI
def test_region_sums_entry_points_validate_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    lib = _hip.load()
    for name in ("qp_region_sums", "qp_region_sums_workspace_bytes"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    chunk = 8192                                           # kRegionChunk of csrc/qp_misc.hip
    assert lib.qp_region_sums_workspace_bytes(12, 1024 * 1024, 1, 3) == 8 * 12 * 3 * (1024 * 1024 // chunk)
    assert lib.qp_region_sums_workspace_bytes(1, chunk + 1, 5, 8) == 8 * 5 * 8 * 2
    assert lib.qp_region_sums_workspace_bytes(1, 1, 1, 1) == 8
    for bad in ((0, 64, 1, 1), (1, 0, 1, 1), (1, 64, 0, 1), (1, 64, 1, 0)):
        assert lib.qp_region_sums_workspace_bytes(*bad) == 0
    ok = [8, 8, 1, 64, 1, 1, 8, 8, 0]          # state, bits, nfield, ncell_member, members, nregion, workspace, out, stream
    for at, value in ((0, 0), (1, 0), (6, 0), (7, 0), (2, 0), (3, 0), (4, 0), (3, -5), (5, 0), (5, 9), (5, -1)):
        args = list(ok)
        args[at] = value
        assert lib.qp_region_sums(*args) == -1, (at, value)
        assert b"qp_region_sums" in lib.qp_last_error()
