"""Any number of samplers, host side (no GPU): the time loops know cadences, not kinds.

Three ``Sampler`` s of cadences 3, 5 and 2 (in that order, so the order of the tuple is not the order of the cadences) whose
``reduce`` only logs run over the recording fake of ``test_timeloop_trace.py``.  They reach the loops as the time traces and
the coarse frames do - through plans handed out by ``solver._sampling_plans`` - so the runs go through the public functions
with their real setup and delivery; only the plans are stand-ins.

13 steps (12 of 0.1 and one of 0.05), stored every 7th: a step *halts* when it is stored (7, 13) or due for a sampler.
"""
from __future__ import annotations

import pytest

import test_timeloop_trace as TT
from qpsim_amd import ensemble as ENS
from qpsim_amd import solver as S
from qpsim_amd.timeloop import Sampler

EVERY = (3, 5, 2)
STEPS, STORE_EVERY = 13, 7
STORED = [7, 13]
DUE = {every: [k for k in range(1, STEPS + 1) if k % every == 0 or k == STEPS] for every in EVERY}
HALTING = sorted(set(STORED).union(*DUE.values()))


class LogPlan:
    """The plan interface of ``solver.py`` for a sampler that writes its cadence into the engine log and nothing else."""

    def __init__(self, every):
        self.every = every

    def row_shape(self, nfield):
        return (nfield,)

    def sampler(self, eng, mask, sched, members, nfield):
        return Sampler(eng, sched, self.every, members, self.row_shape(nfield),
                       lambda state, row: eng.log.append(["sample", self.every, list(row.shape)]))

    def result(self, times, rows, E_bins, dx, dE):
        return {"times": list(times), "rows": rows.shape}


def _run(monkeypatch, name, ensemble):
    """Runs a case of ``test_timeloop_trace`` with the three logging samplers; returns (engine log, their sinks)."""
    case = TT.CASES[name]
    common, members = TT._arguments(case)
    common.update(total_time=1.25, store_every=STORE_EVERY)
    sinks = [[] if ensemble else {} for _ in EVERY]
    monkeypatch.setattr(S, "_sampling_plans", lambda *args: [(LogPlan(every), sink) for every, sink in zip(EVERY, sinks)])
    if ensemble:
        common.update(sweep=case.get("sweep"), errors=case.get("errors", "raise"))
    with TT._fakes(case, ensemble=ensemble) as log:
        def call():
            if ensemble:
                return ENS.run_2d_crank_nicolson_ensemble(members, **common)
            return S.run_2d_crank_nicolson(**dict(common, **members[0]))
        out = TT._outcome(call, log)
    assert out["error"] is None, out["error"]
    assert len(out["raw"][0][0] if ensemble else out["raw"][0]) == 1 + len(STORED)
    return out["trace"], sinks


def _walk(trace):
    """(samples as (step, cadence) in log order, the step count after every diffusion call, log index at which step k
    begins, log index at which the guard of step k is read)."""
    step, samples, ends, begins, read_at = 0, [], [], {}, {}
    for at, call in enumerate(trace):
        if call[0] in ("adi_step", "adi_steps"):
            begins[step + 1] = at
            step += call[2] if call[0] == "adi_steps" else 1
            ends.append(step)
        elif call[0] == "sample":
            samples.append((step, call[1]))
        elif call[0] in ("pauli_stats_result", "pauli_stats_members_result"):
            read_at[call[1]] = at
    assert step == STEPS
    return samples, ends, begins, read_at


def _check_samples(samples, sinks, members, nfield, trace):
    for every, sink in zip(EVERY, sinks):
        # t = 0, its own steps and the last step, nothing else
        assert [step for step, e in samples if e == every] == [0] + DUE[every]
        for got in (sink if members > 1 else [sink]):
            assert len(got["times"]) == 1 + len(DUE[every]) and got["rows"] == (1 + len(DUE[every]), nfield)
            assert got["times"][0] == 0.0 and got["times"][-1] == pytest.approx(1.25)
    # samplers due at the same step are called in the order of the tuple
    for step in [0] + HALTING:
        assert [e for s, e in samples if s == step] == [e for e in EVERY if step == 0 or step in DUE[e]]
    assert all(call[2] == [members, nfield] for call in trace if call[0] == "sample")


@pytest.mark.parametrize("ensemble", [False, True], ids=["lone", "ensemble"])
def test_three_samplers_in_a_coupled_run_with_pair_passes(monkeypatch, ensemble):
    trace, sinks = _run(monkeypatch, "full_adi_constant_pair", ensemble)
    samples, ends, begins, read_at = _walk(trace)
    assert HALTING == [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13] and ends == list(range(1, STEPS + 1))
    _check_samples(samples, sinks, 3 if ensemble else 1, 8, trace)
    # no pair pass across a halting step: it closes exactly the steps that neither halt nor are the last
    pair = "collide_pair_guarded_members" if ensemble else "collide_pair_guarded"
    paired = [k for k in range(1, STEPS + 1)
              if any(call[0] == pair for call in trace[begins[k]:begins.get(k + 1, len(trace))])]
    assert paired == [k for k in range(1, STEPS) if k not in HALTING] == [1, 11]
    # the guard of a halting step is read before the next step begins, that of any other step stays in flight
    for k in range(1, STEPS):
        assert (read_at[k] < begins[k + 1]) == (k in HALTING), k
    assert sorted(read_at) == list(range(STEPS + 1))
    # a sample downloads nothing: the downloads are those of the three store points
    per_store = sum(1 for call in trace[:begins[1]] if call[0] == "download_frames_async")
    assert sum(1 for call in trace if call[0] == "download_frames_async") == per_store * (1 + len(STORED))


@pytest.mark.parametrize("ensemble", [False, True], ids=["lone", "ensemble"])
@pytest.mark.parametrize("name", ["scalar_adi", "diffusion_only_one_call"])
def test_three_samplers_end_the_stretches_of_diffusion_steps(monkeypatch, name, ensemble):
    """``scalar_loop`` and the batched-diffusion branch of ``energy_loop``: one diffusion call per stretch, and a stretch
    ends exactly at the steps that halt."""
    trace, sinks = _run(monkeypatch, name, ensemble)
    samples, ends, _, _ = _walk(trace)
    assert ends == HALTING
    _check_samples(samples, sinks, 3 if ensemble else 1, 1 if name == "scalar_adi" else 8, trace)
