"""Host side of the ensemble API (no GPU): per-member / shared key rules, per-step generation amounts, batch splitting,
shard assignment, and the library's new C symbols."""
from __future__ import annotations

import numpy as np
import pytest

from qpsim_amd.distributed import shard_members
from qpsim_amd.ensemble import PER_MEMBER_KEYS, generation_amounts, member_arguments, plan_batches
from qpsim_amd.models import ExternalGenerationSpec


def _common():
    mask = np.ones((4, 6), dtype=bool)
    return dict(mask=mask, edges=[], edge_conditions={}, initial_field=np.zeros(mask.shape), diffusion_coefficient=6.0,
                dt=0.1, total_time=1.0, dx=1.0, energy_gap=180.0, num_energy_bins=12)


def test_per_member_keys_override_and_defaults_apply():
    kws = member_arguments([{}, {"bath_temperature": 0.2, "diffusion_coefficient": 3.0}], _common())
    assert kws[0]["bath_temperature"] == 0.1 and kws[1]["bath_temperature"] == 0.2
    assert kws[0]["diffusion_coefficient"] == 6.0 and kws[1]["diffusion_coefficient"] == 3.0
    assert kws[1]["pauli_warn_threshold"] == 0.5 and kws[1]["diffusion_scheme"] == "cn_exact"
    assert set(PER_MEMBER_KEYS) == {"initial_field", "energy_weights", "initial_condition_spec", "external_generation",
                                    "bath_temperature", "diffusion_coefficient", "phonon_history_out",
                                    "progress_callback"}


@pytest.mark.parametrize("key", ["dt", "mask", "num_energy_bins", "energy_gap", "tau_0", "T_c", "pauli_error_threshold",
                                 "diffusion_scheme", "device", "total_time"])
def test_shared_keys_cannot_be_set_per_member(key):
    with pytest.raises(ValueError, match=rf"member 1: '{key}' is shared by all members"):
        member_arguments([{}, {key: 1.0}], _common())


@pytest.mark.parametrize("shared", [{"gap_expression": "180 + x"}, {"precomputed": {"D_array": np.ones(3)}}])
@pytest.mark.parametrize("key", ["diffusion_coefficient", "bath_temperature"])
def test_per_member_d_and_temperature_need_no_precompute(shared, key):
    with pytest.raises(ValueError, match=rf"'{key}' cannot be set per member together with 'precomputed'"):
        member_arguments([{}, {key: 0.3}], dict(_common(), **shared))


def test_unknown_common_argument_names_the_member():
    with pytest.raises(TypeError, match="member 0:"):
        member_arguments([{}], dict(_common(), not_an_argument=1))


def test_generation_amounts_of_mixed_constant_and_pulse_members():
    specs = [None, ExternalGenerationSpec(mode="constant", rate=2.0),
             ExternalGenerationSpec(mode="pulse", pulse_start=0.2, pulse_duration=0.3, pulse_rate=5.0),
             ExternalGenerationSpec(mode="pulse", pulse_start=0.0, pulse_duration=0.25, pulse_rate=1.0),
             ExternalGenerationSpec(mode="custom", custom_body="E * 0"), ExternalGenerationSpec(mode="none")]
    dt = 0.1
    rows = [generation_amounts(specs, k * dt, dt) for k in range(6)]
    assert rows[0] == [0.0, dt * 2.0, 0.0, dt * 1.0, None, 0.0]
    assert rows[1] == [0.0, dt * 2.0, 0.0, dt * 1.0, None, 0.0]
    assert rows[2] == [0.0, dt * 2.0, dt * 5.0, dt * 1.0, None, 0.0]        # [0.2, 0.5) on, [0, 0.25) on
    assert rows[3] == [0.0, dt * 2.0, dt * 5.0, 0.0, None, 0.0]
    assert rows[5] == [0.0, dt * 2.0, 0.0, 0.0, None, 0.0]
    assert generation_amounts(specs[:2], 0.0, 0.05) == [0.0, 0.05 * 2.0]     # short last step


def test_batches_follow_the_cap_and_the_free_memory():
    ids = list(range(7))
    assert plan_batches(ids, 1.0, None, None) == [ids]
    assert plan_batches(ids, 1.0, None, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert plan_batches(ids, 100.0, 250.0 / 0.8, None) == [[0, 1], [2, 3], [4, 5], [6]]
    assert plan_batches(ids, 100.0, 1.0, None) == [[k] for k in ids]          # at least one member per batch
    assert plan_batches([], 1.0, None, None) == []
    with pytest.raises(ValueError):
        plan_batches(ids, 1.0, None, 0)


def test_shards_cover_every_member_once():
    M, world = 11, 3
    shards = [shard_members(M, world, r) for r in range(world)]
    assert shards[0] == [0, 3, 6, 9] and shards[2] == [2, 5, 8]
    assert sorted(sum(shards, [])) == list(range(M))


def test_library_exports_the_ensemble_symbols():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    lib = _hip.load()
    for name in ("qp_pauli_stats_members", "qp_pauli_members_workspace_bytes", "qp_add_constant_members",
                 "qp_collision_step_guarded_members", "qp_collision_double_step_guarded_members"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert lib.qp_pauli_members_workspace_bytes(4096, 1) == lib.qp_pauli_workspace_bytes()
    assert lib.qp_pauli_members_workspace_bytes(4096, 512) == 512 * 4 * 24
