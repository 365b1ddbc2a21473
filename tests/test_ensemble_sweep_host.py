"""Host side of ensemble parameter sweeps (no GPU): the ``sweep=`` argument rules, per-member resolution of the collision
times, slicing by batches and shards, the collapse of an all-equal sweep, and the library's new C symbol."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from qpsim_amd import ensemble as ENS
from qpsim_amd import solver as S
from qpsim_amd.distributed import shard_members
from qpsim_amd.ensemble import PER_MEMBER_KEYS, SWEEP_KEYS, member_arguments, plan_batches, table_parameters

ROOT = Path(__file__).resolve().parents[1]


def _common(**kw):
    mask = np.ones((4, 6), dtype=bool)
    c = dict(mask=mask, edges=[], edge_conditions={}, initial_field=np.zeros(mask.shape), diffusion_coefficient=6.0,
             dt=0.1, total_time=1.0, dx=1.0, energy_gap=180.0, num_energy_bins=12, enable_recombination=True,
             enable_scattering=True)
    c.update(kw)
    return c


def _taus(kws):
    """(tau_s, tau_r) per member as the run resolves them (solver._checked_run_arguments)."""
    out = []
    for k in kws:
        c = S._checked_run_arguments(k["mask"], k["initial_field"], k["diffusion_coefficient"], k["dt"], k["total_time"],
                                     k["store_every"], k["enable_diffusion"], k["enable_recombination"],
                                     k["enable_scattering"], k["tau_0"], k["tau_s"], k["tau_r"], k["external_generation"],
                                     k["phonon_history_out"])
        out.append((c[4], c[5]))
    return out


def test_sweep_keys_are_the_collision_physics_and_stay_out_of_the_member_keys():
    assert SWEEP_KEYS == ("tau_0", "tau_s", "tau_r", "T_c", "dynes_gamma")
    assert "SWEEP_KEYS" in ENS.__all__
    assert not set(SWEEP_KEYS) & set(PER_MEMBER_KEYS)
    with pytest.raises(ValueError, match=r"member 1: 'tau_0' is shared by all members"):
        member_arguments([{}, {"tau_0": 1.0}], _common(), {"T_c": [1.0, 1.1]})


def test_swept_values_are_substituted_per_member():
    kws = member_arguments([{}, {"bath_temperature": 0.2}, {}], _common(),
                           {"T_c": [1.0, 1.1, 1.2], "dynes_gamma": (0.0, 0.5, 1.0)})
    assert [k["T_c"] for k in kws] == [1.0, 1.1, 1.2]
    assert [k["dynes_gamma"] for k in kws] == [0.0, 0.5, 1.0]
    assert [k["tau_0"] for k in kws] == [440.0] * 3 and kws[1]["bath_temperature"] == 0.2
    c = _common()
    assert member_arguments([{}, {}], c, None) == member_arguments([{}, {}], c)      # same array objects: no element compare
    assert member_arguments([{}, {}], c, {}) == member_arguments([{}, {}], c)


def test_unknown_sweep_key_is_named():
    with pytest.raises(ValueError, match=r"'bath_temperature' cannot be swept"):
        member_arguments([{}, {}], _common(), {"bath_temperature": [0.1, 0.2]})
    with pytest.raises(ValueError, match=r"'dt' cannot be swept"):
        member_arguments([{}, {}], _common(), {"dt": [0.1, 0.2]})


@pytest.mark.parametrize("values", [[1.0], [1.0, 1.1, 1.2], 1.0, "ab"])
def test_wrong_length_is_named(values):
    with pytest.raises(ValueError, match=r"sweep: 'T_c'"):
        member_arguments([{}, {}], _common(), {"T_c": values})


def test_a_swept_key_may_stand_in_common_only_with_the_swept_value():
    with pytest.raises(ValueError, match=r"'tau_0' is also set in the common arguments"):
        member_arguments([{}, {}], _common(tau_0=300.0), {"tau_0": [300.0, 400.0]})
    with pytest.raises(ValueError, match=r"'tau_s' is also set in the common arguments"):
        member_arguments([{}, {}], _common(tau_s=None), {"tau_s": [300.0, 400.0]})
    kws = member_arguments([{}, {}], _common(tau_0=300.0), {"tau_0": [300.0, 300.0]})        # no conflict
    assert [k["tau_0"] for k in kws] == [300.0, 300.0]


@pytest.mark.parametrize("shared", [{"gap_expression": "180 + x"}, {"precomputed": {"D_array": np.ones(3)}}])
@pytest.mark.parametrize("key", SWEEP_KEYS)
def test_sweep_needs_no_precompute(shared, key):
    with pytest.raises(ValueError, match=rf"'{key}' cannot be swept together with 'precomputed' or 'gap_expression'"):
        member_arguments([{}, {}], _common(**shared), {key: [1.0, 2.0]})
    member_arguments([{}, {}], _common(gap_expression="  "), {key: [1.0, 2.0]})           # blank expression: none


def test_tau_s_and_tau_r_default_from_the_members_tau_0():
    kws = member_arguments([{}, {}, {}], _common(), {"tau_0": [100.0, 200.0, 300.0], "tau_r": [None, 50.0, None]})
    assert _taus(kws) == [(100.0, 100.0), (200.0, 50.0), (300.0, 300.0)]
    assert table_parameters(kws, _taus(kws)) == [(0.0, 100.0, 100.0, 1.2), (0.0, 50.0, 200.0, 1.2), (0.0, 300.0, 300.0, 1.2)]


def test_per_member_argument_errors_name_the_member():
    kws = member_arguments([{}, {}], _common(), {"tau_0": [100.0, -1.0]})
    k = kws[1]
    with pytest.raises(ValueError, match=r"^member 7: tau_s must be positive"):
        ENS._prefixed(7, S._checked_run_arguments, k["mask"], k["initial_field"], k["diffusion_coefficient"], k["dt"],
                      k["total_time"], k["store_every"], k["enable_diffusion"], k["enable_recombination"],
                      k["enable_scattering"], k["tau_0"], k["tau_s"], k["tau_r"], k["external_generation"],
                      k["phonon_history_out"])


def test_sweep_lists_follow_the_members_through_batches_and_shards():
    M = 7
    tc = [1.0 + 0.1 * m for m in range(M)]
    kws = member_arguments([{} for _ in range(M)], _common(), {"T_c": tc})
    for batch in plan_batches(list(range(M)), 1.0, None, 3):
        assert [kws[m]["T_c"] for m in batch] == [tc[m] for m in batch]
    world = 3
    seen = []
    for rank in range(world):
        mine = shard_members(M, world, rank)
        for batch in plan_batches(mine, 1.0, None, 2):
            params = table_parameters([kws[m] for m in batch], _taus([kws[m] for m in batch]))
            assert [p[3] for p in params] == [tc[m] for m in batch]
            seen += batch
    assert sorted(seen) == list(range(M))


def test_an_all_equal_sweep_collapses_to_the_shared_argument_set():
    plain = member_arguments([{}, {}, {}], _common(tau_0=300.0, T_c=1.1))
    swept = member_arguments([{}, {}, {}], _common(), {"tau_0": [300.0] * 3, "T_c": [1.1] * 3})
    drop = lambda kws: [{k: v for k, v in kw.items() if k not in ("mask", "initial_field")} for kw in kws]  # noqa: E731
    assert drop(swept) == drop(plain)
    params = table_parameters(swept, _taus(swept))
    assert len(set(params)) == 1 and params == table_parameters(plain, _taus(plain))
    # a sweep over a time whose process is off reaches no table: one table set as well
    off = member_arguments([{}, {}], _common(enable_recombination=False), {"tau_r": [100.0, 200.0]})
    assert len(set(table_parameters(off, _taus(off)))) == 1
    on = member_arguments([{}, {}], _common(), {"tau_r": [100.0, 200.0]})
    assert len(set(table_parameters(on, _taus(on)))) == 2


def test_member_tables_symbol_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    lib = _hip.load()
    name = "qp_collision_member_tables_available"
    header = (ROOT / "include" / "qpsim_hip.h").read_text()
    assert re.search(r"\bint %s\(int32_t ne\);" % name, header)
    assert re.search(r"#define QP_COLL_MEMBER_CLASSES 8u\b", header)
    assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert [ne for ne in range(1, 65) if lib.qp_collision_member_tables_available(ne)] == list(range(4, 17))
    assert all(lib.qp_collision_pair_available(ne) for ne in range(4, 17))
    assert name in (ROOT / "INTEGRATION.md").read_text()
