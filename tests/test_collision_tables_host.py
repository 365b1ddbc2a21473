"""plan_collision_tables, scratch_planes and pair_members_supported, checked without a GPU.

The labels and images pinned here are those the GPU tests assert, at the same sizes.  The label is then held against the
library: qp_collision_route launches nothing and follows no pointer, so the struct built from a plan carries a placeholder
address for every array the plan holds (as in tests/test_collision_route_host.py).  Grids are those of
tests/collision_grids.py; a merged grid exists for the sizes of MERGED_FMAX only."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from collision_grids import MERGED_FMAX, unmerged_fmax

P = 8                                    # a non-null "device pointer" that is never followed
NE_LIST = [2, 4, 12, 16, 17, 18, 24, 30, 33, 50, 64, 65]
MERGED_NE = [ne for ne in NE_LIST if ne in MERGED_FMAX]
PROCESSES = [(1, 1), (1, 0), (0, 1)]
GAPS = np.array([180.0, 171.0, 165.5])
PHYSICS = [(440.0, 440.0, 1.2), (300.0, 520.0, 1.0), (650.0, 250.0, 1.5)]       # (tau_r, tau_s, T_c) per member
SEPARABLE = ("gap_sq", "kr_amp", "ks_amp", "pair_inv")
_PLANS: dict = {}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


def _plan(lib, kind, ne, ncell=64):
    """Plan of one table kind on a full mask of ``ncell`` cells (member tables: three members of ``ncell`` cells each),
    built once."""
    key = (kind, ne, ncell)
    if key not in _PLANS:
        from qpsim_amd import tables as T
        from qpsim_amd.collision_tables import plan_collision_tables
        E, _ = T.build_energy_grid(180.0, 1.0, MERGED_FMAX[ne] if kind == "merged" else unmerged_fmax(ne), ne)
        maps = T.build_phonon_frequency_map(E)[1:]
        mask, kw = np.ones(ncell, dtype=bool), {}
        if kind == "member":
            kr = np.stack([T.recombination_kernel_base(E, 180.0, tr, tc) for tr, _, tc in PHYSICS])
            ks = np.stack([T.scattering_kernel_base(E, 180.0, ts, tc) for _, ts, tc in PHYSICS])
            rho = np.stack([T.dynes_density_of_states(E, 180.0, 0.1)] * 3)
            kw = dict(members=3, member_classes=True)
        elif kind in ("gap", "gap_no_params"):
            kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in GAPS])
            ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in GAPS])
            rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in GAPS])
            kw = dict(cls_packed=np.arange(ncell) % 3)
            if kind == "gap":
                kw["gap_params"] = dict(E=E, gaps=GAPS, tau_r=500.0, tau_s=400.0, T_c=1.2)
        else:
            kr = T.recombination_kernel_base(E, 180.0, 500.0, 1.2)[None]
            ks = T.scattering_kernel_base(E, 180.0, 400.0, 1.2)[None]
            rho = T.dynes_density_of_states(E, 180.0, 0.1)[None]
        _PLANS[key] = plan_collision_tables(lib, ncell, mask, kr, ks, rho, *maps, **kw)
    return _PLANS[key]


def _route(lib, plan, ncell, en_r, en_s, upd, scratch):
    t = plan.struct(dict.fromkeys(plan.arrays, P))
    return lib.qp_collision_route(C.byref(t), ncell, int(en_r), int(en_s), int(upd), int(scratch))


def _family(route):
    from qpsim_amd import _hip as H
    return {H.ROUTE_ONEPASS: "register", H.ROUTE_REGISTER: "register", H.ROUTE_REGISTER_MEMBERS: "register",
            H.ROUTE_ONEPASS_CLASSES: "register", H.ROUTE_REGISTER_CLASSES: "register", H.ROUTE_WAVE: "wave",
            H.ROUTE_GENERIC: "generic"}.get(route)


# ------------------------------------------------------------------------------------------------ pinned labels and images
def test_plan_arrays_are_the_uploaded_layout(lib):
    from qpsim_amd.collision_tables import ARRAY_NAMES
    plan, ne = _plan(lib, "gap", 12), 12
    assert tuple(plan.arrays) == ARRAY_NAMES
    dtypes = {"idx_diff": np.int32, "idx_sum": np.int32, "cls": np.int32, "diag_bin": np.int32, "anti_bin": np.int32,
              "sign": np.int8}
    for name, a in plan.arrays.items():
        if a is not None:
            assert a.flags["C_CONTIGUOUS"] and a.dtype == dtypes.get(name, np.float64), name
    assert plan.arrays["kr0"].shape == (3, ne, ne) and plan.arrays["rho"].shape == (3, ne)
    assert np.array_equal(plan.arrays["cls"], np.arange(64) % 3)
    assert (plan.ne, plan.nw, plan.nclass, plan.flag_bits) == (ne, 3 * ne - 1, 3, 0)


def test_plain_tables_label(lib):
    p = _plan(lib, "plain", 12)
    assert p.kernel == "register" and p.pair and p.fast and p.symmetric and p.merged_slots == 0 and p.flag_bits == 0
    assert _plan(lib, "plain", 17).kernel == "wave" and _plan(lib, "plain", 33).kernel == "wave"
    p = _plan(lib, "plain", 65)
    assert p.kernel == "generic" and not p.fast and not p.pair


@pytest.mark.parametrize("ne", MERGED_NE)
def test_merged_grids_are_tagged(lib, ne):
    p = _plan(lib, "merged", ne)
    assert p.kernel == "register" and p.merged_slots > 0 and p.flag_bits & 4 and not p.pair
    assert p.struct(dict.fromkeys(p.arrays, P)).flags & 4
    assert int(np.count_nonzero(p.arrays["diag_bin"] >> 16)) == p.merged_slots


def test_non_symmetric_tables_run_the_generic_kernel(lib):
    """The tables of test_step_api_with_asymmetric_tables_runs_the_general_kernel (tests/test_gpu_configs.py)."""
    from qpsim_amd import tables as T
    from qpsim_amd.collision_tables import plan_collision_tables
    rng = np.random.default_rng(21)
    ne = 7
    E, _ = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    _, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = T.dynes_density_of_states(E, 180.0, 0.1)
    kr = T.recombination_kernel_base(E, 180.0, 500.0, 1.2) * (1.0 + 0.3 * rng.random((ne, ne)))
    ks = T.scattering_kernel_base(E, 180.0, 400.0, 1.2) * (1.0 + 0.3 * rng.random((ne, ne)))
    idx_d2 = idx_d.copy()
    idx_d2[1, 4] = idx_d[2, 5] + 1
    mask = np.ones(40, dtype=bool)
    p = plan_collision_tables(lib, 40, mask, kr[None], ks[None], rho[None], idx_d2, idx_s, sg)
    assert p.kernel == "generic" and not p.symmetric and p.flag_bits & 1
    assert plan_collision_tables(lib, 40, mask, kr[None] + kr.T[None], None, rho[None], idx_d, idx_s, sg).kernel != "generic"


def test_member_tables_label(lib):
    for ncell in (40, 64, 100):
        p = _plan(lib, "member", 12, ncell)
        assert p.kernel == "register" and p.member_classes and p.flag_bits & 8
        assert np.array_equal(p.arrays["cls"], np.repeat(np.arange(3), ncell))
    for ne in (30, 50):
        p = _plan(lib, "member", ne, 256)
        assert p.kernel == "register" and not p.pair
        assert p.arrays["ks0_diag"].shape == (3, ne, ne) and p.arrays["kr0_anti2"].shape == (3, 2 * ne - 1, ne)
        for ncell in (64, 100, 320):
            p = _plan(lib, "member", ne, ncell)
            assert p.kernel == "wave" and p.arrays["ks0_diag"] is None and p.arrays["kr0_anti2"] is None


def test_gap_class_tables_label(lib):
    p = _plan(lib, "gap", 12)
    assert p.kernel == "register" and all(p.arrays[k] is not None for k in SEPARABLE)
    p = _plan(lib, "gap_no_params", 12)
    assert p.kernel == "wave" and all(p.arrays[k] is None for k in SEPARABLE)


# ------------------------------------------------------------------------------------------------ label against the library
CASES = ([(kind, ne) for ne in NE_LIST for kind in ("plain", "member", "gap", "gap_no_params")]
         + [("merged", ne) for ne in MERGED_NE])


@pytest.mark.parametrize("ncell", [64, 256])
@pytest.mark.parametrize("kind,ne", CASES)
def test_label_is_the_family_of_the_route(lib, monkeypatch, kind, ne, ncell):
    from qpsim_amd.collision_tables import scratch_planes
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    plan = _plan(lib, kind, ne, ncell)
    total = ncell * (3 if kind == "member" else 1)
    for (en_r, en_s) in PROCESSES:
        for upd in (1, 0):
            route = _route(lib, plan, total, en_r, en_s, upd, scratch_planes(plan, en_r, en_s, upd) > 0)
            assert route >= 0, (lib.qp_last_error(), en_r, en_s, upd)
            assert _family(route) == plan.kernel, (route, plan.kernel, en_r, en_s, upd)


@pytest.mark.parametrize("ne", NE_LIST)
def test_members_that_are_not_wave_aligned_take_the_class_map_kernels(lib, monkeypatch, ne):
    """The known exception: the label is a property of the table set, the route of a call."""
    from qpsim_amd import _hip as H
    from qpsim_amd.collision_tables import scratch_planes
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    plan = _plan(lib, "member", ne, 100)
    assert (plan.kernel == "register") == (lib.qp_collision_member_tables_available(ne) == 1)
    for (en_r, en_s) in PROCESSES:
        for upd in (1, 0):
            route = _route(lib, plan, 300, en_r, en_s, upd, scratch_planes(plan, en_r, en_s, upd) > 0)
            if plan.kernel == "register":
                assert route == H.ROUTE_WAVE
            else:
                assert route >= 0 and _family(route) == plan.kernel


# ------------------------------------------------------------------------------------------------ scratch and pair rules
@pytest.mark.parametrize("ne", [12, 18])
def test_merged_bins_need_their_stash_to_stay_on_the_register_kernel(lib, ne):
    from qpsim_amd import _hip as H
    from qpsim_amd.collision_tables import scratch_planes
    plan = _plan(lib, "merged", ne)
    assert scratch_planes(plan, 1, 1, 1) == plan.merged_slots > 0
    assert _route(lib, plan, 64, 1, 1, 1, 1) == H.ROUTE_REGISTER
    assert _route(lib, plan, 64, 1, 1, 1, 0) == H.ROUTE_WAVE
    assert scratch_planes(plan, 1, 1, 0) == scratch_planes(plan, 1, 0, 1) == 0


def test_scratch_planes_of_the_other_kernels(lib):
    from qpsim_amd.collision_tables import scratch_planes
    plan = _plan(lib, "plain", 65)
    assert scratch_planes(plan, 1, 1, 1) == scratch_planes(plan, 0, 1, 1) == plan.nw > 0
    assert scratch_planes(plan, 1, 1, 0) == scratch_planes(plan, 0, 0, 1) == 0
    for kind, ne in CASES:
        for ncell in (64, 256):
            plan = _plan(lib, kind, ne, ncell)
            if plan.kernel != "generic" and not plan.merged_slots:
                assert not any(scratch_planes(plan, r, s, u) for r, s in PROCESSES for u in (1, 0)), (kind, ne)
    handle = {"kernel": "register", "fast": True, "nw": 35, "merged_slots": 3}          # the handle dict reads the same
    assert scratch_planes(handle, 1, 1, 1) == 3 and scratch_planes(handle, 1, 0, 1) == 0


def test_pair_members_rule(lib):
    from qpsim_amd.collision_tables import pair_members_supported
    plan = _plan(lib, "member", 12, 64)
    assert plan.pair and pair_members_supported(plan, 64, 3) and pair_members_supported({"pair": True}, 64, 3)
    assert not pair_members_supported(_plan(lib, "member", 12, 100), 100, 3)
    assert not pair_members_supported(plan, (1 << 28) // 4, 4) and pair_members_supported(plan, (1 << 28) // 4 - 64, 4)
    assert not pair_members_supported({"pair": False}, 64, 3) and not pair_members_supported({}, 64, 3)
