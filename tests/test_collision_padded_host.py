"""Padded bins (QP_COLL_PAD_BINS, opt-in) without a GPU: the ceiling query, the grids of the GPU tests, the host plan with
``pad_bins``, the route rule and the public keyword.

The route query launches nothing and follows no pointer, so the tables carry placeholder addresses (as in
tests/test_collision_route_host.py)."""
from __future__ import annotations

import ctypes as C
import inspect
import re
from dataclasses import fields
from pathlib import Path

import numpy as np
import pytest

import collision_padded_cases as PC

ROOT = Path(__file__).resolve().parents[1]
P = 8                                    # a non-null "device pointer" that is never followed
FORCE_WAVE, SHARED_BINS, MEMBER_CLASSES, PAD_BINS = 2, 4, 8, 16
GAPS = np.array([180.0, 171.0, 165.5])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ C ABI
def test_ceiling_of_every_size(lib):
    want = {ne: 0 for ne in range(1, 71)}
    want.update({ne: 30 for ne in (17, 19, 21, 22, 23, 25, 26, 27, 28, 29)})
    want[31] = 32
    want.update({ne: 40 for ne in range(33, 40)})
    want.update({ne: 50 for ne in range(41, 50)})
    for ne in range(1, 71):
        assert lib.qp_collision_padded_ceiling(ne) == want[ne] == PC.ceiling(ne), ne
        if want[ne]:
            assert lib.qp_collision_onepass_available(want[ne]) and not lib.qp_collision_register_kernel_available(ne)
    assert [ne for ne in range(1, 71) if want[ne]] == PC.PADDED_NE


def test_flag_and_route_constants_match_the_header():
    from qpsim_amd import _hip as H
    text = (ROOT / "include" / "qpsim_hip.h").read_text()
    assert re.search(r"#define QP_COLL_PAD_BINS 16u\b", text) and H.COLL_PAD_BINS == 16 == PAD_BINS
    # the ninth enumerator, implicit after QP_ROUTE_COPY = 7
    assert re.search(r"QP_ROUTE_COPY = 7,[^\n]*\n\s*QP_ROUTE_ONEPASS_PADDED\b(?!\s*=)", text)
    assert H.ROUTE_ONEPASS_PADDED == 8


# ------------------------------------------------------------------------------------------------ grids
@pytest.mark.parametrize("ne,kind", PC.GRIDS)
def test_every_grid_is_structured_and_of_its_kind(ne, kind):
    from qpsim_amd import tables as T
    from qpsim_amd.collision_tables import structured_bin_maps
    E, _ = T.build_energy_grid(180.0, 1.0, PC.FACTOR[kind][ne], ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    assert structured_bin_maps(idx_d, idx_s, sg, allow_shared=True) is not None
    if kind == "merged":
        assert structured_bin_maps(idx_d, idx_s, sg) is None and om.size < 3 * ne - 1
    else:
        assert structured_bin_maps(idx_d, idx_s, sg) is not None and om.size == 3 * ne - 1


# ------------------------------------------------------------------------------------------------ host plan
def _tables_of(ne, factor, gaps=(180.0,)):
    from qpsim_amd import tables as T
    E, _ = T.build_energy_grid(180.0, 1.0, factor, ne)
    maps = T.build_phonon_frequency_map(E)[1:]
    kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in gaps])
    ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in gaps])
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in gaps])
    return E, (kr, ks, rho, *maps)


def _plan(lib, ne, factor, pad, ncell=64, gaps=(180.0,), **kw):
    from qpsim_amd.collision_tables import plan_collision_tables
    E, args = _tables_of(ne, factor, gaps)
    if len(gaps) > 1 and kw.pop("with_gap_params", False):
        kw["gap_params"] = dict(E=E, gaps=np.asarray(gaps), tau_r=500.0, tau_s=400.0, T_c=1.2)
    return plan_collision_tables(lib, ncell, np.ones(ncell, dtype=bool), *args, pad_bins=pad, **kw)


def _same_plan(a, b):
    for f in fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if f.name == "arrays":
            assert list(x) == list(y)
            for name in x:
                assert (x[name] is None) == (y[name] is None), name
                if x[name] is not None:
                    assert x[name].dtype == y[name].dtype and np.array_equal(x[name], y[name]), name
        else:
            assert x == y, f.name


@pytest.mark.parametrize("ne", [25, 45])
def test_padded_plan_builds_the_live_size_images(lib, ne):
    from qpsim_amd.collision_tables import antidiagonal_major, diagonal_major, scratch_planes
    p = _plan(lib, ne, 3.0, True)
    assert p.kernel == "register" and p.fast and not p.pair and p.flag_bits == PAD_BINS and p.merged_slots == 0
    assert p.struct(dict.fromkeys(p.arrays, P)).flags & PAD_BINS
    assert (p.ne, p.nw, p.nclass) == (ne, 3 * ne - 1, 1)
    assert p.arrays["ks0_diag"].shape == (ne, ne) and p.arrays["kr0_anti2"].shape == (2 * ne - 1, ne)
    assert np.array_equal(p.arrays["ks0_diag"], diagonal_major(p.arrays["ks0"][0]))
    assert np.array_equal(p.arrays["kr0_anti2"], antidiagonal_major(p.arrays["kr0"][0], 2.0))
    assert p.arrays["kr0"].shape == (1, ne, ne) and p.arrays["diag_bin"].shape == (ne,)
    assert scratch_planes(p, 1, 1, 1) == 0
    off = _plan(lib, ne, 3.0, False)
    assert off.kernel == "wave" and off.flag_bits == 0 and off.arrays["ks0_diag"] is None
    # merged bins: the stash of a "register" plan
    m = _plan(lib, ne, PC.MERGED[ne], True)
    assert m.kernel == "register" and m.flag_bits == PAD_BINS | SHARED_BINS and m.merged_slots > 0
    assert scratch_planes(m, 1, 1, 1) == m.merged_slots and scratch_planes(m, 1, 0, 1) == 0


def test_padded_plan_of_member_classes(lib):
    ne = 25
    kw = dict(gaps=(180.0, 180.0, 180.0), members=3, member_classes=True)
    p = _plan(lib, ne, 3.0, True, ncell=256, **kw)
    assert p.kernel == "register" and p.flag_bits == PAD_BINS | MEMBER_CLASSES and not p.pair
    assert p.arrays["ks0_diag"].shape == (3, ne, ne) and p.arrays["kr0_anti2"].shape == (3, 2 * ne - 1, ne)
    _same_plan(_plan(lib, ne, 3.0, True, ncell=320, **kw), _plan(lib, ne, 3.0, False, ncell=320, **kw))
    assert _plan(lib, ne, 3.0, True, ncell=320, **kw).kernel == "wave"


@pytest.mark.parametrize("case", ["ne30", "ne12", "gap_classes", "unstructured", "forced_wave", "ne51"])
def test_pad_bins_changes_no_other_plan(lib, case):
    from qpsim_amd.collision_tables import structured_bin_maps
    ne, factor, kw = {"ne30": (30, 3.0, {}), "ne12": (12, 3.0, {}), "ne51": (51, 3.0, {}),
                      "gap_classes": (25, 3.0, dict(gaps=tuple(GAPS), cls_packed=np.arange(64) % 3, with_gap_params=True)),
                      "unstructured": (17, 3.0, {}), "forced_wave": (25, 3.0, dict(kernel="wave"))}[case]
    if case == "unstructured":
        from qpsim_amd import tables as T
        maps = T.build_phonon_frequency_map(T.build_energy_grid(180.0, 1.0, 3.0, 17)[0])[1:]
        assert structured_bin_maps(*maps, allow_shared=True) is None
    on, off = _plan(lib, ne, factor, True, **dict(kw)), _plan(lib, ne, factor, False, **dict(kw))
    _same_plan(on, off)
    assert not on.flag_bits & PAD_BINS
    assert on.kernel == {"ne30": "register", "ne12": "register"}.get(case, "wave")


# ------------------------------------------------------------------------------------------------ route
def _t(ne, nclass=1, **over):
    from qpsim_amd import _hip
    t = _hip.CollisionTables.make(ne, 3 * ne - 1, nclass, P, P, P, P, P, P, P if nclass > 1 else 0)
    for k, v in {"diag_bin": P, "anti_bin": P, "ks0_diag": P, "kr0_anti2": P, "flags": PAD_BINS, **over}.items():
        setattr(t, k, v)
    return t


def _route(lib, t, ncell=128, en_r=1, en_s=1, upd=1, scratch=1):
    return lib.qp_collision_route(C.byref(t), ncell, en_r, en_s, upd, scratch)


def test_padded_route(lib, monkeypatch):
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    for ne in (25, 31, 39, 49):
        assert _route(lib, _t(ne)) == H.ROUTE_ONEPASS_PADDED, ne
        assert _route(lib, _t(ne, flags=0)) == H.ROUTE_WAVE, ne
        assert _route(lib, _t(ne, flags=PAD_BINS | FORCE_WAVE)) == H.ROUTE_WAVE, ne
        assert _route(lib, _t(ne, ks0_diag=0)) == H.ROUTE_WAVE, ne
        assert _route(lib, _t(ne, ks0_diag=0), en_s=0) == H.ROUTE_ONEPASS_PADDED, ne
        assert _route(lib, _t(ne, kr0_anti2=0)) == H.ROUTE_WAVE, ne
        assert _route(lib, _t(ne), en_r=0, en_s=0) == H.ROUTE_WAVE, ne
        assert _route(lib, _t(ne, kr0=0, ks0=0)) == H.ROUTE_WAVE, ne
        assert _route(lib, _t(ne), ncell=(1 << 28) - 1) == H.ROUTE_ONEPASS_PADDED, ne
        assert _route(lib, _t(ne), ncell=1 << 28) == H.ROUTE_WAVE, ne
        shared = _t(ne, flags=PAD_BINS | SHARED_BINS)
        assert _route(lib, shared, scratch=0) == H.ROUTE_WAVE, ne
        assert _route(lib, shared, scratch=1) == H.ROUTE_ONEPASS_PADDED, ne
        assert _route(lib, shared, scratch=0, upd=0) == H.ROUTE_ONEPASS_PADDED, ne
        assert _route(lib, _t(ne, diag_bin=0, anti_bin=0)) == H.ROUTE_WAVE, ne
    monkeypatch.setenv("QPSIM_COLL_ONEPASS", "0")         # read at every call
    assert _route(lib, _t(25)) == H.ROUTE_WAVE


def test_padded_route_of_member_classes_and_other_sizes(lib, monkeypatch):
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    members = dict(nclass=3, cls=P, flags=PAD_BINS | MEMBER_CLASSES)
    assert _route(lib, _t(25, **members), ncell=3 * 256) == H.ROUTE_ONEPASS_PADDED
    assert _route(lib, _t(25, **members), ncell=3 * 512) == H.ROUTE_ONEPASS_PADDED
    assert _route(lib, _t(25, **members), ncell=3 * 320) == H.ROUTE_WAVE
    assert _route(lib, _t(25, **{**members, "flags": MEMBER_CLASSES}), ncell=3 * 256) == H.ROUTE_WAVE
    # gap classes at a padded size: as without the flag
    gap = dict(nclass=3, cls=P, gap_sq=P, pair_inv=P, kr_amp=P, ks_amp=P)
    assert _route(lib, _t(25, **gap)) == H.ROUTE_WAVE
    # sizes with a kernel of their own, and beyond the largest ceiling
    assert _route(lib, _t(30)) == H.ROUTE_ONEPASS and _route(lib, _t(50)) == H.ROUTE_ONEPASS
    assert _route(lib, _t(24)) == H.ROUTE_REGISTER and _route(lib, _t(12)) == H.ROUTE_REGISTER
    assert _route(lib, _t(51)) == H.ROUTE_WAVE and _route(lib, _t(64)) == H.ROUTE_WAVE


# ------------------------------------------------------------------------------------------------ public interface
def test_keyword_of_the_run_function():
    from qpsim_amd import solver as S
    from qpsim_amd.ensemble import PER_MEMBER_KEYS, member_arguments
    par = inspect.signature(S.run_2d_crank_nicolson).parameters["collision_padded_bins"]
    assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert "collision_padded_bins" not in PER_MEMBER_KEYS
    with pytest.raises(ValueError, match="collision_padded_bins.*shared by all members"):
        member_arguments([{"collision_padded_bins": True}], {})
    for fn in (S._collision_tables,):
        assert inspect.signature(fn).parameters["pad_bins"].default is False
    from qpsim_amd.collision_tables import plan_collision_tables
    from qpsim_amd.engine import Engine
    assert inspect.signature(plan_collision_tables).parameters["pad_bins"].default is False
    assert inspect.signature(Engine.make_collision_tables).parameters["pad_bins"].default is False
