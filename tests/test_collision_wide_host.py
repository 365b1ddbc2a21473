"""Wide bins (QP_COLL_WIDE_BINS, opt-in) without a GPU: the availability query, the route rule, the host plan with
``wide_bins`` on the grids of the GPU tests, and the public keyword.

The route query launches nothing and follows no pointer, so the tables carry placeholder addresses (as in
tests/test_collision_route_host.py)."""
from __future__ import annotations

import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from test_collision_padded_host import _same_plan
from test_collision_route_host import INVALID, _route, _tables

ROOT = Path(__file__).resolve().parents[1]
P = 8                                    # a non-null "device pointer" that is never followed
FORCE_GENERIC, FORCE_WAVE, MEMBER_CLASSES, WIDE_BINS = 1, 2, 8, 32
# the grids of tests/test_gpu_collision_wide.py (gap 180, energy_max_factor 3.0): ne -> (nw, structured maps)
GRIDS = {65: (233, False), 72: (215, True), 100: (299, True), 127: (424, False), 128: (383, True)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


# ------------------------------------------------------------------------------------------------ C ABI
def test_flag_and_route_constants_match_the_header():
    from qpsim_amd import _hip as H
    text = (ROOT / "include" / "qpsim_hip.h").read_text()
    assert re.search(r"#define QP_COLL_WIDE_BINS 32u\b", text) and H.COLL_WIDE_BINS == 32 == WIDE_BINS
    # the tenth enumerator, implicit after QP_ROUTE_ONEPASS_PADDED (8)
    assert re.search(r"QP_ROUTE_ONEPASS_PADDED,[^\n]*\n\s*QP_ROUTE_WAVE_WIDE\b(?!\s*=)", text)
    assert H.ROUTE_WAVE_WIDE == 9 and H.ROUTE_ONEPASS_PADDED == 8


def test_availability_query(lib):
    for ne, nw in ((65, 1), (128, 512), (100, 299)):
        assert lib.qp_collision_wide_available(ne, nw) == 1, (ne, nw)
    for ne, nw in ((64, 191), (129, 386), (100, 513), (100, 0)):
        assert lib.qp_collision_wide_available(ne, nw) == 0, (ne, nw)
    assert [ne for ne in range(1, 200) if lib.qp_collision_wide_available(ne, 3 * ne - 1)] == list(range(65, 129))


# ------------------------------------------------------------------------------------------------ route
def test_wide_route(lib):
    from qpsim_amd import _hip as H
    for ne in (65, 72, 100, 127, 128):
        nw = 3 * ne - 1
        for hint in ({}, dict(diag_bin=P, anti_bin=P)):
            for scratch in (0, 1):
                assert _route(lib, _tables(ne, nw, flags=WIDE_BINS, **hint), scratch=scratch) == H.ROUTE_WAVE_WIDE, ne
            assert _route(lib, _tables(ne, nw, flags=WIDE_BINS | FORCE_WAVE, **hint), scratch=0) == H.ROUTE_WAVE_WIDE, ne
            assert _route(lib, _tables(ne, nw, flags=WIDE_BINS | FORCE_GENERIC, **hint)) == H.ROUTE_GENERIC, ne
            assert _route(lib, _tables(ne, nw, flags=WIDE_BINS | FORCE_GENERIC, **hint), scratch=0) == INVALID, ne
            # without the flag: the generic kernel, which needs its scratch
            assert _route(lib, _tables(ne, nw, **hint)) == H.ROUTE_GENERIC, ne
            assert _route(lib, _tables(ne, nw, **hint), scratch=0) == INVALID, ne
            assert _route(lib, _tables(ne, nw, **hint), scratch=0, upd=0) == H.ROUTE_GENERIC, ne
        # gap classes and member classes go through cls
        assert _route(lib, _tables(ne, nw, nclass=4, flags=WIDE_BINS), scratch=0) == H.ROUTE_WAVE_WIDE, ne
        members = _tables(ne, nw, nclass=2, flags=WIDE_BINS | MEMBER_CLASSES, diag_bin=P, anti_bin=P)
        assert _route(lib, members, scratch=0) == H.ROUTE_WAVE_WIDE, ne
        assert _route(lib, _tables(ne, nw, flags=WIDE_BINS), en_r=0, en_s=0, scratch=0) == H.ROUTE_WAVE_WIDE, ne


def test_flag_outside_the_range_changes_nothing(lib):
    from qpsim_amd import _hip as H
    for hint in ({}, dict(diag_bin=P, anti_bin=P)):
        assert _route(lib, _tables(64, 191, flags=WIDE_BINS, **hint), scratch=0) == H.ROUTE_WAVE
        assert _route(lib, _tables(64, 191, **hint), scratch=0) == H.ROUTE_WAVE
        assert _route(lib, _tables(64, 193, flags=WIDE_BINS, **hint)) == H.ROUTE_GENERIC
        for ne, nw in ((129, 386), (100, 513), (128, 513), (200, 599)):
            for flags in (WIDE_BINS, 0):
                assert _route(lib, _tables(ne, nw, flags=flags, **hint)) == H.ROUTE_GENERIC, (ne, nw)
                assert _route(lib, _tables(ne, nw, flags=flags, **hint), scratch=0) == INVALID, (ne, nw)
    assert _route(lib, _tables(12, flags=WIDE_BINS, diag_bin=P, anti_bin=P)) == H.ROUTE_REGISTER
    assert _route(lib, _tables(33, flags=WIDE_BINS)) == H.ROUTE_WAVE


# ------------------------------------------------------------------------------------------------ host plan
def _tables_of(ne, gaps=(180.0,)):
    from qpsim_amd import tables as T
    E, _ = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    maps = T.build_phonon_frequency_map(E)[1:]
    kr = np.stack([T.recombination_kernel_base(E, g, 500.0, 1.2) for g in gaps])
    ks = np.stack([T.scattering_kernel_base(E, g, 400.0, 1.2) for g in gaps])
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in gaps])
    return [kr, ks, rho, *maps]


def _plan(lib, ne, wide, ncell=64, gaps=(180.0,), args=None, **kw):
    from qpsim_amd.collision_tables import plan_collision_tables
    args = _tables_of(ne, gaps) if args is None else args
    return plan_collision_tables(lib, ncell, np.ones(ncell, dtype=bool), *args, wide_bins=wide, **kw)


@pytest.mark.parametrize("ne", sorted(GRIDS))
def test_wide_plan_on_the_grids_of_the_gpu_tests(lib, ne):
    from qpsim_amd.collision_tables import scratch_planes, structured_bin_maps
    nw, structured = GRIDS[ne]
    args = _tables_of(ne)
    assert (structured_bin_maps(*args[3:]) is not None) == structured
    for kernel in ("auto", "wave"):
        p = _plan(lib, ne, True, args=args, kernel=kernel)
        assert p.flag_bits == WIDE_BINS | (FORCE_WAVE if kernel == "wave" else 0)
        assert p.kernel == "wave" and p.fast and not p.pair and p.symmetric and (p.ne, p.nw, p.nclass) == (ne, nw, 1)
        assert p.struct(dict.fromkeys(p.arrays, P)).flags & WIDE_BINS
        assert (p.arrays["diag_bin"] is not None) == structured and p.arrays["ks0_diag"] is None
        assert scratch_planes(p, True, True, True) == 0
    off = _plan(lib, ne, False, args=args)
    assert off.kernel == "generic" and not off.fast and not off.pair and off.flag_bits == 0
    assert scratch_planes(off, True, True, True) == nw
    # the arrays are those of the plan without the key
    on = _plan(lib, ne, True, args=args)
    for name in on.arrays:
        assert (on.arrays[name] is None) == (off.arrays[name] is None), name
        assert on.arrays[name] is None or np.array_equal(on.arrays[name], off.arrays[name]), name


def test_wide_plan_of_gap_and_member_classes(lib):
    from qpsim_amd.collision_tables import scratch_planes
    gaps = (180.0, 171.0, 165.5)
    g = _plan(lib, 72, True, gaps=gaps, cls_packed=np.arange(64) % 3)
    assert g.kernel == "wave" and g.fast and g.flag_bits == WIDE_BINS and g.nclass == 3 and scratch_planes(g, 1, 1, 1) == 0
    m = _plan(lib, 72, True, ncell=128, gaps=(180.0,) * 3, members=3, member_classes=True)
    assert m.kernel == "wave" and m.fast and not m.pair and m.flag_bits == WIDE_BINS | MEMBER_CLASSES
    assert scratch_planes(m, 1, 1, 1) == 0
    assert _plan(lib, 72, False, ncell=128, gaps=(180.0,) * 3, members=3, member_classes=True).kernel == "generic"


@pytest.mark.parametrize("ne", [12, 33, 50, 64])
def test_wide_bins_changes_no_plan_at_other_sizes(lib, ne):
    args = _tables_of(ne)
    for kw in ({}, dict(kernel="wave"), dict(kernel="generic")):
        on, off = _plan(lib, ne, True, args=args, **kw), _plan(lib, ne, False, args=args, **kw)
        _same_plan(on, off)
        assert not on.flag_bits & WIDE_BINS


def test_asymmetric_and_forced_generic_tables_still_plan_generic(lib):
    from qpsim_amd.collision_tables import scratch_planes
    args = _tables_of(72)
    args[0] = args[0].copy()
    args[0][0, 3, 5] *= 1.5          # K^r_0[3][5] != K^r_0[5][3]
    for kw in ({}, dict(kernel="wave")):
        p = _plan(lib, 72, True, args=args, **kw)
        assert not p.symmetric and p.kernel == "generic" and not p.fast and not p.flag_bits & WIDE_BINS
        assert scratch_planes(p, 1, 1, 1) == p.nw
    forced = _plan(lib, 72, True, kernel="generic")
    assert forced.kernel == "generic" and forced.flag_bits == FORCE_GENERIC and not forced.fast
    _same_plan(forced, _plan(lib, 72, False, kernel="generic"))
    _same_plan(_plan(lib, 72, True, allow_fast=False), _plan(lib, 72, False, allow_fast=False))


# ------------------------------------------------------------------------------------------------ public interface
def test_keyword_of_the_run_function():
    from qpsim_amd import solver as S
    from qpsim_amd.collision_tables import plan_collision_tables
    from qpsim_amd.engine import Engine
    from qpsim_amd.ensemble import PER_MEMBER_KEYS, member_arguments
    params = inspect.signature(S.run_2d_crank_nicolson).parameters
    par = params["collision_wide_bins"]
    assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY
    names = list(params)
    assert abs(names.index("collision_wide_bins") - names.index("collision_padded_bins")) == 1
    assert "collision_wide_bins" not in PER_MEMBER_KEYS
    with pytest.raises(ValueError, match="collision_wide_bins.*shared by all members"):
        member_arguments([{"collision_wide_bins": True}], {})
    for fn in (S._collision_tables, plan_collision_tables, Engine.make_collision_tables):
        assert inspect.signature(fn).parameters["wide_bins"].default is False
