"""qp_collision_route: which kernel family a collision step takes, asked of the library without a GPU.

The query launches nothing and follows no table pointer, so the tables here carry dummy non-null addresses.  The
expected routes and availability lists are those of the dispatch code before the route function existed."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
P = 8                                    # a non-null "device pointer" that is never followed
FORCE_GENERIC, FORCE_WAVE, SHARED_BINS, MEMBER_CLASSES = 1, 2, 4, 8
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


def _tables(ne, nw=None, nclass=1, **over):
    """Plain complete tables (both processes, maps, no structure hint); `over` sets members by name."""
    from qpsim_amd import _hip
    t = _hip.CollisionTables.make(ne, 2 * ne - 1 if nw is None else nw, nclass, P, P, P, P, P, P,
                                  P if nclass > 1 else 0)
    for k, v in over.items():
        setattr(t, k, v)
    return t


def _structured(ne, **over):
    return _tables(ne, **{"diag_bin": P, "anti_bin": P, **over})


def _onepass(ne, **over):
    return _structured(ne, **{"ks0_diag": P, "kr0_anti2": P, **over})


def _members(ne, nclass=2, **over):
    return _structured(ne, **{"nclass": nclass, "cls": P, "flags": MEMBER_CLASSES, **over})


def _gap(ne, nclass=3, **over):
    return _structured(ne, **{"nclass": nclass, "cls": P, "gap_sq": P, "pair_inv": P, "kr_amp": P, "ks_amp": P, **over})


def _route(lib, t, ncell=128, en_r=1, en_s=1, upd=1, scratch=1):
    return lib.qp_collision_route(C.byref(t), ncell, en_r, en_s, upd, scratch)


def test_route_constants_match_the_header():
    from qpsim_amd import _hip
    text = (ROOT / "include" / "qpsim_hip.h").read_text()
    declared = dict(re.findall(r"\bQP_(ROUTE_[A-Z_]+) = (\d+)", text))
    assert len(declared) == 8
    for name, value in declared.items():
        assert getattr(_hip, name) == int(value), name


def test_plain_tables(lib):
    from qpsim_amd import _hip as H
    assert _route(lib, _structured(12)) == H.ROUTE_REGISTER
    assert _route(lib, _tables(12)) == H.ROUTE_WAVE
    assert _route(lib, _structured(12, flags=FORCE_GENERIC)) == H.ROUTE_GENERIC
    assert _route(lib, _structured(12, flags=FORCE_WAVE)) == H.ROUTE_WAVE
    assert _route(lib, _structured(17)) == H.ROUTE_WAVE
    assert _route(lib, _structured(33)) == H.ROUTE_WAVE
    assert _route(lib, _tables(65)) == H.ROUTE_GENERIC
    assert _route(lib, _tables(65), scratch=0) == INVALID and b"qp_collision_route" in lib.qp_last_error()
    assert _route(lib, _tables(64, nw=193)) == H.ROUTE_GENERIC


def test_one_pass_one_gap_class(lib, monkeypatch):
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    for ne in (50, 40, 32, 30):
        assert _route(lib, _onepass(ne)) == H.ROUTE_ONEPASS, ne
    assert _route(lib, _onepass(50, kr0_anti2=0), en_r=1) == H.ROUTE_REGISTER
    assert _route(lib, _onepass(50, kr0_anti2=0), en_r=0) == H.ROUTE_ONEPASS
    assert _route(lib, _onepass(24)) == H.ROUTE_REGISTER
    monkeypatch.setenv("QPSIM_COLL_ONEPASS", "0")         # read at every call
    assert _route(lib, _onepass(50)) == H.ROUTE_REGISTER
    monkeypatch.setenv("QPSIM_COLL_ONEPASS", "1")
    assert _route(lib, _onepass(50)) == H.ROUTE_ONEPASS


def test_no_process(lib):
    from qpsim_amd import _hip as H
    assert _route(lib, _structured(12), en_r=0, en_s=0) == H.ROUTE_COPY
    assert _route(lib, _structured(12, kr0=0, ks0=0)) == H.ROUTE_COPY
    assert _route(lib, _structured(17), en_r=0, en_s=0) == H.ROUTE_WAVE


def test_merged_bins(lib):
    from qpsim_amd import _hip as H
    t = _structured(18, flags=SHARED_BINS)
    assert _route(lib, t, scratch=0) == H.ROUTE_WAVE
    assert _route(lib, t, scratch=1) == H.ROUTE_REGISTER
    assert _route(lib, t, scratch=0, upd=0) == H.ROUTE_REGISTER


def test_member_classes(lib):
    from qpsim_amd import _hip as H
    assert _route(lib, _members(12), ncell=128) == H.ROUTE_REGISTER_MEMBERS
    assert _route(lib, _members(12), ncell=200) == H.ROUTE_WAVE          # 100 cells per member: waves would straddle
    assert _route(lib, _members(12), ncell=129) == INVALID and b"multiple of nclass" in lib.qp_last_error()
    assert _route(lib, _members(12), ncell=128, en_r=0, en_s=0) == H.ROUTE_WAVE
    assert _route(lib, _members(50), ncell=128) == H.ROUTE_WAVE
    assert _route(lib, _members(12, nclass=1)) == H.ROUTE_REGISTER
    assert _route(lib, _members(12, cls=0)) == INVALID and b"cls" in lib.qp_last_error()


def test_gap_classes(lib, monkeypatch):
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    assert _route(lib, _gap(12)) == H.ROUTE_REGISTER_CLASSES
    assert _route(lib, _gap(12, ks_amp=0), en_s=1) == H.ROUTE_WAVE
    assert _route(lib, _gap(12, ks_amp=0), en_s=0) == H.ROUTE_REGISTER_CLASSES
    assert _route(lib, _gap(12, gap_sq=0)) == H.ROUTE_WAVE
    assert _route(lib, _gap(50)) == H.ROUTE_ONEPASS_CLASSES
    assert _route(lib, _gap(50, nclass=17)) == H.ROUTE_REGISTER_CLASSES
    assert _route(lib, _gap(40)) == H.ROUTE_REGISTER_CLASSES
    assert _route(lib, _gap(33)) == H.ROUTE_WAVE
    monkeypatch.setenv("QPSIM_COLL_ONEPASS", "0")
    assert _route(lib, _gap(50)) == H.ROUTE_REGISTER_CLASSES


def test_size_limit_of_the_register_kernels(lib):
    from qpsim_amd import _hip as H
    assert _route(lib, _structured(12), ncell=(1 << 28) - 1) == H.ROUTE_REGISTER
    assert _route(lib, _structured(12), ncell=1 << 28) == H.ROUTE_WAVE


def test_refusals_are_those_of_the_step(lib):
    """Tables qp_collision_step refuses get the same status from the query (and nothing is launched by either)."""
    bad = _structured(12)
    bad.struct_size = 64
    assert _route(lib, bad) == INVALID and b"struct_size" in lib.qp_last_error()
    assert lib.qp_collision_step(C.byref(bad), P, 128, P, 2 * P, P, 0, 1.0, 0.1, 1, 1, 1, 0) == INVALID
    assert lib.qp_collision_route(None, 128, 1, 1, 1, 1) == INVALID
    for t in (_tables(12, rho=0), _tables(12, idx_sum=0), _tables(12, nclass=2, cls=0), _tables(12, diag_bin=P),
              _tables(0), _members(12, nclass=5)):
        assert _route(lib, t) == INVALID
        assert lib.qp_collision_step(C.byref(t), P, 128, P, 2 * P, P, 0, 1.0, 0.1, 1, 1, 1, 0) == INVALID
    assert _route(lib, _structured(12), ncell=0) == INVALID


REGISTER_NE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 24, 30, 32, 40, 50]
AVAILABLE = {
    "qp_collision_register_kernel_available": REGISTER_NE,
    "qp_collision_register_kernel_classes": REGISTER_NE,
    "qp_collision_onepass_available": [30, 32, 40, 50],
    "qp_collision_member_tables_available": list(range(4, 17)),
    "qp_collision_pair_available": list(range(4, 17)),
}


@pytest.mark.parametrize("name", sorted(AVAILABLE))
def test_availability_queries_are_unchanged(lib, name):
    assert [ne for ne in range(1, 71) if getattr(lib, name)(ne) == 1] == AVAILABLE[name]
    assert {getattr(lib, name)(ne) for ne in range(1, 71)} == {0, 1}
