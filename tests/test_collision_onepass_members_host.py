"""Member tables (QP_COLL_MEMBER_CLASSES) at the one-pass sizes NE = 30, 32, 40, 50, checked without a GPU: which route
qp_collision_route answers (the query launches nothing and follows no pointer, so the tables carry placeholder addresses,
as in tests/test_collision_route_host.py), and the layout of the per-member diagonal-major tables the engine uploads."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

P = 8                                    # a non-null "device pointer" that is never followed
FORCE_WAVE, MEMBER_CLASSES = 2, 8
ONEPASS_NE = [30, 32, 40, 50]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


def _members(ne, nclass=2, **over):
    """Complete structured member-class tables with the diagonal-major images of both processes."""
    from qpsim_amd import _hip
    t = _hip.CollisionTables.make(ne, 2 * ne - 1, nclass, P, P, P, P, P, P, P)
    for k, v in {"diag_bin": P, "anti_bin": P, "flags": MEMBER_CLASSES, "ks0_diag": P, "kr0_anti2": P, **over}.items():
        setattr(t, k, v)
    return t


def _route(lib, t, ncell=512, en_r=1, en_s=1, upd=1, scratch=1):
    return lib.qp_collision_route(C.byref(t), ncell, en_r, en_s, upd, scratch)


@pytest.mark.parametrize("ne", ONEPASS_NE)
def test_member_tables_take_the_one_pass_route_when_blocks_do_not_straddle(lib, monkeypatch, ne):
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    assert lib.qp_collision_onepass_available(ne) == 1 and lib.qp_collision_member_tables_available(ne) == 0
    assert _route(lib, _members(ne), ncell=512) == H.ROUTE_ONEPASS            # 256 cells per member
    assert _route(lib, _members(ne), ncell=128) == H.ROUTE_WAVE               # 64
    assert _route(lib, _members(ne), ncell=640) == H.ROUTE_WAVE               # 320: a block would hold two members
    assert _route(lib, _members(ne, kr0_anti2=0), en_r=1) == H.ROUTE_WAVE     # no member form of the split kernels
    assert _route(lib, _members(ne, kr0_anti2=0), en_r=0) == H.ROUTE_ONEPASS
    assert _route(lib, _members(ne, flags=MEMBER_CLASSES | FORCE_WAVE)) == H.ROUTE_WAVE
    assert _route(lib, _members(ne), en_r=0, en_s=0) == H.ROUTE_WAVE
    monkeypatch.setenv("QPSIM_COLL_ONEPASS", "0")                             # read at every call
    assert _route(lib, _members(ne)) == H.ROUTE_WAVE
    monkeypatch.setenv("QPSIM_COLL_ONEPASS", "1")
    assert _route(lib, _members(ne)) == H.ROUTE_ONEPASS


def test_other_sizes_keep_their_member_routes(lib, monkeypatch):
    from qpsim_amd import _hip as H
    monkeypatch.delenv("QPSIM_COLL_ONEPASS", raising=False)
    assert _route(lib, _members(24), ncell=512) == H.ROUTE_WAVE
    assert _route(lib, _members(12), ncell=512) == H.ROUTE_REGISTER_MEMBERS


def test_stacked_diagonal_major_tables_are_the_members_own_tables_concatenated():
    """What a member's block stages is what its lone call uploads: image m of the stack is the image of table m alone."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import antidiagonal_major, diagonal_major, onepass_tables
    ne = 30
    E, _ = T.build_energy_grid(180.0, 1.0, 3.0, ne)
    physics = [(440.0, 440.0, 1.2), (300.0, 520.0, 1.0), (650.0, 250.0, 1.5)]
    kr = np.stack([T.recombination_kernel_base(E, 180.0, tr, tc) for tr, _, tc in physics])
    ks = np.stack([T.scattering_kernel_base(E, 180.0, ts, tc) for _, ts, tc in physics])
    assert not np.array_equal(kr[0], kr[1]) and not np.array_equal(ks[1], ks[2])
    ksd, kra = onepass_tables(ks, kr, 3, ne)
    assert ksd.shape == (3, ne, ne) and kra.shape == (3, 2 * ne - 1, ne)
    assert ksd.dtype == np.float64 and kra.dtype == np.float64
    assert np.array_equal(ksd.ravel(), np.concatenate([diagonal_major(ks[m]).ravel() for m in range(3)]))
    assert np.array_equal(kra.ravel(), np.concatenate([antidiagonal_major(kr[m], 2.0).ravel() for m in range(3)]))
    # the offsets the kernel applies for member m: m NE^2 and m (2 NE - 1) NE; the entries it reads from there
    m, k, i = 2, 7, 19
    assert ksd.ravel()[m * ne * ne + k * ne + i] == ks[m][i, i - k]
    assert kra.ravel()[m * (2 * ne - 1) * ne + (i + 3) * ne + i] == 2.0 * kr[m][i, 3]
    # one table, flat [ne, ne] input, a missing process
    one_s, one_r = onepass_tables(ks[1].ravel(), None, 1, ne)
    assert one_r is None and np.array_equal(one_s[0], diagonal_major(ks[1]))
