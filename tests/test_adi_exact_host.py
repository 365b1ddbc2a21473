"""The per-cell error criterion of the diffusion tests, checked without a GPU.

Every other diffusion test divides by the largest value of a whole batch of planes (`rel_err`, `_rel`) on dense inputs with
a dynamic range of 2.  tests/test_gpu_adi_elementwise.py bounds |got - exact| / (u max(T, 1e-4 max T)) plane by plane
instead (tests/adi_exact.py).  Here: K_ref64, the K of the fp64 oracle, lies in a window for every case of the GPU file (a
condition on the cases, not a measurement); three wrong variants of the fp64 oracle pass `rel_err < 2e-13` over their batch
and miss the new limit; and an fp64 solve that eliminates from the other end of every line stays inside it."""
from __future__ import annotations

import platform

import numpy as np
import pytest

import adi_exact as X
from golden_utils import rel_err
from test_gpu_collision_instantiations import HAVE_X87

if platform.machine() in ("x86_64", "AMD64"):
    assert HAVE_X87, "x86-64 has an 80-bit long double"
pytestmark = pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")

# one entry per set of references: the fine-tile modes share theirs
UNIQUE = list({(c["geom"], c["sides"], c["dset"], c["variant"], X.chunk_of(c["path"]), c["steps"]): c
               for c in X.CASES}.values())
WINDOWED = [c for c in UNIQUE if c["geom"] != ("rect", 1, 1)]       # the single cell has a bound of its own
OLD_TOL = 2e-13          # `rel_err` over the batch, the tolerance of the existing ADI tests


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


def test_stiff_cases_run_one_step_only():
    """At r D = 2.7 the multi-step T is loose by decades (K_ref64 = 0.05 at two steps on 64 x 96)."""
    assert X.STIFF_ONE_STEP and any(c["dset"] == "stiff" for c in X.CASES)


@pytest.mark.parametrize("case", WINDOWED, ids=[c["id"] for c in WINDOWED])
def test_k_of_the_fp64_reference_lies_in_the_window(case):
    """0.1 <= K_ref64 <= 16 for every plane, step count and the preconditioner solve of every GPU case, K_ref64 being the
    larger K of the oracle's two elimination orders.  A plane with D = 0 is returned unchanged by the oracle: its K_ref64
    is 0 and the limit demands the input back to 4 units per step."""
    p = X.problem(case)
    refs = X.references(case)
    lo, hi = X.WINDOW
    for k, name in enumerate(X.PLANES):
        ks = {n: refs[k]["steps"][n][2] for n in case["steps"]}
        ks["solve"] = refs[k]["solve"][2]
        print(f"{case['id']} {name}: K_ref64 " + " ".join(f"{n}: {v:.2f}" for n, v in ks.items()))
        if X.is_frozen(p["D"][k]):
            assert all(v == 0.0 for v in ks.values())
            for n in case["steps"]:
                assert np.array_equal(refs[k]["steps"][n][1], n * np.abs(p["u0"][k]).astype(X.LD))       # T = |u| per step
            continue
        for n, v in ks.items():
            assert v <= hi, (name, n, v)
            # the lower end on the oracle's own order too: the larger of two orders must not hide a truth that collapsed
            # onto the fp64 oracle
            assert v >= lo and refs[k]["orders"][n][0] >= lo, (name, n, v, refs[k]["orders"][n])


def test_the_single_cell_is_judged_by_an_explicit_bound():
    """On the 1 x 1 grid K is one rounding sample (0.01 ... 1.1 for the oracle), so K_ref64 means nothing there and the case
    stays out of the window: the GPU file holds it to `limit(0)` = 4 units of T, which both orders of the oracle meet."""
    singles = [c for c in X.CASES if X.single_cell(c)]
    assert [c["geom"] for c in singles] == [("rect", 1, 1)] and not any(X.single_cell(c) for c in WINDOWED)
    for case in singles:
        assert X.case_limit(case, 100.0) == X.limit(0.0) == 4.0
        for k, name in enumerate(X.PLANES):
            for which, both in X.references(case)[k]["orders"].items():
                print(f"{case['id']} {name} {which}: K of the oracle's two orders {both[0]:.2f} {both[1]:.2f}")
                assert max(both) <= 4.0


@pytest.mark.parametrize("case", UNIQUE, ids=[c["id"] for c in UNIQUE])
def test_elimination_from_the_other_end_stays_inside_the_limit(case):
    """The fp64 oracle with every implicit solve eliminating from the far end of its line (`steps64(reverse=True)`) against
    the limit formed from the oracle's own K alone: the limit is not tied to one operation order.  (K_ref64 of the GPU
    file is the larger of the two orders.)"""
    refs = X.references(case)
    for k, name in enumerate(X.PLANES):
        for which, (forward, backward) in refs[k]["orders"].items():
            print(f"{case['id']} {name} {which}: K eliminating from the other end {backward:.2f} (oracle {forward:.2f})")
            assert backward <= X.limit(forward), (name, which, backward, forward)
            assert max(forward, backward) == (refs[k]["solve"] if which == "solve" else refs[k]["steps"][which])[2]


# ------------------------------------------------------------------------------------------------ sensitivity
def _rect(ny, nx, by_side):
    from qpsim_amd.geometry import extract_edge_segments
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    return mask, edges, {e.edge_id: by_side[e.normal] for e in edges}


def _report(tag, old, k, kref):
    print(f"{tag}: rel_err over the batch {old:.2e} (tolerance {OLD_TOL:g}); K of the plane {k:.3g} "
          f"(limit {X.limit(kref):.3g}, K_ref64 {kref:.2f})")
    assert old < OLD_TOL
    assert k > X.limit(kref)


def test_a_dropped_side_source_on_a_small_plane_passes_the_batch_norm_and_misses_the_cell_limit(O):
    """Two planes on 64 x 96: the suite's sides at scale 1, and the same problem at 1e-9 - input and boundary values - whose
    upper side carries a weak flux (Neumann -1e-5, times 1e-9).  The wrong variant drops that side's source term on the
    small plane."""
    from qpsim_amd.models import BoundaryCondition as BC
    ny, nx, D, s = 64, 96, 6.0, 1e-9
    big = X.side_conditions("mixed")
    small = {"left": BC("dirichlet", 0.7 * s), "right": BC("robin", 0.4, 0.2 * s), "up": BC("neumann", -1e-5 * s),
             "down": BC("absorbing")}
    rng = np.random.default_rng(1)
    u0 = [rng.random((ny, nx)), s * rng.random((ny, nx))]
    ops = [O.build_grid_ops(*_rect(ny, nx, sides), X.DX) for sides in (big, small)]
    ref = [O.ADIStepper(ops[k], D, X.DT).step_grid(u0[k]) for k in range(2)]
    wrong = O.ADIStepper(ops[1], D, X.DT)
    sry = wrong.cf["sry"].copy()
    assert np.all(sry[0] != 0.0)
    sry[0] = 0.0
    wrong.src = wrong.h * (wrong.cf["srx"] + sry)
    got = [ref[0], wrong.step_grid(u0[1])]
    tr, t = X.truth_and_T(ops[1], D, X.DT, u0[1], (1,))[1]
    kref, _ = X.K(ref[1], tr, t)
    assert X.WINDOW[0] <= kref <= X.WINDOW[1]
    _report("dropped side source, plane at 1e-9", rel_err(np.stack(got), np.stack(ref)), X.K(got[1], tr, t)[0], kref)


def test_a_wrong_tail_behind_a_chunk_interface_passes_the_batch_norm_and_misses_the_cell_limit(O):
    """A delta next to a 32-cell chunk interface, one stiff step (r D = 2.7: the tail falls by 0.55 per cell and is 1e-9 of
    the peak one chunk away; at r D = 0.41 it is 1e-20 there, below the floor of the metric by design).  The wrong variant
    scales every cell more than one chunk from the delta by 1 + 1e-6."""
    ny, nx, D = 64, 96, 40.0
    ops = O.build_grid_ops(*_rect(ny, nx, X.side_conditions("homogeneous")), X.DX)
    u0 = np.zeros((ny, nx))
    u0[31, 31] = 1.0
    flat = np.random.default_rng(2).random((ny, nx))
    ref = [O.ADIStepper(ops, D, X.DT).step_grid(v) for v in (flat, u0)]
    y, x = np.indices((ny, nx))
    far = np.maximum(np.abs(y - 31), np.abs(x - 31)) > 32
    got = [ref[0], np.where(far, ref[1] * (1.0 + 1e-6), ref[1])]
    tr, t = X.truth_and_T(ops, D, X.DT, u0, (1,))[1]
    kref, _ = X.K(ref[1], tr, t)
    assert X.WINDOW[0] <= kref <= X.WINDOW[1]
    _report("tail beyond one chunk from a delta", rel_err(np.stack(got), np.stack(ref)), X.K(got[1], tr, t)[0], kref)


def test_a_perturbed_small_plane_passes_the_batch_norm_and_misses_the_cell_limit(O):
    """A plane at 1e-12 of its neighbour, wrong by 1e-3 of itself."""
    ny, nx, D = 64, 96, 2.0
    ops = O.build_grid_ops(*_rect(ny, nx, X.side_conditions("homogeneous")), X.DX)
    rng = np.random.default_rng(3)
    u0 = [rng.random((ny, nx)), 1e-12 * rng.random((ny, nx))]
    ref = [O.ADIStepper(ops, D, X.DT).step_grid(v) for v in u0]
    got = [ref[0], ref[1] * (1.0 + 1e-3)]
    tr, t = X.truth_and_T(ops, D, X.DT, u0[1], (1,))[1]
    kref, _ = X.K(ref[1], tr, t)
    assert X.WINDOW[0] <= kref <= X.WINDOW[1]
    _report("plane at 1e-12 wrong by 1e-3", rel_err(np.stack(got), np.stack(ref)), X.K(got[1], tr, t)[0], kref)


def test_a_cell_without_conditioning_must_be_equal():
    """T = 0 (a plane of zeros without sources): any difference is counted, not divided."""
    z = np.zeros((3, 4))
    got = z.copy()
    got[1, 2] = 1e-300
    assert X.K(z, z.astype(X.LD), z.astype(X.LD)) == (0.0, 0)
    assert X.K(got, z.astype(X.LD), z.astype(X.LD)) == (0.0, 1)
