"""Inputs, cases and references of the per-cell diffusion tests (tests/test_adi_exact_host.py without a GPU,
tests/test_gpu_adi_elementwise.py with one): the counterpart of tests/collision_exact.py for the ADI half of the time loop.

`truth` steps `oracle.qp_oracle.ADIStepper` in 80-bit long double on the SAME fp64 coefficients (cf, ax, ay, src are cast,
not re-derived).  `T` is the conditioning of every output cell: the step evaluated on magnitudes,

    |E_dir| t = (1 + h (w- + w+ + |dg|)) t + h (w- t- + w+ t+)         the explicit half, terms as they are evaluated
    T_loc(u)  = Sy^-1 ( |E_x| Sx^-1 ( |E_y| |u| + |s| ) + |s| )         the implicit solves are the real ones (inverses >= 0)
    T_n       = T_loc(|u_{n-1}|) + P_abs T_{n-1}                       u_{n-1} the long-double truth

with P_abs one step whose explicit entries are the true magnitudes |1 - h (w- + w+ + dg)|, h w-, h w+ and no sources.

K = max over the cells of a plane of |got - exact| / (u max(T, 1e-4 max_plane T)), u = 2^-53, one number PER PLANE.  The floor:
the tiled paths drop chunk couplings below 1e-22 of a line's values by design, at the floor the unit u 1e-4 max T = 1.1e-20
max T is 100 such drops; without a floor the fp64 oracle itself reaches K = 20 ... 30 in the far tail of a delta.  A kernel
must stay within `collision_exact.limit(K_ref64)` = 4 K_ref64 + 4, K_ref64 being the same statistic of the fp64 `ADIStepper`:
the larger of its K and that of the same stepper eliminating every line from the other end (`steps64(reverse=True)`), an
fp64 NumPy model of the same factorisation - a reference, never the kernel.  The direction matters in the tail of a delta:
finishing at the delta's end costs the oracle one rounding per tail cell, from the other end it costs three, and a kernel
that splits a line into chunks does some of each."""
from __future__ import annotations

import numpy as np

from collision_exact import limit  # noqa: F401  (the limit of both per-element files: imported, not re-declared)

LD = np.longdouble
U = 2.0 ** -53
FLOOR = 1e-4
WINDOW = (0.1, 16.0)        # K_ref64 of every plane of every case: outside it the case checks nothing or too much
DX, DT = 0.9, 0.11          # r = dt / (2 dx^2) = 0.0679: D = 6 -> r D = 0.407, D = 4.5 -> 0.306, D = 40 -> 2.72
PLANES = ("flat", "pulse", "ramp", "delta")
SCALES = {"mixed": (1.0, 1.0, 1.0, 1.0), "homogeneous": (1.0, 1e-9, 1e-18, 1e-100)}
DSETS = {"mild": (6.0, 0.35, 2.0, 4.4), "zero": (6.0, 0.0, 2.0, 0.35), "stiff": (40.0, 6.0, 0.35, 13.0),
         "fine": (4.5, 0.35, 2.0, 3.0), "fine_zero": (4.5, 3.0, 0.0, 0.35)}

_PROBLEMS: dict = {}
_REFS: dict = {}


def _O():
    from oracle import qp_oracle
    return qp_oracle


# ---------------------------------------------------------------------------------------------------- the metric
def stepper80(ops, D, dt):
    """`ADIStepper` built in fp64, its coefficient arrays cast to long double."""
    st = _O().ADIStepper(ops, D, dt)
    st.cf = {k: np.asarray(v).astype(LD) for k, v in st.cf.items()}
    st.ax = tuple(np.asarray(a).astype(LD) for a in st.ax)
    st.ay = tuple(np.asarray(a).astype(LD) for a in st.ay)
    st.src = np.asarray(st.src).astype(LD)
    return st


def _solve(st, rhs, axis, reverse=False):
    """(I - h L_axis)^-1 rhs by the oracle's Thomas recurrences; `reverse`: eliminating from the far end of every line."""
    O = _O()
    a, b, c = st.ax if axis == "x" else (np.swapaxes(t, -1, -2) for t in st.ay)
    d = rhs if axis == "x" else np.swapaxes(rhs, -1, -2)
    if reverse:
        flip = lambda t: np.ascontiguousarray(t[..., ::-1])          # noqa: E731
        x = flip(O.thomas_batched(flip(c), flip(b), flip(a), flip(d)))
    else:
        x = O.thomas_batched(a, b, c, d)
    return x if axis == "x" else np.swapaxes(x, -1, -2)


def _abs_explicit(st, t, axis, true_entries):
    """|E_dir| t for t >= 0: the magnitudes of the terms as evaluated, or (`true_entries`) of the matrix entries."""
    O, cf, h = _O(), st.cf, st.h
    wm, wp, dg = (cf["wxm"], cf["wxp"], cf["dgx"]) if axis == "x" else (cf["wym"], cf["wyp"], cf["dgy"])
    tm, tp = (O._shift(t, 0, -1), O._shift(t, 0, 1)) if axis == "x" else (O._shift(t, -1, 0), O._shift(t, 1, 0))
    diag = np.abs(1.0 - h * (wm + wp + dg)) if true_entries else 1.0 + h * (wm + wp + np.abs(dg))
    return diag * t + h * (wm * tm + wp * tp)


def _t_loc(st, au):
    s = np.abs(st.src)
    x = _solve(st, _abs_explicit(st, au, "y", False) + s, "x")
    return np.where(st.mask, _solve(st, _abs_explicit(st, x, "x", False) + s, "y"), 0.0)


def _p_abs(st, t):
    x = _solve(st, _abs_explicit(st, t, "y", True), "x")
    return np.where(st.mask, _solve(st, _abs_explicit(st, x, "x", True), "y"), 0.0)


def truth_and_T(ops, D, dt, u0, steps):
    """{n: (truth, T) after n steps} for n in `steps`, one long-double pass; `u0` a full [ny, nx] grid (holes 0)."""
    st = stepper80(ops, D, dt)
    u = np.where(st.mask, np.asarray(u0), 0.0).astype(LD)
    t = np.zeros_like(u)
    out = {}
    for n in range(1, max(steps) + 1):
        t = _t_loc(st, np.abs(u)) + (_p_abs(st, t) if n > 1 else 0.0)
        u = st.step_grid(u)
        if n in steps:
            out[n] = (u, t)
    return out


def truth(ops, D, dt, u0, nsteps):
    return truth_and_T(ops, D, dt, u0, (nsteps,))[nsteps][0]


def T(ops, D, dt, u0, nsteps):
    return truth_and_T(ops, D, dt, u0, (nsteps,))[nsteps][1]


def solve_truth_and_T(ops, D, dt, x):
    """(Sy^-1 Sx^-1 x, Sy^-1 Sx^-1 |x|) in long double: the preconditioner and its conditioning."""
    st = stepper80(ops, D, dt)
    x = np.where(st.mask, np.asarray(x), 0.0).astype(LD)
    return tuple(np.where(st.mask, _solve(st, _solve(st, v, "x"), "y"), 0.0) for v in (x, np.abs(x)))


def solve64(ops, D, dt, x, reverse=False):
    st = _O().ADIStepper(ops, D, dt)
    return np.where(st.mask, _solve(st, _solve(st, np.where(st.mask, x, 0.0), "x", reverse), "y", reverse), 0.0)


def steps64(ops, D, dt, u0, steps, reverse=False):
    """The fp64 `ADIStepper` ({n: plane after n steps}); `reverse`: the same operators with every implicit solve eliminating
    from the far end of its line - a second fp64 rounding pattern of the same factorisation."""
    st = _O().ADIStepper(ops, D, dt)
    u, out = np.where(st.mask, u0, 0.0), {}
    for n in range(1, max(steps) + 1):
        if reverse:
            x = _solve(st, st._explicit(u, "y") + st.src, "x", True)
            u = np.where(st.mask, _solve(st, st._explicit(x, "x") + st.src, "y", True), 0.0)
        else:
            u = st.step_grid(u)
        if n in steps:
            out[n] = u
    return out


def K(got, exact, T, mask=None):
    """(K of one plane, number of cells with T = 0 that differ)."""
    sel = slice(None) if mask is None else mask
    d = np.abs(np.asarray(got).astype(LD) - exact)[sel].ravel()
    t = np.asarray(T)[sel].ravel()
    tmax = t.max() if t.size else 0.0
    bad = int(np.count_nonzero(d[t == 0]))
    if tmax == 0:
        return 0.0, bad
    return float(np.max(d / (U * np.maximum(t, FLOOR * tmax)))), bad


# ---------------------------------------------------------------------------------------------------- problems
def _bc(kind, *v):
    from qpsim_amd.models import BoundaryCondition
    return BoundaryCondition(kind, *v)


def side_conditions(sides):
    if sides == "mixed":      # the suite's usual sides
        return {"left": _bc("dirichlet", 0.7), "right": _bc("robin", 0.4, 0.2), "up": _bc("neumann", -0.3),
                "down": _bc("absorbing")}
    return {"left": _bc("reflective"), "right": _bc("absorbing"), "up": _bc("robin", 0.4, 0.0), "down": _bc("dirichlet", 0.0)}


def _geometry(geom, sides):
    """(mask, edges, bcs) of ("rect", ny, nx), ("hole", ny, nx) - a rectangle with a rectangular hole, a condition per
    face normal - or ("masked", kind): `_masked_problem` of tests/test_gpu_parity.py, whose random per-edge conditions are
    replaced by their zero-source counterparts for the `homogeneous` side set."""
    from qpsim_amd.geometry import extract_edge_segments
    if geom[0] == "masked":
        from test_gpu_parity import _masked_problem
        _, mask, edges, bcs = _masked_problem(geom[1], 11)
        if sides == "homogeneous":
            zero = {"reflective": _bc("reflective"), "dirichlet": _bc("dirichlet", 0.0), "absorbing": _bc("absorbing"),
                    "neumann": _bc("reflective"), "robin": _bc("robin", 0.5, 0.0)}
            bcs = {k: zero[str(v.kind)] for k, v in bcs.items()}
        return mask, edges, bcs
    _, ny, nx = geom
    mask = np.ones((ny, nx), dtype=bool)
    if geom[0] == "hole":
        mask[ny // 2 - 6:ny // 2 + 5, nx // 3:nx // 3 + 25] = False
    edges = extract_edge_segments(mask)
    by_side = side_conditions(sides)
    return mask, edges, {e.edge_id: by_side[e.normal] for e in edges}


def _nearest_active(mask, row, col):
    rr, cc = np.nonzero(mask)
    k = int(np.argmin((rr - row) ** 2 + (cc - col) ** 2))
    return int(rr[k]), int(cc[k])


def planes(mask, seed, variant, chunk, scales):
    """The four planes [4, ny, nx] (holes 0).  `variant` 0: ramp along x, delta in the last cell before a chunk interface
    (row and column `chunk` - 1); 1: ramp along y, delta in the first cell behind it (`chunk`); 2: ramp along x, delta
    mid-chunk.  On grids shorter than that the delta sits in the last row / column."""
    ny, nx = mask.shape
    rng = np.random.default_rng(seed)
    y, x = np.indices(mask.shape)
    flat = rng.random(mask.shape)
    cy, cx = _nearest_active(mask, ny // 2, nx // 2)
    pulse = np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * 3.0 ** 2)) + 1e-8 * (1.0 + rng.random(mask.shape))
    frac = (y / ny) if variant == 1 else (x / nx)
    ramp = 10.0 ** (-12.0 * frac) * (1.0 + rng.random(mask.shape))
    at = (chunk - 1, chunk, chunk // 2)[variant]
    dy, dx_ = _nearest_active(mask, min(at, ny - 1), min(at, nx - 1))
    delta = np.zeros(mask.shape)
    delta[dy, dx_] = 1.0
    out = np.stack([flat, pulse, ramp, delta]) * np.asarray(scales)[:, None, None]
    return np.where(mask[None], out, 0.0)


def d_field(mask, seed):
    """Per-cell diffusivities of the four planes, r D in [0.014, 0.407]."""
    d = 0.2 + 5.8 * np.random.default_rng(seed + 77).random((4,) + mask.shape)
    return np.where(mask[None], d, 0.0)


def _case(path, geom, sides, dset, steps, variant):
    tag = "x".join(str(g) for g in geom[1:])
    return dict(id=f"{path}-{geom[0]}{tag}-{sides}-{dset}-v{variant}", path=path, geom=geom, sides=sides, dset=dset,
                steps=tuple(steps), variant=variant)


FINE_MODES = {"fine_two_sweep": "0", "fine_fused": "1", "fine_onepass": "2"}       # QPSIM_ADI_FUSED
_FINE = [(("rect", 64, 64), "mixed", "fine", 0), (("rect", 64, 320), "homogeneous", "fine", 1),
         (("rect", 192, 64), "mixed", "fine_zero", 2), (("rect", 128, 192), "homogeneous", "fine", 0),
         (("rect", 128, 192), "mixed", "fine", 1)]
CASES = (
    # one thread per line (allow_fast=False): any mask, scalar D or a D field
    [_case("lines", ("hole", 70, 65), "mixed", "mild", (1, 3), 0),
     _case("lines", ("hole", 70, 65), "homogeneous", "field", (1, 3), 1),
     _case("lines", ("hole", 70, 65), "mixed", "stiff", (1,), 2),
     _case("lines", ("rect", 1, 48), "mixed", "zero", (1, 3), 0),
     _case("lines", ("rect", 50, 1), "mixed", "mild", (1, 3), 1)]
    # full rectangle on 64 x 64 tiles, chunks decoupled wherever the remainder chunk allows
    + [_case("rect64", ("rect", 64, 64), "mixed", "mild", (1, 2, 5), 0),
       _case("rect64", ("rect", 64, 63), "homogeneous", "mild", (1, 2, 5), 1),
       _case("rect64", ("rect", 3, 200), "mixed", "zero", (1, 2, 5), 0),
       _case("rect64", ("rect", 1, 1), "homogeneous", "mild", (1, 2, 5), 2),
       _case("rect64", ("rect", 128, 192), "homogeneous", "mild", (1, 2, 5), 0),
       _case("rect64", ("rect", 128, 192), "mixed", "mild", (1, 2, 5), 1)]
    # the same tiles with the banded reduced systems (force_banded=True); a remainder chunk; stiff D
    + [_case("banded", ("rect", 129, 257), "mixed", "mild", (1, 2, 5), 0),
       _case("banded", ("rect", 70, 65), "homogeneous", "zero", (1, 2, 5), 1),
       _case("banded", ("rect", 64, 63), "mixed", "mild", (1, 2, 5), 2),
       _case("banded", ("rect", 128, 192), "homogeneous", "mild", (1, 2, 5), 1),
       _case("banded", ("rect", 128, 192), "mixed", "stiff", (1,), 0)]
    # fine tiles (32-cell chunks): two sweeps, reduce + fused, one pass
    + [_case(mode, geom, sides, dset, (1, 2, 5, 20), variant) for mode in FINE_MODES for geom, sides, dset, variant in _FINE]
    # masked grids on 64 x 64 tiles driven by per-cell codes: uniform D and a D field
    + [_case("tile", ("masked", kind), sides, dset, (1, 3), variant)
       for kind, sides, dset, variant in (("holes", "mixed", "mild", 0), ("holes", "homogeneous", "field", 1),
                                          ("donut", "homogeneous", "zero", 0), ("donut", "mixed", "field", 2),
                                          ("small", "mixed", "field", 0), ("small", "homogeneous", "mild", 1))])
STIFF_ONE_STEP = all(c["steps"] == (1,) for c in CASES if c["dset"] == "stiff")


def chunk_of(path):
    return 32 if path in FINE_MODES else 64


def problem(case):
    """Geometry, oracle operators, diffusivities and inputs of a case; shared by the cases that differ in the path only."""
    key = (case["geom"], case["sides"], case["dset"], case["variant"], chunk_of(case["path"]))
    if key not in _PROBLEMS:
        mask, edges, bcs = _geometry(case["geom"], case["sides"])
        seed = 100 * sum(mask.shape) + 10 * case["variant"] + len(case["sides"])
        u0 = planes(mask, seed, case["variant"], chunk_of(case["path"]), SCALES[case["sides"]])
        D = list(d_field(mask, seed)) if case["dset"] == "field" else list(DSETS[case["dset"]])
        u0.setflags(write=False)
        _PROBLEMS[key] = dict(key=key, mask=mask, edges=edges, bcs=bcs, dx=DX, dt=DT, D=D, u0=u0,
                              ops=_O().build_grid_ops(mask, edges, bcs, DX))
    return _PROBLEMS[key]


def single_cell(case):
    """The 1 x 1 grid: K of its one cell is a single rounding sample, not a maximum, so it is judged outside the window of
    K_ref64 (`case_limit`)."""
    return int(problem(case)["mask"].sum()) == 1


def case_limit(case, k_ref):
    """`limit(K_ref64)`; on the single cell `limit(0)` = 4 units of T per plane, what the limit grants a kernel whatever the
    reference does (the bound of a D = 0 plane as well): no share of a reference that is one sample."""
    return limit(0.0) if single_cell(case) else limit(k_ref)


def is_frozen(D):
    """A plane with D = 0 everywhere: the step is the identity, T = |u| and K_ref64 = 0."""
    return not np.any(np.asarray(D) != 0.0)


def references(case):
    """Per plane k: dict(steps={n: (truth, T, K_ref64)}, solve=(truth, T, K_ref64), orders={n or "solve": (K of the oracle,
    K of the oracle eliminating from the other end)}), computed once per problem.  K_ref64 is the larger of the two orders:
    both are the fp64 reference, the same factorisation in the two directions a line can be eliminated in (a delta at the
    end the oracle finishes at costs it one rounding per tail cell; from the other end it costs three)."""
    p = problem(case)
    key = (p["key"], case["steps"])
    if key not in _REFS:
        out = []
        for k in range(4):
            args = (p["ops"], p["D"][k], p["dt"], p["u0"][k])
            ex = truth_and_T(*args, case["steps"])
            r64 = [steps64(*args, case["steps"], reverse=rev) for rev in (False, True)]
            steps, orders = {}, {}
            for n, (tr, t) in ex.items():
                both = [K(r[n], tr, t, p["mask"]) for r in r64]
                assert all(bad == 0 for _, bad in both)
                orders[n] = tuple(kk for kk, _ in both)
                steps[n] = (tr, t, max(orders[n]))
            tr, t = solve_truth_and_T(*args)
            both = [K(solve64(*args, reverse=rev), tr, t, p["mask"]) for rev in (False, True)]
            assert all(bad == 0 for _, bad in both)
            orders["solve"] = tuple(kk for kk, _ in both)
            out.append(dict(steps=steps, solve=(tr, t, max(orders["solve"])), orders=orders))
        _REFS[key] = out
    return _REFS[key]


def k_ref64(case, plane, nsteps):
    return references(case)[plane]["steps"][nsteps][2]
