"""Stream-mode, table-form and launch-form variants of the tiled ADI kernels (`csrc/qp_adi_rect.hip`, `qp_adi_fine.inc`,
`qp_adi_tile.hip`).  The kernels are a matrix of template instantiations of which plan SIZE picks one: non-temporal plane
accesses above 192 / 384 MiB of carried planes (`stream_mode`), unmerged clean / general launches above 1024 general tiles,
full tables where a plan is not compact.  Here the knobs `QPSIM_STREAM_MODE`, `QPSIM_COMPACT_TABLES`, `QPSIM_TILE_MERGE`,
`QPSIM_TILE_FORK` (with `QPSIM_FINE_TILES`, `QPSIM_ADI_FUSED`, `QPSIM_PR_CARRIED` fixing the path) force every instantiation
at grids of a few tiles.  Each variant is held to

  1. the CPU oracle, with the bound the base variant already has in the existing tests of its path: 2e-13 against
     `O.ADIStepper` for ADI steps and for the ADI solve (the preconditioner: the two tridiagonal solves of the oracle's
     stepper, x then y), 1e-11 against `O.CNStepper` for whatever runs a Peaceman-Rachford cycle;
  2. the base variant (stream mode 0, default table form, default launch form) BIT FOR BIT: a non-temporal hint, a table
     fetched entry by entry instead of prefix / middle / suffix, and two launches instead of one change no arithmetic;

and one profiler trace per knob family shows, by the template arguments in the kernel names, that the forced
instantiation is the one that ran.

A cycle of J = 6 Peaceman-Rachford iterations reduces the error of its starting guess by the cycle's worst-case factor
(`peaceman_rachford_cycle`: 3e-9 at r D = 0.41, 8e-6 at r D = 2.7), so one cycle from the old field cannot reach 1e-11 of
the unsplit solution by construction.  The cycle is therefore applied n times, n the smallest count with factor^n <= 1e-14
(2 and 3 here), and the result of the LAST application is compared with the oracle; the result of the FIRST application
(rough data, full-size corrections) is compared bit for bit with the base variant as well.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DX, DT = 0.9, 0.11                  # r = 0.0679, as in the existing tests of every path below
ADI_TOL = 2e-13                     # test_rect_fast_path_..., test_fine_tiles_match_oracle_..., test_tile_path_..., test_hip_blocks_...
CN_TOL = 1e-11                      # test_exact_cn_step_on_fine_tiles_matches_superlu, test_exact_cn_iteration_on_the_fast_path_...
ONEPASS_TOL = 1e-14                 # test_gpu_adi_onepass.py: one-pass steps against the two-sweep form
PR_J = 6

_KNOB = {"stream": "QPSIM_STREAM_MODE", "compact": "QPSIM_COMPACT_TABLES", "fine": "QPSIM_FINE_TILES",
         "fused": "QPSIM_ADI_FUSED", "merge": "QPSIM_TILE_MERGE", "fork": "QPSIM_TILE_FORK", "carried": "QPSIM_PR_CARRIED"}


def _env(mp, **knobs):
    """Exactly these knobs are set (None: unset); everything else that selects a kernel variant is cleared."""
    for name in list(_KNOB.values()) + ["QPSIM_CN_PR"]:
        mp.delenv(name, raising=False)
    for k, v in knobs.items():
        if v is not None:
            mp.setenv(_KNOB[k], str(v))


def _served(mode):
    """STREAM template value that serves a plan's stream mode (1 is served by the kernels of 3)."""
    return {0: 0, 1: 3, 2: 2, 3: 3}[int(mode)]


def rel_err(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.fixture(scope="module")
def O():
    from oracle import qp_oracle
    return qp_oracle


# ------------------------------------------------------------------------------------------------------------------
# references (host only, once per problem) and cached device runs
# ------------------------------------------------------------------------------------------------------------------
_REF: dict = {}
_RUN: dict = {}


def _solve_oracle(O, st, x_packed):
    """(I - h Ly)^-1 (I - h Lx)^-1 x with the tridiagonal pieces of the oracle's ADI stepper."""
    g = np.zeros(st.mask.shape)
    g[st.mask] = x_packed
    y = O.thomas_batched(*st.ax, g)
    a, b, c = (np.swapaxes(t, -1, -2) for t in st.ay)
    out = np.swapaxes(O.thomas_batched(a, b, c, np.swapaxes(y, -1, -2)), -1, -2)
    return out[st.mask]


def _reference(O, key, gops, Ds, steps, seed, cn):
    """Inputs and oracle results for fields with diffusivities `Ds` (scalars or full-grid planes) on `gops`: u0, x0
    [nfield, n_interior]; want["steps<k>"], want["solve"]; with `cn` also b = (I + rL) u0 + 2 r S and want["cn"]."""
    if key in _REF:
        return _REF[key]
    rng = np.random.default_rng(seed)
    n, nf = int(gops.mask.sum()), len(Ds)
    u0, x0 = rng.random((nf, n)), rng.random((nf, n))
    want = {f"steps{k}": np.empty((nf, n)) for k in steps}
    want["solve"] = np.empty((nf, n))
    b = np.empty((nf, n)) if cn else None
    if cn:
        want["cn"] = np.empty((nf, n))
    for f, D in enumerate(Ds):
        st = O.ADIStepper(gops, D, DT)
        w = u0[f].copy()
        for s in range(1, max(steps) + 1):
            w = st.step(w)
            if s in steps:
                want[f"steps{s}"][f] = w
        want["solve"][f] = _solve_oracle(O, st, x0[f])
        if cn:
            stepper = O.CNStepper(gops, D, DT)
            b[f] = stepper.B @ u0[f] + stepper.rhs_src
            want["cn"][f] = stepper.step(u0[f])
    _REF[key] = {"u0": u0, "x0": x0, "b": b, "want": want}
    return _REF[key]


def _rect_geometry(ny, nx):
    """Full rectangle with a different boundary kind on every side (test_rect_fast_path_matches_oracle_adi_and_general_kernels)."""
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((ny, nx), dtype=bool)
    edges = extract_edge_segments(mask)
    side_bc = {"left": BoundaryCondition("dirichlet", 0.7), "right": BoundaryCondition("robin", 0.4, 0.2),
               "up": BoundaryCondition("neumann", -0.3), "down": BoundaryCondition("absorbing")}
    return mask, edges, {e.edge_id: side_bc[e.normal] for e in edges}


def _download(eng, t):
    eng.torch.cuda.synchronize()
    return eng.download_packed(t)


def _steps(eng, op, u0, k):
    a = eng.upload_packed(u0)
    eng.adi_steps(op, a, k)
    return _download(eng, a)


def _solve(eng, op, x0):
    x = eng.upload_packed(x0)
    eng._precondition(op, x)
    return _download(eng, x)


def _cycles_needed(op):
    from qpsim_amd.engine import _pr_bounds, peaceman_rachford_cycle
    factor = peaceman_rachford_cycle(*_pr_bounds(op), PR_J)[1]
    assert 0.0 < factor < 1e-3, factor
    return math.ceil(math.log(1e-14) / math.log(factor))


def _pr_cycles(eng, op, u0, b, fine):
    """`qp_adi_rect_pr_cycle` with the plans of `_pr_cycle(op, 6)`, applied `_cycles_needed` times from the guess u0:
    (result of the first application, result of the last)."""
    from qpsim_amd import _hip
    from qpsim_amd.engine import _pr_cycle, _ptr
    cycle = _pr_cycle(op, PR_J)
    assert cycle is not None and len(cycle) == PR_J
    assert all(p.fine for p in cycle) if fine else not any(p.fine for p in cycle)
    handles = (C.POINTER(_hip.RectPlan) * len(cycle))(*[p.handle for p in cycle])
    u, rhs = eng.upload_packed(u0), eng.upload_packed(b)
    first = None
    for _ in range(_cycles_needed(op)):
        _hip.check(eng.lib.qp_adi_rect_pr_cycle(handles, len(cycle), _ptr(u), _ptr(rhs), eng.stream), "qp_adi_rect_pr_cycle")
        if first is None:
            first = _download(eng, u)
    return first, _download(eng, u)


_KERNEL = re.compile(r"(\w+_kernel)(?:<([^<>]*)>)?")


def _traced_kernels(fn):
    """{(kernel, template arguments as strings)} of the device kernels launched by fn() (profiler trace)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    found = set()
    for e in prof.events():
        m = _KERNEL.search(e.name)
        if m:
            found.add((m.group(1), tuple(a.strip() for a in m.group(2).split(",")) if m.group(2) else ()))
    return found


def _assert_only(found, kernels, position, value):
    """Every traced instantiation of `kernels` carries `value` as template argument number `position`."""
    bad = sorted(k for k in found if k[0] in kernels and k[1][position] != value)
    assert not bad, bad


def _check(got, base, want, tol, ctx):
    for call, arr in got.items():
        assert arr.shape == base[call].shape and np.all(np.isfinite(arr)), (ctx, call)
        assert np.array_equal(arr, base[call]), (ctx, call, "differs from the base variant", float(np.max(np.abs(arr - base[call]))))
        if call in want:
            err = rel_err(arr, want[call])
            print(f"{ctx} {call}: {err:.2e} from the oracle (bound {tol(call):.0e})")
            assert err < tol(call), (ctx, call, "oracle", err)


def _tol(call):
    return CN_TOL if "pr" in call or "cn" in call else ADI_TOL


# ------------------------------------------------------------------------------------------------------------------
# 1. rectangle, 64 x 64 tiles
# ------------------------------------------------------------------------------------------------------------------
RECT_SHAPES = [(128, 192), (129, 257), (64, 64)]
RECT_DC = [6.0, 0.35, 0.0]          # compact tables wherever the extents are multiples of 64
STIFF_DC = [40.0, 6.0]              # r D = 2.7: not compact, banded reduced systems (on (128, 192) only)


def _rect_operators(shape):
    return [("", RECT_DC)] + ([("stiff/", STIFF_DC)] if shape == (128, 192) else [])


def _rect_run(mp, O, shape, mode, compact):
    """steps (k = 1, 3), `qp_adi_rect_solve`, Peaceman-Rachford cycles of fresh 64 x 64 plans built under the knobs."""
    key = ("rect", shape, mode, compact)
    if key in _RUN:
        return _RUN[key]
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    _env(mp, stream=mode, fine=0, compact=compact)
    mask, edges, bcs = _rect_geometry(*shape)
    gops = O.build_grid_ops(mask, edges, bcs, DX)
    eng = Engine(compile_geometry(mask, edges, bcs, DX))
    out = {}
    for tag, Dc in _rect_operators(shape):
        ref = _reference(O, ("rect", shape, tag), gops, Dc, (1, 3), shape[0] * 1000 + shape[1] + len(Dc), cn=True)
        op = DiffusionOperator(eng, len(Dc), DT, dcoef=Dc)
        assert op.rect is not None and not op.rect.fine
        if tag:                             # r D = 2.7 keeps 64-cell chunks coupled: rect_reduced_kernel runs
            assert op.rect.decoupled != (True, True)
        else:                               # ... and so does a one-cell remainder chunk, in both directions of 129 x 257
            assert op.rect.decoupled == ((False, False) if shape == (129, 257) else (True, True))
        for k in (1, 3):
            out[f"{tag}steps{k}"] = _steps(eng, op, ref["u0"], k)
        out[f"{tag}solve"] = _solve(eng, op, ref["x0"])
        out[f"{tag}pr_first_cycle"], out[f"{tag}pr"] = _pr_cycles(eng, op, ref["u0"], ref["b"], fine=False)
    _RUN[key] = out
    return out


def _rect_want(shape):
    want = {}
    for tag, _ in _rect_operators(shape):
        w = _REF[("rect", shape, tag)]["want"]
        want.update({f"{tag}steps1": w["steps1"], f"{tag}steps3": w["steps3"], f"{tag}solve": w["solve"], f"{tag}pr": w["cn"]})
    return want


@pytest.mark.parametrize("compact", [None, 0], ids=["tables-default", "tables-full"])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("shape", RECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rect_tiles_stream_modes_and_table_forms(O, monkeypatch, shape, mode, compact):
    """`rect_x_kernel` / `rect_y_kernel<*, STREAM, COMPACT, SRC>` at STREAM 2 and 3 (mode 1 is served by 3) in both table
    forms: every tile full (128 x 192: every access non-temporal), full and partial tiles with banded reduced systems
    (129 x 257), the single-chunk variant (64 x 64), a stiff non-compact operator; steps, solve, three-pass cycles."""
    base = _rect_run(monkeypatch, O, shape, 0, None)
    got = _rect_run(monkeypatch, O, shape, mode, compact)
    _check(got, base, _rect_want(shape), _tol, (shape, f"stream={mode}", f"compact={compact}"))


@pytest.mark.parametrize("compact", [None, 0], ids=["tables-default", "tables-full"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_rect_tiles_variant_runs_the_instantiation_it_names(O, monkeypatch, mode, compact):
    """Trace of steps + solve + one three-pass Peaceman-Rachford iteration sequence on 128 x 192: every rect_x / rect_y kernel
    carries the STREAM value that serves the mode and the table form asked for, with and without SRC."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    _env(monkeypatch, stream=mode, fine=0, compact=compact)
    shape = (128, 192)
    mask, edges, bcs = _rect_geometry(*shape)
    eng = Engine(compile_geometry(mask, edges, bcs, DX))
    op = DiffusionOperator(eng, len(RECT_DC), DT, dcoef=RECT_DC)
    rng = np.random.default_rng(0)
    u0 = rng.random((len(RECT_DC), shape[0] * shape[1]))

    def calls():
        _steps(eng, op, u0, 2)
        _solve(eng, op, u0)
        _pr_cycles(eng, op, u0, u0, fine=False)
    found = _traced_kernels(calls)
    S, Cf = str(_served(mode)), "false" if compact == 0 else "true"
    for inst in [("rect_y_kernel", ("0", S, Cf, "false")), ("rect_x_kernel", ("true", S, Cf, "false")),
                 ("rect_y_kernel", ("1", S, Cf, "false")), ("rect_y_kernel", ("2", S, Cf, "false")),
                 ("rect_y_kernel", ("3", S, Cf, "false")), ("rect_x_kernel", ("false", S, Cf, "false")),
                 ("rect_y_kernel", ("0", S, Cf, "true")), ("rect_x_kernel", ("true", S, Cf, "true"))]:
        assert inst in found, (inst, sorted(found))
    _assert_only(found, ("rect_x_kernel", "rect_y_kernel"), 1, S)
    _assert_only(found, ("rect_x_kernel", "rect_y_kernel"), 2, Cf)
    assert not any(k[0].startswith("fine_") for k in found), sorted(found)


# ------------------------------------------------------------------------------------------------------------------
# 2. rectangle, fine tiles
# ------------------------------------------------------------------------------------------------------------------
FINE_SHAPES = [(64, 64), (128, 192), (64, 320)]
FINE_DC = [4.4, 0.35, 0.0]          # r D <= 0.30: chunks of 32 cells decouple
FINE_STEPS = (1, 2, 5)


def _fine_reference(O, shape):
    mask, edges, bcs = _rect_geometry(*shape)
    gops = O.build_grid_ops(mask, edges, bcs, DX)
    return (mask, edges, bcs), _reference(O, ("fine", shape), gops, FINE_DC, FINE_STEPS, shape[0] * 7 + shape[1], cn=True)


def _fine_run(mp, O, shape, mode, fused):
    """steps (k = 1, 2, 5) in step form `fused`; with the two-sweep form also `qp_adi_rect_solve` and the Peaceman-Rachford
    cycle, carried and three-pass (neither depends on the step form)."""
    key = ("fine", shape, mode, fused)
    if key in _RUN:
        return _RUN[key]
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    (mask, edges, bcs), ref = _fine_reference(O, shape)
    _env(mp, stream=mode, fine=1, fused=fused)
    eng = Engine(compile_geometry(mask, edges, bcs, DX))
    op = DiffusionOperator(eng, len(FINE_DC), DT, dcoef=FINE_DC)
    assert op.rect is not None and op.rect.fine
    out = {f"steps{k}": _steps(eng, op, ref["u0"], k) for k in FINE_STEPS}
    if fused == 0:
        out["solve"] = _solve(eng, op, ref["x0"])
        for carried in (1, 0):
            mp.setenv("QPSIM_PR_CARRIED", str(carried))
            out[f"pr_carried{carried}_first_cycle"], out[f"pr_carried{carried}"] = _pr_cycles(eng, op, ref["u0"], ref["b"], fine=True)
        mp.delenv("QPSIM_PR_CARRIED")
    _RUN[key] = out
    return out


@pytest.mark.parametrize("fused", [0, 1, 2], ids=["two-sweep", "fused", "one-pass"])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("shape", FINE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fine_tiles_stream_modes_in_every_step_form(O, monkeypatch, shape, mode, fused):
    """`fine_*_kernel<..., STREAM, ...>` at STREAM 2 and 3: bit-equal to the same step form at mode 0; the two-sweep form
    (with the solve and both cycle forms: `fine_y_next_kernel`, the SRC passes) against the oracle; the fused form bit-equal
    to the two-sweep form and the one-pass form within 1e-14 of it (k = 1: bit-equal to the fused form), as at mode 0."""
    base = _fine_run(monkeypatch, O, shape, 0, fused)
    got = _fine_run(monkeypatch, O, shape, mode, fused)
    ctx = (shape, f"stream={mode}", f"fused={fused}")
    want = {}
    if fused == 0:
        w = _REF[("fine", shape)]["want"]
        want = {**{f"steps{k}": w[f"steps{k}"] for k in FINE_STEPS}, "solve": w["solve"], "pr_carried1": w["cn"], "pr_carried0": w["cn"]}
    _check(got, base, want, _tol, ctx)
    if fused:
        plain = _fine_run(monkeypatch, O, shape, mode, 0)
        for k in FINE_STEPS:
            if fused == 1:
                assert np.array_equal(got[f"steps{k}"], plain[f"steps{k}"]), (ctx, k)
            else:
                err = rel_err(got[f"steps{k}"], plain[f"steps{k}"])
                print(f"{ctx} steps{k}: one-pass {err:.2e} from two-sweep (bound {ONEPASS_TOL:.0e})")
                assert err <= ONEPASS_TOL, (ctx, k, err)
        if fused == 2:
            assert np.array_equal(got["steps1"], _fine_run(monkeypatch, O, shape, mode, 1)["steps1"]), ctx


@pytest.mark.parametrize("shape", FINE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fine_tiles_exact_cn_step_at_stream_mode_3(O, monkeypatch, shape):
    """The default scheme as production runs it above 384 MiB (1024^2 x 50 bins): `cn_exact_step` through the carried cycle on
    mode-3 fine plans against the oracle's SuperLU solve, and bit-equal (same cycle length) to mode 0."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    (mask, edges, bcs), ref = _fine_reference(O, shape)
    res = {}
    for mode in (0, 3):
        _env(monkeypatch, stream=mode, fine=1)
        eng = Engine(compile_geometry(mask, edges, bcs, DX))
        op = DiffusionOperator(eng, len(FINE_DC), DT, dcoef=FINE_DC)
        assert op.rect.fine
        a = eng.upload_packed(ref["u0"])
        its = eng.cn_exact_step(op, a)
        cycles = [c for c in op._pr_cycles.values() if c is not None]
        assert cycles and all(p.fine for c in cycles for p in c)      # the carried cycle ran, on fine plans
        res[mode] = (its, _download(eng, a))
    err = rel_err(res[3][1], ref["want"]["cn"])
    print(f"{shape} cn_exact_step at stream mode 3: {err:.2e} from the oracle (bound {CN_TOL:.0e}), {res[3][0]} iterations")
    assert err < CN_TOL, (shape, err)
    assert res[3][0] == res[0][0] and np.array_equal(res[3][1], res[0][1]), (shape, res[3][0], res[0][0])


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_fine_tiles_variant_runs_the_instantiation_it_names(O, monkeypatch, mode):
    """Trace of 3 steps in each step form, the solve and the carried cycle on 128 x 192: every fine kernel that has a STREAM
    template argument carries the value that serves the mode."""
    from qpsim_amd.engine import DiffusionOperator, Engine, compile_geometry
    shape = (128, 192)
    mask, edges, bcs = _rect_geometry(*shape)
    eng = Engine(compile_geometry(mask, edges, bcs, DX))
    ops = []
    for fused in (0, 1, 2):
        _env(monkeypatch, stream=mode, fine=1, fused=fused)
        ops.append(DiffusionOperator(eng, len(FINE_DC), DT, dcoef=FINE_DC))
    _env(monkeypatch, stream=mode, fine=1, carried=1)
    rng = np.random.default_rng(1)
    u0 = rng.random((len(FINE_DC), shape[0] * shape[1]))

    def calls():
        for op in ops:
            _steps(eng, op, u0, 3)
        _solve(eng, ops[0], u0)
        _pr_cycles(eng, ops[0], u0, u0, fine=True)
    found = _traced_kernels(calls)
    S = str(_served(mode))
    for inst in [("fine_y_kernel", ("0", S, "false")), ("fine_x_kernel", ("true", S, "false")), ("fine_y_kernel", ("1", S, "false")),
                 ("fine_y_kernel", ("2", S, "false")), ("fine_y_kernel", ("3", S, "false")), ("fine_x_kernel", ("false", S, "false")),
                 ("fine_reduce_kernel", (S,)), ("fine_fused_kernel", ("1", S)), ("fine_fused_kernel", ("2", S)),
                 ("fine_onepass_kernel", ("1", S)), ("fine_onepass_kernel", ("2", S)), ("fine_ghostsum_kernel", ()),
                 ("fine_y_kernel", ("0", S, "true")), ("fine_x_kernel", ("true", S, "true")), ("fine_y_next_kernel", (S,))]:
        assert inst in found, (inst, sorted(found))
    _assert_only(found, ("fine_x_kernel", "fine_y_kernel", "fine_fused_kernel", "fine_onepass_kernel"), 1, S)
    _assert_only(found, ("fine_reduce_kernel", "fine_y_next_kernel"), 0, S)
    assert not any(k[0] in ("rect_x_kernel", "rect_y_kernel") for k in found), sorted(found)


# ------------------------------------------------------------------------------------------------------------------
# 3. masked grids, one diffusivity per field: unmerged launches, side stream, table forms, stream modes
# ------------------------------------------------------------------------------------------------------------------
MASKED_DC = [6.0, 0.35, 0.0]
MASKED_BASE = dict(stream=0)
MASKED_VARIANTS = {
    "unmerged-stream0": dict(merge=0, stream=0), "unmerged-stream1": dict(merge=0, stream=1),
    "unmerged-stream2": dict(merge=0, stream=2), "unmerged-stream3": dict(merge=0, stream=3),
    "unmerged-full-tables": dict(merge=0, stream=0, compact=0), "unmerged-full-tables-stream2": dict(merge=0, stream=2, compact=0),
    "unmerged-full-tables-stream3": dict(merge=0, stream=3, compact=0), "merged": dict(merge=1, stream=0),
    "unmerged-fork": dict(merge=0, fork=1, stream=0),
}


def _masked_geometry(O, kind):
    """The `donut` (empty, clean and general tiles) and `slab` (a second boundary term on part of the left wall) problems of
    test_gpu_parity.py, the per-cell override of the slab applied to the device geometry and to the oracle's operator alike."""
    from qpsim_amd.engine import compile_geometry
    from test_gpu_parity import _masked_problem
    key = ("masked-geometry", kind)
    if key not in _REF:
        _, mask, edges, bcs = _masked_problem(kind, 11)
        gops = O.build_grid_ops(mask, edges, bcs, DX)
        if kind == "slab":
            gops.e_x[:100, 0] *= 0.5
            gops.s_x[:100, 0] *= 0.25
        _REF[key] = (mask, edges, bcs, gops)
    mask, edges, bcs, gops = _REF[key]
    geom = compile_geometry(mask, edges, bcs, DX)
    if kind == "slab":
        geom.ex[:100, 0] *= 0.5
        geom.sx[:100, 0] *= 0.25
    return mask, geom, gops


def _tile_calls(eng, op, mask, ref):
    """steps (k = 1, 3) and `qp_adi_tile_solve` on the engine's default stream, synchronised before reading; holes stay 0."""
    out = {}
    holes = ~mask.reshape(-1)
    for call, src, run in [("steps1", "u0", lambda t: eng.adi_steps(op, t, 1)), ("steps3", "u0", lambda t: eng.adi_steps(op, t, 3)),
                           ("solve", "x0", lambda t: eng._precondition(op, t))]:
        t = eng.upload_packed(ref[src])
        run(t)
        out[call] = _download(eng, t)
        assert np.all(t.cpu().numpy()[:, holes] == 0.0), (call, "cells outside the mask must stay exactly 0")
    return out


def _masked_run(mp, O, kind, name, knobs):
    key = ("masked", kind, name)
    if key in _RUN:
        return _RUN[key]
    from qpsim_amd.engine import DiffusionOperator, Engine
    mask, geom, gops = _masked_geometry(O, kind)
    ref = _reference(O, ("masked", kind), gops, MASKED_DC, (1, 3), 11, cn=False)
    _env(mp, fine=0, **knobs)
    eng = Engine(geom)
    op = DiffusionOperator(eng, len(MASKED_DC), DT, dcoef=MASKED_DC)
    assert op.rect is None and op.tile is not None, op.tile_refused
    counts = op.tile.tile_counts
    assert counts["clean"] > 0 and counts["general"] > 0 and (kind != "donut" or counts["empty"] > 0), counts
    _RUN[key] = _tile_calls(eng, op, mask, ref)
    return _RUN[key]


@pytest.mark.parametrize("variant", list(MASKED_VARIANTS))
@pytest.mark.parametrize("kind", ["donut", "slab"])
def test_masked_tiles_launch_forms_stream_modes_and_table_forms(O, monkeypatch, kind, variant):
    """The clean-tile kernels `tile_x_kernel<0, ...>` / `tile_y_kernel<0, ...>` launched on their own (what a ring in 4096^2
    with four bins runs), at every stream mode (general tiles: the run-time branch of STREAM = -1), with full tables, with the
    general tiles on the side stream - and the merged launch pinned as the base: oracle, bit-equality, holes exactly 0."""
    base = _masked_run(monkeypatch, O, kind, "base", MASKED_BASE)
    got = _masked_run(monkeypatch, O, kind, variant, MASKED_VARIANTS[variant])
    _check(got, base, _REF[("masked", kind)]["want"], _tol, (kind, variant))


@pytest.mark.parametrize("variant", ["base"] + list(MASKED_VARIANTS))
def test_masked_tiles_variant_runs_the_launches_it_names(O, monkeypatch, variant):
    """Trace of 2 steps + the solve on the donut: merged plans launch `tile_*_merged_kernel` alone; unmerged plans launch
    `tile_*_kernel<0, ..., STREAM, COMPACT>` and `tile_*_kernel<1, ..., -1, false>` and no merged kernel - with fork on, too."""
    from qpsim_amd.engine import DiffusionOperator, Engine
    knobs = MASKED_BASE if variant == "base" else MASKED_VARIANTS[variant]
    mask, geom, _ = _masked_geometry(O, "donut")
    _env(monkeypatch, fine=0, **knobs)
    eng = Engine(geom)
    op = DiffusionOperator(eng, len(MASKED_DC), DT, dcoef=MASKED_DC)
    u0 = np.random.default_rng(2).random((len(MASKED_DC), int(mask.sum())))

    def calls():
        _steps(eng, op, u0, 2)
        _solve(eng, op, u0)
    found = _traced_kernels(calls)
    names = {k[0] for k in found}
    if knobs.get("merge", 1) != 0:
        for inst in [("tile_y_merged_kernel", ("0",)), ("tile_x_merged_kernel", ("true",)), ("tile_y_merged_kernel", ("1",)),
                     ("tile_y_merged_kernel", ("2",)), ("tile_y_merged_kernel", ("3",)), ("tile_x_merged_kernel", ("false",))]:
            assert inst in found, (inst, sorted(found))
        assert "tile_x_kernel" not in names and "tile_y_kernel" not in names, sorted(found)
        return
    assert "tile_x_merged_kernel" not in names and "tile_y_merged_kernel" not in names, sorted(found)
    S, Cf = str(_served(knobs["stream"])), "false" if knobs.get("compact") == 0 else "true"
    for mode, explicit in (("0", None), ("1", "true"), ("2", None), ("3", "false")):
        for cls, s, c in (("0", S, Cf), ("1", "-1", "false")):
            assert ("tile_y_kernel", (cls, mode, s, c)) in found, (cls, mode, sorted(found))
            if explicit:
                assert ("tile_x_kernel", (cls, explicit, s, c)) in found, (cls, explicit, sorted(found))
    clean = {k for k in found if k[0] in ("tile_x_kernel", "tile_y_kernel") and k[1][0] == "0"}
    _assert_only(clean, ("tile_x_kernel", "tile_y_kernel"), 2, S)
    _assert_only(clean, ("tile_x_kernel", "tile_y_kernel"), 3, Cf)


# ------------------------------------------------------------------------------------------------------------------
# 4. masked grids, one diffusivity per cell: STREAM = -1, the run-time branch of load_cols / store_cols
# ------------------------------------------------------------------------------------------------------------------
def _var_run(mp, O, mode):
    key = ("var", mode)
    if key in _RUN:
        return _RUN[key]
    from qpsim_amd.engine import DiffusionOperator, Engine
    mask, geom, gops = _masked_geometry(O, "donut")
    n, B = int(mask.sum()), 3
    if ("var-D",) not in _REF:
        rng = np.random.default_rng(17)
        Dp = 0.2 + 5.8 * rng.random((B, n))
        Dp[2] *= 0.05                                   # a nearly frozen bin, as in test_tile_path_variable_diffusivity_...
        _REF[("var-D",)] = Dp
    Dp = _REF[("var-D",)]
    planes = []
    for k in range(B):
        Dg = np.zeros(mask.shape)
        Dg[mask] = Dp[k]
        planes.append(Dg)
    ref = _reference(O, ("var",), gops, planes, (1, 3), 18, cn=False)
    _env(mp, stream=mode, fine=0)
    eng = Engine(geom)
    op = DiffusionOperator(eng, B, DT, dfield=np.stack([p.reshape(-1) for p in planes]))
    assert op.rect is None and op.tile is not None, op.tile_refused
    assert op.tile.tile_counts["clean"] == 0 and op.tile.tile_counts["general"] > 0
    _RUN[key] = _tile_calls(eng, op, mask, ref)
    return _RUN[key]


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_masked_tiles_variable_diffusivity_stream_modes(O, monkeypatch, mode):
    """Per-cell D on the donut: every tile runs `tile_*_kernel<2, ..., -1>`, which takes the plan's stream mode at run time
    (so its name cannot show the mode: the oracle and the bit-equality carry this case)."""
    base = _var_run(monkeypatch, O, 0)
    got = _var_run(monkeypatch, O, mode)
    _check(got, base, _REF[("var",)]["want"], _tol, ("variable D", f"stream={mode}"))


# ------------------------------------------------------------------------------------------------------------------
# 5. decomposed blocks at stream mode 3 (what every rank of a multi-bin run gets: >= 384 MiB per block)
# ------------------------------------------------------------------------------------------------------------------
def _blocks_run(mp, scheme, mode, trace=False):
    import torch
    from qpsim_amd.distributed import (BlockTopology, HipBlockBackend, HipOverlapBlock, lockstep_adi_steps,
                                       lockstep_overlap_steps)
    from test_distributed_cpu import _oracle_steps, _problem
    py, px, gny, gnx = (2, 2, 128, 240) if scheme == "exact" else (2, 2, 192, 256)
    mask, edges, bcs, dx, dt, D, bc_diag, bc_src, u0 = _problem(gny, gnx)
    if ("blocks", scheme) not in _REF:
        _REF[("blocks", scheme)] = _oracle_steps(mask, edges, bcs, dx, dt, D, u0, 3)
    _env(mp, stream=mode, fine=0)
    topos = [BlockTopology(gny, gnx, py, px, r) for r in range(py * px)]
    if scheme == "exact":
        blocks = [HipBlockBackend(t, dx, dt, D, bc_diag, bc_src) for t in topos]
        run = lambda: lockstep_adi_steps(blocks, topos, 3)  # noqa: E731
    else:
        blocks = [HipOverlapBlock(t, dx, dt, D, bc_diag, bc_src, steps_per_exchange=2) for t in topos]   # one refresh in 3 steps
        run = lambda: lockstep_overlap_steps(blocks, 3)  # noqa: E731
    for b in blocks:
        b.set_field(u0)
    found = _traced_kernels(run) if trace else run()
    torch.cuda.synchronize()
    got = np.zeros_like(u0)
    for b, t in zip(blocks, topos):
        j0, i0, ny, nx = t.block
        got[:, j0:j0 + ny, i0:i0 + nx] = b.get_field()
    return got, found


@pytest.mark.parametrize("scheme", ["exact", "overlap"])
def test_decomposed_blocks_at_stream_mode_3(monkeypatch, scheme):
    """2 x 2 blocks of 128 x 240 driven phase by phase (`HipBlockBackend`, interface rows exchanged) and of 192 x 256 with
    overlapped halos (`HipOverlapBlock`), 3 lock-step steps, plans built at mode 3: bit-equal to mode 0, 2e-13 from the oracle,
    and every tile kernel of the trace is a `<*, 3, ...>` instantiation."""
    base, _ = _blocks_run(monkeypatch, scheme, 0)
    got, found = _blocks_run(monkeypatch, scheme, 3, trace=True)
    want = _REF[("blocks", scheme)]
    assert np.array_equal(got, base), (scheme, float(np.max(np.abs(got - base))))
    err = rel_err(got, want)
    print(f"{scheme} blocks at stream mode 3: {err:.2e} from the oracle (bound {ADI_TOL:.0e})")
    assert err < ADI_TOL, (scheme, err)
    ran = {(k[0],) + k[1][:2] for k in found}       # (the table form follows the ragged extents of the blocks)
    for inst in [("rect_y_kernel", "0", "3"), ("rect_x_kernel", "true", "3"), ("rect_y_kernel", "1", "3"), ("rect_y_kernel", "2", "3")]:
        assert inst in ran, (inst, sorted(found))
    _assert_only(found, ("rect_x_kernel", "rect_y_kernel"), 1, "3")
