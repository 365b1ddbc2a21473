"""Shared cases of the device-evaluated custom generation tests (host hook and GPU): grids, bodies, the NumPy reference,
the extended-precision truth of the approximate class and the call of ``qp_expr_eval_host``."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

EPS = float(np.finfo(np.float64).eps)
T_VALUES = (0.3, 0.4)                    # either side of the `t < 0.35` slots below
E_BINS = {3: np.linspace(180.0, 540.0, 3), 12: np.linspace(181.5, 538.25, 12)}


def _framed_9x11():
    mask = np.zeros((9, 11), dtype=bool)
    mask[1:-1, 1:-1] = True              # one-cell empty frame: the device grid is 7 x 9 at offset (1, 1)
    mask[3:5, 4:6] = False               # holes inside
    mask[6, 2] = False
    return mask


GRIDS = {"full_6x10": np.ones((6, 10), dtype=bool), "framed_9x11": _framed_9x11(), "full_17x31": np.ones((17, 31), dtype=bool)}

# (body, params): every op of the exact class, the four special powers (literal, through params, through np.power, switched
# by t), comparisons as factors and as np.where conditions, slots in E, t and params, a body without x and y
EXACT = [
    ("1e-6*(1.0+x)*t", {}),
    ("(x>0.3)*(x<0.6)*1e-6", {}),
    ("np.where(y<0.5, 1e-6, 0.0)*(1.0 if t<0.35 else 0.0)", {}),
    ("1e-6*E/(1.0+x)", {}),
    ("np.sqrt(x*y)+np.abs(x-0.5)/(y+0.25)", {}),
    ("np.maximum(x,y)-np.minimum(x,0.3)+np.clip(y,0.2,0.7)*params.get('s', 2.0)", {"s": 1.75}),
    ("np.heaviside(x-0.5, 0.5)*params['a']+np.heaviside(x-x, 0.25)+(x==y)*2.0+(x!=y)*(x>=0.5)*(y<=0.5)*1.5", {"a": 3e-7}),
    ("(x-0.5)**2+y**0.5+(1.0+x)**-1+y**1+np.power(x,2)+np.power(y+1.0,params['p'])", {"p": -1}),
    ("x**(2 if t<0.35 else 0.5)*math.exp(-t)*E", {}),
    ("-x*E*1e-9+ +y", {}),
    ("1e-6*t*np.sqrt(E)", {}),
    ("np.where((x>0.25)*(y<=0.75), x/y, -y)", {}),
]
# one function per case on an argument of the exact class: (function, argument body, range it covers on the unit square);
# the ranges keep every function well conditioned (away from the zeros of cos, the poles of tan, |a| = 1 of arcsin / arccos,
# a = 1 of log)
APPROXIMATE = [
    ("np.exp", "6.0*x*y-3.0", (-3.0, 3.0)),
    ("np.log", "1.5+3.0*x*y", (1.5, 4.5)),
    ("np.log10", "1.5+3.0*x*y", (1.5, 4.5)),
    ("np.sin", "3.0*x*y-1.5", (-1.5, 1.5)),
    ("np.cos", "2.4*x*y-1.2", (-1.2, 1.2)),
    ("np.tan", "2.4*x*y-1.2", (-1.2, 1.2)),
    ("np.arcsin", "1.8*x*y-0.9", (-0.9, 0.9)),
    ("np.arccos", "1.8*x*y-0.9", (-0.9, 0.9)),
    ("np.arctan", "6.0*x*y-3.0", (-3.0, 3.0)),
    ("np.sinh", "6.0*x*y-3.0", (-3.0, 3.0)),
    ("np.cosh", "6.0*x*y-3.0", (-3.0, 3.0)),
    ("np.tanh", "6.0*x*y-3.0", (-3.0, 3.0)),
]
# general powers: (body, base body, exponent)
POWERS = [("(0.5+x*y)**2.5", "0.5+x*y", 2.5), ("np.power(1.0+x*y, -1.7)", "1.0+x*y", -1.7)]
# a product of k factors with one approximate call each
PRODUCT = [APPROXIMATE[0], APPROXIMATE[3], APPROXIMATE[10]]


def window(mask):
    """(device mask, (ny_full, nx_full, row0, col0)) of the bounding-box crop the solver applies."""
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    r0, c0 = int(rows[0]), int(cols[0])
    return np.ascontiguousarray(mask[r0:int(rows[-1]) + 1, c0:int(cols[-1]) + 1]), mask.shape + (r0, c0)


def compiled(body, params, E_bins, t):
    """(program, words, slot table) of ``body`` at ``t``; asserts that the device takes it."""
    from qpsim_amd import device_expr as D
    assert D.explain(body, params) == "", D.explain(body, params)
    prog = D.compile_program(body, params)
    words, table = prog.instructions_for(t), prog.slot_table(E_bins, t)
    assert words is not None and table is not None
    return prog, words, table


def numpy_reference(body, params, mask, E_bins, t):
    """[NE, n] of the host path (``solver._CustomGeneration``), warnings of its divisions silenced."""
    from qpsim_amd.models import ExternalGenerationSpec
    from qpsim_amd.solver import _CustomGeneration
    spec = ExternalGenerationSpec(mode="custom", custom_body=body, custom_params=dict(params))
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return _CustomGeneration(spec, mask)(E_bins, t, int(mask.sum()))


def host_hook(body, params, mask, E_bins, t):
    """[NE, n] of ``qp_expr_eval_host`` on the interior cells of ``mask`` (packed as the reference packs them)."""
    from qpsim_amd import _hip
    lib = _hip.load()
    _, words, table = compiled(body, params, E_bins, t)
    dev_mask, (ny_full, nx_full, r0, c0) = window(mask)
    ny, nx = dev_mask.shape
    table = np.ascontiguousarray(table, dtype=np.float64)
    prog = _hip.GenerationProgram.make(ny, nx, ny_full, nx_full, r0, c0, len(E_bins), table.shape[1], words.size,
                                       words.ctypes.data, table.ctypes.data if table.size else 0)
    out = np.full((len(E_bins), ny * nx), np.nan)
    _hip.check(lib.qp_expr_eval_host(C.byref(prog), out.ctypes.data), "qp_expr_eval_host")
    return out[:, dev_mask.reshape(-1)]


def bits_equal(a, b) -> bool:
    """Same doubles bit for bit, except that any NaN equals any NaN (payload and sign of a NaN are not values)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))


def ulp_error(got, truth) -> float:
    """max |got - truth| in units of the fp64 spacing at |truth| (``truth`` in np.longdouble)."""
    truth = np.asarray(truth, dtype=np.longdouble)
    spacing = np.spacing(np.abs(truth).astype(np.float64)).astype(np.longdouble)
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - truth) / spacing))


def long_function(name):
    return getattr(np, name.split(".")[1])


def limit(k_np: float) -> float:
    """The rule of tests/test_gpu_collision_elementwise.py: 4 K_ref + 4."""
    return 4.0 * k_np + 4.0
