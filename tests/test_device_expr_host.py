"""Host compiler of custom generation expressions (``qpsim_amd.device_expr``) and the evaluator it feeds, run on the CPU
through the test hook ``qp_expr_eval_host`` (the same ``__host__ __device__`` function the kernel runs): no GPU needed.

Two parity classes.  Exact: arithmetic, sqrt, abs, max / min / clip / where / heaviside, comparisons and the four special
powers are bit-equal to the host path (``solver._CustomGeneration``).  Approximate: pow and the transcendental functions
are bounded against an ``np.longdouble`` truth by K_dev <= 4 K_np + 4 ulp, K_np being NumPy's own error against the same
truth (the rule of tests/test_gpu_collision_elementwise.py)."""
from __future__ import annotations

import numpy as np
import pytest

import generation_expr_cases as G

HAVE_X87 = np.finfo(np.longdouble).nmant >= 63
needs_x87 = pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()


ACCEPTED = [("1e-6*(1.0+x)*t", {}), ('np.exp(-((x-0.5)**2+(y-0.5)**2)/params["w"])', {"w": 0.02}), ("(x>0.3)*(x<0.6)*1e-6", {}),
            ("np.where(y<0.5, 1e-6, 0.0)*(1.0 if t<0.35 else 0.0)", {}), ("1e-6*E/(1.0+x)", {}),
            ("return 1e-6 * (1.0 + x) * t", {})]
REFUSED = [("x.size*1e-9", {}, "not elementwise"), ("1e-6 if x<0.5 else 0.0", {}, "not elementwise"),
           ("math.sin(x)", {}, "not elementwise"), ("x//0.1", {}, "FloorDiv"),
           ("(x>0.5)+(y>0.5)", {}, "only accepted as the condition of np.where or as an operand of *"),
           ('params["w"]*x', {"w": np.array([1.0, 2.0])}, "params['w'] is not a real scalar"),
           ("x%0.5", {}, "Mod"), ("np.arange(x)", {}, "not elementwise"), ("np.zeros_like(x)", {}, "not elementwise"),
           ("np.clip(x, a_min=0.2, a_max=0.4)", {}, "keyword"), ("__import__('os').getcwd()", {}, "not a valid custom expression"),
           ("+".join(f"{k}.5*x" for k in range(20)), {}, "more than 16 host-evaluated"),
           ("(x*y)+(" * 9 + "x*y" + ")" * 9, {}, "more than 8 live temporaries"),
           ("+".join(["x*y"] * 40), {}, "more than 64 instructions")]


@pytest.mark.parametrize("body,params", ACCEPTED)
def test_accepted(body, params):
    from qpsim_amd import device_expr as D
    assert D.explain(body, params) == ""
    prog = D.compile_program(body, params)
    words = prog.instructions_for(0.1)
    assert words.dtype == np.uint32 and 1 <= words.size <= D.MAX_WORDS and prog.nslot <= D.MAX_SLOTS
    assert prog.slot_table(G.E_BINS[3], 0.1).shape == (3, prog.nslot)


@pytest.mark.parametrize("body,params,reason", REFUSED)
def test_refused_with_reason(body, params, reason):
    from qpsim_amd import device_expr as D
    assert D.compile_program(body, params) is None
    assert reason in D.explain(body, params)


def test_split_keeps_python_semantics_in_slots():
    """What names neither x nor y is a slot evaluated by the sandbox: no instruction is spent on it."""
    from qpsim_amd import device_expr as D
    prog = D.compile_program("math.sin(t)*params['a']**3/(1+E)*x", {"a": 2})
    assert prog.slot_sources == ["math.sin(t) * params['a'] ** 3 / (1 + E)"]
    assert [D.OPS[int(w) & 0xff] for w in prog.instructions_for(0.2)] == ["mul"]
    table = prog.slot_table(np.array([1.0, 3.0]), 0.2)
    import math
    assert np.array_equal(table[:, 0], math.sin(0.2) * 2 ** 3 / (1 + np.array([1.0, 3.0])))


def test_special_powers_follow_the_exponent_of_the_step():
    from qpsim_amd import device_expr as D
    prog = D.compile_program("x**(2 if t<0.35 else 2.5)+y**E", {})
    ops = lambda t: [D.OPS[int(w) & 0xff] for w in prog.instructions_for(t)]       # noqa: E731
    assert ops(0.3) == ["square", "pow", "add"] and ops(0.4) == ["pow", "pow", "add"]
    assert not prog.is_exact_at(0.3)
    for exponent, op in ((2, "square"), (0.5, "sqrt"), (-1, "recip"), (1, "copy"), (3, "pow"), (-2.0, "pow")):
        prog = D.compile_program("np.power(x, params['p'])", {"p": exponent})
        assert [D.OPS[int(w) & 0xff] for w in prog.instructions_for(0.0)] == [op]
        assert prog.is_exact_at(0.0) == (op != "pow")


def test_a_slot_that_is_no_real_scalar_refuses_the_step():
    from qpsim_amd import device_expr as D
    E = G.E_BINS[3]
    assert D.compile_program("x*params[t]", {0.1: 2.0, 0.2: [1.0, 2.0], 0.3: 2 ** 60, 0.4: 1j}).slot_table(E, 0.1) is not None
    for t in (0.2, 0.3, 0.4, 0.5):                                # a list, an int above 2^53, a complex, a KeyError
        assert D.compile_program("x*params[t]", {0.1: 2.0, 0.2: [1.0, 2.0], 0.3: 2 ** 60, 0.4: 1j}).slot_table(E, t) is None
    # np.where over two integer slots is an integer array in NumPy: left to the host path
    assert D.compile_program("np.where(x<0.5, 1, 2)/3", {}).slot_table(E, 0.0) is None
    assert D.compile_program("np.where(x<0.5, 1.0, 2)/3", {}).slot_table(E, 0.0) is not None


def test_library_rejects_malformed_programs():
    """Every word is checked before anything runs: unknown op, unwritten register, slot beyond the table, struct size."""
    import ctypes as C
    from qpsim_amd import _hip
    from qpsim_amd import device_expr as D
    lib = _hip.load()
    out = np.zeros(4)
    slots = np.zeros(1)

    def call(words, nslot=1, **over):
        words = np.asarray(words, dtype=np.uint32)
        prog = _hip.GenerationProgram.make(2, 2, 2, 2, 0, 0, 1, nslot, words.size, words.ctypes.data, slots.ctypes.data)
        for key, value in over.items():
            setattr(prog, key, value)
        return lib.qp_expr_eval_host(C.byref(prog), out.ctypes.data)

    word = lambda op, dst, a, b=0, c=0: D.OP[op] | dst << 8 | a << 12 | b << 18 | c << 24      # noqa: E731
    assert call([word("add", 0, D.OPERAND_X, D.OPERAND_SLOT0)]) == 0
    assert call([200]) == -1 and b"unknown op" in lib.qp_last_error()
    assert call([word("add", 0, 3, D.OPERAND_X)]) == -1 and b"unwritten register" in lib.qp_last_error()
    assert call([word("add", 0, D.OPERAND_X, D.OPERAND_SLOT0 + 1)]) == -1
    assert call([word("copy", 9, D.OPERAND_X)]) == -1
    assert call([word("copy", 0, 12)]) == -1
    assert call([word("copy", 0, D.OPERAND_X)], struct_size=8) == -1 and b"struct_size" in lib.qp_last_error()
    assert call([word("copy", 0, D.OPERAND_X)], nword=65) == -1
    assert call([word("copy", 0, D.OPERAND_X)], row0=1) == -1 and b"full mask" in lib.qp_last_error()
    assert lib.qp_add_generation_expr(None, 0, 1, 0, 1, 0, 0.1, 0, 0) == -1


@pytest.mark.parametrize("ne", [3, 12])
@pytest.mark.parametrize("grid", sorted(G.GRIDS))
@pytest.mark.parametrize("case", range(len(G.EXACT)))
def test_exact_class_is_bit_equal_to_the_host_path(case, grid, ne):
    body, params = G.EXACT[case]
    mask, E = G.GRIDS[grid], G.E_BINS[ne]
    for t in G.T_VALUES:
        prog, _, _ = G.compiled(body, params, E, t)
        assert prog.is_exact_at(t)
        assert G.bits_equal(G.host_hook(body, params, mask, E, t), G.numpy_reference(body, params, mask, E, t)), (body, t)


def test_nan_propagates_through_maximum_and_minimum():
    body = "np.maximum(x, np.sqrt(x-0.5))+np.minimum(np.sqrt(y-0.5), y)"
    mask, E = G.GRIDS["full_6x10"], G.E_BINS[3]
    got, ref = G.host_hook(body, {}, mask, E, 0.0), G.numpy_reference(body, {}, mask, E, 0.0)
    assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert G.bits_equal(got, ref)


def _k_values(body, truth_of, mask, E, evaluate):
    """(K_dev, K_np): errors in ulp of ``evaluate`` and of NumPy against the np.longdouble truth of ``body``."""
    truth = truth_of(mask, E)
    k_dev = G.ulp_error(evaluate(body, {}, mask, E, 0.0), truth)
    k_np = G.ulp_error(G.numpy_reference(body, {}, mask, E, 0.0), truth)
    return k_dev, k_np


def function_truth(name, arg):
    """np.longdouble value of ``name(arg)`` on the fp64 argument that both NumPy and the evaluator compute exactly."""
    return lambda mask, E: G.long_function(name)(G.numpy_reference(arg, {}, mask, E, 0.0).astype(np.longdouble))


def power_truth(base, exponent):
    return lambda mask, E: np.power(G.numpy_reference(base, {}, mask, E, 0.0).astype(np.longdouble), np.longdouble(exponent))


@needs_x87
@pytest.mark.parametrize("name,arg,span", G.APPROXIMATE)
def test_approximate_class_one_function(name, arg, span):
    mask, E = G.GRIDS["full_17x31"], G.E_BINS[3]
    a = G.numpy_reference(arg, {}, mask, E, 0.0)
    assert G.bits_equal(G.host_hook(arg, {}, mask, E, 0.0), a)      # the argument itself is of the exact class
    assert span[0] <= a.min() and a.max() <= span[1]
    k_dev, k_np = _k_values(f"{name}({arg})", function_truth(name, arg), mask, E, G.host_hook)
    print(f"{name} on [{span[0]}, {span[1]}]: K_dev {k_dev:.3f} ulp, K_np {k_np:.3f} ulp")
    assert k_dev <= G.limit(k_np)


@needs_x87
@pytest.mark.parametrize("body,base,exponent", G.POWERS)
def test_approximate_class_general_power(body, base, exponent):
    mask, E = G.GRIDS["full_17x31"], G.E_BINS[3]
    k_dev, k_np = _k_values(body, power_truth(base, exponent), mask, E, G.host_hook)
    print(f"{body}: K_dev {k_dev:.3f} ulp, K_np {k_np:.3f} ulp")
    assert k_dev <= G.limit(k_np)


def product_bound_and_error(evaluate):
    """(relative error of the product of ``G.PRODUCT`` in units of eps, its bound).  Factor f is off by at most
    4 K_np,f + 4 ulp (the rule above), an ulp is at most eps relative, each of the k - 1 multiplications rounds once
    (eps / 2 each), and the truth is rounded nowhere: sum_f (4 K_np,f + 4) + k covers it to first order with room left."""
    mask, E = G.GRIDS["full_17x31"], G.E_BINS[3]
    truth, bound = np.longdouble(1.0), float(len(G.PRODUCT))
    for name, arg, _ in G.PRODUCT:
        factor = function_truth(name, arg)(mask, E)
        bound += G.limit(G.ulp_error(G.numpy_reference(f"{name}({arg})", {}, mask, E, 0.0), factor))
        truth = truth * factor
    body = "*".join(f"{name}({arg})" for name, arg, _ in G.PRODUCT)
    got = evaluate(body, {}, mask, E, 0.0).astype(np.longdouble)
    return float(np.max(np.abs(got - truth) / np.abs(truth))) / G.EPS, bound


@needs_x87
def test_product_of_approximate_factors():
    error, bound = product_bound_and_error(G.host_hook)
    print(f"product of {len(G.PRODUCT)} factors: {error:.3f} eps, bound {bound:.3f} eps")
    assert error <= bound
