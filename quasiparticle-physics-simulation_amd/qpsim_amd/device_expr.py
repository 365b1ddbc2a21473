"""Host compiler of custom expressions g(E, x, y, t, params) for the device evaluator (pure Python, no GPU).

``compile_program(body, params)`` splits a validated expression between host and device.  Every maximal sub-expression
that names neither ``x`` nor ``y`` is a *slot*: it keeps its exact Python / NumPy semantics, is evaluated by the existing
sandbox (``safe_eval.compile_safe_expression``) once per step for all energy bins and reaches the kernel as a table
``slots[NE][nslot]`` of doubles.  Only what mixes ``x``, ``y`` with slots becomes a register program for
``qp_add_generation_expr`` (``include/qpsim_hip.h``).  Whatever the device cannot serve is refused - ``compile_program``
returns None, ``explain`` says why - and the caller keeps the host path.

Limits (the header's ``QP_EXPR_MAX_*``): 64 instruction words, 8 live temporaries, 16 slots.

Slots are evaluated the way the host path evaluates them inside the whole expression: with ``E`` the column of all energy
bins (``_CustomGeneration._on_grid``).  The precondition ``expression_is_elementwise`` guarantees that ``E`` is only used
element by element, so the values are the ones the host path computes, bit for bit; a slot that raises there, or that does
not come out as real scalars, refuses the step.

The instruction words are produced per step because ``**`` follows NumPy: an exponent slot that does not depend on ``E`` and
is exactly 2, 0.5, -1 or 1 at this step becomes square, sqrt, reciprocal or copy (``x**2 == x*x`` etc. bit for bit in
NumPy, also through ``np.power``); every other exponent is a general ``pow``.

The module is written for generation expressions; nothing in it is specific to them beyond the variable names, so
initial-condition and gap expressions can follow.
"""
from __future__ import annotations

import ast

import numpy as np

from .safe_eval import _strip_return, compile_safe_expression, expression_is_elementwise

MAX_WORDS, MAX_REGS, MAX_SLOTS = 64, 8, 16
OPERAND_X, OPERAND_Y, OPERAND_SLOT0 = 8, 9, 16
VARIABLES = ("E", "x", "y", "t", "params")

# qp_expr_op of include/qpsim_hip.h, in its order
OPS = ("copy neg add sub mul div pow square sqrt recip abs max min where heaviside lt le gt ge eq ne exp log log10 sin cos "
       "tan asin acos atan sinh cosh tanh").split()
OP = {name: code for code, name in enumerate(OPS)}
# ops whose device result is bit-equal to NumPy's (the exact class); the rest is bounded in ulp (the approximate class)
EXACT_OPS = frozenset(OPS[:OP["exp"]]) - {"pow"}

_BINOPS = {ast.Add: "add", ast.Sub: "sub", ast.Mult: "mul", ast.Div: "div", ast.Pow: "pow"}
_COMPARES = {ast.Lt: "lt", ast.LtE: "le", ast.Gt: "gt", ast.GtE: "ge", ast.Eq: "eq", ast.NotEq: "ne"}
_NP_UNARY = {"abs": "abs", "sqrt": "sqrt", "exp": "exp", "log": "log", "log10": "log10", "sin": "sin", "cos": "cos",
             "tan": "tan", "arcsin": "asin", "arccos": "acos", "arctan": "atan", "sinh": "sinh", "cosh": "cosh",
             "tanh": "tanh"}
_NP_BINARY = {"maximum": "max", "minimum": "min", "power": "pow", "heaviside": "heaviside"}
_SPECIAL_POWERS = {2.0: "square", 0.5: "sqrt", -1.0: "recip", 1.0: "copy"}

_STATS = {"device_steps": 0, "host_steps": 0}


def last_run_stats() -> dict:
    """``{"device_steps": .., "host_steps": ..}`` of the last run / ensemble call on this process: member-steps whose
    custom generation the device evaluated, and member-steps evaluated on the host."""
    return dict(_STATS)


def reset_run_stats() -> None:
    _STATS.update(device_steps=0, host_steps=0)


def count_steps(device: int = 0, host: int = 0) -> None:
    _STATS["device_steps"] += device
    _STATS["host_steps"] += host


class Refused(Exception):
    """The expression is outside the device subset (the message is the reason ``explain`` reports)."""


def _touches_xy(node: ast.AST) -> bool:
    return any(isinstance(n, ast.Name) and n.id in ("x", "y") for n in ast.walk(node))


def _names(node: ast.AST, name: str) -> bool:
    return any(isinstance(n, ast.Name) and n.id == name for n in ast.walk(node))


def _is_real_scalar(v) -> bool:
    return isinstance(v, (bool, int, float, np.bool_, np.integer, np.floating)) and not isinstance(v, complex)


class _Builder:
    """Walks the AST once: slots for what names neither x nor y, instructions for the rest.

    An instruction is ``[op, dst, a, b, c]`` with operands already encoded; a ``pow`` keeps its exponent slot so that
    ``Program.instructions_for`` can specialise it.  A value is ``(operand, is_bool)``: comparisons (and products of
    comparisons) are boolean in NumPy and only multiply or select."""

    def __init__(self):
        self.slot_sources: list[str] = []
        self.slot_nodes: list[ast.AST] = []
        self.code: list[list] = []
        self.free = list(range(MAX_REGS))
        self.int_guards: list[tuple[int, int]] = []      # np.where branches that must not both be integers

    # -- operands ---------------------------------------------------------------------------------------------
    def slot(self, node: ast.AST) -> int:
        source = ast.unparse(node)
        if source in self.slot_sources:
            return OPERAND_SLOT0 + self.slot_sources.index(source)
        if len(self.slot_sources) >= MAX_SLOTS:
            raise Refused(f"more than {MAX_SLOTS} host-evaluated sub-expressions")
        self.slot_sources.append(source)
        self.slot_nodes.append(node)
        return OPERAND_SLOT0 + len(self.slot_sources) - 1

    def release(self, operand: int) -> None:
        if operand < MAX_REGS:
            self.free.insert(0, operand)

    def emit(self, op: str, a: int, b=None, c=None, pow_slot=None) -> int:
        for operand in (a, b, c):
            if operand is not None:
                self.release(operand)
        b, c = b or 0, c or 0                                    # an operand the op does not read is encoded as 0
        if not self.free:
            raise Refused(f"more than {MAX_REGS} live temporaries")
        if len(self.code) >= MAX_WORDS:
            raise Refused(f"more than {MAX_WORDS} instructions")
        dst = self.free.pop(0)
        self.code.append([op, dst, a, b, c, pow_slot])
        return dst

    # -- nodes ------------------------------------------------------------------------------------------------
    def value(self, node: ast.AST, *, boolean_ok: bool = False):
        operand, is_bool = self._value(node)
        if is_bool and not boolean_ok:
            raise Refused("a comparison of x or y is only accepted as the condition of np.where or as an operand of *")
        return operand, is_bool

    def number(self, node: ast.AST) -> int:
        return self.value(node)[0]

    def _value(self, node: ast.AST):
        if not _touches_xy(node):
            return self.slot(node), False
        if isinstance(node, ast.Name):
            return (OPERAND_X if node.id == "x" else OPERAND_Y), False
        if isinstance(node, ast.UnaryOp):
            if isinstance(node.op, ast.UAdd):
                return self.number(node.operand), False
            if isinstance(node.op, ast.USub):
                return self.emit("neg", self.number(node.operand)), False
            raise Refused(f"unary operator {type(node.op).__name__} on x or y")
        if isinstance(node, ast.BinOp):
            op = _BINOPS.get(type(node.op))
            if op is None:
                raise Refused(f"operator {type(node.op).__name__} on x or y (only + - * / ** run on the device)")
            if op == "mul":
                (a, a_bool), (b, b_bool) = self.value(node.left, boolean_ok=True), self.value(node.right, boolean_ok=True)
                return self.emit("mul", a, b), a_bool and b_bool
            if op == "pow":
                return self.power(node.left, node.right), False
            a = self.number(node.left)
            return self.emit(op, a, self.number(node.right)), False
        if isinstance(node, ast.Compare):
            if len(node.ops) != 1:
                raise Refused("chained comparison of x or y")
            op = _COMPARES.get(type(node.ops[0]))
            if op is None:
                raise Refused(f"comparison {type(node.ops[0]).__name__} on x or y")
            a = self.number(node.left)
            return self.emit(op, a, self.number(node.comparators[0])), True
        if isinstance(node, ast.Call):
            return self.call(node), False
        if isinstance(node, ast.IfExp):
            raise Refused("a conditional expression on x or y (use np.where)")
        raise Refused(f"{type(node).__name__} on x or y")

    def power(self, base: ast.AST, exponent: ast.AST) -> int:
        a = self.number(base)
        b = self.number(exponent)
        # only an exponent that is one number for all bins can take NumPy's scalar fast paths
        special = b if (b >= OPERAND_SLOT0 and not _names(self.slot_nodes[b - OPERAND_SLOT0], "E")) else None
        return self.emit("pow", a, b, pow_slot=special)

    def call(self, node: ast.Call) -> int:
        if node.keywords:
            raise Refused("keyword arguments in a call on x or y")
        fn = node.func
        if isinstance(fn, ast.Name) and fn.id == "abs" and len(node.args) == 1:
            return self.emit("abs", self.number(node.args[0]))
        if not (isinstance(fn, ast.Attribute) and isinstance(fn.value, ast.Name) and fn.value.id == "np"):
            name = ast.unparse(fn)
            raise Refused(f"{name}() on x or y (only np.* functions run on the device)")
        name, args = fn.attr, node.args
        if any(isinstance(a, ast.Starred) for a in args):
            raise Refused("starred arguments in a call on x or y")
        if name in _NP_UNARY and len(args) == 1:
            return self.emit(_NP_UNARY[name], self.number(args[0]))
        if name in _NP_BINARY and len(args) == 2:
            if name == "power":
                return self.power(args[0], args[1])
            a = self.number(args[0])
            return self.emit(_NP_BINARY[name], a, self.number(args[1]))
        if name == "clip" and len(args) == 3:                    # np.clip = minimum(maximum(a, lo), hi)
            a = self.number(args[0])
            lower = self.emit("max", a, self.number(args[1]))
            return self.emit("min", lower, self.number(args[2]))
        if name == "where" and len(args) == 3:
            cond, _ = self.value(args[0], boolean_ok=True)
            a = self.number(args[1])
            b = self.number(args[2])
            if a >= OPERAND_SLOT0 and b >= OPERAND_SLOT0:
                self.int_guards.append((a - OPERAND_SLOT0, b - OPERAND_SLOT0))
            return self.emit("where", a, b, cond)
        raise Refused(f"np.{name} with {len(args)} argument(s) on x or y")


def _static_params_reason(tree: ast.AST, params: dict) -> str:
    """A ``params[...]`` / ``params.get(...)`` with a constant key whose entry is not a real scalar."""
    for node in ast.walk(tree):
        key = None
        if isinstance(node, ast.Subscript) and isinstance(node.value, ast.Name) and node.value.id == "params":
            key = node.slice
        elif (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "get"
              and isinstance(node.func.value, ast.Name) and node.func.value.id == "params" and node.args):
            key = node.args[0]
        if isinstance(key, ast.Constant) and key.value in params and not _is_real_scalar(params[key.value]):
            return f"params[{key.value!r}] is not a real scalar ({type(params[key.value]).__name__})"
    return ""


class Program:
    """A compiled expression: slot evaluators + the instruction template."""

    def __init__(self, body: str, params: dict, builder: _Builder):
        self.body, self.params = body, params
        self.slot_sources = list(builder.slot_sources)
        self.nslot = len(self.slot_sources)
        self._slot_fns = [compile_safe_expression(src, variable_names=VARIABLES) for src in self.slot_sources]
        self._code = builder.code
        self._int_guards = builder.int_guards

    def _slot_value(self, k: int, t: float, E):
        return self._slot_fns[k](E=E, x=None, y=None, t=t, params=self.params)

    def instructions_for(self, t: float):
        """The instruction words of the step at time ``t`` as uint32, or None when an exponent slot cannot be evaluated
        (the step then takes the host path)."""
        words = np.empty(len(self._code), dtype=np.uint32)
        for i, (op, dst, a, b, c, pow_slot) in enumerate(self._code):
            if pow_slot is not None:
                try:
                    exponent = self._slot_value(pow_slot - OPERAND_SLOT0, t, None)
                    special = _SPECIAL_POWERS.get(float(exponent)) if _is_real_scalar(exponent) else None
                except Exception:       # noqa: BLE001 - whatever the sandbox raises means "not on the device"
                    return None
                if special is not None:
                    op, b = special, 0
            words[i] = OP[op] | dst << 8 | a << 12 | b << 18 | c << 24
        return words

    def is_exact_at(self, t: float) -> bool:
        """Whether the program of this step uses only ops of the exact class."""
        words = self.instructions_for(t)
        return words is not None and all(OPS[int(w) & 0xff] in EXACT_OPS for w in words)

    def slot_table(self, E_bins, t: float):
        """``slots[NE][nslot]`` of the step at ``t`` (float64), or None when a slot raises or is not a real scalar per bin."""
        E = np.asarray(E_bins, dtype=float)
        table = np.empty((E.size, self.nslot), dtype=np.float64)
        integer = [False] * self.nslot
        for k in range(self.nslot):
            try:
                value = self._slot_value(k, t, E[:, None])
            except Exception:           # noqa: BLE001
                return None
            if isinstance(value, np.ndarray):
                if value.dtype.kind not in "biuf" or value.shape not in ((), (1, 1), (E.size, 1)):
                    return None
                if value.dtype.kind in "iu" and value.size and int(np.abs(value).max()) > 2 ** 53:
                    return None
                integer[k] = value.dtype.kind != "f"
                table[:, k] = np.broadcast_to(value.astype(np.float64), (E.size, 1))[:, 0]
            elif _is_real_scalar(value):
                if isinstance(value, (int, np.integer)) and abs(int(value)) > 2 ** 53:
                    return None
                integer[k] = not isinstance(value, (float, np.floating))
                table[:, k] = float(value)
            else:
                return None
        # np.where over two integer branches is an integer array in NumPy (other division / power rules): host path
        if any(integer[a] and integer[b] for a, b in self._int_guards):
            return None
        return table


def _compile(body: str, params):
    params = dict(params or {})
    source = _strip_return(body)
    try:
        compile_safe_expression(source, variable_names=VARIABLES)          # the sandbox validates first, as always
    except ValueError as exc:
        return None, f"not a valid custom expression: {exc}"
    if not expression_is_elementwise(source, array_variables=("E", "x", "y")):
        return None, "not elementwise in E, x, y (subscript, .size / .shape, conditional, and / or, builtin or math.* on them)"
    tree = ast.parse(source, mode="eval")
    reason = _static_params_reason(tree, params)
    if reason:
        return None, reason
    builder = _Builder()
    try:
        result, _ = builder.value(tree.body, boolean_ok=True)
        if result >= MAX_REGS or not builder.code:       # the body is x, y or one slot: a program needs one word
            builder.emit("copy", result)
        return Program(source, params, builder), ""
    except Refused as exc:
        return None, str(exc)
    except ValueError as exc:                            # a slot the sandbox does not take on its own
        return None, f"sub-expression refused by the sandbox: {exc}"


def compile_program(body: str, params=None):
    """The device program of ``body`` with ``params``, or None when the expression is outside the device subset."""
    return _compile(body, params)[0]


def explain(body: str, params=None) -> str:
    """"" when ``body`` compiles for the device, else the reason for the refusal."""
    return _compile(body, params)[1]
