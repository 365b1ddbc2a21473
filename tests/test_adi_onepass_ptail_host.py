"""P of the one-pass step, formed y-elimination first (`fine_fused_body<1, STREAM, true>`, `csrc/qp_adi_fine.inc`).

P(q, c) is the y-elimination (first / last entry of A_y^-1 over the 32 rows of y-chunk q) of the zero-ghost x-front
(x-solve, then explicit x-operator with its sources) of the rhs1' tile.  The x-front acts along the columns of an x-chunk
and is the same affine map for every row up to the row source; the y-elimination is a fixed linear form over the rows and
the same for every column.  So

    P_f(q, c) = sum_c' M[c][c'] r_f(c') + bias_f(c),    r_f(c') = ends_f over the rows of rhs1'[., c']    (likewise _l)

with M the x-front of the unit vectors (table `xmap`, stored transposed) and bias the old order applied to an all-zero tile
(table `pbias`).  This file mirrors both orders in NumPy with the kernel's summation orders - every fma of the kernel is one
`_fma` here - and holds each of them to a rounding bound against a long-double evaluation.

Bound.  u = 2^-53.  At a <= 0.31 every coefficient of the x-solve and of the explicit operator is positive (asserted), so
the computed x-front of a row is a sum over paths of positive weights times the inputs, and a value that passes n rounded
operations on its way carries a factor (1 + theta), |theta| <= n u (first order).  The same holds for the y-elimination,
whose weights w_k are products of positive table entries.  With W = sum_k |w_k|, E = max |e|, A = max |source term| and
|M|_inf = max row sum of M (<= 1), every intermediate of either order is bounded by B = W (|M|_inf E + A), and:
  * x-front of one row: the forward sweep rounds the product e_k W_k and one fma per cell (a term entering at cell j passes at
    most 2 + 31 roundings), the backward sweep one fma per cell (32), the explicit operator the neighbour sum and two
    fmas (3): 68 u.
  * a 32-term weighted sum as `ends32` forms it (one fma per row, then the product with the last pivot): 33 u.
  * old order (x-front per row, then the weighted sum over rows): (68 + 33) u B = 101 u B.
  * new order: the weighted sum first (33 u), then the accumulation as `fine_p_map` orders it - each half-wave sums its 16
    rows of the map from zero, c' ascending, one fma per row, and the result is (bias + rows 0..15) + rows 16..31: at most
    16 + 2 roundings on the way of any term, which the 33 u of a 33-term accumulation in any order covers - with the
    entries of M each computed by an x-front of a unit vector (68 u relative, no cancellation) and the bias by the old
    order: (33 + 33 + 68) u B = 134 u B.
The two orders differ by at most the sum, 235 u B.  The factor 1.01 covers the higher orders in u, the 2^-11 relative error
of the long-double reference and the 2^-10 u by which `_fma` (product and sum rounded to 64 bits, then to 53) may exceed one
rounding."""
import numpy as np
import pytest

FS = 32
U = 2.0 ** -53
C_XFRONT, C_SUM = 68, 33
C_OLD = C_XFRONT + C_SUM
C_NEW = C_SUM + 33 + C_XFRONT
LD = np.longdouble


def _fma64(a, b, c):
    return np.asarray(LD(a) * LD(b) + LD(c), dtype=np.float64)


def _fma_ld(a, b, c):
    return LD(a) * LD(b) + LD(c)


class _Arith:
    """fp64 as the kernel rounds (one rounding per fma) or long double throughout."""

    def __init__(self, exact):
        self.fma = _fma_ld if exact else _fma64
        self.dtype = LD if exact else np.float64

    def arr(self, x):
        return np.array(x, dtype=self.dtype)


def _tables(a, var, e_lo, e_hi, s_lo, s_hi):
    """Table entries of a 32-cell chunk (`build_chunk_table`, scaled eliminations of `fine_plan_prepare`), fp64.
    var 0 interior, 1 first (wall face e_lo / s_lo at cell 0), 2 last (e_hi / s_hi at cell 31)."""
    first, last = var == 1, var == 2
    links = np.full(FS, 2.0)
    e = np.zeros(FS)
    src = np.zeros(FS)
    if first:
        links[0], e[0], src[0] = 1.0, e_lo, a * s_lo
    if last:
        links[-1], e[-1], src[-1] = 1.0, e_hi, a * s_hi
    bd = 1.0 + a * (links + e)
    w = np.zeros(FS)
    v = np.zeros(FS)
    for k in range(FS):
        w[k] = 1.0 / (bd[k] - (a * a * w[k - 1] if k > 0 else 0.0))
    for k in range(FS - 1, -1, -1):
        v[k] = 1.0 / (bd[k] - (a * a * v[k + 1] if k < FS - 1 else 0.0))
    awf = a * w
    awf[0] = 0.0
    awb = a * w
    awb[-1] = 0.0
    eav = a * v
    eav[-1] = 0.0
    eawf = np.zeros(FS)
    eawf[1:] = awf[1:] * w[:-1] / w[1:]
    eavs = np.zeros(FS)
    eavs[:-1] = eav[:-1] * v[1:] / v[:-1]
    c0 = 1.0 - a * (links + e)
    return dict(W=w, AWF=awf, AWB=awb, C0=c0, SRC=src, EAWF=eawf, EAV=eavs, EV0=v[0], EWL=w[-1], a=a)


def _x_front(rows, T, srow, ar, sources=True):
    """thomas32 then explicit32 with gl = gr = 0 on every row of `rows` [n][FS]; srow [n] is the row source."""
    e = ar.arr(rows).copy()
    n = e.shape[0]
    dp = ar.arr(np.zeros(n))
    for k in range(FS):
        prod = ar.arr(ar.arr(e[:, k]) * ar.arr(T["W"][k]))
        dp = ar.fma(T["AWF"][k], dp, prod)
        e[:, k] = dp
    x = ar.arr(np.zeros(n))
    for k in range(FS - 1, -1, -1):
        x = ar.fma(T["AWB"][k], x, e[:, k])
        e[:, k] = x
    out = e.copy()
    zero = ar.arr(np.zeros(n))
    extra = ar.arr(srow) if sources else zero
    for k in range(FS):
        prev = e[:, k - 1] if k > 0 else zero
        nxt = e[:, k + 1] if k + 1 < FS else zero
        add = ar.arr(T["SRC"][k] + extra) if (sources and k in (0, FS - 1)) else extra
        out[:, k] = ar.fma(T["a"], ar.arr(prev + nxt), ar.fma(T["C0"][k], e[:, k], add))
    return out


def _ends(tile, T, ar):
    """ends32 along axis 0 of `tile` [FS rows][n]: (yf, yl) per column."""
    n = tile.shape[1]
    dp = ar.arr(np.zeros(n))
    bp = ar.arr(np.zeros(n))
    for k in range(FS):
        j = FS - 1 - k
        dp = ar.fma(T["EAWF"][k], dp, tile[k])
        bp = ar.fma(T["EAV"][j], bp, tile[j])
    return ar.arr(bp * ar.arr(T["EV0"])), ar.arr(dp * ar.arr(T["EWL"]))


def _end_weights(T):
    """w_f, w_l with ends_f(e) = sum_k w_f[k] e_k (long double): the weights the bound is stated in."""
    wf = np.zeros(FS, dtype=LD)
    wl = np.zeros(FS, dtype=LD)
    wf[0] = LD(T["EV0"])
    for k in range(1, FS):
        wf[k] = wf[k - 1] * LD(T["EAV"][k - 1])
    wl[-1] = LD(T["EWL"])
    for k in range(FS - 2, -1, -1):
        wl[k] = wl[k + 1] * LD(T["EAWF"][k + 1])
    return wf, wl


def _old_order(tile, Tx, Ty, srow, ar):
    return _ends(_x_front(tile, Tx, srow, ar), Ty, ar)


def _new_order(tile, Tx, Ty, srow):
    ar = _Arith(False)
    Mt = _x_front(np.eye(FS), Tx, np.zeros(FS), ar, sources=False)       # row c' = column c' of M: Mt[c'][c]
    bias_f, bias_l = _old_order(np.zeros((FS, FS)), Tx, Ty, srow, ar)
    r_f, r_l = _ends(ar.arr(tile), Ty, ar)
    out = []
    for bias, r in ((bias_f, r_f), (bias_l, r_l)):
        halves = []
        for half in range(2):               # a half-wave sums its 16 rows of the map from zero, c' ascending
            acc = np.zeros(FS)
            for cp in range(16 * half, 16 * half + 16):
                acc = ar.fma(Mt[cp], r[cp], acc)
            halves.append(acc)
        out.append((bias + halves[0]) + halves[1])
    return out[0], out[1], Mt


SIDES = dict(e_lo=2.0, e_hi=0.4, s_lo=0.6, s_hi=-0.25)        # a Dirichlet-like and a Robin-like face, non-zero sources
SIDES_Y = dict(e_lo=0.0, e_hi=1.0, s_lo=-0.1, s_hi=0.35)      # a Neumann-like and an absorbing-like face


@pytest.mark.parametrize("a", [0.05, 0.3, 0.31])
@pytest.mark.parametrize("kind", ["random", "offset"])
def test_y_first_order_matches_x_first_order_within_rounding(a, kind):
    assert np.finfo(LD).nmant >= 63, "the reference needs an extended long double"
    rng = np.random.default_rng(int(1000 * a) + (kind == "offset"))
    exact, fp = _Arith(True), _Arith(False)
    worst_new = worst_old = worst_diff = 0.0
    for xv in range(3):
        Tx = _tables(a, xv, **SIDES)
        for yv in range(3):
            Ty = _tables(a, yv, **SIDES_Y)
            tile = rng.uniform(-1.0, 1.0, (FS, FS)) if kind == "random" else 1e-4 * (1.0 + rng.random((FS, FS)))
            srow = np.zeros(FS)                     # y-face sources sit in rows 0 and ny - 1 (fine_row_source)
            if yv == 1:
                srow[0] = a * SIDES_Y["s_lo"]
            if yv == 2:
                srow[-1] = a * SIDES_Y["s_hi"]
            for name in ("W", "AWF", "AWB", "C0", "EAWF", "EAV"):
                assert np.all(Tx[name] >= 0.0) and np.all(Ty[name] >= 0.0), (a, xv, yv, name)
            ref = _old_order(tile, Tx, Ty, srow, exact)
            old = _old_order(tile, Tx, Ty, srow, fp)
            new_f, new_l, Mt = _new_order(tile, Tx, Ty, srow)
            assert np.all(Mt > 0.0)
            m_inf = float(Mt.sum(axis=0).max())                  # row sums of M = column sums of Mt
            assert m_inf <= 1.0 + 1e-12, m_inf
            A = float(np.abs(Tx["SRC"]).max() + np.abs(srow).max())
            E = float(np.abs(tile).max())
            for got_new, got_old, want, w in zip((new_f, new_l), old, ref, _end_weights(Ty)):
                B = float(np.abs(w).sum()) * (m_inf * E + A)
                err_new = float(np.max(np.abs(LD(got_new) - want)))
                err_old = float(np.max(np.abs(LD(got_old) - want)))
                diff = float(np.max(np.abs(got_new - got_old)))
                worst_new = max(worst_new, err_new / (U * B))
                worst_old = max(worst_old, err_old / (U * B))
                worst_diff = max(worst_diff, diff / (U * B))
                assert err_old <= 1.01 * C_OLD * U * B, (a, xv, yv, err_old / (U * B))
                assert err_new <= 1.01 * C_NEW * U * B, (a, xv, yv, err_new / (U * B))
                assert diff <= 1.01 * (C_OLD + C_NEW) * U * B, (a, xv, yv, diff / (U * B))
                assert float(np.max(np.abs(want))) > 0.0
    print(f"a={a} {kind}: old {worst_old:.2f} u B, new {worst_new:.2f} u B, old - new {worst_diff:.2f} u B")


def test_bias_is_the_old_order_of_a_zero_tile_and_vanishes_without_sources():
    """Reflective walls (no diagonal term, no source): P of a zero tile is zero, in every variant pair."""
    fp = _Arith(False)
    for xv in range(3):
        for yv in range(3):
            Tx = _tables(0.3, xv, 0.0, 0.0, 0.0, 0.0)
            Ty = _tables(0.3, yv, 0.0, 0.0, 0.0, 0.0)
            bf, bl = _old_order(np.zeros((FS, FS)), Tx, Ty, np.zeros(FS), fp)
            assert not bf.any() and not bl.any()
