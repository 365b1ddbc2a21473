"""Reference of the phonon rate traces (tests/test_phonon_rates_host.py without a GPU, tests/test_gpu_phonon_rates.py with
one): its own restatement of the four channels per pixel and phonon bin from (n, N, tables), and the kernel cases.  Inputs,
regions, `exact_sum` and `bound` are those of tests/collision_rates_ref.py.

Per pixel, with q = rho max(1 - n / max(rho, 1e-30), 0), the base sums per phonon bin w

  E_w = dE sum n_i ks0[i][j] q_j   over the pairs with E_i > E_j and idx_diff[i][j] = w
  A_w = the same sum               over the pairs with E_i < E_j
  R_w = dE sum n_i kr0[i][j] n_j   over all (i, j) with idx_sum[i][j] = w (both orders, diagonal included)
  B_w = dE sum q_i kr0[i][j] q_j   over the same pairs

(the reference's phonon equation is dN_w/dt = (E_w + R_w)(1 + N_w) - (A_w + B_w) N_w) and the channels

  0 scattering_emission       E_w (1 + N_w)
  1 scattering_absorption     A_w N_w
  2 recombination_emission    R_w (1 + N_w)
  3 pair_breaking_absorption  B_w N_w

The sums are taken as the reference takes them: the pair lists of `np.nonzero` and one scatter-add per list.  In fp64 that
is `np.bincount`, which adds the pairs of a bin in list order - i ascending, which on the |i - j| / i + j maps is the kernel's
order j ascending - with the term (x_i K) y_j, then dE times the sum, then the occupation factor: the kernel's association
up to its fused last product.  `np.bincount` has no extended-precision weights, so `dtype=np.longdouble` scatters with
`np.add.at`.  q is formed in fp64 in both (an INPUT of the error model, as in collision_rates_ref).

Error model: `collision_rates_ref.bound`.  A pixel's channel value has 2 roundings per term, at most NE terms per bin and
channel (one diagonal or one anti-diagonal feeds an array) with NE - 1 accumulations, 1 for dE, 2 for the occupation factor:
NE + 4 <= NE + 8."""
from __future__ import annotations

import numpy as np

from collision_rates_ref import (CHUNK, KERNEL_CASES as RATE_CASES, MANY_CHUNK_CASES, U, bound, case_inputs, case_tables,  # noqa: F401
                                 exact_sum, region_sums)

CHANNELS = ("scattering_emission", "scattering_absorption", "recombination_emission", "pair_breaking_absorption")

# The kernel is specialised on (regions rounded up to 1, 2, 4, 8) x (phonon bins per lane: NW <= 64, <= 128, <= 191).  On
# plain grids NW = 3 NE - 1 would put NE = 21 / 22 and 43 / 44 either side of the two boundaries, but the grids of
# `host_setup` have unstructured maps at those sizes (tests/collision_grids.py: the 12-digit rounding splits a diagonal), which
# the kernel does not serve.  The nearest sizes with structured maps: NE = 24 merged (NW = 64, the last size with one bin
# per lane) / NE = 24 plain (71), and NE = 40 (119) / NE = 45 (134).  NE = 30 adds the two instantiations with two bins per
# lane that no other case reaches.  NE = 64 with 8 regions (NW = 191) is among RATE_CASES.
KERNEL_CASES = RATE_CASES + [
    (24, "merged", 129, 1, 2, (1, 1), "one"),
    (24, "plain", 130, 1, 8, (1, 1), "one"),
    (40, "plain", 127, 1, 3, (1, 1), "classes"),
    (45, "plain", 130, 1, 2, (1, 1), "one"),
    (30, "plain", 9, 1, 1, (1, 1), "one"),
    (30, "merged", 17, 3, 2, (1, 1), "classes"),
]


def bins_per_lane(nw: int) -> int:
    return (nw + 63) // 64


def _scatter(nw, idx, vals, dtype):
    """out[w, p] = sum over the pairs k with idx[k] = w of vals[k, p], added in list order."""
    npair, P = vals.shape
    if dtype == np.float64:
        flat = (np.asarray(idx)[:, None] * P + np.arange(P)[None, :]).reshape(-1)
        return np.bincount(flat, weights=vals.reshape(-1), minlength=nw * P).reshape(nw, P)
    out = np.zeros((nw, P), dtype=dtype)
    np.add.at(out, np.asarray(idx), vals)
    return out


def pixel_channels(n, p, kr, ks, rho, idx_diff, idx_sum, sign, dE, en_r=True, en_s=True, dtype=np.float64):
    """n [NE, P], p [NW, P] in fp64, one table set (kr, ks [NE, NE] or None; rho [NE]).  Returns (ch [4, NW, P], base
    [4, NW, P]) in `dtype`: the channels and the base sums E, A, R, B."""
    n = np.asarray(n, dtype=np.float64)
    p64 = np.asarray(p, dtype=np.float64)
    rho_c = np.asarray(rho, dtype=np.float64)[:, None]
    q = rho_c * np.maximum(1.0 - n / np.maximum(rho_c, 1e-30), 0.0)       # fp64, as the kernel and the reference form it
    T = dtype
    n, q, N = n.astype(T), q.astype(T), p64.astype(T)
    dE, one = T(dE), T(1.0)
    nw, P = N.shape
    idx_diff, idx_sum, sign = np.asarray(idx_diff), np.asarray(idx_sum), np.asarray(sign)
    base = np.zeros((4, nw, P), dtype=T)
    if en_s and ks is not None:
        ks = np.asarray(ks).astype(T)
        for slot, pairs in ((0, sign > 0), (1, sign < 0)):                # sign[i][j] = sign(E_i - E_j)
            i, j = np.nonzero(pairs)
            base[slot] = dE * _scatter(nw, idx_diff[i, j], (n[i] * ks[i, j, None]) * q[j], T)
    if en_r and kr is not None:
        kr = np.asarray(kr).astype(T)
        i, j = np.nonzero(np.ones_like(idx_sum, dtype=bool))
        base[2] = dE * _scatter(nw, idx_sum[i, j], (n[i] * kr[i, j, None]) * n[j], T)
        base[3] = dE * _scatter(nw, idx_sum[i, j], (q[i] * kr[i, j, None]) * q[j], T)
    up = one + N
    return np.stack([base[0] * up, base[1] * N, base[2] * up, base[3] * N]), base


def channels(n, p, tables, cls, en_r=True, en_s=True, dtype=np.float64):
    """`pixel_channels` over pixels of several classes (tables and cls as `collision_rates_ref.channels` takes them).
    Returns (ch [4, NW, P], base [4, NW, P])."""
    idx_d, idx_s, sg = tables["maps"]
    n, p, cls = np.asarray(n), np.asarray(p), np.asarray(cls)
    ch = np.zeros((4,) + p.shape, dtype=dtype)
    base = np.zeros_like(ch)
    for c in np.unique(cls):
        px = np.flatnonzero(cls == c)
        ch[:, :, px], base[:, :, px] = pixel_channels(
            n[:, px], p[:, px], None if tables["kr"] is None else tables["kr"][c],
            None if tables["ks"] is None else tables["ks"][c], tables["rho"][c], idx_d, idx_s, sg, tables["dE"], en_r, en_s,
            dtype)
    return ch, base


_EXACT: dict = {}


def case_exact(case_key):
    """(case, ch64, chld, baseld) of a kernel case, once: the channels [4, NW, members, ncm] in fp64 and in extended
    precision, and the extended-precision base sums."""
    if case_key not in _EXACT:
        ne, kind, ncm, members, nregion, (en_r, en_s), family = case_key
        case = case_inputs(ne, kind, ncm, members, nregion, family)
        flat = lambda a: a.reshape(a.shape[0], -1)  # noqa: E731
        args = (flat(case["state"]), flat(case["ph"]), case_tables(case, en_r, en_s), case["cls"].reshape(-1), en_r, en_s)
        shape = (4, case["nw"], members, ncm)
        ch64 = channels(*args, dtype=np.float64)[0].reshape(shape)
        chld, baseld = (a.reshape(shape) for a in channels(*args, dtype=np.longdouble))
        for a in (ch64, chld, baseld):
            a.setflags(write=False)
        _EXACT[case_key] = (case, ch64, chld, baseld)
    return _EXACT[case_key]
