"""Reference of the collision rate traces (tests/test_collision_rates_host.py without a GPU, tests/test_gpu_collision_rates.py
with one): its own restatement of the four channels per pixel from (n, N, tables), and the inputs of the kernel cases.

Per pixel and bin i, with q = rho max(1 - n / max(rho, 1e-30), 0), N the phonon occupation of the pair's bin and
Ks_eff[a][b] = ks0[a][b] (1 + N_|a-b|) where E_a > E_b, ks0[a][b] N_|a-b| where E_a < E_b, 0 where a == b:

  0 scattering_in    dE q_i sum_j Ks_eff[j][i] n_j
  1 scattering_out   n_i dE sum_j Ks_eff[i][j] q_j
  2 recombination    n_i 2 dE sum_j kr0[i][j] (1 + N_{i+j}) n_j
  3 pair_breaking    2 dE q_i sum_j kr0[i][j] N_{i+j} q_j

`pixel_channels(..., dtype=np.float64)` evaluates them in the kernel's association - each sum over j = 0 ... NE-1 in order,
term = (K * factor) * x_j, prefactors (dE q_i), (n_i dE), (n_i (2 dE)), ((2 dE) q_i) - and `dtype=np.longdouble` in extended
precision.  In both, f = n / max(rho, 1e-30), 1 - f and q = rho max(1 - f, 0) are taken in fp64: three IEEE operations the
kernel reproduces bit for bit, so q is an INPUT of the error model and every term is a product of non-negative factors.

Error model (`bound`): a channel value of a pixel is within (NE + 8) u, u = 2^-53, of exact - 3 roundings per term (1 + N, K
times it, times x_j; the kernel fuses the last with the accumulation), NE - 1 accumulations, at most 4 in the prefactor (2
here: 2 dE is exact) - and a region sum of c cells adds (c - 1) u, whatever the order (all values are >= 0)."""
from __future__ import annotations

import math

import numpy as np

from collision_exact import GAPS, host_setup

U = 2.0 ** -53
CHUNK = 1024          # QP_RATES_CHUNK of include/qpsim_hip.h: the cells of a member grid one block reduces
CHANNELS = ("scattering_in", "scattering_out", "recombination", "pair_breaking")


def bound(ne: int, cells: int) -> float:
    """Relative error bound of a region sum over `cells` cells (of a pixel value for cells = 1)."""
    return (ne + 8 + max(cells - 1, 0)) * U


def pixel_channels(n, p, kr, ks, rho, idx_diff, idx_sum, sign, dE, en_r=True, en_s=True, dtype=np.float64):
    """n [NE, P], p [NW, P] in fp64, one table set (kr, ks [NE, NE] or None; rho [NE]).  Returns (ch [4, NE, P], loss
    [2, NE, P]) in `dtype`: the channels and the two loss sums without their factor n_i (dE sum_j Ks_eff[i][j] q_j and
    2 dE sum_j kr0[i][j] (1 + N_{i+j}) n_j), so that ch[1] = n loss[0] and ch[2] = n loss[1] up to the association."""
    n = np.asarray(n, dtype=np.float64)
    p64 = np.asarray(p, dtype=np.float64)
    rho_c = np.asarray(rho, dtype=np.float64)[:, None]
    f = n / np.maximum(rho_c, 1e-30)
    q = rho_c * np.maximum(1.0 - f, 0.0)                 # fp64, as the kernel and the reference form it
    T = dtype
    n, q, p = n.astype(T), q.astype(T), p64.astype(T)
    dE, one = T(dE), T(1.0)
    NE = n.shape[0]
    zero = np.zeros_like(n)
    g_s, l_s, g_r, l_r = zero.copy(), zero.copy(), zero.copy(), zero.copy()
    if en_s and ks is not None:
        ks = np.asarray(ks).astype(T)
        for j in range(NE):
            # pairs (i, j) for all i: Ks_eff[j][i] and Ks_eff[i][j]
            s_ji, s_ij = np.asarray(sign)[j, :, None], np.asarray(sign)[:, j, None]
            N_ji, N_ij = p[np.asarray(idx_diff)[j, :]], p[np.asarray(idx_diff)[:, j]]
            f_ji = np.where(s_ji > 0, one + N_ji, np.where(s_ji < 0, N_ji, T(0.0)))
            f_ij = np.where(s_ij > 0, one + N_ij, np.where(s_ij < 0, N_ij, T(0.0)))
            g_s = g_s + (ks[j, :, None] * f_ji) * n[j][None, :]
            l_s = l_s + (ks[:, j, None] * f_ij) * q[j][None, :]
    if en_r and kr is not None:
        kr = np.asarray(kr).astype(T)
        for j in range(NE):
            N = p[np.asarray(idx_sum)[:, j]]
            l_r = l_r + (kr[:, j, None] * (one + N)) * n[j][None, :]
            g_r = g_r + (kr[:, j, None] * N) * q[j][None, :]
    dE2 = T(2.0) * dE
    ch = np.stack([(dE * q) * g_s, (n * dE) * l_s, (n * dE2) * l_r, (dE2 * q) * g_r])
    return ch, np.stack([dE * l_s, dE2 * l_r])


def channels(n, p, tables, cls, en_r=True, en_s=True, dtype=np.float64):
    """`pixel_channels` over pixels of several classes: tables = dict(kr [C, NE, NE] | None, ks, rho [C, NE], maps, dE),
    cls [P] the class of every pixel.  Returns ch [4, NE, P]."""
    idx_d, idx_s, sg = tables["maps"]
    n, p, cls = np.asarray(n), np.asarray(p), np.asarray(cls)
    out = np.zeros((4,) + n.shape, dtype=dtype)
    for c in np.unique(cls):
        px = np.flatnonzero(cls == c)
        out[:, :, px] = pixel_channels(n[:, px], p[:, px], None if tables["kr"] is None else tables["kr"][c],
                                       None if tables["ks"] is None else tables["ks"][c], tables["rho"][c], idx_d, idx_s,
                                       sg, tables["dE"], en_r, en_s, dtype)[0]
    return out


def exact_sum(values) -> float:
    """The sum of extended-precision values, correctly rounded to fp64: every value is split into an fp64 head and tail
    (exact for a 64-bit significand), and math.fsum adds them without error."""
    v = np.asarray(values, dtype=np.longdouble).reshape(-1)
    head = v.astype(np.float64)
    tail = (v - head).astype(np.float64)
    return math.fsum(np.concatenate([head, tail]))


def region_sums(ch, region) -> np.ndarray:
    """[4, NE] exact region sums of ch [4, NE, P] over the pixels of `region` (bool [P])."""
    sel = ch[:, :, np.asarray(region, dtype=bool)]
    return np.array([[exact_sum(sel[c, i]) for i in range(ch.shape[1])] for c in range(4)])


# ---------------------------------------------------------------------------------------------------- kernel cases
# (ne, grid kind, ncell_member, members, nregion, (en_r, en_s), family): family "one" = one table set, "classes" = four
# gap classes through cls, "members" = one table set per member (member classes; members = 3).
# ncell_member: 1; around a group of 8; the chunk edges; three chunks with a ragged last one.  Not omitted: ne = 64 with 8
# regions, ne = 2, an odd ncm with 3 members, the three-chunk ragged case with gap classes, member classes with 3 members.
# The last two have 2 regions (the NR = 2 instantiation of the collision kernel): within one wave, and across three chunks
# with gap classes.
KERNEL_CASES = [
    (2, "plain", 1, 1, 1, (1, 1), "one"),
    (2, "plain", 9, 3, 3, (1, 1), "classes"),
    (12, "plain", 7, 3, 8, (1, 0), "one"),
    (12, "merged", 8, 1, 3, (0, 1), "one"),
    (12, "plain", CHUNK - 1, 1, 1, (1, 1), "classes"),
    (12, "plain", CHUNK, 3, 3, (1, 1), "members"),
    (12, "merged", CHUNK + 1, 1, 8, (1, 1), "one"),
    (12, "plain", 2 * CHUNK + 77, 3, 8, (1, 1), "classes"),
    (50, "plain", 9, 1, 3, (1, 1), "classes"),
    (50, "merged", 65, 3, 8, (0, 1), "members"),
    (50, "plain", CHUNK + 1, 1, 1, (1, 0), "one"),
    (64, "plain", 130, 1, 8, (1, 1), "one"),
    (64, "plain", 7, 3, 1, (1, 0), "members"),
    (12, "plain", 9, 1, 2, (1, 1), "one"),
    (50, "merged", 2 * CHUNK + 3, 1, 2, (1, 1), "classes"),
]
# Stage 2 (rates_final_kernel, shared by both rate kernels) adds the chunk partials in batches of FINAL_BATCH loads and then
# one by one: exactly one batch; a batch and a remainder with three members (the m nchunk per offset of a member with
# nchunk >= 32); two batches and a remainder.  At most 3 regions, so that the exact sums stay around a second.  A list of
# its own (the host-side soundness tests take seconds per case here); the GPU tests and the soundness tests of both rate
# kernels run it beside KERNEL_CASES.
MANY_CHUNK_CASES = [
    (12, "plain", 32 * CHUNK, 1, 1, (1, 1), "one"),
    (12, "plain", 37 * CHUNK + 77, 3, 3, (1, 1), "classes"),
    (12, "merged", 69 * CHUNK + 5, 1, 3, (1, 1), "one"),
]
FINAL_BATCH = 32      # B of rates_final_kernel: chunk partials loaded before the first of them is added


def final_rounds(ncm: int) -> tuple:
    """(chunks, whole batches, chunks added one by one) of the stage-2 kernels for a member grid of `ncm` cells."""
    nchunk = (ncm + CHUNK - 1) // CHUNK
    return nchunk, nchunk // FINAL_BATCH, nchunk % FINAL_BATCH


assert [final_rounds(c[2]) for c in MANY_CHUNK_CASES] == [(32, 1, 0), (38, 1, 6), (70, 2, 6)]
assert all(final_rounds(c[2])[1] == 0 for c in KERNEL_CASES)
LEVELS = [1e-9, 1e-5, 1e-2, 0.5, 0.95]
_INPUTS: dict = {}


def region_bits(rng, ncm, nregion):
    """The regions of tests/test_gpu_trace.py `_region_bits`: everything, nothing, two identical random ones, another
    random one, the first cell only, the last cell only, a sparse one.  Returns (names, regions, bits)."""
    twin = rng.random(ncm) < 0.5
    kinds = {"all": np.ones(ncm, dtype=bool), "empty": np.zeros(ncm, dtype=bool), "twin": twin,
             "other": rng.random(ncm) < 0.3, "first": np.arange(ncm) == 0, "last": np.arange(ncm) == ncm - 1,
             "sparse": rng.random(ncm) < 0.01}
    order = {1: ["other"], 2: ["all", "empty"]}.get(nregion,
                                                    ["all", "empty", "twin", "twin", "other", "first", "last", "sparse"][:nregion])
    regions = [kinds[k] for k in order]
    bits = np.zeros(ncm, dtype=np.uint8)
    for r, region in enumerate(regions):
        bits |= region.astype(np.uint8) << r
    return order, regions, bits


def case_inputs(ne, kind, ncm, members, nregion, family):
    """The inputs of a kernel case, once: dict(tables, cls [members, ncm], state [ne, members, ncm], ph [nw, members, ncm],
    names, regions, bits).  Tables, energy grid and phonon grid are those of `host_setup(ne, kind)`; occupations span
    1e-9 ... 0.95 of rho pixel by pixel, phonons are thermal at 0.3 K times 0.5 ... 1.5."""
    key = (ne, kind, ncm, members, nregion, family)
    if key in _INPUTS:
        return _INPUTS[key]
    from qpsim_amd import tables as T
    h = host_setup(ne, kind)
    rng = np.random.default_rng([ne, len(kind), ncm, members, nregion, len(family)])
    nclass = {"one": 1, "classes": GAPS.size, "members": members}[family]
    if family == "members":
        cls = np.repeat(np.arange(members), ncm).reshape(members, ncm)
    else:
        cls = np.tile(rng.integers(0, nclass, size=ncm), (members, 1))         # the class map of a member grid, repeated
    tables = dict(kr=h["kr"][:nclass], ks=h["ks"][:nclass], rho=h["rho"][:nclass], maps=h["maps"], dE=h["dE"])
    level = rng.choice(LEVELS, size=(members, ncm))
    state = rng.random((ne, members, ncm)) * np.moveaxis(tables["rho"][cls], -1, 0) * level[None]
    om = T.build_phonon_frequency_map(h["E"])[0]
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None, None] * (0.5 + rng.random((om.size, members, ncm)))
    names, regions, bits = region_bits(rng, ncm, nregion)
    out = dict(tables=tables, cls=cls, state=state, ph=ph, names=names, regions=regions, bits=bits, nw=int(om.size))
    for a in (state, ph, bits, cls):
        a.setflags(write=False)
    _INPUTS[key] = out
    return out


def case_tables(case, en_r, en_s):
    """The tables of a case with the tables of a disabled process removed."""
    t = dict(case["tables"])
    if not en_r:
        t["kr"] = None
    if not en_s:
        t["ks"] = None
    return t
