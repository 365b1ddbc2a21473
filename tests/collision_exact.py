"""Inputs, cases and references of the per-element collision tests (tests/test_collision_exact_host.py without a GPU,
tests/test_gpu_collision_elementwise.py with one).

`host_setup` rebuilds the inputs of `_setup` in tests/test_gpu_collision_instantiations.py from the same seeds without an
engine (the GPU test asserts that the two agree bit for bit), so that the fp64 oracle, the extended-precision evaluation
`oracle.qp_oracle.collision_step_exact` and K_ref64 are the same numbers in both files.

K = max over the active elements of |got - exact| / T (`error_units`), formed for the state planes and for the phonon
planes; a kernel must stay within `limit(K_ref64)` of each, K_ref64 being the K of `O.collision_step` in fp64."""
from __future__ import annotations

import numpy as np

from collision_grids import MERGED_FMAX, unmerged_fmax

GAPS = np.array([180.0, 171.0, 165.5, 176.25])
LEVELS = {"plain": [1e-5, 1e-2, 0.5, 0.95], "merged": [1e-5, 1e-2, 0.5, 0.95], "regimes": [1e-9, 1e-5, 1e-2, 0.5, 0.95]}
NCELL = 407
TAU_R, TAU_S, T_C = 500.0, 400.0, 1.2
COMBOS = [(True, True, True), (True, False, True), (False, True, True)]
ALL_ON = (True, True, True)
SWEEP_NE, SWEEP_DT = [12, 24, 30, 50], [3e-3, 25.0, 400.0, 800.0]
GENERIC_NE, WAVE_NE, LONE_DT = [12, 50, 65], [12, 50, 64], [1e-7, 0.37, 400.0]
DILUTE = 1e-5          # pixels at or below this occupation level are the ones the level-maximum norm cannot see

_HOST: dict = {}
_REFS: dict = {}


def limit(k_ref64):
    """4 K_ref64 + 4: the factor of X87_RULE; the additive part covers roundings the fp64 oracle does not have - the
    polynomial exponential (<= 1 ulp = 2 u), the Newton reciprocal (u) and the final fma (u), each relative to the new
    value, and T >= u times the new value."""
    return 4.0 * k_ref64 + 4.0


def active_cells():
    """The 407-cell mask of `_engine` in tests/test_gpu_collision_instantiations.py."""
    active = np.random.default_rng(407).random(NCELL) > 0.2
    active[64:128] = False
    active[0], active[128] = True, False
    return active


def host_setup(ne, kind):
    """The host arrays of `_setup(ne, kind)`: same seeds, same order of draws."""
    key = (ne, kind)
    if key in _HOST:
        return _HOST[key]
    from qpsim_amd import tables as T
    n = NCELL
    E, dE = T.build_energy_grid(180.0, 1.0, MERGED_FMAX[ne] if kind == "merged" else unmerged_fmax(ne), ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in GAPS])
    kr = np.stack([T.recombination_kernel_base(E, g, TAU_R, T_C) for g in GAPS])
    ks = np.stack([T.scattering_kernel_base(E, g, TAU_S, T_C) for g in GAPS])
    rng = np.random.default_rng(1000 * ne + len(kind))
    cls = rng.integers(0, GAPS.size, size=n)
    level = rng.choice(LEVELS[kind], size=n)
    u = rng.random((ne, n))
    state = {"one": u * rho[0][:, None] * level[None, :], "classes": u * rho[cls].T * level[None, :]}
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    ks_amp = (1.0 / TAU_S) * (E[:, None] - E[None, :]) ** 2 / (T.KB_UEV_PER_K * T_C) ** 3      # CollFastView::ks_amp
    np.fill_diagonal(ks_amp, 0.0)
    active = active_cells()
    h = dict(ne=ne, kind=kind, E=E, dE=float(dE), nw=om.size, maps=(idx_d, idx_s, sg), rho=rho, kr=kr, ks=ks, cls=cls,
             level=level[active], active=active, state=state, ph=ph, ks_amp=ks_amp)
    _HOST[key] = h
    return h


def oracle_tables(h, family, combo, kr=None):
    """The `tables` of `O.collision_step` for the active cells of one family; `kr` replaces the recombination tables."""
    en_r, en_s, _ = combo
    px = h["active"]
    nc = 1 if family == "one" else GAPS.size
    idx_d, idx_s, sg = h["maps"]
    kr = h["kr"] if kr is None else kr
    return {"rho": h["rho"][:nc], "Kr0": kr[:nc] if en_r else None, "Ks0": h["ks"][:nc] if en_s else None,
            "cls": h["cls"][px] if nc > 1 else np.zeros(int(px.sum()), dtype=int), "idx_diff": idx_d, "idx_sum": idx_s,
            "sign": sg, "dE": h["dE"]}


def run_oracle64(O, h, family, combo, dt, kr=None):
    """`O.collision_step` in fp64 on the active cells: (state, phonons)."""
    px = h["active"]
    s_ref, p_ref = h["state"][family][:, px].copy(), h["ph"][:, px].copy()
    O.collision_step(s_ref, p_ref, oracle_tables(h, family, combo, kr), dt, en_r=combo[0], en_s=combo[1],
                     update_phonons=combo[2])
    return s_ref, p_ref


def exact(O, h, family, combo, dt):
    """The extended-precision evaluation on the active cells, once per case: dict(n, p, T_n, T_ph, window, x)."""
    key = ("exact", h["ne"], h["kind"], family, combo, dt)
    if key not in _REFS:
        px = h["active"]
        tables = oracle_tables(h, family, combo)
        if family == "classes":
            tables["ks_mag"] = h["ks_amp"]
        out = O.collision_step_exact(h["state"][family][:, px], h["ph"][:, px], tables, dt, en_r=combo[0], en_s=combo[1])
        for a in out:
            a.setflags(write=False)
        _REFS[key] = dict(zip(("n", "p", "T_n", "T_ph", "window", "x"), out))
    return _REFS[key]


def error_k(O, got_s, got_p, ex, pixels=slice(None)):
    """((K of the state planes, K of the phonon planes), number of T = 0 elements that differ) over `pixels`."""
    ks, bad_s = O.error_units(got_s[:, pixels], ex["n"][:, pixels], ex["T_n"][:, pixels])
    kp, bad_p = O.error_units(got_p[:, pixels], ex["p"][:, pixels], ex["T_ph"][:, pixels])
    return (ks, kp), bad_s + bad_p


def k_ref64(O, h, family, combo, dt):
    """K of the fp64 oracle, once per case: ((state, phonons), T = 0 elements that differ)."""
    key = ("kref", h["ne"], h["kind"], family, combo, dt)
    if key not in _REFS:
        _REFS[key] = error_k(O, *run_oracle64(O, h, family, combo, dt), exact(O, h, family, combo, dt))
    return _REFS[key]


def register_cases(sizes_of_family):
    """(family, grid kind, ne, combo, dt) of the register / one-pass kernels; `sizes_of_family` = {"one": [...], "classes":
    [...]}.  Every size on the `regimes` grid at dt = 1e-7 and 0.37 with three process combinations; every merged grid at
    0.37; the time-step sweep."""
    out = []
    for family, sizes in sizes_of_family.items():
        out += [(family, "regimes", ne, combo, dt) for ne in sizes for combo in COMBOS for dt in (1e-7, 0.37)]
        out += [(family, "merged", ne, ALL_ON, 0.37) for ne in sorted(MERGED_FMAX)]
        out += [(family, "regimes", ne, ALL_ON, dt) for ne in SWEEP_NE for dt in SWEEP_DT]
    return out


def lone_cases():
    """The generic and the one-wave-per-pixel kernel, one gap class: what every other test compares against."""
    return [(kernel, "regimes", ne, ALL_ON, dt) for kernel, sizes in (("generic", GENERIC_NE), ("wave", WAVE_NE))
            for ne in sizes for dt in LONE_DT]
