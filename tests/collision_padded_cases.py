"""Grids and inputs of the padded-bins collision tests (tests/test_collision_padded_host.py without a GPU,
tests/test_gpu_collision_padded.py with one): every size in 17 ... 49 without a collision kernel of its own, on energy grids
(gap 180, energy_min_factor 1.0) whose phonon bin maps are structured.

`host_setup` builds what `collision_exact.host_setup` builds - same seeds, same order of draws, same 407-cell mask - with an
explicit energy_max_factor, so that `collision_exact.exact / k_ref64 / error_k / limit` serve these grids as they serve the
instantiated sizes; their caches key on (ne, kind), and no size here is one of theirs."""
from __future__ import annotations

import numpy as np

import collision_exact as X

# ne -> energy_max_factor.  "regimes": 3 ne - 1 distinct phonon bins; "merged": bins shared between a diagonal and an
# anti-diagonal (QP_COLL_SHARED_BINS, the stash path).  Eleven sizes have structured maps only with merged bins.
UNMERGED = {17: 3.125, 21: 2.75, 22: 2.375, 25: 3.0, 26: 2.625, 27: 3.0, 28: 2.75, 33: 2.375, 34: 7.375, 35: 2.75, 36: 3.0,
            39: 2.625, 42: 2.75, 44: 2.375, 45: 3.0, 48: 3.0}
MERGED = {19: 3.375, 23: 3.875, 29: 4.625, 31: 4.875, 37: 5.625, 38: 3.375, 41: 6.125, 43: 6.375, 46: 3.875, 47: 6.875,
          49: 7.125, 25: 3.5, 36: 4.0, 45: 3.5}
FACTOR = {"regimes": UNMERGED, "merged": MERGED}
GRIDS = [(ne, "regimes") for ne in sorted(UNMERGED)] + [(ne, "merged") for ne in sorted(MERGED)]
# qp_collision_padded_ceiling as the issue states it: the sizes without a one-pass or register kernel of their own
OWN_KERNEL = set(range(2, 17)) | {18, 20, 24, 30, 32, 40, 50}
PADDED_NE = [ne for ne in range(17, 50) if ne not in OWN_KERNEL]
# the lowest and the highest live size of every ceiling; 42 = exactly three 14-bin target blocks of ceiling 50; 28 and 29
# end inside the second 16-bin block of ceiling 30
BOUNDARY_NE = [17, 28, 29, 31, 33, 39, 41, 42, 49]

assert sorted({ne for ne, _ in GRIDS}) == PADDED_NE and len(GRIDS) == 30 and len(PADDED_NE) == 27
assert not OWN_KERNEL & set(PADDED_NE)

_HOST: dict = {}


def ceiling(ne: int) -> int:
    """The mapping of the issue (not the library's answer: the host test compares the two)."""
    if ne <= 16 or ne >= 50 or ne in OWN_KERNEL:
        return 0
    return 30 if ne < 30 else 32 if ne < 32 else 40 if ne < 40 else 50


def kind_of(ne: int) -> str:
    """The grid kind a size is tested on where one is enough (merged only where no unmerged grid was found)."""
    return "regimes" if ne in UNMERGED else "merged"


def host_setup(ne, kind):
    """`collision_exact.host_setup(ne, kind)` with energy_max_factor = FACTOR[kind][ne]."""
    key = (ne, kind)
    if key in _HOST:
        return _HOST[key]
    from qpsim_amd import tables as T
    n = X.NCELL
    E, dE = T.build_energy_grid(180.0, 1.0, FACTOR[kind][ne], ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = np.stack([T.dynes_density_of_states(E, g, 0.1) for g in X.GAPS])
    kr = np.stack([T.recombination_kernel_base(E, g, X.TAU_R, X.T_C) for g in X.GAPS])
    ks = np.stack([T.scattering_kernel_base(E, g, X.TAU_S, X.T_C) for g in X.GAPS])
    rng = np.random.default_rng(1000 * ne + len(kind))
    cls = rng.integers(0, X.GAPS.size, size=n)
    level = rng.choice(X.LEVELS[kind], size=n)
    u = rng.random((ne, n))
    state = {"one": u * rho[0][:, None] * level[None, :], "classes": u * rho[cls].T * level[None, :]}
    ph = T.thermal_phonon_occupation(om, 0.3)[:, None] * (0.5 + rng.random((om.size, n)))
    ks_amp = (1.0 / X.TAU_S) * (E[:, None] - E[None, :]) ** 2 / (T.KB_UEV_PER_K * X.T_C) ** 3
    np.fill_diagonal(ks_amp, 0.0)
    active = X.active_cells()
    h = dict(ne=ne, kind=kind, E=E, dE=float(dE), nw=om.size, maps=(idx_d, idx_s, sg), rho=rho, kr=kr, ks=ks, cls=cls,
             level=level[active], active=active, state=state, ph=ph, ks_amp=ks_amp)
    _HOST[key] = h
    return h


def one_class_args(h):
    """Positional arguments of `plan_collision_tables` / `make_collision_tables` for the one gap class of `h`."""
    return (h["kr"][:1], h["ks"][:1], h["rho"][:1], *h["maps"])
