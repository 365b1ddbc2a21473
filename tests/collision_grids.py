"""Energy grids on which the collision tests reach the register kernels (gap 180, energy_min_factor 1.0).

``build_phonon_frequency_map`` rounds |Ei - Ej| and Ei + Ej to 12 digits, as the reference does.  On some grids that rounding
splits one diagonal into two phonon bins, `structured_bin_maps` returns None and the tables run the one-wave-per-pixel
kernel instead: with ``energy_max_factor = 3.0`` that happens at NE = 7, 13 and 14.  `unmerged_fmax` / `MERGED_FMAX` name,
for every instantiated size, a factor whose maps are structured; tests/test_collision_grids_host.py checks them without a
GPU, and every GPU test still asserts the route it means to exercise."""
from __future__ import annotations

_UNMERGED_EXCEPTIONS = {7: 6.0, 13: 2.5, 14: 2.75}
# 2 E_min / dE integer inside the difference range: 1 ... 15 phonon bins shared between a diagonal and an anti-diagonal
# (QP_COLL_SHARED_BINS).  NE = 2 has no such grid.
MERGED_FMAX = {3: 7.0, 4: 5.0, 5: 6.0, 6: 4.0, 7: 4.5, 8: 5.0, 9: 4.0, 10: 3.5, 11: 3.75, 12: 4.0, 13: 4.25, 14: 4.5, 15: 3.5,
               16: 5.0, 18: 4.0, 20: 3.5, 24: 4.0, 30: 3.5, 32: 5.0, 40: 3.5, 50: 3.5}


def unmerged_fmax(ne: int) -> float:
    """energy_max_factor with structured maps and 3 NE - 1 distinct phonon bins."""
    return _UNMERGED_EXCEPTIONS.get(ne, 3.0)
