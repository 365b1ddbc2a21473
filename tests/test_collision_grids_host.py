"""The energy grids of tests/collision_grids.py give the bin-map structure the GPU collision tests rely on (no GPU)."""
from __future__ import annotations

import pytest

from collision_grids import MERGED_FMAX, unmerged_fmax
from test_collision_route_host import AVAILABLE

REGISTER_NE = AVAILABLE["qp_collision_register_kernel_available"]


def _maps(ne, fmax):
    from qpsim_amd import tables as T
    E, _ = T.build_energy_grid(180.0, 1.0, fmax, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    return om.size, idx_d, idx_s, sg


@pytest.mark.parametrize("ne", REGISTER_NE)
def test_unmerged_grid_of_every_register_size_is_structured(ne):
    from qpsim_amd.engine import structured_bin_maps
    nw, idx_d, idx_s, sg = _maps(ne, unmerged_fmax(ne))
    assert structured_bin_maps(idx_d, idx_s, sg) is not None and nw == 3 * ne - 1


def test_the_default_factor_loses_the_structure_at_7_13_14():
    from qpsim_amd.engine import structured_bin_maps
    lost = [ne for ne in REGISTER_NE if structured_bin_maps(*_maps(ne, 3.0)[1:], allow_shared=True) is None]
    assert lost == [7, 13, 14]


def test_merged_grid_of_every_register_size_shares_bins():
    from qpsim_amd.engine import structured_bin_maps, tag_merged_bins
    assert sorted(MERGED_FMAX) == [ne for ne in REGISTER_NE if ne != 2]
    for ne, fmax in MERGED_FMAX.items():
        nw, idx_d, idx_s, sg = _maps(ne, fmax)
        assert structured_bin_maps(idx_d, idx_s, sg) is None, ne
        shared = structured_bin_maps(idx_d, idx_s, sg, allow_shared=True)
        assert shared is not None, ne
        slots = tag_merged_bins(*shared)[2]
        assert 1 <= slots <= 15 and nw == 3 * ne - 1 - slots, ne
