"""bench.py's options: a plain run measures only the headline, `--dump-outputs` writes a bounded, reproducible sample."""
from __future__ import annotations

import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_extra_figures_are_opt_in(monkeypatch):
    args = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not args.full and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    assert parse(monkeypatch, "--full").full
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")


def test_small_outputs_are_dumped_whole(tmp_path):
    u = torch.rand(3, 40, dtype=torch.float64)
    bench.dump_outputs(SimpleNamespace(u=u), tmp_path)
    got = np.load(tmp_path / "field.npy")
    assert got.dtype == np.float64 and np.array_equal(got, u.numpy())


def test_large_outputs_are_a_fixed_sample_of_cells_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 4000)
    ne, nw, npix = 12, 35, 5000
    wl = SimpleNamespace(state=torch.rand(ne, npix, dtype=torch.float64), phonon=torch.rand(nw, npix, dtype=torch.float64))
    for d in ("a", "b"):
        bench.dump_outputs(wl, tmp_path / d)
    s, p = np.load(tmp_path / "a" / "qp_state.npy"), np.load(tmp_path / "a" / "phonon.npy")
    assert s.size + p.size <= 4000 and s.shape[0] == ne and p.shape[0] == nw and s.shape[1] == p.shape[1]
    for name in ("qp_state", "phonon"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy"))
    cols = [int(np.flatnonzero(wl.state[0].numpy() == v)[0]) for v in s[0]]      # the same cells in both arrays
    assert cols == sorted(cols) and np.array_equal(p, wl.phonon.numpy()[:, cols])
