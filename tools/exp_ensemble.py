#!/usr/bin/env python3
"""ms per step of the ensemble API `run_2d_crank_nicolson_ensemble`:
  (a) at the c4 shape (64 members x 256^2, NE = 12, full physics, dynamic phonons) next to the `--workload c4` loop that
      drives the same kernels with one global guard;
  (b) 512 members x 64^2 at NE = 50 next to 512 sequential lone `run_2d_crank_nicolson` calls.
Each figure is the difference of two run lengths (setup, first / last store excluded).  python tools/exp_ensemble.py"""
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "quasiparticle-physics-simulation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from qpsim_amd import bench_workloads as W  # noqa: E402
from qpsim_amd.ensemble import last_run_stats, run_2d_crank_nicolson_ensemble  # noqa: E402
from qpsim_amd.geometry import extract_edge_segments  # noqa: E402
from qpsim_amd.models import BoundaryCondition  # noqa: E402
from qpsim_amd.solver import run_2d_crank_nicolson  # noqa: E402

warnings.simplefilter("ignore")


def per_step(fn, short, long):
    el = []
    for k in (short, long):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        el.append(time.perf_counter() - t0)
    return 1e3 * (el[1] - el[0]) / (long - short)


def common(N, ne):
    mask = np.ones((N, N), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    return dict(mask=mask, edges=edges, edge_conditions=bcs, diffusion_coefficient=6.0, dt=0.1, dx=1.0, energy_gap=180.0,
                energy_max_factor=3.0, num_energy_bins=ne, enable_recombination=True, enable_scattering=True,
                diffusion_scheme="adi")


def main():
    dev = torch.device("cuda", torch.cuda.current_device())
    # (a) c4 shape
    wl = W.build("c4", dev)
    wl.run(3)
    c4 = per_step(wl.run, 5, 105)
    del wl
    torch.cuda.empty_cache()
    N, M = 256, 64
    rng = np.random.default_rng(0)
    members = [{"initial_field": 1e-4 * (1.0 + rng.random((N, N)))} for _ in range(M)]
    kw = common(N, 12)
    run = lambda k: run_2d_crank_nicolson_ensemble(members, total_time=0.1 * k, store_every=k, **kw)  # noqa: E731
    run(3)
    api = per_step(run, 5, 105)
    pairs = last_run_stats()["pair_passes"]
    print(f"c4 shape {M} x {N}^2 NE=12: workload {c4:.3f} ms/step, ensemble API {api:.3f} ms/step "
          f"({api / c4:.2f}x), pair passes in the 105-step run: {pairs}")
    torch.cuda.empty_cache()
    # (b) 512 x 64^2 at NE = 50
    N, M, ne = 64, 512, 50
    members = [{"initial_field": 1e-4 * (1.0 + rng.random((N, N)))} for _ in range(M)]
    kw = common(N, ne)
    run = lambda k: run_2d_crank_nicolson_ensemble(members, total_time=0.1 * k, store_every=k, **kw)  # noqa: E731
    run(2)
    ens = per_step(run, 2, 32)
    lone_kw = dict(kw, initial_field=members[0]["initial_field"])
    lone = lambda k: run_2d_crank_nicolson(total_time=0.1 * k, store_every=k, **lone_kw)  # noqa: E731
    lone(2)
    one = per_step(lone, 4, 104)
    print(f"{M} x {N}^2 NE={ne}: ensemble {ens:.3f} ms/step, {M} sequential lone calls {M * one:.3f} ms/step "
          f"({one:.3f} per call), speed-up {M * one / ens:.1f}x")


if __name__ == "__main__":
    main()
