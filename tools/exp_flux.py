#!/usr/bin/env python3
"""ms per step of `run_2d_crank_nicolson` with and without boundary outflow traces, on two workloads:
  coupled   N^2 (default 1024) cells, NE = 12, recombination + scattering, dynamic phonons, ADI (the c-workload parameters:
            gap 180, factors 1-3, tau_0 440, T_c 1.2, T_b 0.1, D0 6, dt 0.1, dx 1), absorbing walls (4 N faces)
  scalar    N^2 (default 4096) cells, energy_gap = 0, ADI, absorbing walls
and four variants:
  off       store_every = steps, no sink                        (the fast run of today)
  flux1     store_every = steps, flux_every = 1, 4 surfaces     (the outflow of every wall per step, kept on the device)
  flux10    store_every = steps, flux_every = 10
  store1    store_every = 1, no sink                            (the only way to the boundary term without the trace)
A package without the `flux_out` keyword (the parent commit: `--package DIR`) runs `off` and `store1` only.
One process per package; per round the variants alternate, each timed with a host clock around the call and a device
synchronise at two run lengths `--steps SHORT LONG`: ms per step = (t_long - t_short) / (LONG - SHORT), which drops the
set-up of a run (tables, plans, uploads, the stores at t = 0 and the end).  `store1` keeps every frame on the host and runs
`--store-steps SHORT LONG` instead.  Reported per variant: median and spread (max - min) over the rounds, the ratios to
`off`, and
  off_no_slower_than(other file)   is checked by hand against the JSON of the parent run (same script, same workloads)
  flux1_beats_store1               store1 - flux1 > spread(store1) + spread(flux1)
`--kernel` also times qp_boundary_flux alone (device events around `--calls` calls) on the walls of an N^2 rectangle (4 N
faces, 4 surfaces) and on a mask with random holes (one surface of every face), and reports the bytes a sample moves: 20 B
per face of index and coefficients per chunk block (once per plane), 8 B per face and plane gathered from the state (a
32-byte sector each where the faces are not neighbours), 8 B per chunk, plane and stage of partials, 8 B per output.
python tools/exp_flux.py [--workloads coupled scalar] [--rounds 5] [--steps 50 450] [--store-steps 10 30] [--kernel] [--package DIR] [--json FILE]"""
import argparse
import gc
import inspect
import json
import statistics
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def problem(name, n):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((n, n), dtype=bool)
    edges = extract_edge_segments(mask)
    kw = dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BoundaryCondition("absorbing") for e in edges},
              initial_field=1e-4 * (1.0 + np.random.default_rng(0).random(mask.shape)), diffusion_coefficient=6.0, dt=0.1,
              dx=1.0, diffusion_scheme="adi")
    if name == "coupled":
        kw.update(energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=12, enable_recombination=True,
                  enable_scattering=True, tau_0=440.0, T_c=1.2, bath_temperature=0.1)
    return kw, {e.normal: [e.edge_id] for e in edges}


def variants(fluxed: bool, surfaces):
    out = [("off", lambda steps: dict(store_every=steps))]
    if fluxed:
        out += [("flux1", lambda steps: dict(store_every=steps, flux_out={}, flux_surfaces=surfaces, flux_every=1)),
                ("flux10", lambda steps: dict(store_every=steps, flux_out={}, flux_surfaces=surfaces, flux_every=10))]
    return out + [("store1", lambda steps: dict(store_every=1))]


def timed(run, torch, kw, extra, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run(**kw, total_time=steps * kw["dt"], **extra(steps))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    assert len(res[0]) == (steps + 1 if extra(steps)["store_every"] == 1 else 2)
    del res
    gc.collect()
    return 1e3 * (t1 - t0)


def measure(run, torch, kw, todo, rounds, steps, store_steps):
    found = {name: [] for name, _ in todo}
    lengths = {name: store_steps if name == "store1" else steps for name, _ in todo}
    for name, extra in todo:                    # warm-up of every variant: code objects, plans, pinned staging buffers
        timed(run, torch, kw, extra, lengths[name][0])
    for _ in range(rounds):
        for name, extra in todo:
            short, long = lengths[name]
            a = timed(run, torch, kw, extra, short)
            b = timed(run, torch, kw, extra, long)
            found[name].append((b - a) / (long - short))
    return found


def wall_faces(mask, nsurface):
    """Every boundary face of ``mask`` as absorbing, by direction: four surfaces (up, down, left, right) or one of all."""
    from qpsim_amd.engine import BoundaryFaces, flux_chunks
    from qpsim_amd.geometry import boundary_face_masks
    sides = [np.flatnonzero(side.reshape(-1)) for side in boundary_face_masks(mask).values()]
    if nsurface == 1:
        sides = [np.sort(np.concatenate(sides), kind="stable")]
    begin = np.concatenate([[0], np.cumsum([s.size for s in sides])]).astype(np.int32)
    cell = np.concatenate(sides).astype(np.int32)
    return BoundaryFaces(cell, np.full(cell.size, 2.0), np.zeros(cell.size), begin, flux_chunks(begin))


def kernel_alone(torch, label, mask, nplane, nsurface, calls, rounds):
    from qpsim_amd.engine import CompiledGeometry, DiffusionOperator, Engine, link_flags
    z = np.zeros((1, 1))
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    faces = wall_faces(mask, nsurface)
    dev = eng.upload_boundary_faces(faces)
    op = DiffusionOperator(eng, nplane, 0.1, dcoef=np.linspace(1.0, 6.0, nplane), allow_fast=False)
    state = torch.rand(nplane, eng.ncell, dtype=torch.float64, device=eng.device)
    out = eng.empty(1, nsurface, nplane)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):
        eng.boundary_flux(dev, op, state, 1, out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        ev[0].record()
        for _ in range(calls):
            eng.boundary_flux(dev, op, state, 1, out)
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / calls)
    nface, nchunk = int(faces.face_cell.size), int(faces.chunks.shape[0])
    # per plane: 20 B per face of index and coefficients, the gather from the state, 12 B per chunk of table, its partial
    # written and read again, the outputs
    nbytes = nplane * (20.0 * nface + 8.0 * nface + 28.0 * nchunk + 8.0 * nsurface)
    med = statistics.median(ms)
    return dict(mask=label, cells=int(mask.size), faces=nface, chunks=nchunk, nplane=nplane, nsurface=nsurface,
                ms=round(med, 5), spread_ms=round(max(ms) - min(ms), 5), bytes_requested=nbytes,
                bytes_of_32B_sectors=nplane * (20.0 * nface + 32.0 * nface + 28.0 * nchunk + 8.0 * nsurface),
                state_bytes_a_stored_frame_moves=8.0 * nplane * mask.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["coupled", "scalar"], choices=["coupled", "scalar"])
    ap.add_argument("--n-coupled", type=int, default=1024)
    ap.add_argument("--n-scalar", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, nargs=2, default=[50, 450], metavar=("SHORT", "LONG"))
    ap.add_argument("--store-steps", type=int, nargs=2, default=[10, 30], metavar=("SHORT", "LONG"))
    ap.add_argument("--kernel", action="store_true", help="also time qp_boundary_flux alone")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--package", default=None, help="tree to import qpsim_amd from (default: this checkout)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternations"
    pkg = Path(args.package).resolve() if args.package else ROOT
    for p in (str(pkg), str(pkg / "quasiparticle-physics-simulation_amd")):
        sys.path.insert(0, p)
    import torch
    from qpsim_amd import _hip
    from qpsim_amd.solver import run_2d_crank_nicolson as run
    fluxed = "flux_out" in inspect.signature(run).parameters
    rows = []
    warnings.simplefilter("ignore")
    for name in args.workloads:
        n = args.n_coupled if name == "coupled" else args.n_scalar
        kw, surfaces = problem(name, n)
        found = measure(run, torch, kw, variants(fluxed, surfaces), args.rounds, args.steps, args.store_steps)
        med = {k: statistics.median(v) for k, v in found.items()}
        spread = {k: max(v) - min(v) for k, v in found.items()}
        row = dict(workload=name, n=n, ms_per_step={k: round(v, 4) for k, v in med.items()},
                   spread_ms={k: round(v, 4) for k, v in spread.items()},
                   rounds_ms={k: [round(x, 4) for x in v] for k, v in found.items()},
                   over_off={k: round(v / med["off"], 3) for k, v in med.items()})
        if fluxed:
            row["flux1_beats_store1"] = bool(med["store1"] - med["flux1"] > spread["store1"] + spread["flux1"])
            row["store1_over_flux1"] = round(med["store1"] / med["flux1"], 2)
        rows.append(row)
        print(f"{name} {n}^2: " + "  ".join(f"{k} {med[k]:.4f} (+-{spread[k]:.4f})" for k in med) + " ms/step"
              + (f";  flux1 beats store1: {row['flux1_beats_store1']} (x{row['store1_over_flux1']})" if fluxed else ""),
              flush=True)
        torch.cuda.empty_cache()
    kernel = []
    if args.kernel and fluxed:
        holes = np.random.default_rng(1).random((args.n_coupled, args.n_coupled)) >= 0.1
        for label, mask, nplane, nsurface in ((f"rectangle {args.n_scalar}^2", np.ones((args.n_scalar,) * 2, dtype=bool), 1, 4),
                                              (f"rectangle {args.n_scalar}^2", np.ones((args.n_scalar,) * 2, dtype=bool), 12, 4),
                                              (f"random holes {args.n_coupled}^2", holes, 1, 1),
                                              (f"random holes {args.n_coupled}^2", holes, 12, 1)):
            kernel.append(kernel_alone(torch, label, mask, nplane, nsurface, args.calls, args.rounds))
            k = kernel[-1]
            print(f"qp_boundary_flux {label} x {nplane} planes, {k['faces']} faces in {k['chunks']} chunks, {nsurface} "
                  f"surfaces: {k['ms']:.4f} ms (+-{k['spread_ms']:.4f}), {k['bytes_requested'] / 1e3:.1f} kB requested "
                  f"against {k['state_bytes_a_stored_frame_moves'] / 1e6:.1f} MB of a stored frame", flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(dict(
            what="ms per step of run_2d_crank_nicolson, (t_long - t_short) / (long - short) with a host clock around the call "
                 "and a device synchronise; median and spread (max - min) over the rounds, variants alternating; store1 "
                 "at its own, shorter run lengths (it keeps every frame on the host)",
            device=torch.cuda.get_device_name(0), build=json.loads(_hip.load().qp_build_info().decode()),
            package="this checkout" if args.package is None else "another tree (--package)", flux=fluxed,
            rounds=args.rounds, steps=args.steps, store1_steps=args.store_steps, rows=rows, boundary_flux_alone=kernel),
            indent=1) + "\n")


if __name__ == "__main__":
    main()
