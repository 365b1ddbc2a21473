#!/usr/bin/env python3
"""ms per step of `run_2d_crank_nicolson` with and without collision rate traces, on two workloads:
  coupled12   N^2 (default 1024) cells, NE = 12, recombination + scattering, dynamic phonons, ADI (the c-workload
              parameters: gap 180, factors 1-3, tau_0 440, T_c 1.2, T_b 0.1, D0 6, dt 0.1, dx 1, reflective walls)
  coupled50   the same at NE = 50
and these variants:
  off       store_every = steps, no sink                          (the fast run of today)
  rates10   store_every = steps, rates_every = 10, 3 regions
  rates1    store_every = steps, rates_every = 1
  trace10   store_every = steps, trace_every = 10, 3 regions      (same halting steps as rates10: isolates the kernel from
  trace1    store_every = steps, trace_every = 1                   the lost pair passes and the guard read-back)
  store1    store_every = 1 with a phonon history                 (what the rates replace, before any NumPy evaluation)
A package without the `rates_out` keyword (the parent commit: `--package DIR`) runs `off`, the traces and `store1` only;
`--variants` restricts the list.  One process per package; per round the variants alternate, each timed with a host clock
around the call and a device synchronise at two run lengths `--steps SHORT LONG`: ms per step = (t_long - t_short) /
(LONG - SHORT), which drops the set-up of a run.  `store1` keeps every frame on the host and runs `--store-steps` instead.
Reported per variant: median and spread (max - min) over the rounds.  `off` against the parent commit is this script run
on both trees in alternating processes, compared by hand: the difference must lie inside the two spreads.
`--kernel` also times qp_collision_rates alone (device events around `--calls` calls) on 1024^2 planes at NE = 12 and 50
with 1 and 8 regions covering the grid and one region covering 1 % of it, beside qp_collision_step on the
one-wave-per-pixel route (QP_COLL_FORCE_WAVE) on the same planes.
python tools/exp_rates.py [--workloads coupled12 coupled50] [--rounds 5] [--steps 50 250] [--store-steps 3 9] [--kernel]
                          [--variants off rates1 ...] [--package DIR] [--json FILE]"""
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
PHYSICS = dict(energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, tau_0=440.0, T_c=1.2, bath_temperature=0.1)


def problem(ne, n):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((n, n), dtype=bool)
    edges = extract_edge_segments(mask)
    kw = dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BoundaryCondition("reflective") for e in edges},
              initial_field=1e-4 * (1.0 + np.random.default_rng(0).random(mask.shape)), diffusion_coefficient=6.0, dt=0.1,
              dx=1.0, diffusion_scheme="adi", num_energy_bins=ne, enable_recombination=True, enable_scattering=True, **PHYSICS)
    inner = np.zeros_like(mask)
    inner[n // 4:3 * n // 4, n // 4:3 * n // 4] = True
    strip = np.zeros_like(mask)
    strip[:, :n // 8] = True
    return kw, {"all": mask, "inner": inner, "strip": strip}


def variants(rated: bool, regions, wanted):
    out = [("off", lambda steps: dict(store_every=steps))]
    for every in (10, 1):
        if rated:
            out.append((f"rates{every}", lambda steps, e=every: dict(store_every=steps, rates_out={}, rates_regions=regions,
                                                                     rates_every=e)))
        out.append((f"trace{every}", lambda steps, e=every: dict(store_every=steps, trace_out={}, trace_regions=regions,
                                                                 trace_every=e)))
    out.append(("store1", lambda steps: dict(store_every=1, phonon_history_out={})))
    return [v for v in out if wanted is None or v[0] in wanted]


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


def kernel_alone(torch, n, ne, calls, rounds):
    """qp_collision_rates on n^2 cells with three region sets, and qp_collision_step (wave route) on the same planes."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((n, n), dtype=bool)
    z = np.zeros((1, 1))
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    gap = PHYSICS["energy_gap"]
    E, dE = T.build_energy_grid(gap, 1.0, 3.0, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = T.dynes_density_of_states(E, gap, 0.0)
    kr, ks = T.recombination_kernel_base(E, gap, 440.0, 1.2), T.scattering_kernel_base(E, gap, 440.0, 1.2)
    tabs = eng.make_collision_tables(kr[None], ks[None], rho[None], idx_d, idx_s, sg, kernel="wave")
    gen = torch.Generator(device=eng.device).manual_seed(0)
    level = 1e-3 * torch.rand(1, eng.ncell, dtype=torch.float64, device=eng.device, generator=gen)
    state = torch.rand(ne, eng.ncell, dtype=torch.float64, device=eng.device, generator=gen) * level * eng.upload_vector(rho)[:, None]
    ph = (eng.upload_vector(T.thermal_phonon_occupation(om, 0.1))[:, None]
          * (0.5 + torch.rand(om.size, eng.ncell, dtype=torch.float64, device=eng.device, generator=gen)))
    state_out, ph_work = torch.empty_like(state), ph.clone()
    small = np.zeros_like(mask)
    small[:n // 10, :n // 10] = True
    region_sets = {"1_region_all": [mask], "8_regions_all": [mask] * 8, "1_region_1pct": [small]}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def clock(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            ev[0].record()
            for _ in range(calls):
                call()
            ev[1].record()
            ev[1].synchronize()
            ms.append(ev[0].elapsed_time(ev[1]) / calls)
        return dict(ms=round(statistics.median(ms), 5), spread_ms=round(max(ms) - min(ms), 5))

    row = dict(n=n, ne=ne, nw=int(om.size))
    for name, regions in region_sets.items():
        bits = eng.region_bits(regions)
        out = eng.empty(1, len(regions), 4, ne)
        row[name] = clock(lambda: eng.collision_rates(tabs, state, ph, bits, 1, float(dE), True, True, out))
    # frozen phonons and the same input every call: the update cannot drift over the repetitions
    row["collision_step_wave_frozen_phonons"] = clock(lambda: eng.collide(tabs, state, state_out, ph_work, float(dE), 0.05, True,
                                                                          True, False))
    row["collision_step_wave"] = clock(lambda: (ph_work.copy_(ph), eng.collide(tabs, state, state_out, ph_work, float(dE), 0.05,
                                                                               True, True, True)))
    row["phonon_copy_alone"] = clock(lambda: ph_work.copy_(ph))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["coupled12", "coupled50"], choices=["coupled12", "coupled50"])
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, nargs=2, default=[50, 250], metavar=("SHORT", "LONG"))
    ap.add_argument("--store-steps", type=int, nargs=2, default=[3, 9], metavar=("SHORT", "LONG"))
    ap.add_argument("--variants", nargs="+", default=None)
    ap.add_argument("--kernel", action="store_true", help="also time qp_collision_rates alone")
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
    rated = "rates_out" in inspect.signature(run).parameters
    rows = []
    warnings.simplefilter("ignore")
    for name in args.workloads:
        ne = int(name[len("coupled"):])
        kw, regions = problem(ne, args.n)
        found = measure(run, torch, kw, variants(rated, regions, args.variants), args.rounds, args.steps, args.store_steps)
        med = {k: statistics.median(v) for k, v in found.items()}
        spread = {k: max(v) - min(v) for k, v in found.items()}
        rows.append(dict(workload=name, n=args.n, ms_per_step={k: round(v, 4) for k, v in med.items()},
                         spread_ms={k: round(v, 4) for k, v in spread.items()},
                         rounds_ms={k: [round(x, 4) for x in v] for k, v in found.items()}))
        print(f"{name} {args.n}^2: " + "  ".join(f"{k} {med[k]:.4f} (+-{spread[k]:.4f})" for k in med) + " ms/step", flush=True)
        torch.cuda.empty_cache()
    kernel = []
    if args.kernel and rated:
        for ne in (12, 50):
            kernel.append(kernel_alone(torch, args.n, ne, args.calls, args.rounds))
            print(json.dumps(kernel[-1]), flush=True)
            torch.cuda.empty_cache()
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(dict(
            what="ms per step of run_2d_crank_nicolson, (t_long - t_short) / (long - short) with a host clock around the call "
                 "and a device synchronise; median and spread (max - min) over the rounds, variants alternating; store1 "
                 "(with a phonon history) at its own, shorter run lengths (it keeps every frame on the host)",
            device=torch.cuda.get_device_name(0), build=json.loads(_hip.load().qp_build_info().decode()),
            package="this checkout" if args.package is None else "another tree (--package)", rates=rated,
            rounds=args.rounds, steps=args.steps, store1_steps=args.store_steps, rows=rows, kernel_alone=kernel), indent=1) + "\n")


if __name__ == "__main__":
    main()
