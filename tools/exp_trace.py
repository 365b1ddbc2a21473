#!/usr/bin/env python3
"""ms per step of `run_2d_crank_nicolson` with and without time traces, on two workloads:
  coupled   N^2 (default 1024) cells, NE = 12, recombination + scattering, dynamic phonons, ADI (the c-workload parameters:
            gap 180, factors 1-3, tau_0 440, T_c 1.2, T_b 0.1, D0 6, dt 0.1, dx 1, reflective walls)
  scalar    N^2 (default 4096) cells, energy_gap = 0, ADI
and four variants:
  off       store_every = steps, no trace                       (the fast run of today)
  trace1    store_every = steps, trace_every = 1, 3 regions     (a sum per step, kept on the device)
  trace10   store_every = steps, trace_every = 10
  store1    store_every = 1, no trace                           (the only way to a time curve without traces)
A package without the `trace_out` keyword (the parent commit: `--package DIR`) runs `off` and `store1` only.
One process; per round the variants alternate, each timed with a host clock around the call and a device synchronise at two
run lengths `--steps SHORT LONG`: ms per step = (t_long - t_short) / (LONG - SHORT), which drops the set-up of a run
(tables, plans, uploads, the stores at t = 0 and the end).  The set-up varies by milliseconds from call to call, so the
window is hundreds of steps; `store1` keeps every frame on the host and runs `--store-steps SHORT LONG` instead.
Reported per variant: median and spread (max - min) over the rounds, the ratios to `off`, and
  off_no_slower_than(other file)   is checked by hand against the JSON of the parent run (same script, same workloads)
  trace1_beats_store1              store1 - trace1 > spread(store1) + spread(trace1)
`--kernel` also times qp_region_sums alone (device events around `--calls` calls) on the planes of both workloads and
reports the bytes it moves (8 B per cell and field + 1 B per cell of bits) over 8 TB/s.
python tools/exp_trace.py [--workloads coupled scalar] [--rounds 5] [--steps 50 450] [--store-steps 10 30] [--kernel] [--package DIR] [--json FILE]"""
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
HBM_PEAK_GBS = 8000.0


def problem(name, n):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    mask = np.ones((n, n), dtype=bool)
    edges = extract_edge_segments(mask)
    kw = dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BoundaryCondition("reflective") for e in edges},
              initial_field=1e-4 * (1.0 + np.random.default_rng(0).random(mask.shape)), diffusion_coefficient=6.0, dt=0.1,
              dx=1.0, diffusion_scheme="adi")
    if name == "coupled":
        kw.update(energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=12, enable_recombination=True,
                  enable_scattering=True, tau_0=440.0, T_c=1.2, bath_temperature=0.1)
    inner = np.zeros_like(mask)
    inner[n // 4:3 * n // 4, n // 4:3 * n // 4] = True
    strip = np.zeros_like(mask)
    strip[:, :n // 8] = True
    return kw, {"all": mask, "inner": inner, "strip": strip}


def variants(traced: bool, regions):
    out = [("off", lambda steps: dict(store_every=steps))]
    if traced:
        out += [("trace1", lambda steps: dict(store_every=steps, trace_out={}, trace_regions=regions, trace_every=1)),
                ("trace10", lambda steps: dict(store_every=steps, trace_out={}, trace_regions=regions, trace_every=10))]
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


def kernel_alone(torch, n, nfield, nregion, calls, rounds):
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((n, n), dtype=bool)
    z = np.zeros((1, 1))
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    state = torch.rand(nfield, eng.ncell, dtype=torch.float64, device=eng.device)
    regions = [mask] + [np.random.default_rng(r).random(mask.shape) < 0.5 for r in range(1, nregion)]
    bits = eng.region_bits(regions)
    out = eng.empty(1, nregion, nfield)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):
        eng.region_sums(state, bits, 1, out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        ev[0].record()
        for _ in range(calls):
            eng.region_sums(state, bits, 1, out)
        ev[1].record()
        ev[1].synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / calls)
    nbytes = eng.ncell * (8.0 * nfield + 1.0)
    med = statistics.median(ms)
    return dict(n=n, nfield=nfield, nregion=nregion, ms=round(med, 5), spread_ms=round(max(ms) - min(ms), 5),
                bytes=nbytes, gbs=round(nbytes / med / 1e6, 1), share_of_8tbs=round(nbytes / med / 1e6 / HBM_PEAK_GBS, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["coupled", "scalar"], choices=["coupled", "scalar"])
    ap.add_argument("--n-coupled", type=int, default=1024)
    ap.add_argument("--n-scalar", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, nargs=2, default=[50, 450], metavar=("SHORT", "LONG"))
    ap.add_argument("--store-steps", type=int, nargs=2, default=[10, 30], metavar=("SHORT", "LONG"))
    ap.add_argument("--kernel", action="store_true", help="also time qp_region_sums alone")
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
    traced = "trace_out" in inspect.signature(run).parameters
    rows = []
    warnings.simplefilter("ignore")
    for name in args.workloads:
        n = args.n_coupled if name == "coupled" else args.n_scalar
        kw, regions = problem(name, n)
        found = measure(run, torch, kw, variants(traced, regions), args.rounds, args.steps, args.store_steps)
        med = {k: statistics.median(v) for k, v in found.items()}
        spread = {k: max(v) - min(v) for k, v in found.items()}
        row = dict(workload=name, n=n, ms_per_step={k: round(v, 4) for k, v in med.items()},
                   spread_ms={k: round(v, 4) for k, v in spread.items()},
                   rounds_ms={k: [round(x, 4) for x in v] for k, v in found.items()},
                   over_off={k: round(v / med["off"], 3) for k, v in med.items()})
        if traced:
            row["trace1_beats_store1"] = bool(med["store1"] - med["trace1"] > spread["store1"] + spread["trace1"])
            row["store1_over_trace1"] = round(med["store1"] / med["trace1"], 2)
        rows.append(row)
        print(f"{name} {n}^2: " + "  ".join(f"{k} {med[k]:.4f} (+-{spread[k]:.4f})" for k in med) + " ms/step"
              + (f";  trace1 beats store1: {row['trace1_beats_store1']} (x{row['store1_over_trace1']})" if traced else ""),
              flush=True)
        torch.cuda.empty_cache()
    kernel = []
    if args.kernel and traced:
        for n, nfield, nregion in ((args.n_coupled, 12, 3), (args.n_coupled, 12, 8), (args.n_scalar, 1, 3), (args.n_scalar, 1, 8)):
            kernel.append(kernel_alone(torch, n, nfield, nregion, args.calls, args.rounds))
            k = kernel[-1]
            print(f"qp_region_sums {n}^2 x {nfield} planes, {nregion} regions: {k['ms']:.4f} ms (+-{k['spread_ms']:.4f}), "
                  f"{k['gbs']:.0f} GB/s = {k['share_of_8tbs']:.3f} of 8 TB/s", flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(dict(
            what="ms per step of run_2d_crank_nicolson, (t_long - t_short) / (long - short) with a host clock around the call "
                 "and a device synchronise; median and spread (max - min) over the rounds, variants alternating; store1 "
                 "at its own, shorter run lengths (it keeps every frame on the host)",
            device=torch.cuda.get_device_name(0), build=json.loads(_hip.load().qp_build_info().decode()),
            package="this checkout" if args.package is None else "another tree (--package)", traces=traced,
            rounds=args.rounds, steps=args.steps, store1_steps=args.store_steps, rows=rows, region_sums_alone=kernel), indent=1) + "\n")


if __name__ == "__main__":
    main()
