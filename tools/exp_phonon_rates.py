#!/usr/bin/env python3
"""ms per step of `run_2d_crank_nicolson` with and without phonon rate traces, on the two workloads of tools/exp_rates.py
(coupled 1024^2, NE = 12 and NE = 50, ADI, dynamic phonons) and these variants:
  off        store_every = steps, no sink                              (the fast run of today)
  phonon10   store_every = steps, phonon_rates_every = 10, 3 regions
  phonon1    store_every = steps, phonon_rates_every = 1
  rates10    store_every = steps, rates_every = 10, 3 regions          (the quasiparticle-side sampler at the same cadence)
  rates1     store_every = steps, rates_every = 1
  store1     store_every = 1 with a phonon history                     (what the traces replace, before any NumPy evaluation)
A package without the `phonon_rates_out` keyword (the parent commit: `--package DIR`) runs `off`, the `rates` variants and
`store1` only; `--variants` restricts the list.  Timing is that of tools/exp_rates.py: one process per package, the variants
alternating per round, ms per step = (t_long - t_short) / (LONG - SHORT) with a host clock around the call and a device
synchronise, median and spread (max - min) over the rounds.  `off` against the parent commit is this script run on both
trees in alternating processes, compared by hand: the difference must lie inside the two spreads.
`--kernel` also times qp_phonon_rates alone (device events around `--calls` calls) on 1024^2 planes at NE = 12 and 50 with 1
and 8 regions covering the grid, beside qp_collision_rates on the same planes and regions and qp_collision_step on the
one-wave-per-pixel route with dynamic phonons, and reports the ratios.
python tools/exp_phonon_rates.py [--workloads coupled12 coupled50] [--rounds 5] [--steps 50 250] [--store-steps 3 9]
                                 [--kernel] [--variants off phonon1 ...] [--package DIR] [--json FILE]"""
import argparse
import inspect
import json
import statistics
import sys
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
from exp_rates import PHYSICS, measure, problem  # noqa: E402


def variants(params, regions, wanted):
    out = [("off", lambda steps: dict(store_every=steps))]
    for every in (10, 1):
        if "phonon_rates_out" in params:
            out.append((f"phonon{every}", lambda steps, e=every: dict(store_every=steps, phonon_rates_out={},
                                                                      phonon_rates_regions=regions, phonon_rates_every=e)))
        if "rates_out" in params:
            out.append((f"rates{every}", lambda steps, e=every: dict(store_every=steps, rates_out={}, rates_regions=regions,
                                                                     rates_every=e)))
    out.append(("store1", lambda steps: dict(store_every=1, phonon_history_out={})))
    return [v for v in out if wanted is None or v[0] in wanted]


def kernel_alone(torch, n, ne, calls, rounds):
    """qp_phonon_rates and qp_collision_rates on n^2 cells with 1 and 8 regions covering the grid, and qp_collision_step
    (wave route, dynamic phonons) on the same planes."""
    from qpsim_amd import tables as T
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((n, n), dtype=bool)
    z = np.zeros((1, 1))
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    gap = PHYSICS["energy_gap"]
    E, dE = T.build_energy_grid(gap, 1.0, 3.0, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    nw = int(om.size)
    rho = T.dynes_density_of_states(E, gap, 0.0)
    kr, ks = T.recombination_kernel_base(E, gap, 440.0, 1.2), T.scattering_kernel_base(E, gap, 440.0, 1.2)
    tabs = eng.make_collision_tables(kr[None], ks[None], rho[None], idx_d, idx_s, sg, kernel="wave")
    gen = torch.Generator(device=eng.device).manual_seed(0)
    level = 1e-3 * torch.rand(1, eng.ncell, dtype=torch.float64, device=eng.device, generator=gen)
    state = torch.rand(ne, eng.ncell, dtype=torch.float64, device=eng.device, generator=gen) * level * eng.upload_vector(rho)[:, None]
    ph = (eng.upload_vector(T.thermal_phonon_occupation(om, 0.1))[:, None]
          * (0.5 + torch.rand(nw, eng.ncell, dtype=torch.float64, device=eng.device, generator=gen)))
    state_out, ph_work = torch.empty_like(state), ph.clone()
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

    row = dict(n=n, ne=ne, nw=nw)
    for name, regions in {"1_region_all": [mask], "8_regions_all": [mask] * 8}.items():
        bits = eng.region_bits(regions)
        out_p, out_q = eng.empty(1, len(regions), 4, nw), eng.empty(1, len(regions), 4, ne)
        row["phonon_rates_" + name] = clock(lambda: eng.phonon_rates(tabs, state, ph, bits, 1, float(dE), True, True, out_p))
        row["collision_rates_" + name] = clock(lambda: eng.collision_rates(tabs, state, ph, bits, 1, float(dE), True, True,
                                                                            out_q))
        row["ratio_" + name] = round(row["phonon_rates_" + name]["ms"] / row["collision_rates_" + name]["ms"], 3)
    step = clock(lambda: (ph_work.copy_(ph), eng.collide(tabs, state, state_out, ph_work, float(dE), 0.05, True, True, True)))
    copy = clock(lambda: ph_work.copy_(ph))
    row["collision_step_wave"], row["phonon_copy_alone"] = step, copy
    row["ratio_to_wave_update_1_region"] = round(row["phonon_rates_1_region_all"]["ms"] / (step["ms"] - copy["ms"]), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["coupled12", "coupled50"], choices=["coupled12", "coupled50"])
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, nargs=2, default=[50, 250], metavar=("SHORT", "LONG"))
    ap.add_argument("--store-steps", type=int, nargs=2, default=[3, 9], metavar=("SHORT", "LONG"))
    ap.add_argument("--variants", nargs="+", default=None)
    ap.add_argument("--kernel", action="store_true", help="also time qp_phonon_rates alone")
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
    params = inspect.signature(run).parameters
    rows = []
    warnings.simplefilter("ignore")
    for name in args.workloads:
        ne = int(name[len("coupled"):])
        kw, regions = problem(ne, args.n)
        found = measure(run, torch, kw, variants(params, regions, args.variants), args.rounds, args.steps, args.store_steps)
        med = {k: statistics.median(v) for k, v in found.items()}
        spread = {k: max(v) - min(v) for k, v in found.items()}
        rows.append(dict(workload=name, n=args.n, ms_per_step={k: round(v, 4) for k, v in med.items()},
                         spread_ms={k: round(v, 4) for k, v in spread.items()},
                         rounds_ms={k: [round(x, 4) for x in v] for k, v in found.items()}))
        print(f"{name} {args.n}^2: " + "  ".join(f"{k} {med[k]:.4f} (+-{spread[k]:.4f})" for k in med) + " ms/step", flush=True)
        torch.cuda.empty_cache()
    kernel = []
    if args.kernel and "phonon_rates_out" in params:
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
            package="this checkout" if args.package is None else "another tree (--package)",
            phonon_rates="phonon_rates_out" in params, rounds=args.rounds, steps=args.steps, store1_steps=args.store_steps,
            rows=rows, kernel_alone=kernel), indent=1) + "\n")


if __name__ == "__main__":
    main()
