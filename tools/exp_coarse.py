#!/usr/bin/env python3
"""ms per step of `run_2d_crank_nicolson` with and without coarse frames, on two workloads:
  coupled   N^2 (default 1024) cells, NE = 12, recombination + scattering, dynamic phonons, ADI (the c-workload parameters:
            gap 180, factors 1-3, tau_0 440, T_c 1.2, T_b 0.1, D0 6, dt 0.1, dx 1, reflective walls)
  scalar    N^2 (default 4096) cells, energy_gap = 0, ADI
and four variants:
  off       store_every = steps, no coarse frames                     (the fast run of today)
  coarse1   store_every = steps, coarse_every = 1, coarse_bin = 8     (a coarse frame per step, kept on the device)
  coarse10  store_every = steps, coarse_every = 10, coarse_bin = 8
  store1    store_every = 1, no coarse frames                         (the only way to a movie without coarse frames)
A package without the `coarse_out` keyword (the parent commit) runs `off` and `store1`; this checkout runs `off`, `coarse1`
and `coarse10` (`--store1` adds `store1`).

One process per package.  `--parent DIR` (a checkout of the parent commit with its library built) makes this script the
driver: it starts a child process on this checkout, one on DIR, and one more on this checkout, so that the parent runs
between two runs of this tree, and writes everything to `--json` (default profiles/coarse_ab.json).  `--control` repeats the
three processes with the parent's variants only (`off` and `store1` in all three), so that `off` is compared between
processes that did the same things.  Without `--parent` the script measures the package of `--package` (default: this
checkout) in its own process, `--only NAMES` restricting the variants.

Per round the variants alternate, each timed with a host clock around the call and a device synchronise at two run lengths
`--steps SHORT LONG`: ms per step = (t_long - t_short) / (LONG - SHORT), which drops the set-up of a run (tables, plans,
uploads, the stores at t = 0 and the end, the one transfer of the coarse frames' set-up).  `store1` keeps every frame on the
host and runs `--store-steps SHORT LONG` instead; `coarse1` runs `--coarse1-steps SHORT LONG`, short enough for its buffer
(one coarse frame of every plane per step) to stay under the 256 MiB limit on both workloads.  Reported per variant: median
and spread (max - min) over the rounds, and
  off_inside_parent_spread   min(parent off rounds) <= median(off of this tree) <= max(parent off rounds), per run of this
                             tree; `off_no_slower_than_parent` asks only for the upper end
  coarse1_beats_store1       store1(parent) - coarse1 > max(spread(store1), spread(coarse1))
`--kernel` also times qp_block_sums (b = 8) alone with device events around `--calls` calls on the planes of both workloads,
and qp_region_sums with 3 regions on the same planes in the same process, and reports the bytes a call moves (8 B per cell
and field + 1 B per cell of flags or bits) over 8 TB/s.
python tools/exp_coarse.py [--parent DIR] [--workloads coupled scalar] [--rounds 5] [--steps 50 450] [--store-steps 10 30] [--coarse1-steps 30 120] [--kernel] [--control] [--json FILE]"""
import argparse
import gc
import inspect
import json
import statistics
import subprocess
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
HBM_PEAK_GBS = 8000.0
BIN = 8


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
    return kw


def variants(coarse: bool, store1: bool, only=None):
    if only:
        return [v for v in variants(coarse, True) if v[0] in only]
    out = [("off", lambda steps: dict(store_every=steps))]
    if coarse:
        out += [("coarse1", lambda steps: dict(store_every=steps, coarse_out={}, coarse_bin=BIN, coarse_every=1)),
                ("coarse10", lambda steps: dict(store_every=steps, coarse_out={}, coarse_bin=BIN, coarse_every=10))]
    if store1:
        out.append(("store1", lambda steps: dict(store_every=1)))
    return out


def timed(run, torch, kw, extra, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    more = extra(steps)
    res = run(**kw, total_time=steps * kw["dt"], **more)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    assert len(res[0]) == (steps + 1 if more["store_every"] == 1 else 2)
    if "coarse_out" in more:
        assert len(more["coarse_out"]["times"]) == 1 + -(-steps // more["coarse_every"])
    del res, more
    gc.collect()
    return 1e3 * (t1 - t0)


def measure(run, torch, kw, todo, rounds, steps, store_steps, coarse1_steps):
    found = {name: [] for name, _ in todo}
    lengths = {name: {"store1": store_steps, "coarse1": coarse1_steps}.get(name, steps) for name, _ in todo}
    for name, extra in todo:                    # warm-up of every variant: code objects, plans, pinned staging buffers
        timed(run, torch, kw, extra, lengths[name][0])
    for _ in range(rounds):
        for name, extra in todo:
            short, long = lengths[name]
            a = timed(run, torch, kw, extra, short)
            b = timed(run, torch, kw, extra, long)
            found[name].append((b - a) / (long - short))
    return found


def kernels_alone(torch, n, nfield, calls, rounds):
    """qp_block_sums (b = 8) and qp_region_sums (3 regions) on the same planes: ms per call from device events."""
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((n, n), dtype=bool)
    z = np.zeros((1, 1))
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    state = torch.rand(nfield, eng.ncell, dtype=torch.float64, device=eng.device)
    regions = [mask] + [np.random.default_rng(r).random(mask.shape) < 0.5 for r in (1, 2)]
    bits = eng.region_bits(regions)
    region_out = eng.empty(1, 3, nfield)
    block_out = eng.empty(1, nfield, -(-n // BIN), -(-n // BIN))
    todo = {"qp_block_sums": lambda: eng.block_sums(state, 1, BIN, 0, 0, block_out),
            "qp_region_sums": lambda: eng.region_sums(state, bits, 1, region_out)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {name: [] for name in todo}
    for call in todo.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, call in todo.items():
            ev[0].record()
            for _ in range(calls):
                call()
            ev[1].record()
            ev[1].synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]) / calls)
    nbytes = eng.ncell * (8.0 * nfield + 1.0)
    rows = []
    for name, found in ms.items():
        med = statistics.median(found)
        rows.append(dict(kernel=name, n=n, nfield=nfield, ms=round(med, 5), spread_ms=round(max(found) - min(found), 5),
                         bytes=nbytes, gbs=round(nbytes / med / 1e6, 1), share_of_8tbs=round(nbytes / med / 1e6 / HBM_PEAK_GBS, 3)))
        print(f"{name} {n}^2 x {nfield} planes: {rows[-1]['ms']:.4f} ms (+-{rows[-1]['spread_ms']:.4f}), "
              f"{rows[-1]['gbs']:.0f} GB/s = {rows[-1]['share_of_8tbs']:.3f} of 8 TB/s", flush=True)
    return rows


def measure_package(args):
    """This process measures one package and returns its record."""
    pkg = Path(args.package).resolve() if args.package else ROOT
    for p in (str(pkg), str(pkg / "quasiparticle-physics-simulation_amd")):
        sys.path.insert(0, p)
    import torch
    from qpsim_amd import _hip
    from qpsim_amd.solver import run_2d_crank_nicolson as run
    coarse = "coarse_out" in inspect.signature(run).parameters
    rows = []
    warnings.simplefilter("ignore")
    for name in args.workloads:
        n = args.n_coupled if name == "coupled" else args.n_scalar
        found = measure(run, torch, problem(name, n), variants(coarse, args.store1 or not coarse, args.only), args.rounds, args.steps,
                        args.store_steps, args.coarse1_steps)
        med = {k: statistics.median(v) for k, v in found.items()}
        spread = {k: max(v) - min(v) for k, v in found.items()}
        rows.append(dict(workload=name, n=n, ms_per_step={k: round(v, 4) for k, v in med.items()},
                         spread_ms={k: round(v, 4) for k, v in spread.items()},
                         rounds_ms={k: [round(x, 4) for x in v] for k, v in found.items()},
                         over_off={k: round(v / med["off"], 3) for k, v in med.items()}))
        print(f"{name} {n}^2: " + "  ".join(f"{k} {med[k]:.4f} (+-{spread[k]:.4f})" for k in med) + " ms/step", flush=True)
        torch.cuda.empty_cache()
    kernel = []
    if args.kernel and coarse:
        for n, nfield in ((args.n_coupled, 12), (args.n_scalar, 1)):
            kernel += kernels_alone(torch, n, nfield, args.calls, args.rounds)
    return dict(package="this checkout" if args.package is None else "another tree (--package)", coarse_frames=coarse,
                device=torch.cuda.get_device_name(0), build=json.loads(_hip.load().qp_build_info().decode()), rows=rows,
                kernels_alone=kernel)


def child(args, package, kernel: bool, out: Path, only=()) -> dict:
    """A fresh process for one package (the driver itself never opens the device)."""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--workloads", *args.workloads, "--n-coupled", str(args.n_coupled),
           "--n-scalar", str(args.n_scalar), "--rounds", str(args.rounds), "--steps", *map(str, args.steps), "--store-steps",
           *map(str, args.store_steps), "--coarse1-steps", *map(str, args.coarse1_steps), "--calls", str(args.calls), "--json", str(out)]
    if package is not None:
        cmd += ["--package", str(package)]
    if kernel:
        cmd.append("--kernel")
    if only:
        cmd += ["--only", *only]
    subprocess.run(cmd, check=True, timeout=args.child_timeout)
    return json.loads(out.read_text())


def compare_off(this_runs, parent):
    """Condition 1 alone, per workload (the control: every process ran `off` and `store1`)."""
    verdicts = []
    for k, prow in enumerate(parent["rows"]):
        off_parent = prow["rounds_ms"]["off"]
        offs = [run["rows"][k]["ms_per_step"]["off"] for run in this_runs]
        verdicts.append(dict(workload=prow["workload"], n=prow["n"], parent_off_ms=prow["ms_per_step"]["off"],
                             parent_off_min_max=[min(off_parent), max(off_parent)], this_off_ms=offs,
                             this_off_spread_ms=[run["rows"][k]["spread_ms"]["off"] for run in this_runs],
                             off_inside_parent_spread=[bool(min(off_parent) <= off <= max(off_parent)) for off in offs],
                             off_no_slower_than_parent=[bool(off <= max(off_parent)) for off in offs]))
        print("control " + json.dumps(verdicts[-1]), flush=True)
    return verdicts


def compare(this_runs, parent):
    """The two conditions, per workload."""
    verdicts = []
    for k, prow in enumerate(parent["rows"]):
        off_parent = prow["rounds_ms"]["off"]
        store1, store1_spread = prow["ms_per_step"]["store1"], prow["spread_ms"]["store1"]
        v = dict(workload=prow["workload"], n=prow["n"], parent_off_ms=prow["ms_per_step"]["off"],
                 parent_off_min_max=[min(off_parent), max(off_parent)], parent_store1_ms=store1,
                 parent_store1_spread_ms=store1_spread, this=[])
        for run in this_runs:
            row = run["rows"][k]
            off, c1, c1_spread = row["ms_per_step"]["off"], row["ms_per_step"]["coarse1"], row["spread_ms"]["coarse1"]
            v["this"].append(dict(
                off_ms=off, off_spread_ms=row["spread_ms"]["off"], off_over_parent_off=round(off / prow["ms_per_step"]["off"], 4),
                off_inside_parent_spread=bool(min(off_parent) <= off <= max(off_parent)),
                off_no_slower_than_parent=bool(off <= max(off_parent)),
                coarse1_ms=c1, coarse1_spread_ms=c1_spread, coarse10_ms=row["ms_per_step"]["coarse10"],
                coarse1_over_off=round(c1 / off, 3), coarse10_over_off=round(row["ms_per_step"]["coarse10"] / off, 3),
                store1_over_coarse1=round(store1 / c1, 2),
                coarse1_beats_store1=bool(store1 - c1 > max(store1_spread, c1_spread))))
        verdicts.append(v)
        print(json.dumps(v), flush=True)
    return verdicts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["coupled", "scalar"], choices=["coupled", "scalar"])
    ap.add_argument("--n-coupled", type=int, default=1024)
    ap.add_argument("--n-scalar", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, nargs=2, default=[50, 450], metavar=("SHORT", "LONG"))
    ap.add_argument("--store-steps", type=int, nargs=2, default=[10, 30], metavar=("SHORT", "LONG"))
    ap.add_argument("--coarse1-steps", type=int, nargs=2, default=[30, 120], metavar=("SHORT", "LONG"))
    ap.add_argument("--store1", action="store_true", help="run store1 on a package with coarse frames too")
    ap.add_argument("--kernel", action="store_true", help="also time qp_block_sums and qp_region_sums alone")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--package", default=None, help="tree to import qpsim_amd from (default: this checkout)")
    ap.add_argument("--parent", default=None, help="checkout of the parent commit: drive this tree, the parent, this tree")
    ap.add_argument("--control", action="store_true", help="driver: three more processes with `off` and `store1` only")
    ap.add_argument("--only", nargs="+", default=None, help="measure these variants only")
    ap.add_argument("--child-timeout", type=float, default=500.0, help="seconds one child process may take")
    ap.add_argument("--json", default=None, help="write the figures to this file (driver: profiles/coarse_ab.json)")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternations"
    if args.parent is None:
        record = measure_package(args)
        if args.json:
            Path(args.json).parent.mkdir(parents=True, exist_ok=True)
            Path(args.json).write_text(json.dumps(record, indent=1) + "\n")
        return
    target = Path(args.json) if args.json else ROOT / "profiles" / "coarse_ab.json"
    target.parent.mkdir(parents=True, exist_ok=True)
    part = lambda k: target.with_name(f"{target.stem}.part{k}.json")      # noqa: E731
    first = child(args, None, args.kernel, part(0))
    parent = child(args, Path(args.parent).resolve(), False, part(1))
    second = child(args, None, False, part(2))
    assert not parent["coarse_frames"], "--parent must be a tree without coarse frames"
    record = dict(
        what="ms per step of run_2d_crank_nicolson, (t_long - t_short) / (long - short) with a host clock around the call "
             "and a device synchronise; median and spread (max - min) over the rounds, variants alternating inside a process; "
             "processes in the order this tree, parent commit, this tree; store1 and coarse1 at their own, shorter run lengths",
        rounds=args.rounds, steps=args.steps, store1_steps=args.store_steps, coarse1_steps=args.coarse1_steps, coarse_bin=BIN,
        this_tree_first=first, parent=parent, this_tree_second=second, conditions=compare([first, second], parent))
    if args.control:
        same = ("off", "store1")
        runs = [child(args, None, False, part(0), same), child(args, Path(args.parent).resolve(), False, part(1), same),
                child(args, None, False, part(2), same)]
        record["control_off_and_store1_in_every_process"] = dict(
            this_tree_first=runs[0], parent=runs[1], this_tree_second=runs[2], condition_1=compare_off([runs[0], runs[2]], runs[1]))
    target.write_text(json.dumps(record, indent=1) + "\n")
    for k in range(3):
        part(k).unlink()


if __name__ == "__main__":
    main()
