#!/usr/bin/env python3
"""ms per collision call at sizes without a kernel of their own, with and without padded bins (QP_COLL_PAD_BINS):
  (a) the one-wave-per-pixel kernel at ne (`kernel="wave"`: what the same tables run without the switch);
  (b) the padded one-pass kernel at ne (`pad_bins=True`: the kernel of the ceiling size C on the ne live bins);
  (c) the native one-pass kernel at the ceiling C, on C's own grid (energy_max_factor 3.0).
N^2 cells (default 1024), full mask, recombination + scattering with dynamic phonons, gap 180; the live grids are those of
tests/collision_padded_cases.py (structured bin maps; 29, 31 and 49 with merged bins, i.e. with the stash).  Within one
process, per ne, the three variants alternate for `--rounds` rounds after a warm-up of each; a figure is the time between
two device events around `--calls` calls.  Reported: the median over the rounds and the spread (max - min), and
  b_beats_a   a - b > spread(a) + spread(b)        (the condition for the size to stay in qp_collision_padded_ceiling)
  b_over_c    b / c beside ne^2 / C^2              (b does a subset of c's work: a ratio well above 1 points at the guards)
  b_within_c  b <= c + spread(c)
python tools/exp_padded_bins.py [--n 1024] [--rounds 5] [--calls 3] [--ne 17 25 ...] [--json FILE]"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "quasiparticle-physics-simulation_amd"), str(ROOT / "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import collision_padded_cases as PC  # noqa: E402
from qpsim_amd import _hip  # noqa: E402
from qpsim_amd import tables as T  # noqa: E402
from qpsim_amd.engine import CompiledGeometry, Engine, link_flags  # noqa: E402

DEFAULT_NE = [17, 25, 29, 31, 36, 45, 48, 49]
DT = 0.37


def problem(eng, ne, factor, **table_kw):
    """Tables and inputs of one size on the engine's grid: (handle, state, state_out, phonons, dE)."""
    E, dE = T.build_energy_grid(180.0, 1.0, factor, ne)
    om, idx_d, idx_s, sg = T.build_phonon_frequency_map(E)
    rho = T.dynes_density_of_states(E, 180.0, 0.1)
    kr = T.recombination_kernel_base(E, 180.0, 500.0, 1.2)
    ks = T.scattering_kernel_base(E, 180.0, 400.0, 1.2)
    tab = eng.make_collision_tables(kr[None], ks[None], rho[None], idx_d, idx_s, sg, **table_kw)
    gen = torch.Generator(device=eng.device).manual_seed(1000 * ne)
    rnd = lambda *shape: torch.rand(*shape, dtype=torch.float64, device=eng.device, generator=gen)          # noqa: E731
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=eng.device)          # noqa: E731
    state = rnd(ne, eng.ncell) * dev(rho)[:, None] * 0.3
    ph = dev(T.thermal_phonon_occupation(om, 0.3))[:, None] * (0.5 + rnd(om.size, eng.ncell))
    return tab, state, torch.empty_like(state), ph, float(dE)


def route(eng, tab):
    return eng.lib.qp_collision_route(C.byref(tab["struct"]), eng.ncell, 1, 1, 1, int(bool(tab["merged_slots"])))


def measure(eng, variants, rounds, calls):
    """{name: [ms per call, one per round]}: the variants alternate within a round."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    found = {name: [] for name, _ in variants}

    def run(p):
        tab, state, out, ph, dE = p
        eng.collide(tab, state, out, ph, dE, DT, True, True, True)
    for _, p in variants:          # warm-up of each shape (code objects, scratch, caches)
        for _ in range(2):
            run(p)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, p in variants:
            ev[0].record()
            for _ in range(calls):
                run(p)
            ev[1].record()
            ev[1].synchronize()
            found[name].append(ev[0].elapsed_time(ev[1]) / calls)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--ne", type=int, nargs="+", default=DEFAULT_NE)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternations"
    mask = np.ones((args.n, args.n), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    rows = []
    for ne in args.ne:
        kind = PC.kind_of(ne)
        ceil = PC.ceiling(ne)
        assert ceil and eng.lib.qp_collision_onepass_available(ceil)
        variants = [("a", problem(eng, ne, PC.FACTOR[kind][ne], kernel="wave")),
                    ("b", problem(eng, ne, PC.FACTOR[kind][ne], pad_bins=True)),
                    ("c", problem(eng, ceil, 3.0))]
        routes = [route(eng, p[0]) for _, p in variants]
        if routes != [_hip.ROUTE_WAVE, _hip.ROUTE_ONEPASS_PADDED, _hip.ROUTE_ONEPASS]:
            # a size the ceiling query excludes has no (b): report what ran instead of a figure under a wrong name
            print(f"ne={ne}: routes {routes}: skipped")
            continue
        found = measure(eng, variants, args.rounds, args.calls)
        med = {k: statistics.median(v) for k, v in found.items()}
        spread = {k: max(v) - min(v) for k, v in found.items()}
        row = dict(ne=ne, ceiling=ceil, grid=kind, energy_max_factor=PC.FACTOR[kind][ne],
                   merged_slots=variants[1][1][0]["merged_slots"],
                   ms={k: round(med[k], 4) for k in "abc"}, spread_ms={k: round(spread[k], 4) for k in "abc"},
                   rounds_ms={k: [round(x, 4) for x in v] for k, v in found.items()},
                   b_beats_a=bool(med["a"] - med["b"] > spread["a"] + spread["b"]),
                   a_over_b=round(med["a"] / med["b"], 3), b_over_c=round(med["b"] / med["c"], 3),
                   work_ratio=round(ne * ne / (ceil * ceil), 3), b_within_c=bool(med["b"] <= med["c"] + spread["c"]))
        rows.append(row)
        print(f"ne={ne:2d} C={ceil} {kind:7s}: a {med['a']:.3f} (+-{spread['a']:.3f})  b {med['b']:.3f} (+-{spread['b']:.3f})  "
              f"c {med['c']:.3f} (+-{spread['c']:.3f}) ms/call;  a/b {row['a_over_b']}  b/c {row['b_over_c']} "
              f"(ne^2/C^2 {row['work_ratio']})  b beats a: {row['b_beats_a']}  b within c: {row['b_within_c']}", flush=True)
        del variants
        torch.cuda.empty_cache()
    if args.json:
        info = json.loads(eng.lib.qp_build_info().decode())
        Path(args.json).write_text(json.dumps(dict(
            what="ms per collision call: a = wave kernel at ne, b = padded one-pass kernel at ne, c = native one-pass kernel "
                 "at the ceiling; median and spread (max - min) over the rounds, device events",
            device=torch.cuda.get_device_name(0), build=info, n=args.n, cells=args.n * args.n, rounds=args.rounds,
            calls_per_round=args.calls, dt=DT, physics="recombination + scattering, dynamic phonons, one gap class",
            rows=rows), indent=1) + "\n")


if __name__ == "__main__":
    main()
