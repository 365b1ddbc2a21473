#!/usr/bin/env python3
"""ms per collision call at 65 ... 128 energy bins, with and without wide bins (QP_COLL_WIDE_BINS):
  (a)  the generic one-thread-per-cell kernel with its 2 nw ncell doubles of scratch (`kernel="generic"`: what the size runs
       without the switch);
  (b)  the two-bins-per-lane wave kernel (`wide_bins=True`);
  (c)  once per grid, as an anchor: the one-wave-per-pixel kernel at ne = 64.
N^2 cells (default 512), full mask, recombination + scattering with dynamic phonons, gap 180, energy_max_factor 3.0 (65 has
unstructured bin maps there and runs the atomic form; 72, 96, 100, 128 are structured).  Within one process, per ne, the
variants alternate for `--rounds` rounds after a warm-up of each; a figure is the time between two device events around
`--calls` calls.  Reported: the median over the rounds and the spread (max - min), the scratch bytes of (a), and
  b_beats_a   a - b > spread(a) + spread(b)        (the condition for the size to stay in qp_collision_wide_available)
  b_over_c    b / c beside (ne / 64)^2             (a diagnostic, not a criterion)
Run it under a `timeout` of its own, one process per grid size:
python tools/exp_wide_bins.py [--n 512] [--rounds 5] [--calls 3] [--ne 65 72 ...] [--json FILE]"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "quasiparticle-physics-simulation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from qpsim_amd import _hip  # noqa: E402
from qpsim_amd import tables as T  # noqa: E402
from qpsim_amd.collision_tables import scratch_planes  # noqa: E402
from qpsim_amd.engine import CompiledGeometry, Engine, link_flags  # noqa: E402

DEFAULT_NE = [65, 72, 96, 100, 128]
DT = 0.37


def problem(eng, ne, **table_kw):
    """Tables and inputs of one size on the engine's grid: (handle, state, state_out, phonons, dE)."""
    E, dE = T.build_energy_grid(180.0, 1.0, 3.0, ne)
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
    scratch = scratch_planes(tab, True, True, True) > 0
    return eng.lib.qp_collision_route(C.byref(tab["struct"]), eng.ncell, 1, 1, 1, int(scratch))


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
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--ne", type=int, nargs="+", default=DEFAULT_NE)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternations"
    mask = np.ones((args.n, args.n), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    anchor = problem(eng, 64, kernel="wave")
    assert route(eng, anchor[0]) == _hip.ROUTE_WAVE
    c = measure(eng, [("c", anchor)], args.rounds, args.calls)["c"]
    c_med, c_spread = statistics.median(c), max(c) - min(c)
    print(f"anchor: wave kernel at ne=64: c {c_med:.3f} (+-{c_spread:.3f}) ms/call", flush=True)
    del anchor
    torch.cuda.empty_cache()
    rows = []
    for ne in args.ne:
        generic, wide = problem(eng, ne, kernel="generic"), problem(eng, ne, wide_bins=True)
        variants = [("a", generic), ("b", wide)]
        routes = [route(eng, generic[0]), route(eng, wide[0])]
        if routes != [_hip.ROUTE_GENERIC, _hip.ROUTE_WAVE_WIDE]:
            # a size the query excludes has no (b): report what ran instead of a figure under a wrong name
            print(f"ne={ne}: routes {routes}: skipped")
            continue
        nw = generic[0]["nw"]
        scratch = 2 * scratch_planes(generic[0], True, True, True) * eng.ncell * 8
        assert scratch == 2 * nw * eng.ncell * 8 and scratch_planes(wide[0], True, True, True) == 0
        found = measure(eng, variants, args.rounds, args.calls)
        med = {k: statistics.median(v) for k, v in found.items()}
        spread = {k: max(v) - min(v) for k, v in found.items()}
        row = dict(ne=ne, nw=nw, structured=wide[0]["diag_bin"] is not None, scratch_bytes_a=scratch,
                   ms={k: round(med[k], 4) for k in med}, spread_ms={k: round(spread[k], 4) for k in spread},
                   rounds_ms={k: [round(x, 4) for x in v] for k, v in found.items()},
                   b_beats_a=bool(med["a"] - med["b"] > spread["a"] + spread["b"]),
                   a_over_b=round(med["a"] / med["b"], 3), b_over_c=round(med["b"] / c_med, 3),
                   work_ratio=round(ne * ne / 4096.0, 3))
        rows.append(row)
        print(f"ne={ne:3d} nw={nw}: a {med['a']:.3f} (+-{spread['a']:.3f}; scratch {scratch / 2**30:.2f} GiB)  "
              f"b {med['b']:.3f} (+-{spread['b']:.3f}) ms/call;  a/b {row['a_over_b']}  b/c {row['b_over_c']} "
              f"((ne/64)^2 {row['work_ratio']})  b beats a: {row['b_beats_a']}",
              flush=True)
        del variants, generic, wide
        eng._scratch.pop("coll_acc", None)          # the accumulator planes of (a): sized per ne
        torch.cuda.empty_cache()
    if args.json:
        info = json.loads(eng.lib.qp_build_info().decode())
        Path(args.json).write_text(json.dumps(dict(
            what="ms per collision call: a = generic kernel at ne (with scratch_bytes_a of accumulator planes), b = wide wave "
                 "kernel at ne, c = wave kernel at ne = 64 on the same grid; median and "
                 "spread (max - min) over the rounds, device events",
            device=torch.cuda.get_device_name(0), build=info, n=args.n, cells=args.n * args.n, rounds=args.rounds,
            calls_per_round=args.calls, dt=DT, physics="recombination + scattering, dynamic phonons, one gap class",
            anchor_c=dict(ne=64, ms=round(c_med, 4), spread_ms=round(c_spread, 4), rounds_ms=[round(x, 4) for x in c]),
            rows=rows), indent=1) + "\n")


if __name__ == "__main__":
    main()
