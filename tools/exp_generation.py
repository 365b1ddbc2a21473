#!/usr/bin/env python3
"""ms per step of a run with a `custom` generation expression, evaluated on the host and on the device:
  (a) `generation_on_device=False`: NumPy on [NE, n], upload, qp_add_scaled (the path of every earlier revision);
  (b) `generation_on_device=True`: slots on the host, qp_add_generation_expr on the device;
  (c) `constant` generation of the same run: the floor (one qp_add_constant per step).
N^2 cells (default 1024), NE = 12, full physics (ADI diffusion, recombination, scattering, dynamic phonons), a Gaussian spot
with a t-window as the body.  Each figure is the difference of two run lengths (setup, first / last store excluded); the
three variants alternate within a round after a warm-up of each.  Then the generation call alone (device events): host path
(evaluation + upload + qp_add_scaled, wall clock, as it blocks the host) against the one kernel.
python tools/exp_generation.py [--n 1024] [--repeat 3] [--steps 20] [--json FILE]"""
import argparse
import json
import sys
import time
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "quasiparticle-physics-simulation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from qpsim_amd import device_expr  # noqa: E402
from qpsim_amd.geometry import extract_edge_segments  # noqa: E402
from qpsim_amd.models import BoundaryCondition, ExternalGenerationSpec  # noqa: E402
from qpsim_amd.solver import _Generation, build_energy_grid, run_2d_crank_nicolson  # noqa: E402

warnings.simplefilter("ignore")
BODY = "params['a']*np.exp(-((x-0.5)**2+(y-0.5)**2)/params['w'])*(1.0 if t<1e9 else 0.0)"
SPOT = ExternalGenerationSpec(mode="custom", custom_body=BODY, custom_params={"a": 2e-6, "w": 0.02})
CONSTANT = ExternalGenerationSpec(mode="constant", rate=2e-6)
NE = 12


def per_step(fn, short, long):
    el = []
    for k in (short, long):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        el.append(time.perf_counter() - t0)
    return 1e3 * (el[1] - el[0]) / (long - short)


def common(N):
    mask = np.ones((N, N), dtype=bool)
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    init = 1e-4 * (1.0 + np.random.default_rng(0).random((N, N)))
    return dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1, dx=1.0,
                energy_gap=180.0, energy_max_factor=3.0, num_energy_bins=NE, enable_recombination=True,
                enable_scattering=True, diffusion_scheme="adi")


def runs(N, repeat, steps, short=3):
    kw = common(N)
    variants = [("a: custom on the host", SPOT, False), ("b: custom on the device", SPOT, True), ("c: constant", CONSTANT, False)]

    def runner(spec, on):
        return lambda k: run_2d_crank_nicolson(total_time=0.1 * k, store_every=k, external_generation=spec,
                                               generation_on_device=on, **kw)

    for _, spec, on in variants:
        runner(spec, on)(2)
    found = {name: [] for name, _, _ in variants}
    for r in range(repeat):
        for name, spec, on in variants:
            ms = per_step(runner(spec, on), short, short + steps)
            found[name].append(round(ms, 4))
            print(f"{N}^2 NE={NE}, round {r}: {name}: {ms:.3f} ms/step  {device_expr.last_run_stats()}", flush=True)
    return found


def generation_alone(N, repeat, calls=5):
    """The generation call of one step alone: (a) wall clock of evaluation + upload + qp_add_scaled until the device is done,
    (b) device time of qp_add_generation_expr with its table upload and status read-back, by events."""
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    mask = np.ones((N, N), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z))
    E, _ = build_energy_grid(180.0, 1.0, 3.0, NE)
    gen = _Generation(SPOT, mask, E, on_device=True)
    assert gen.program is not None
    state = eng.empty(NE, eng.ncell).zero_()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    found = {"a: host path, wall ms": [], "b: device kernel, event ms": [], "b: device path, wall ms": []}
    for r in range(repeat + 1):                                  # round 0 warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(calls):
            eng.add_scaled(state, eng.upload_packed(gen.rates(0.1 * k)), 0.1)
        torch.cuda.synchronize()
        host = 1e3 * (time.perf_counter() - t0) / calls
        t0 = time.perf_counter()
        ev[0].record()
        for k in range(calls):
            ticket = eng.add_generation_expr(state, gen.window, [gen.device_step(0.1 * k) + (None,)], 0.1, 1, eng.d_flags)
            assert eng.generation_status(ticket) == [(False, False)]
        ev[1].record()
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0) / calls
        if r:
            found["a: host path, wall ms"].append(round(host, 4))
            found["b: device kernel, event ms"].append(round(ev[0].elapsed_time(ev[1]) / calls, 4))
            found["b: device path, wall ms"].append(round(wall, 4))
            print(f"generation alone {N}^2 NE={NE}, round {r - 1}: host path {host:.3f} ms, device {wall:.3f} ms wall, "
                  f"{found['b: device kernel, event ms'][-1]:.3f} ms by events", flush=True)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="step difference of the two run lengths")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    found = runs(args.n, args.repeat, args.steps)
    alone = generation_alone(args.n, args.repeat)
    a, b, c = (np.array(found[k]) for k in found)
    print(f"b/a per round: {np.round(b / a, 3).tolist()}  b/c per round: {np.round(b / c, 3).tolist()}")
    if args.json:
        Path(args.json).write_text(json.dumps(
            {"grid": [args.n, args.n], "num_energy_bins": NE, "steps": args.steps, "body": BODY,
             "device": torch.cuda.get_device_name(), "ms_per_step": found, "b_over_a": np.round(b / a, 4).tolist(),
             "b_over_c": np.round(b / c, 4).tolist(), "generation_alone_ms": alone}, indent=1) + "\n")


if __name__ == "__main__":
    main()
