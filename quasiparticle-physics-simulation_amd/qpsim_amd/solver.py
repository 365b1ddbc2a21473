"""MI355X-native drop-in for ``qpsim.solver``: same run / step API, HIP kernels underneath.

``run_2d_crank_nicolson`` keeps the reference's signature, defaults, return tuple, error types and
messages (``/root/reference/qpsim/solver.py:999-1587``); the state lives on the GPU for the whole run
and only crosses PCIe at store points.  Additive keyword arguments (all optional):

``diffusion_scheme``
    ``"cn_exact"`` (default) reproduces the reference's unsplit Crank-Nicolson step to ``cn_rtol`` by an
    ADI-preconditioned iteration built from the same two sweep kernels; ``"adi"`` takes the single
    Peaceman-Rachford step (the benchmarked kernel; identical on one-cell-thick strips, O(dt^3) splitting
    error per step on true 2-D grids).
``device``
    torch device (default: current CUDA/HIP device).
``generation_on_device``
    ``True`` evaluates a ``custom`` generation expression inside the device subset of ``device_expr`` in a HIP kernel
    instead of NumPy + an upload per step; its non-finite / negative check then arrives with the Pauli guard of the step
    (up to ``Engine.GUARD_LAG`` steps late, before anything is stored).  Expressions outside the subset, every other
    generation mode and the default ``False`` run exactly as before.
``collision_padded_bins``
    ``True`` lets a ``num_energy_bins`` between 17 and 49 that has no collision kernel of its own (every size but 18, 20,
    24, 30, 32, 40) run the one-pass kernel of the next instantiated size (30, 32, 40, 50) on its live bins instead of the
    one-wave-per-pixel kernel, where the phonon bin maps are structured and the gap is uniform (``QP_COLL_PAD_BINS``).
    Sizes 51 ... 64, non-uniform gaps at any size and the double half-step pass (``num_energy_bins`` <= 16) are not
    affected; the default ``False`` runs exactly as before.  Results agree with the default to rounding (another
    summation order), not bit for bit.
``collision_wide_bins``
    ``True`` lets a ``num_energy_bins`` between 65 and 128 (at most 512 phonon bins) run a one-wave-per-pixel collision
    kernel with two energy bins per lane instead of the generic one-thread-per-cell kernel (``QP_COLL_WIDE_BINS``): no
    ``2 nw ncell`` accumulator planes are allocated, uniform and non-uniform gaps and ensemble sweeps alike.  Every other
    size ignores it; the default ``False`` runs exactly as before.  Results agree with the default to rounding (another
    summation order), not bit for bit.
``trace_out``, ``trace_regions``, ``trace_every``
    Time traces without stored frames: with a dict as ``trace_out`` the sums of every energy plane over up to 8 named
    regions (``trace_regions``: name -> boolean array of the mask's shape, regions may overlap; None: one region ``"all"``
    = the mask) are reduced on the device at t = 0, every ``trace_every``-th step and the last step, kept there, and
    fetched once when the run ends.  ``trace_out`` is cleared at entry and filled on normal return with ``times`` [S],
    ``regions`` (names), ``cells`` (interior cells per region), ``energy_bins`` (None in scalar mode), ``density``
    [S, R, NE] = sum over the region's cells of each plane (scalar mode: NE = 1, the plane is u) and ``number`` [S, R] =
    dx^2 dE sum_i density (scalar mode: dx^2 density).  A sampled step is sequenced like a stored one (no fused pair pass
    across it), so its state is bit for bit the state a run with ``store_every = trace_every`` stores there.  The default
    ``trace_out=None`` runs exactly as before.
``coarse_out``, ``coarse_bin``, ``coarse_every``
    Coarse frames without stored frames - where the quasiparticles are as they evolve: with a dict as ``coarse_out`` the
    sums of every energy plane over blocks of ``coarse_bin`` x ``coarse_bin`` cells (2, 4, 8, 16, 32 or 64; aligned to the
    origin of the mask's frame) are taken on the device at t = 0, every ``coarse_every``-th step and the last step, kept
    there, and fetched once when the run ends.  ``coarse_out`` is cleared at entry and filled on normal return with
    ``times`` [S], ``bin``, ``cells`` [cy, cx] (in-mask cells per block, cy = ceil(H / bin), cx = ceil(W / bin)),
    ``energy_bins`` (None in scalar mode, where NE = 1 and the plane is u), ``energy_sums`` [S, NE, cy, cx] (the device
    sums, 0.0 in blocks the mask's bounding box does not touch), ``energy_frames`` [S, NE, cy, cx] = ``energy_sums / cells``
    and ``frames`` [S, cy, cx] = the block mean of the integrated density, dE sum_i ``energy_sums[:, i]`` / ``cells`` (scalar
    mode: ``energy_sums[:, 0] / cells``); both are NaN where ``cells == 0``.  A sampled step is sequenced like a stored one,
    as for the traces; with both sinks each samples at the steps of its own cadence.  Not covered: phonon planes,
    domain-decomposed runs, rectangular or non-power-of-two blocks.  The default ``coarse_out=None`` runs exactly as before.
``rates_out``, ``rates_regions``, ``rates_every``
    Collision rate traces - where the quasiparticles go: with a dict as ``rates_out`` the four per-bin collision terms
    (``channels`` = scattering_in, scattering_out, recombination, pair_breaking, each >= 0 in units of dn_i/dt; the header
    of ``qp_collision_rates`` has the formulas) are evaluated on the device from the state and the phonons at t = 0, every
    ``rates_every``-th step and the last step, summed over up to 8 named regions (``rates_regions``, as ``trace_regions``),
    kept there, and fetched once when the run ends.  ``rates_out`` is cleared at entry and filled on normal return with
    ``times`` [S], ``regions``, ``cells``, ``energy_bins``, ``channels``, ``rates`` [S, R, 4, NE] and ``number_rates``
    [S, R, 4] = dx^2 dE sum_i rates.  A sampled step is sequenced like a stored one and sees the state and the phonons
    after its closing half-step, with the run's ``enable_recombination`` / ``enable_scattering`` (a disabled process gives
    exact zeros).  Served: uniform and non-uniform gaps, ensembles and their sweeps, 2 to 64 energy bins.  Refused with a
    ``ValueError``: scalar mode, both processes off, more than 64 energy bins (also with ``collision_wide_bins``).  Not
    covered here: rates per phonon bin, which ``phonon_rates_out`` gives.  The default ``rates_out=None`` runs exactly as
    before.
``phonon_rates_out``, ``phonon_rates_regions``, ``phonon_rates_every``
    Phonon rate traces - what the quasiparticles emit and what is absorbed again, per phonon bin: with a dict as
    ``phonon_rates_out`` the four terms of the phonon equation (``channels`` = scattering_emission, scattering_absorption,
    recombination_emission, pair_breaking_absorption, each >= 0 in units of dN_w/dt; the header of ``qp_phonon_rates`` has
    the formulas) are evaluated on the device from the state and the phonons at t = 0, every ``phonon_rates_every``-th step
    and the last step, summed over up to 8 named regions (``phonon_rates_regions``, as ``trace_regions``), kept there, and
    fetched once when the run ends.  The sink is cleared at entry and filled on normal return with ``times`` [S],
    ``regions``, ``cells``, ``channels``, ``phonon_energy_bins`` [NW], ``rates`` [S, R, 4, NW] and ``integrated_rates``
    [S, R, 4] = dx^2 sum_w width_w rates with the integration widths of the phonon frames.  The rates are defined whether
    or not the run updates its phonons (frozen phonons: what the bath receives).  Sequencing, process switches, what is
    served and what is refused are those of ``rates_out``.  Not covered: unstructured phonon-bin maps, domain-decomposed
    runs, region sums of the phonon occupations themselves.  The default ``phonon_rates_out=None`` runs exactly as before.
``flux_out``, ``flux_surfaces``, ``flux_every``
    Boundary outflow traces - what leaves through the walls: with a dict as ``flux_out`` the diffusive loss through up to 64
    named surfaces (``flux_surfaces``: name -> non-empty list of edge ids of ``edges``, surfaces may overlap; None: one
    surface ``"all"`` made of every edge) is evaluated on the device from the state at t = 0, every ``flux_every``-th step
    and the last step, kept there, and fetched once when the run ends.  A boundary face belongs to the edge whose boundary
    condition the operator applies to it (the last edge listing it) and carries (diag, src) in 1/dx^2 units: reflective
    (0, 0), absorbing (2, 0), dirichlet g (2, 2 g), neumann q (0, q dx), robin beta, gamma (beta dx, gamma dx); it adds
    D (-diag u + src) / dx^2 to du/dt of its cell, D being the bin's coefficient (the cell's own D with a non-uniform gap).
    ``outflow[s, i]`` = sum over the faces of surface s of D (diag u_i - src) is positive when quasiparticles leave and
    negative for an injecting source; it is minus the boundary contribution to d/dt sum_p u_i dx^2.  Faces with diag = src =
    0 are dropped on the host (their cells are never read); a surface left without faces reports +0.0.  ``flux_out`` is
    cleared at entry and filled on normal return with ``times`` [S], ``surfaces`` (names), ``faces`` (count per surface
    after dropping), ``energy_bins`` (None in scalar mode), ``outflow`` [S, surfaces, planes] and ``number_outflow``
    [S, surfaces] = dE sum_i outflow (scalar mode: outflow[..., 0]), the rate at which the run's ``mass`` is lost through
    the surface.  A sampled step is sequenced like a stored one.  Served: scalar and energy-resolved mode, both diffusion
    schemes, uniform and non-uniform gaps, ensembles and their sweeps.  Refused with a ``ValueError``:
    ``enable_diffusion=False`` (no operator, no boundary term).  Not covered: domain-decomposed runs (they do not pass
    through this call; ``Engine.boundary_flux`` refuses their block plans), phonon planes (they do not diffuse), per-face
    output, time integration on the device.  The default ``flux_out=None`` runs exactly as before.

Table builders and helpers the reference exports from ``qpsim.solver`` are re-exported here under
the same names.
"""
from __future__ import annotations

import warnings
from typing import Any, Callable

import numpy as np

from . import tables as _tb
from .engine import (COARSE_BINS, FLUX_SURFACES, BoundaryAssignmentError, DiffusionOperator, Engine, coarse_layout,
                     compile_boundary_faces, compile_geometry)
from .models import (
    BoundaryCondition,
    EdgeSegment,
    ExternalGenerationSpec,
    InitialConditionSpec,
    SimulationParameters,
    normalize_collision_solver_name,
)
from . import device_expr
from .safe_eval import compile_safe_expression
from .timeloop import EnergyRun, Outputs, Sampler, Schedule, energy_loop, scalar_loop

# names the reference exposes from qpsim.solver
build_energy_grid = _tb.build_energy_grid
integration_widths_from_centers = _tb.integration_widths_from_centers
_bcs_density_of_states = _tb.bcs_density_of_states
_dynes_density_of_states = _tb.dynes_density_of_states
thermal_phonon_occupation = _tb.thermal_phonon_occupation
thermal_qp_weights = _tb.thermal_qp_weights
recombination_kernel_base = _tb.recombination_kernel_base
scattering_kernel_base = _tb.scattering_kernel_base
recombination_kernel = _tb.recombination_kernel
scattering_kernel = _tb.scattering_kernel
_build_phonon_frequency_map = _tb.build_phonon_frequency_map
_KB_UEV_PER_K = _tb.KB_UEV_PER_K

__all__ = [
    "BoundaryAssignmentError", "run_2d_crank_nicolson", "reconstruct_field", "build_fixed_phonon_history",
    "evaluate_external_generation", "build_energy_grid", "integration_widths_from_centers",
    "thermal_phonon_occupation", "thermal_qp_weights", "recombination_kernel_base", "scattering_kernel_base",
    "recombination_kernel", "scattering_kernel", "apply_collision_step_fischer_catelani_uniform",
    "apply_collision_step_fischer_catelani_nonuniform", "apply_scattering_step", "apply_recombination_step",
    "build_laplacian_with_boundaries", "build_variable_diffusion_laplacian",
]


def reconstruct_field(mask: np.ndarray, values: np.ndarray) -> np.ndarray:
    """Interior values -> NaN-padded [ny, nx] frame (solver.py:215-218)."""
    out = np.full(mask.shape, np.nan, dtype=float)
    out[mask] = values
    return out


def build_fixed_phonon_history(*, mask: np.ndarray, times, bath_temperature: float,
                               phonon_energy_bins: np.ndarray | None = None):
    """Constant-temperature phonon outputs aligned with stored times (solver.py:373-426)."""
    mask_b = np.asarray(mask, dtype=bool)
    n = int(mask_b.sum())
    if n == 0:
        raise ValueError("Geometry mask has no interior points.")
    if len(times) <= 0:
        raise ValueError("times must contain at least one stored timepoint.")
    base = reconstruct_field(mask_b, np.full(n, float(bath_temperature)))
    frames = [base.copy() for _ in range(len(times))]
    eframes = None
    bins = None
    if phonon_energy_bins is not None:
        bins = np.asarray(phonon_energy_bins, dtype=float).copy()
        if bins.ndim != 1:
            raise ValueError("phonon_energy_bins must be a 1D array.")
        if np.any(~np.isfinite(bins)):
            raise ValueError("phonon_energy_bins must contain only finite values.")
        if np.any(bins < 0):
            raise ValueError("phonon_energy_bins must be non-negative.")
        per_bin = [reconstruct_field(mask_b, np.full(n, float(v)))
                   for v in thermal_phonon_occupation(bins, float(bath_temperature))]
        eframes = [[f.copy() for f in per_bin] for _ in range(len(times))]
    meta = {"mode": "fixed_temperature", "phonon_temperature_K": float(bath_temperature), "field_units": "K",
            "energy_frame_units": "occupation", "omega_bins_match_qp_energy_bins": bool(phonon_energy_bins is not None)}
    return frames, eframes, bins, meta


def _validated_generation(rates: np.ndarray, mode: str, shape: tuple[int, int]) -> np.ndarray:
    """Shape / finiteness / sign checks every generation mode goes through (messages of solver.py:889-902)."""
    if rates.shape != shape:
        raise ValueError(f"External generation mode '{mode}' returned invalid shape {rates.shape}; expected {shape}.")
    if not np.isfinite(rates).all():
        raise ValueError(f"External generation mode '{mode}' produced non-finite values.")
    if (rates < 0).any():
        raise ValueError(f"External generation mode '{mode}' produced negative values. "
                         "Generation rates must be non-negative.")
    return rates


class _CustomGeneration:
    """A ``custom`` generation expression g(E, x, y, t, params) compiled once, evaluated on [NE, n_spatial].

    Three evaluation strategies, tried in this order, each falling through to the next on ANY exception:
      grid      one call with E as a column and x, y as rows - only for expressions that are elementwise in E, x, y
                (``safe_eval.expression_is_elementwise``), where broadcasting cannot change a value;
      per bin   one call per energy bin with E a scalar and x, y arrays: the reference's vectorised attempt
                (solver.py:933-948), incl. its rule that a bin yields a scalar or exactly n_spatial values;
      per cell  one call per (bin, pixel) with plain floats: the reference's scalar fallback (solver.py:949-961), whose
                exceptions are the caller's.
    x, y are the normalised pixel-centre coordinates of the interior cells in argwhere order (solver.py:924-929)."""

    def __init__(self, spec: ExternalGenerationSpec, mask: np.ndarray):
        from .safe_eval import expression_is_elementwise
        body = spec.custom_body.strip() or "0.0"
        self._fn = compile_safe_expression(body, variable_names=("E", "x", "y", "t", "params"))
        self._gridwise = expression_is_elementwise(body, array_variables=("E", "x", "y"))
        self._params = dict(spec.custom_params or {})
        mask = np.asarray(mask, dtype=bool)
        ny, nx = mask.shape
        rows, cols = np.nonzero(mask)
        self._x = (cols + 0.5) / max(1, nx)
        self._y = (rows + 0.5) / max(1, ny)

    def _on_grid(self, E: np.ndarray, t: float, shape) -> np.ndarray:
        value = self._fn(E=E[:, None], x=self._x[None, :], y=self._y[None, :], t=t, params=self._params)
        return np.array(np.broadcast_to(np.asarray(value, dtype=float), shape))

    def _per_bin(self, E: np.ndarray, t: float, shape) -> np.ndarray:
        n = shape[1]
        out = np.empty(shape, dtype=float)
        for row, energy in zip(out, E):
            value = np.asarray(self._fn(E=energy, x=self._x, y=self._y, t=t, params=self._params), dtype=float)
            if value.ndim and value.size != n:
                raise ValueError("Vectorized custom generation must return a scalar or "
                                 f"exactly {n} values per energy bin; got {value.size}.")
            row[...] = value.reshape(-1) if value.ndim else float(value)
        return out

    def _per_cell(self, E: np.ndarray, t: float, shape) -> np.ndarray:
        cells = list(zip(self._x.tolist(), self._y.tolist()))
        return np.array([[float(self._fn(E=energy, x=x, y=y, t=t, params=self._params)) for x, y in cells]
                         for energy in E.tolist()], dtype=float).reshape(shape)

    def __call__(self, E_bins: np.ndarray, t: float, n_spatial: int) -> np.ndarray:
        E = np.asarray(E_bins, dtype=float)
        shape = (E.size, int(n_spatial))
        for attempt in ((self._on_grid,) if self._gridwise else ()) + (self._per_bin,):
            try:
                return attempt(E, t, shape)
            except Exception:      # noqa: BLE001 - any failure of a vectorised attempt means "try the next strategy"
                continue
        return self._per_cell(E, t, shape)


def evaluate_external_generation(spec: ExternalGenerationSpec, E_bins: np.ndarray, n_spatial: int, t: float,
                                 mask: np.ndarray, _compiled: "_CustomGeneration | None" = None) -> np.ndarray | None:
    """g_ext(E, x, t) as an [NE, n_spatial] host array, None for mode "none" (semantics of solver.py:878-964).

    The run loop only calls this for ``custom`` mode (constant / pulse rates are added on the device) and passes the
    expression it compiled once per run as ``_compiled``.
    """
    mode = spec.mode.strip().lower()
    shape = (len(E_bins), int(n_spatial))
    if mode == "constant":
        level = spec.rate
    elif mode == "pulse":
        level = spec.pulse_rate if spec.pulse_start <= t < spec.pulse_start + spec.pulse_duration else 0.0
    elif mode == "custom":
        custom = _compiled if _compiled is not None else _CustomGeneration(spec, mask)
        return _validated_generation(custom(E_bins, t, n_spatial), mode, shape)
    else:                      # "none" and anything validate() would have rejected
        return None
    return _validated_generation(np.full(shape, level, dtype=float), mode, shape)


def _crop_to_bounding_box(mask: np.ndarray, edges: list[EdgeSegment]):
    """(mask, edges) restricted to the bounding box of the interior cells; faces are re-indexed, ids kept."""
    rows = np.flatnonzero(mask.any(axis=1))
    cols = np.flatnonzero(mask.any(axis=0))
    r0, r1, c0, c1 = int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1
    if (r0, c0) == (0, 0) and (r1, c1) == mask.shape:
        return mask, edges
    from .models import BoundaryFace
    shifted = [EdgeSegment(e.edge_id, e.x0 - c0, e.y0 - r0, e.x1 - c0, e.y1 - r0, e.normal,
                           [BoundaryFace(f.row - r0, f.col - c0, f.direction) for f in e.faces]) for e in edges]
    return np.ascontiguousarray(mask[r0:r1, c0:c1]), shifted


def _color_limits(frames: list[np.ndarray]) -> list[float]:
    stack = np.stack(frames)
    lo, hi = float(np.nanmin(stack)), float(np.nanmax(stack))
    if abs(hi - lo) < 1e-12:
        hi = lo + 1e-9
    return [lo, hi]


class _Diffuser:
    """Per-run diffusion operators (regular dt and the optional short last step)."""

    def __init__(self, eng: Engine, nfield: int, dt: float, rem: float, scheme: str, rtol: float,
                 dcoef=None, dfield=None):
        if scheme not in ("cn_exact", "adi"):
            raise ValueError("diffusion_scheme must be 'cn_exact' or 'adi'.")
        self.eng, self.scheme, self.rtol = eng, scheme, rtol
        self.op = DiffusionOperator(eng, nfield, dt, dcoef=dcoef, dfield=dfield)
        self.op_last = DiffusionOperator(eng, nfield, rem, dcoef=dcoef, dfield=dfield) if rem > 0.0 else None
        self.iterations = 0

    def step(self, u, final: bool) -> None:
        op = self.op_last if final else self.op
        if op is None:
            raise RuntimeError("Internal error: final-step solver not initialized.")
        if self.scheme == "adi":
            self.eng.adi_step(op, u)
        else:
            self.iterations += self.eng.cn_exact_step(op, u, rtol=self.rtol)

    def advance(self, u, first: int, last: int, full_steps: int) -> None:
        """Steps ``first..last`` (1-based, inclusive) with nothing in between, as in the reference's scalar loop
        (solver.py:1540-1555).  With the ADI scheme the regular steps of the stretch are ONE library call: the carried
        right-hand side is never materialised in between (32 B instead of 48 B per cell-update)."""
        if self.scheme != "adi":
            for step in range(first, last + 1):
                self.step(u, step > full_steps)
            return
        regular = min(last, full_steps) - first + 1
        if regular > 0:
            self.eng.adi_steps(self.op, u, regular)
        if last > full_steps:
            self.step(u, True)


def _checked_run_arguments(mask, initial_field, diffusion_coefficient, dt, total_time, store_every, enable_diffusion,
                           enable_recombination, enable_scattering, tau_0, tau_s, tau_r, external_generation,
                           phonon_history_out):
    """Argument checks of a run, in the reference's order and with its messages (solver.py:1040-1080); clears
    ``phonon_history_out``.  Returns (mask, initial_field, store_every, n interior cells, tau_s, tau_r)."""
    mask = np.asarray(mask, dtype=bool)
    initial_field = np.asarray(initial_field)
    if dt <= 0 or total_time <= 0:
        raise ValueError("dt and total_time must be positive.")
    if enable_diffusion and diffusion_coefficient <= 0:
        raise ValueError("Diffusion coefficient must be positive.")
    if store_every <= 0:
        store_every = 1
    if initial_field.shape != mask.shape:
        raise ValueError("Initial field shape must match mask shape.")
    n = int(np.sum(mask))
    if n == 0:
        raise ValueError("Geometry mask has no interior points.")
    if phonon_history_out is not None:
        phonon_history_out.clear()
    tau_s_eff = float(tau_s if tau_s is not None else tau_0)
    tau_r_eff = float(tau_r if tau_r is not None else tau_0)
    if enable_scattering and tau_s_eff <= 0:
        raise ValueError("tau_s must be positive when scattering is enabled.")
    if enable_recombination and tau_r_eff <= 0:
        raise ValueError("tau_r must be positive when recombination is enabled.")
    if external_generation is not None:
        external_generation.validate()
    return mask, initial_field, store_every, n, tau_s_eff, tau_r_eff


# Time traces and coarse frames are the two kinds of sampler (timeloop.Sampler).  The checked arguments of each are a plan;
# the two plan classes have the same methods, and everything below them handles a plan without knowing its kind:
#   every                                        the cadence
#   row_shape(nfield)                            the shape of one member's row of the device buffer
#   sampler(eng, mask, sched, members, nfield)   the Sampler of a run on eng (whose grid is the bounding box of mask)
#   result(times, rows, E_bins, dx, dE)          what the sink receives for one problem; rows [S, *row_shape] of that problem
#   too_large(nbytes, rows, members, nfield)     the message for a buffer above the limit
SAMPLE_BUFFER_LIMIT = 256 << 20     # bytes of the device buffer of one sampler (samples x members x row shape x 8)


class _TracePlan:
    """Checked time-trace arguments of a run: region ``names``, their boolean arrays on the full mask (``regions``), the
    interior ``cells`` of each and ``every``."""

    def __init__(self, names, regions, cells, every):
        self.names, self.regions, self.cells, self.every = names, regions, cells, every

    def row_shape(self, nfield: int) -> tuple:
        return len(self.names), nfield

    def sampler(self, eng, mask, sched: Schedule, members: int, nfield: int) -> Sampler:
        offset = (int(np.flatnonzero(mask.any(axis=1))[0]), int(np.flatnonzero(mask.any(axis=0))[0]))
        bits = eng.region_bits(self.regions, offset)
        return Sampler(eng, sched, self.every, members, self.row_shape(nfield),
                       lambda state, row: eng.region_sums(state, bits, members, row))

    def result(self, times, density: np.ndarray, E_bins, dx: float, dE) -> dict:
        """``density`` [S, R, planes]."""
        density = np.ascontiguousarray(density)
        number = dx * dx * (density[..., 0] if E_bins is None else dE * np.sum(density, axis=-1))
        return {"times": list(times), "regions": list(self.names), "cells": list(self.cells),
                "energy_bins": None if E_bins is None else np.array(E_bins, dtype=float), "density": density, "number": number}

    def too_large(self, nbytes: int, rows: int, members: int, nfield: int) -> str:
        return (f"trace_every={self.every} gives a trace buffer of {nbytes / 2 ** 20:.0f} MiB ({rows} samples x "
                f"{members} members x {len(self.names)} regions x {nfield} planes x 8 B), above the limit of "
                f"{SAMPLE_BUFFER_LIMIT >> 20} MiB; use a larger trace_every.")


def _trace_plan(mask: np.ndarray, tracing: bool, trace_regions, trace_every, kind: str = "trace", plan=_TracePlan):
    """The ``_TracePlan`` of a run, None when traces are off (``tracing``: a sink was given).  ``ValueError`` naming the
    argument for ``trace_every`` < 1, regions without a sink, not 1 ... 8 regions, a region of another shape than the mask.
    The collision rate traces take their regions by the same rules (``kind="rates"``, ``plan=_RatesPlan``)."""
    if isinstance(trace_every, bool) or not isinstance(trace_every, (int, np.integer)) or trace_every < 1:
        raise ValueError(f"{kind}_every must be an integer >= 1, got {trace_every!r}.")
    if not tracing:
        if trace_regions is not None:
            raise ValueError(f"{kind}_regions needs {kind}_out: without a sink no trace is taken.")
        return None
    if trace_regions is None:
        trace_regions = {"all": mask}
    if not isinstance(trace_regions, dict) or not 1 <= len(trace_regions) <= 8:
        raise ValueError(f"{kind}_regions must map 1 to 8 region names to boolean arrays"
                         + (f", got {len(trace_regions)} regions." if isinstance(trace_regions, dict) else "."))
    names, regions = [], []
    for name, region in trace_regions.items():
        region = np.asarray(region)
        if region.shape != mask.shape:
            raise ValueError(f"{kind}_regions['{name}'] has shape {region.shape}; expected the mask's shape {mask.shape}.")
        names.append(str(name))
        regions.append(region.astype(bool))
    return plan(names, regions, [int(np.sum(r & mask)) for r in regions], int(trace_every))


RATE_CHANNELS = ("scattering_in", "scattering_out", "recombination", "pair_breaking")
PHONON_RATE_CHANNELS = ("scattering_emission", "scattering_absorption", "recombination_emission", "pair_breaking_absorption")


class _RatesReduce:
    """The ``reduce`` of a rate sampler: ``method`` names the engine call (``collision_rates``, ``phonon_rates``).  The
    samplers of a run are built before its tables and phonon planes exist, so the run object is bound late: ``_bind_rates``
    sets ``run`` once ``_LoneRun`` / ``_MembersRun`` is complete, and every sample reads the run's current phonon planes,
    tables and process switches."""
    run = None

    def __init__(self, eng, bits, members: int, method: str = "collision_rates"):
        self.eng, self.bits, self.members, self.method = eng, bits, members, method

    def __call__(self, state, row) -> None:
        run = self.run
        en_r, en_s, _ = run.physics
        getattr(self.eng, self.method)(run.ctab, state, run.phonon, self.bits, self.members, run.dE, en_r, en_s, row)


class _PhononRatesReduce(_RatesReduce):
    """``_RatesReduce`` on ``Engine.phonon_rates``."""

    def __init__(self, eng, bits, members: int):
        super().__init__(eng, bits, members, "phonon_rates")


def _bind_rates(samplers, run) -> None:
    for sampler in samplers:
        if isinstance(sampler.reduce, _RatesReduce):
            sampler.reduce.run = run


class _RatePlan:
    """Checked rate-trace arguments of a run, as ``_TracePlan``: region ``names``, their boolean arrays on the full mask,
    the interior ``cells`` of each and ``every``.  A kind of rate trace states ``kind`` (the prefix of its keywords),
    ``channels``, ``method`` (the engine call of its reduce, ``qp_<method>_available`` its size query), ``bin_word``,
    ``bins(nfield)`` of a row and what ``extra`` adds to the result."""

    def __init__(self, names, regions, cells, every):
        self.names, self.regions, self.cells, self.every = names, regions, cells, every

    def row_shape(self, nfield: int) -> tuple:
        return len(self.names), len(self.channels), self.bins(nfield)

    def sampler(self, eng, mask, sched: Schedule, members: int, nfield: int) -> Sampler:
        offset = (int(np.flatnonzero(mask.any(axis=1))[0]), int(np.flatnonzero(mask.any(axis=0))[0]))
        return Sampler(eng, sched, self.every, members, self.row_shape(nfield),
                       _RatesReduce(eng, eng.region_bits(self.regions, offset), members, self.method))

    def result(self, times, rates: np.ndarray, E_bins, dx: float, dE) -> dict:
        """``rates`` [S, R, 4, bins]."""
        rates = np.ascontiguousarray(rates)
        return {"times": list(times), "regions": list(self.names), "cells": list(self.cells),
                "channels": list(self.channels), "rates": rates, **self.extra(rates, E_bins, dx, dE)}

    def too_large(self, nbytes: int, rows: int, members: int, nfield: int) -> str:
        return (f"{self.kind}_every={self.every} gives a rate buffer of {nbytes / 2 ** 20:.0f} MiB ({rows} samples x "
                f"{members} members x {len(self.names)} regions x {len(self.channels)} channels x {self.bins(nfield)} "
                f"{self.bin_word} x 8 B), above the limit of {SAMPLE_BUFFER_LIMIT >> 20} MiB; use a larger {self.kind}_every.")

    def set_phonon_grid(self, omega_bins, dE) -> None:
        """The phonon grid of the run's energy grid, for a plan that keeps it."""


class _RatesPlan(_RatePlan):
    """The collision rate traces: a row holds the energy planes."""
    kind, channels, method, bin_word = "rates", RATE_CHANNELS, "collision_rates", "bins"

    def bins(self, nfield: int) -> int:
        return nfield

    def extra(self, rates, E_bins, dx, dE) -> dict:
        return {"energy_bins": np.array(E_bins, dtype=float), "number_rates": dx * dx * dE * np.sum(rates, axis=-1)}


class _PhononRatesPlan(_RatePlan):
    """The phonon rate traces: a row holds phonon bins, not energy planes, so the plan also carries the phonon grid of the
    run's energy grid: ``omega_bins`` [NW], ``nw`` and the integration ``widths`` of the phonon frames."""
    kind, channels, method, bin_word = "phonon_rates", PHONON_RATE_CHANNELS, "phonon_rates", "phonon bins"
    omega_bins = widths = None
    nw = 0

    def bins(self, nfield: int) -> int:
        return self.nw

    def extra(self, rates, E_bins, dx, dE) -> dict:
        return {"phonon_energy_bins": np.array(self.omega_bins, dtype=float),
                "integrated_rates": dx * dx * np.sum(self.widths * rates, axis=-1)}

    def set_phonon_grid(self, omega_bins, dE) -> None:
        self.omega_bins, self.nw = np.asarray(omega_bins, dtype=float), int(omega_bins.size)
        self.widths = integration_widths_from_centers(self.omega_bins, fallback_width=dE)


def _rate_trace_grid(run_args, sink: str, available):
    """(omega_bins, dE) of the phonon grid of a run whose sink ``sink`` (``"rates_out"``, ``"phonon_rates_out"``) is on, on
    the host.  ``ValueError`` naming the sink for a run its kernel does not serve: scalar mode, no collision process, a
    ``num_energy_bins`` / phonon grid for which ``available(ne, nw)`` is 0."""
    a = run_args
    if not a["energy_gap"] > 0.0:
        raise ValueError(f"{sink} needs an energy-resolved run (energy_gap > 0): scalar mode has no collision terms.")
    if not (a["enable_recombination"] or a["enable_scattering"]):
        raise ValueError(f"{sink} needs enable_recombination or enable_scattering: with both off there is no rate.")
    ne = int(a["num_energy_bins"])
    nw, omega_bins, dE = 0, None, None
    if 2 <= ne <= 64:         # the phonon grid of this energy grid (host only)
        E_bins, dE = build_energy_grid(a["energy_gap"], a["energy_min_factor"], a["energy_max_factor"], ne)
        omega_bins = _build_phonon_frequency_map(E_bins)[0]
        nw = int(omega_bins.size)
    if not available(ne, nw):
        raise ValueError(f"{sink}: num_energy_bins={ne}" + (f" with {nw} phonon bins" if nw else "") + " is outside the "
                         "rate kernel's range (2 to 64 energy bins, at most 191 phonon bins; collision_wide_bins does not "
                         "extend it).")
    return omega_bins, dE


def _rate_plan(kind, mask: np.ndarray, wanted: bool, regions, every, run_args):
    """The plan of class ``kind`` of a run, None when its traces are off (``wanted``: a sink was given).  ``ValueError``
    naming the argument for what ``_trace_plan`` refuses and, with a sink, for a run the kernel does not serve: scalar mode,
    no collision process, a ``num_energy_bins`` / phonon grid outside the kernel's size query.  ``run_args``: the keyword
    arguments of the run (``energy_gap``, the two switches and the energy grid are read)."""
    plan = _trace_plan(mask, wanted, regions, every, kind.kind, kind)
    if plan is None:
        return None
    from . import _hip
    plan.set_phonon_grid(*_rate_trace_grid(run_args, f"{kind.kind}_out", getattr(_hip.load(), f"qp_{kind.method}_available")))
    return plan


def _rates_plan(mask: np.ndarray, wanted: bool, rates_regions, rates_every, run_args):
    return _rate_plan(_RatesPlan, mask, wanted, rates_regions, rates_every, run_args)


def _phonon_rates_plan(mask: np.ndarray, wanted: bool, regions, every, run_args):
    return _rate_plan(_PhononRatesPlan, mask, wanted, regions, every, run_args)


class _CoarsePlan:
    """Checked coarse-frame arguments of a run: ``bin``, ``every`` and the ``engine.CoarseLayout`` of the mask."""

    def __init__(self, bin, every, layout):
        self.bin, self.every, self.layout = bin, every, layout

    def row_shape(self, nfield: int) -> tuple:
        return (nfield,) + self.layout.window[2:]

    def sampler(self, eng, mask, sched: Schedule, members: int, nfield: int) -> Sampler:
        oy, ox = self.layout.offset
        return Sampler(eng, sched, self.every, members, self.row_shape(nfield),
                       lambda state, row: eng.block_sums(state, members, self.bin, oy, ox, row))

    def result(self, times, sums: np.ndarray, E_bins, dx, dE) -> dict:
        """``sums`` [S, planes, cny, cnx], as fetched.  The arrays of a long run are large, so each is formed in one pass: a
        division by NaN marks the blocks without cells."""
        lay = self.layout
        wy, wx, cny, cnx = lay.window
        if (cny, cnx) == lay.shape:
            energy_sums = np.ascontiguousarray(sums)
        else:
            energy_sums = np.zeros(sums.shape[:2] + lay.shape)
            energy_sums[:, :, wy:wy + cny, wx:wx + cnx] = sums
        cells = np.where(lay.cells == 0, np.nan, lay.cells.astype(float))
        energy_frames = energy_sums / cells
        if E_bins is None:
            frames = energy_frames[:, 0].copy()
        else:
            frames = np.sum(energy_sums, axis=1)
            frames *= dE
            frames /= cells
        return {"times": list(times), "bin": self.bin, "cells": lay.cells.copy(),
                "energy_bins": None if E_bins is None else np.array(E_bins, dtype=float), "energy_sums": energy_sums,
                "energy_frames": energy_frames, "frames": frames}

    def too_large(self, nbytes: int, rows: int, members: int, nfield: int) -> str:
        cny, cnx = self.layout.window[2:]
        return (f"coarse_every={self.every}, coarse_bin={self.bin} give a coarse-frame buffer of "
                f"{nbytes / 2 ** 20:.0f} MiB ({rows} samples x {members} members x {nfield} planes x "
                f"{cny} x {cnx} blocks x 8 B), above the limit of {SAMPLE_BUFFER_LIMIT >> 20} MiB; use a larger "
                f"coarse_every or coarse_bin.")


def _coarse_plan(mask: np.ndarray, wanted: bool, coarse_bin, coarse_every):
    """The ``_CoarsePlan`` of a run, None when coarse frames are off (``wanted``: a sink was given).  ``ValueError`` naming
    the argument for a ``coarse_bin`` that is no block edge, ``coarse_every`` < 1, and either of them set without a sink."""
    if isinstance(coarse_bin, bool) or not isinstance(coarse_bin, (int, np.integer)) or int(coarse_bin) not in COARSE_BINS:
        raise ValueError(f"coarse_bin must be one of {', '.join(map(str, COARSE_BINS))}, got {coarse_bin!r}.")
    if isinstance(coarse_every, bool) or not isinstance(coarse_every, (int, np.integer)) or coarse_every < 1:
        raise ValueError(f"coarse_every must be an integer >= 1, got {coarse_every!r}.")
    if not wanted:
        if int(coarse_bin) != 8:
            raise ValueError("coarse_bin needs coarse_out: without a sink no coarse frame is taken.")
        if int(coarse_every) != 1:
            raise ValueError("coarse_every needs coarse_out: without a sink no coarse frame is taken.")
        return None
    return _CoarsePlan(int(coarse_bin), int(coarse_every), coarse_layout(mask, int(coarse_bin)))


class _FluxReduce:
    """The ``reduce`` of a flux sampler.  The samplers of a run are built before its diffuser exists, so the operator is bound
    late, as the run of ``_RatesReduce`` is: ``_bind_flux`` sets ``op`` to the ``DiffusionOperator`` the diffuser holds, whose
    coefficients on the device (``dcoef`` or ``dfield``) every sample reads - no second copy is uploaded."""
    op = None

    def __init__(self, eng, faces, members: int):
        self.eng, self.faces, self.members = eng, faces, members

    def __call__(self, state, row) -> None:
        self.eng.boundary_flux(self.faces, self.op, state, self.members, row)


def _bind_flux(samplers, diffuser) -> None:
    for sampler in samplers:
        if isinstance(sampler.reduce, _FluxReduce):
            sampler.reduce.op = diffuser.op


class _FluxPlan:
    """Checked boundary-outflow arguments of a run: surface ``names``, the ``engine.BoundaryFaces`` of the device grid
    (``faces``; ``counts``: faces per surface after the reflective ones are dropped) and ``every``."""

    def __init__(self, names, faces, every):
        self.names, self.faces, self.counts, self.every = names, faces, faces.counts, every

    def row_shape(self, nfield: int) -> tuple:
        return len(self.names), nfield

    def sampler(self, eng, mask, sched: Schedule, members: int, nfield: int) -> Sampler:
        return Sampler(eng, sched, self.every, members, self.row_shape(nfield),
                       _FluxReduce(eng, eng.upload_boundary_faces(self.faces), members))

    def result(self, times, outflow: np.ndarray, E_bins, dx: float, dE) -> dict:
        """``outflow`` [S, surfaces, planes]."""
        outflow = np.ascontiguousarray(outflow)
        number = outflow[..., 0].copy() if E_bins is None else dE * np.sum(outflow, axis=-1)
        return {"times": list(times), "surfaces": list(self.names), "faces": list(self.counts),
                "energy_bins": None if E_bins is None else np.array(E_bins, dtype=float), "outflow": outflow,
                "number_outflow": number}

    def too_large(self, nbytes: int, rows: int, members: int, nfield: int) -> str:
        return (f"flux_every={self.every} gives a flux buffer of {nbytes / 2 ** 20:.0f} MiB ({rows} samples x "
                f"{members} members x {len(self.names)} surfaces x {nfield} planes x 8 B), above the limit of "
                f"{SAMPLE_BUFFER_LIMIT >> 20} MiB; use a larger flux_every.")


def _flux_plan(mask: np.ndarray, wanted: bool, flux_surfaces, flux_every, run_args):
    """The ``_FluxPlan`` of a run, None when the outflow traces are off (``wanted``: a sink was given).  ``ValueError`` naming
    the argument for ``flux_every`` < 1, surfaces without a sink, not 1 ... 64 surfaces, an empty surface list, an unknown
    edge id, and a sink on a run without diffusion.  ``run_args``: the keyword arguments of the run (``edges``,
    ``edge_conditions``, ``dx`` and ``enable_diffusion`` are read)."""
    if isinstance(flux_every, bool) or not isinstance(flux_every, (int, np.integer)) or flux_every < 1:
        raise ValueError(f"flux_every must be an integer >= 1, got {flux_every!r}.")
    if not wanted:
        if flux_surfaces is not None:
            raise ValueError("flux_surfaces needs flux_out: without a sink no outflow is taken.")
        return None
    a = run_args
    if not a.get("enable_diffusion", True):
        raise ValueError("flux_out needs enable_diffusion: without diffusion there is no operator and no boundary term.")
    edges = list(a["edges"])
    if flux_surfaces is None:
        flux_surfaces = {"all": [e.edge_id for e in edges]}
    if not isinstance(flux_surfaces, dict) or not 1 <= len(flux_surfaces) <= FLUX_SURFACES:
        raise ValueError(f"flux_surfaces must map 1 to {FLUX_SURFACES} surface names to lists of edge ids"
                         + (f", got {len(flux_surfaces)} surfaces." if isinstance(flux_surfaces, dict) else "."))
    known = {e.edge_id for e in edges}
    names, lists = [], []
    for name, ids in flux_surfaces.items():
        ids = [ids] if isinstance(ids, str) else list(ids)
        if not ids:
            raise ValueError(f"flux_surfaces['{name}'] is empty: a surface is a non-empty list of edge ids.")
        for edge_id in ids:
            if edge_id not in known:
                raise ValueError(f"flux_surfaces['{name}'] names the unknown edge id {edge_id!r}.")
        names.append(str(name))
        lists.append(ids)
    dev_mask, dev_edges = _crop_to_bounding_box(mask, edges)
    return _FluxPlan(names, compile_boundary_faces(dev_mask, dev_edges, a["edge_conditions"], float(a["dx"]), lists),
                     int(flux_every))


def _sample_buffer_bytes(plan, sched: Schedule, members: int, nfield: int) -> int:
    return 8 * sched.rows(plan.every) * members * int(np.prod(plan.row_shape(nfield)))


def _check_sample_buffer(plan, sched: Schedule, members: int, nfield: int) -> None:
    if plan is None:
        return
    nbytes = _sample_buffer_bytes(plan, sched, members, nfield)
    if nbytes > SAMPLE_BUFFER_LIMIT:
        raise ValueError(plan.too_large(nbytes, sched.rows(plan.every), members, nfield))


def _sampling_plans(mask, trace_out, trace_regions, trace_every, coarse_out, coarse_bin, coarse_every, rates_out=None,
                    rates_regions=None, rates_every=1, run_args=None, phonon_rates_out=None, phonon_rates_regions=None,
                    phonon_rates_every=1, flux_out=None, flux_surfaces=None, flux_every=1) -> list:
    """The active ``(plan, sink)`` pairs of a run: trace, coarse frames, collision rates, phonon rates, boundary outflow, in
    that order; all arguments are checked before a sink is cleared.  ``run_args``: the keyword arguments of the run, read by
    ``_rates_plan``, ``_phonon_rates_plan`` and ``_flux_plan``."""
    kinds = ((_trace_plan(mask, trace_out is not None, trace_regions, trace_every), trace_out),
             (_coarse_plan(mask, coarse_out is not None, coarse_bin, coarse_every), coarse_out),
             (_rates_plan(mask, rates_out is not None, rates_regions, rates_every, run_args), rates_out),
             (_phonon_rates_plan(mask, phonon_rates_out is not None, phonon_rates_regions, phonon_rates_every, run_args),
              phonon_rates_out),
             (_flux_plan(mask, flux_out is not None, flux_surfaces, flux_every, run_args), flux_out))
    active = [(plan, sink) for plan, sink in kinds if plan is not None]
    for _, sink in active:
        sink.clear()
    return active


def _deliver_samples(sampling, samplers, E_bins, dx, dE) -> None:
    """Fills the sinks of a lone run (member 0 of its samplers) from ``sampling``, the pairs of ``_sampling_plans``."""
    for (plan, sink), sampler in zip(sampling, samplers):
        sink.update(plan.result(sampler.times, sampler.fetch()[:, 0], E_bins, dx, dE))


def _run_geometry(mask, edges, edge_conditions, dx, enable_diffusion):
    """Compiled geometry of the device grid = bounding box of the mask."""
    dev_mask, dev_edges = _crop_to_bounding_box(mask, edges)
    if enable_diffusion:
        return compile_geometry(dev_mask, dev_edges, edge_conditions, dx)
    # no operator needed: boundary conditions are not consulted (solver.py:1081-1083)
    from .engine import CompiledGeometry, link_flags
    z = np.zeros(dev_mask.shape)
    return CompiledGeometry(dev_mask, float(dx), link_flags(dev_mask), z, z, z, z)


def _initial_qp_state(mask, initial_field, E_bins, dE, gap, dynes_gamma, energy_weights, initial_condition_spec):
    """[NE, n] initial quasiparticle densities (solver.py:1240-1283)."""
    NE, n = len(E_bins), int(np.sum(mask))
    custom_state = None
    if initial_condition_spec is not None:
        from .initial_conditions import build_initial_qp_energy_state
        custom_state = build_initial_qp_energy_state(mask=mask, E_bins=E_bins, spec=initial_condition_spec)
    if custom_state is not None:
        state_host = np.asarray(custom_state, dtype=float)
        if state_host.shape != (NE, n):
            raise ValueError(f"Full custom quasiparticle profile must have shape ({NE}, {n}); got {state_host.shape}.")
        if not np.all(np.isfinite(state_host)):
            raise ValueError("Full custom quasiparticle profile produced non-finite values.")
        if np.any(state_host < 0):
            raise ValueError("Full custom quasiparticle profile must be non-negative.")
        return state_host
    spatial = initial_field[mask].astype(float)
    if energy_weights is not None:
        raw = np.asarray(energy_weights, dtype=float)
        if raw.ndim != 1:
            raise ValueError("energy_weights must be a 1D array.")
        if raw.shape[0] != NE:
            raise ValueError(f"energy_weights must have length {NE}, got {raw.shape[0]}.")
        if not np.all(np.isfinite(raw)):
            raise ValueError("energy_weights must contain only finite values.")
        if np.any(raw < 0):
            raise ValueError("energy_weights must be non-negative.")
    else:
        raw = _dynes_density_of_states(E_bins, gap, dynes_gamma)
    integral = np.sum(raw) * dE
    weights = raw / integral if integral > 0 else np.ones(NE, dtype=float) / (NE * dE)
    state_host = np.empty((NE, n), dtype=float)
    for i in range(NE):
        state_host[i] = spatial * weights[i]
    return state_host


def _initial_phonon_state(mask, omega_bins, bath_temperature, initial_condition_spec):
    """[Nw, n] initial phonon occupations: thermal at the bath temperature or from the initial-condition spec."""
    n = int(np.sum(mask))
    if initial_condition_spec is not None:
        from .initial_conditions import build_initial_phonon_energy_state
        return build_initial_phonon_energy_state(mask=mask, omega_bins=omega_bins, spec=initial_condition_spec,
                                                 bath_temperature=bath_temperature)
    return thermal_phonon_occupation(omega_bins, bath_temperature)[:, None] * np.ones((1, n), dtype=float)


def _collision_tables(eng, E_bins, gap, nonuniform_pre, n, dynes_gamma, tau_r_eff, tau_s_eff, T_c, enable_recombination,
                      enable_scattering, idx_diff, idx_sum, diff_sign, members: int = 1, member_params=None,
                      member_ids=None, pad_bins: bool = False, wide_bins: bool = False):
    """(device collision tables, rho per gap class) (solver.py:1189-1238); ``nonuniform_pre``: the precomputed arrays of a
    non-uniform gap (one class per distinct gap value), None for one gap.  ``member_params`` (ensemble parameter sweeps, one
    gap): ``(dynes_gamma, tau_r, tau_s, T_c)`` per member - one table set per member, each built exactly as that member's
    lone run builds its own, uploaded as member classes; the rho returned is then [members, NE].  ``pad_bins``
    (``collision_padded_bins``) goes to the one-gap and the member-class tables; gap classes ignore it.  ``wide_bins``
    (``collision_wide_bins``) goes to all three."""
    if member_params is not None:
        built: dict = {}
        for j, key in enumerate(member_params):
            if key in built:
                continue
            gamma, tau_r, tau_s, tc = key
            try:
                built[key] = (_dynes_density_of_states(E_bins, float(gap), gamma),
                              recombination_kernel_base(E_bins, float(gap), tau_r, tc) if enable_recombination else None,
                              scattering_kernel_base(E_bins, float(gap), tau_s, tc) if enable_scattering else None)
            except (ValueError, TypeError) as exc:
                raise type(exc)(f"member {j if member_ids is None else member_ids[j]}: {exc}") from exc
        rho_tab = np.stack([built[key][0] for key in member_params])
        kr_tab = np.stack([built[key][1] for key in member_params]) if enable_recombination else None
        ks_tab = np.stack([built[key][2] for key in member_params]) if enable_scattering else None
        ctab = eng.make_collision_tables(kr_tab, ks_tab, rho_tab, idx_diff, idx_sum, diff_sign, None,
                                         members=len(member_params), member_classes=True, pad_bins=pad_bins,
                                         wide_bins=wide_bins)
        return ctab, rho_tab
    if nonuniform_pre is not None:
        gap_values = nonuniform_pre.get("gap_values")
        gap_values = np.full(n, gap, dtype=float) if gap_values is None else np.asarray(gap_values, dtype=float)
        class_gaps, cls = np.unique(gap_values, return_inverse=True)
    else:
        class_gaps, cls = np.array([gap], dtype=float), None
    rho_tab = np.stack([_dynes_density_of_states(E_bins, float(g), dynes_gamma) for g in class_gaps])
    kr_tab = (np.stack([recombination_kernel_base(E_bins, float(g), tau_r_eff, T_c) for g in class_gaps])
              if enable_recombination else None)
    ks_tab = (np.stack([scattering_kernel_base(E_bins, float(g), tau_s_eff, T_c) for g in class_gaps])
              if enable_scattering else None)
    ctab = eng.make_collision_tables(kr_tab, ks_tab, rho_tab, idx_diff, idx_sum, diff_sign, cls,
                                     gap_params=dict(E=E_bins, gaps=class_gaps, tau_r=tau_r_eff, tau_s=tau_s_eff, T_c=T_c),
                                     members=members, pad_bins=bool(pad_bins and nonuniform_pre is None),
                                     wide_bins=wide_bins)
    return ctab, rho_tab


def _generation_amount(spec, t_start: float, dt_of_step: float):
    """dt g_ext of a step that starts at ``t_start`` when it is one number for all bins and pixels (constant / pulse
    modes), None when it is not (custom mode); 0.0 without generation (the reference gates on the raw mode string,
    solver.py:1459)."""
    if spec is None or spec.mode == "none":
        return 0.0
    mode = spec.mode.strip().lower()
    if mode == "constant":
        return dt_of_step * float(spec.rate)
    if mode == "pulse":
        on = spec.pulse_start <= t_start < spec.pulse_start + spec.pulse_duration
        return dt_of_step * float(spec.pulse_rate) if on else 0.0
    return None if mode == "custom" else 0.0


def _pauli_verdict(stats, step_idx: int, time_ns: float, E_bins, coords, cell_to_px, warned: bool, enforce_pauli: bool,
                   warn_threshold, error_threshold):
    """What the Pauli guard of one step does (solver.py:1296-1344): (error message or None, warning message or None,
    warned).  At most one of the two messages is set."""
    max_occ, (ie_max, cell_max), forb = stats
    if forb is not None:
        r, c = coords[cell_to_px[forb[1]]]
        msg = (f"Detected non-zero quasiparticle density in forbidden state (rho≈0): step={step_idx}, "
               f"t={time_ns:.6g} ns, E={E_bins[forb[0]]:.6g} μeV, pixel=({int(r)},{int(c)}).")
        if enforce_pauli:
            return msg, None, warned
        if not warned:
            return None, msg, True
    r, c = coords[cell_to_px[cell_max]]
    if error_threshold is not None and max_occ > error_threshold:
        msg = (f"Pauli occupation exceeded limit: f={max_occ:.6g} > {error_threshold:.6g} "
               f"at step={step_idx}, t={time_ns:.6g} ns, E={E_bins[ie_max]:.6g} μeV, pixel=({int(r)},{int(c)}).")
        if enforce_pauli:
            return msg, None, warned
        if not warned:
            return None, msg, True
    if warn_threshold is not None and max_occ > warn_threshold and not warned:
        return None, ("High occupation detected (Pauli blocking regime): "
                      f"max f={max_occ:.6g} at step={step_idx}, t={time_ns:.6g} ns, "
                      f"E={E_bins[ie_max]:.6g} μeV, pixel=({int(r)},{int(c)})."), True
    return None, None, warned


def _on_run_device(fn):
    """Runs ``fn`` with the HIP device of its ``device=`` argument current in the calling thread (kernel launches through
    the C ABI go to the thread's current device; the reference's GUI calls the solver from a worker thread)."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        try:
            import torch
            usable = torch.cuda.is_available()
        except Exception:            # no torch / no GPU: let the body raise its own error after argument validation
            usable = False
        if not usable:
            return fn(*args, **kwargs)
        dev = kwargs.get("device")
        dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


@_on_run_device
def run_2d_crank_nicolson(
    mask: np.ndarray,
    edges: list[EdgeSegment],
    edge_conditions: dict[str, BoundaryCondition],
    initial_field: np.ndarray,
    diffusion_coefficient: float,
    dt: float,
    total_time: float,
    dx: float,
    store_every: int = 1,
    energy_gap: float = 0.0,
    energy_min_factor: float = 1.0,
    energy_max_factor: float = 10.0,
    num_energy_bins: int = 50,
    energy_weights: np.ndarray | None = None,
    enable_diffusion: bool = True,
    enable_recombination: bool = False,
    enable_scattering: bool = False,
    dynes_gamma: float = 0.0,
    collision_solver: str = "fischer_catelani_local",
    tau_0: float = 440.0,
    tau_s: float | None = None,
    tau_r: float | None = None,
    T_c: float = 1.2,
    bath_temperature: float = 0.1,
    external_generation: ExternalGenerationSpec | None = None,
    initial_condition_spec: InitialConditionSpec | None = None,
    gap_expression: str = "",
    precomputed: dict | None = None,
    pauli_warn_threshold: float | None = 0.5,
    pauli_error_threshold: float | None = 1.0,
    enforce_pauli: bool = True,
    pauli_density_floor: float = 1e-18,
    freeze_phonon_dynamics: bool = False,
    phonon_history_out: dict[str, Any] | None = None,
    progress_callback: Callable[[float, np.ndarray], None] | None = None,
    *,
    diffusion_scheme: str = "cn_exact",
    cn_rtol: float = 1e-13,
    device=None,
    generation_on_device: bool = False,
    collision_wide_bins: bool = False,
    collision_padded_bins: bool = False,
    trace_out: dict[str, Any] | None = None,
    trace_regions: dict[str, np.ndarray] | None = None,
    trace_every: int = 1,
    coarse_out: dict[str, Any] | None = None,
    coarse_bin: int = 8,
    coarse_every: int = 1,
    rates_out: dict[str, Any] | None = None,
    rates_regions: dict[str, np.ndarray] | None = None,
    rates_every: int = 1,
    phonon_rates_out: dict[str, Any] | None = None,
    phonon_rates_regions: dict[str, np.ndarray] | None = None,
    phonon_rates_every: int = 1,
    flux_out: dict[str, Any] | None = None,
    flux_surfaces: dict[str, list] | None = None,
    flux_every: int = 1,
):
    """Run the 2-D Crank-Nicolson diffusion (+ local collisions) time loop on the GPU.

    Returns ``(times, frames, mass, color_limits, energy_frames_or_None, energy_bins_or_None)`` exactly
    as the reference does; ``phonon_history_out`` is cleared and filled the same way, and so is ``trace_out`` (module
    docstring) when time traces are wanted, ``coarse_out`` when coarse frames are, ``rates_out`` when collision rate
    traces are, ``phonon_rates_out`` when phonon rate traces are, and ``flux_out`` when boundary outflow traces are.
    """
    mask, initial_field, store_every, n, tau_s_eff, tau_r_eff = _checked_run_arguments(
        mask, initial_field, diffusion_coefficient, dt, total_time, store_every, enable_diffusion, enable_recombination,
        enable_scattering, tau_0, tau_s, tau_r, external_generation, phonon_history_out)
    sampling = _sampling_plans(mask, trace_out, trace_regions, trace_every, coarse_out, coarse_bin, coarse_every, rates_out,
                               rates_regions, rates_every,
                               dict(energy_gap=energy_gap, enable_recombination=enable_recombination,
                                    enable_scattering=enable_scattering, num_energy_bins=num_energy_bins,
                                    energy_min_factor=energy_min_factor, energy_max_factor=energy_max_factor, edges=edges,
                                    edge_conditions=edge_conditions, dx=dx, enable_diffusion=enable_diffusion),
                               phonon_rates_out, phonon_rates_regions, phonon_rates_every, flux_out, flux_surfaces, flux_every)
    device_expr.reset_run_stats()

    # Device grid = bounding box of the mask.  Interior cells keep their argwhere (row-major) order under the crop, so
    # the packed [NE, n] layout of every host-side array is unchanged; frames are still rebuilt on the full mask.  A
    # mask whose interior is a solid rectangle inside a padded frame (the reference's built-in geometry) thereby
    # becomes a full rectangle on the device and takes the tiled ADI path.
    geom = _run_geometry(mask, edges, edge_conditions, dx, enable_diffusion)
    sched = Schedule(total_time, dt, store_every)
    nplanes = num_energy_bins if energy_gap > 0.0 else 1
    for plan, _ in sampling:
        _check_sample_buffer(plan, sched, 1, nplanes)
    eng = Engine(geom, device=device)
    eng.pin_stream()          # one stream for the whole run: skip the per-launch lookup
    out = Outputs(mask, dx, [progress_callback])
    samplers = tuple(plan.sampler(eng, mask, sched, 1, nplanes) for plan, _ in sampling)

    if not energy_gap > 0.0:
        result = _run_scalar(eng, sched, out, [initial_field], [diffusion_coefficient], enable_diffusion, [bath_temperature],
                             [phonon_history_out], diffusion_scheme, cn_rtol, samplers)[0]
        _deliver_samples(sampling, samplers, None, dx, None)
        return result

    # ------------------------------------------------------------------ energy-resolved mode
    gap = energy_gap
    NE = num_energy_bins
    E_bins, dE = build_energy_grid(gap, energy_min_factor, energy_max_factor, NE)
    precomputed = _auto_precomputed(
        precomputed, gap_expression, mask, edges, edge_conditions, diffusion_coefficient=diffusion_coefficient, dt=dt,
        total_time=total_time, mesh_size=dx, energy_gap=energy_gap, energy_min_factor=energy_min_factor,
        energy_max_factor=energy_max_factor, num_energy_bins=num_energy_bins, dynes_gamma=dynes_gamma, tau_0=tau_0,
        tau_s=tau_s_eff, tau_r=tau_r_eff, T_c=T_c, bath_temperature=bath_temperature)
    nonuniform = precomputed is not None and not bool(precomputed.get("is_uniform", True))
    normalize_collision_solver_name(collision_solver)
    diffuser = (_energy_diffuser(eng, sched, diffusion_scheme, cn_rtol, E_bins, gap, precomputed, [diffusion_coefficient])
                if enable_diffusion else None)

    # collision tables (solver.py:1189-1238): phonon grid, thermal phonons, per-gap-class kernels
    omega_bins, idx_diff, idx_sum, diff_sign = _build_phonon_frequency_map(E_bins)
    phonon_host = _initial_phonon_state(mask, omega_bins, bath_temperature, initial_condition_spec)
    ctab, rho_tab = _collision_tables(eng, E_bins, gap, precomputed if nonuniform else None, n, dynes_gamma, tau_r_eff,
                                      tau_s_eff, T_c, enable_recombination, enable_scattering, idx_diff, idx_sum, diff_sign,
                                      pad_bins=collision_padded_bins, wide_bins=collision_wide_bins)

    state_host = _initial_qp_state(mask, initial_field, E_bins, dE, gap, dynes_gamma, energy_weights,
                                   initial_condition_spec)
    state = eng.upload_packed(state_host)
    run = _LoneRun(eng, out, state, eng.empty(NE, eng.ncell), eng.upload_packed(phonon_host), dE,
                   _phonon_widths(eng, omega_bins, dE, [phonon_history_out]))
    run.ctab, run.floor = ctab, pauli_density_floor
    run.physics = (enable_recombination, enable_scattering, not freeze_phonon_dynamics)
    run.generation = _Generation(external_generation, mask, E_bins, on_device=generation_on_device)
    run.verdict = _guard_rule(eng, mask, E_bins, enforce_pauli, pauli_warn_threshold, pauli_error_threshold)
    run.samplers = samplers
    _bind_rates(samplers, run)
    if diffuser is not None:
        _bind_flux(samplers, diffuser)

    collisions = bool(enable_recombination or enable_scattering)
    energy_loop(run, sched, diffuser, collisions=collisions,
                pair_ok=bool(collisions and enable_diffusion and ctab.get("pair")),
                batch_diffusion=_one_call_diffusion(diffuser, collisions, run.generation.active, pauli_warn_threshold,
                                                    pauli_error_threshold, rho_tab),
                guard_lag=eng.GUARD_LAG)

    if phonon_history_out is not None:
        phonon_history_out.clear()
        phonon_history_out.update(_dynamic_phonon_history(out, 0, omega_bins))
    _deliver_samples(sampling, samplers, E_bins, dx, dE)
    return out.times, out.frames[0], out.mass[0], _color_limits(out.frames[0]), out.energy_frames[0], E_bins


class _LoneRun(EnergyRun):
    """One problem, driven by the plain library calls (an ensemble of one would launch other kernels).  ``ctab``, ``floor``,
    ``physics`` = (recombination, scattering, phonon update), ``generation`` and ``verdict`` are set by the caller."""
    warned = False

    def __init__(self, *args):
        super().__init__(*args)
        self.step = 0              # generate() is called once per step: the step its status tickets belong to
        self.status: list = []     # (step, ticket) of the device-evaluated generation, read by guard_check

    def generate(self, t: float, dt_step: float) -> None:
        gen = self.generation
        self.step += 1
        if not gen.active:
            return
        amount = gen.amount(t, dt_step)
        if amount is None:
            launch = gen.device_step(t)
            if launch is not None:                               # custom mode in the device subset: one kernel
                self.status.append((self.step, self.eng.add_generation_expr(
                    self.state, gen.window, [launch + (None,)], dt_step, 1, self.eng.d_flags)))
                device_expr.count_steps(device=1)
                return
            device_expr.count_steps(host=1)                      # custom mode: evaluated on the host (solver.py:918-962)
            g_ext = gen.rates(t)
            if g_ext is not None:
                self.eng.add_scaled(self.state, self.eng.upload_packed(g_ext), dt_step)
        elif gen.constant or amount != 0.0:
            self.eng.add_constant(self.state, amount)

    def pair_amount(self, t_next: float, dt_next: float):
        return self.generation.amount(t_next, dt_next)

    def collide(self, dt_col: float, guarded: bool):
        call = self.eng.collide_guarded if guarded else self.eng.collide
        return call(self.ctab, self.state, self.state_alt, self.phonon, self.dE, dt_col, *self.physics,
                    *((self.floor,) if guarded else ()))

    def collide_pair(self, dt_a: float, dt_b: float, amount: float):
        return self.eng.collide_pair_guarded(self.ctab, self.state, self.state_alt, self.phonon, self.dE, dt_a, dt_b,
                                             amount, *self.physics, self.floor)

    def guard_launch(self):
        return self.eng.pauli_stats_launch(self.state, self.ctab, self.floor)

    def guard_check(self, ticket, step: int, t: float) -> None:  # Pauli guard (solver.py:1296-1344)
        _check_generation_status(self.eng, self.status, step)
        error, warning, self.warned = self.verdict(self.eng.pauli_stats_result(ticket), step, t, self.warned)
        if error is not None:
            raise ValueError(error)
        if warning is not None:
            # guard_check <- guard_flush <- energy_loop <- run_2d_crank_nicolson <- its device wrapper <- the caller
            warnings.warn(warning, stacklevel=6)


def _check_generation_status(eng, tickets: list, step: int) -> None:
    """Reads the status of the device-evaluated generation of every step up to ``step`` (tickets are ``(step, ticket)`` in
    step order) and raises what ``_validated_generation`` raises on the host path, non-finite before negative."""
    while tickets and tickets[0][0] <= step:
        for nonfinite, negative in eng.generation_status(tickets.pop(0)[1]):
            rates = np.array([np.nan if nonfinite else (-1.0 if negative else 0.0)])
            _validated_generation(rates, "custom", rates.shape)


class _Generation:
    """External generation of one problem during a run; a custom expression is compiled at its first use.  With
    ``on_device`` a custom expression is also compiled for the device evaluator; ``program`` stays None when it is
    outside the device subset (or the mode is not custom), and the host path serves it."""

    def __init__(self, spec, mask, E_bins, on_device: bool = False):
        self.spec, self.mask, self.E_bins = spec, mask, E_bins
        # the reference gates on the raw mode string (solver.py:1459)
        self.active = spec is not None and spec.mode != "none"
        self.constant = self.active and spec.mode.strip().lower() == "constant"
        self._compiled = None
        self.program = None
        if on_device and self.active and spec.mode.strip().lower() == "custom":
            self.program = device_expr.compile_program(spec.custom_body.strip() or "0.0", spec.custom_params)
            full = np.asarray(mask, dtype=bool)
            # (ny_full, nx_full, row0, col0): the device grid is the bounding box of the mask (_crop_to_bounding_box)
            self.window = full.shape + (int(np.flatnonzero(full.any(axis=1))[0]), int(np.flatnonzero(full.any(axis=0))[0]))

    def device_step(self, t: float):
        """(instruction words, slot table) of the step starting at ``t``, or None when the host path has to serve it."""
        if self.program is None:
            return None
        words = self.program.instructions_for(t)
        table = None if words is None else self.program.slot_table(self.E_bins, t)
        return None if table is None else (words, table)

    def amount(self, t_start: float, dt_of_step: float):
        return _generation_amount(self.spec, t_start, dt_of_step)

    def rates(self, t: float):
        """g_ext of custom mode at ``t`` as [NE, n] on the host (solver.py:918-962)."""
        if self._compiled is None:
            self._compiled = _CustomGeneration(self.spec, self.mask)
        return evaluate_external_generation(self.spec, self.E_bins, int(np.sum(self.mask)), t, self.mask,
                                            _compiled=self._compiled)


def _auto_precomputed(precomputed, gap_expression: str, mask, edges, edge_conditions, **parameters):
    """``precomputed`` as given, or built from ``gap_expression`` when there is one (solver.py:1106-1124)."""
    if precomputed is None and gap_expression.strip():
        from .precompute import precompute_arrays
        params = SimulationParameters(gap_expression=gap_expression, **parameters)
        precomputed = precompute_arrays(mask, edges, edge_conditions, params, include_collision_kernels=False)
    return precomputed


def _energy_diffuser(eng, sched, scheme, rtol, E_bins, gap, precomputed, coefficients) -> "_Diffuser":
    """Diffusion of NE * M fields, field i * M + m being bin i of member m: ``precomputed["D_array"]`` when there is one (a
    variable D(x) per bin if the gap is not uniform, solver.py:1145-1164), else D(E) of each member's coefficient
    (solver.py:1166-1174)."""
    NE, M = len(E_bins), len(coefficients)
    if precomputed is None:
        per_member = [[float(v) for v in _tb.diffusion_coefficients(E_bins, gap, D)] for D in coefficients]
    else:
        D_array = np.asarray(precomputed["D_array"], dtype=float)
        if not bool(precomputed.get("is_uniform", True)):
            dfield = np.zeros((NE, eng.ncell))
            dfield[:, eng.mask_flat] = D_array
            return _Diffuser(eng, NE * M, sched.dt, sched.rem, scheme, rtol, dfield=np.repeat(dfield, M, axis=0))
        per_member = [[float(D_array[i, 0]) if D_array.ndim == 2 else float(D_array[i]) for i in range(NE)]] * M
    return _Diffuser(eng, NE * M, sched.dt, sched.rem, scheme, rtol,
                     dcoef=[per_member[m][i] for i in range(NE) for m in range(M)])


def _one_call_diffusion(diffuser, collisions: bool, generation: bool, warn_threshold, error_threshold, rho_tab) -> bool:
    """Pure diffusion (no collisions, no generation) with a guard that cannot fire (no thresholds, no forbidden bins):
    nothing but diffusion steps lies between two store points, so the stretch is one call as in scalar mode."""
    return bool(diffuser is not None and not collisions and not generation and diffuser.scheme == "adi"
                and error_threshold is None and warn_threshold is None and float(np.min(rho_tab)) > 1e-30)


def _guard_rule(eng, mask, E_bins, enforce_pauli, warn_threshold, error_threshold):
    """``_pauli_verdict`` of one run as ``rule(stats, step, time, warned)``."""
    coords = np.argwhere(mask)
    cell_to_px = np.cumsum(eng.mask_flat) - 1
    return lambda stats, step, t, warned: _pauli_verdict(stats, step, t, E_bins, coords, cell_to_px, warned, enforce_pauli,
                                                         warn_threshold, error_threshold)


def _phonon_widths(eng, omega_bins, dE, histories):
    """Integration widths of the phonon grid on the device when any member wants phonon frames, else None."""
    if all(h is None for h in histories):
        return None
    return eng.upload_vector(integration_widths_from_centers(omega_bins, fallback_width=dE))


def _dynamic_phonon_history(out: Outputs, m: int, omega_bins) -> dict:
    return {"phonon_frames": out.phonon_frames[m],
            "phonon_energy_frames": out.phonon_energy_frames[m],
            "phonon_energy_bins": np.asarray(omega_bins, dtype=float).copy(),
            "phonon_metadata": {"mode": "dynamic_local_coupled", "field_units": "integrated_occupation",
                                "energy_frame_units": "occupation"}}


def _run_scalar(eng: Engine, sched, out: Outputs, inits, coefficients, enable_diffusion, bath_temperatures, histories,
                scheme, rtol, samplers=()) -> list:
    """Legacy scalar mode, energy_gap == 0 (solver.py:1517-1587), for M members as one [M, ncell] field set; the result
    tuple of every member.  ``samplers``: the samplers of the M fields (one plane per member), fetched by the caller."""
    mask, M = out.mask, out.members
    u_host = np.stack([f[mask].astype(float) for f in inits])
    u = eng.upload_packed(u_host)
    diffuser = (_Diffuser(eng, M, sched.dt, sched.rem, scheme, rtol, dcoef=[float(D) for D in coefficients])
                if enable_diffusion else None)
    if diffuser is not None:
        _bind_flux(samplers, diffuser)
    out.add_host_frames(0.0, [reconstruct_field(mask, v) for v in u_host],
                        [float(np.sum(v) * out.dx * out.dx) for v in u_host])
    scalar_loop(sched, diffuser, u, out, eng, samplers)
    for T_bath, history in zip(bath_temperatures, histories):
        if history is not None:
            f, ef, bins, meta = build_fixed_phonon_history(mask=mask, times=out.times, bath_temperature=T_bath,
                                                           phonon_energy_bins=None)
            history.update({"phonon_frames": f, "phonon_energy_frames": ef, "phonon_energy_bins": bins,
                            "phonon_metadata": meta})
    return [(list(out.times), out.frames[m], out.mass[m], _color_limits(out.frames[m]), None, None) for m in range(M)]


# ------------------------------------------------------------------------------------------------------------ #
# step API (solver.py:794-875): in-place collision steps on host arrays in the reference's packed layout
# ------------------------------------------------------------------------------------------------------------ #
def _collision_step_host(state, phonon_state, kr, ks, rho, idx_diff, idx_sum, sign, dE, dt, en_r, en_s, upd,
                         cls=None, device=None) -> None:
    from .engine import CompiledGeometry, link_flags
    n = state.shape[1]
    if phonon_state.shape[1] != n:
        raise ValueError("phonon_state shape does not match quasiparticle state.")
    mask = np.ones((1, n), dtype=bool)
    z = np.zeros(mask.shape)
    eng = Engine(CompiledGeometry(mask, 1.0, link_flags(mask), z, z, z, z), device=device)
    tab = eng.make_collision_tables(kr, ks, rho, idx_diff, idx_sum, sign, cls)
    if tab["nw"] > phonon_state.shape[0]:
        raise ValueError("phonon_state has fewer bins than the index maps address.")
    s_in = eng.upload_packed(state)
    s_out = eng.empty(*s_in.shape)
    ph = eng.upload_packed(phonon_state)
    eng.collide(tab, s_in, s_out, ph, dE, dt, en_r, en_s, upd)
    state[:, :] = eng.download_packed(s_out)
    if upd:
        phonon_state[:, :] = eng.download_packed(ph)


def _euler_call(state2d: np.ndarray, K_r, G_therm, K_s, rho, dE, dt, rhs_only, device=None) -> np.ndarray:
    import ctypes as C
    from . import _hip
    from .engine import require_gpu
    torch = require_gpu()
    lib = _hip.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)  # noqa: E731
    s_in = up(state2d)
    out = torch.empty_like(s_in)
    kr, g, ks, rh = up(K_r), up(G_therm), up(K_s), up(rho)
    ptr = lambda t: 0 if t is None else int(t.data_ptr())  # noqa: E731
    _hip.check(lib.qp_euler_collision(state2d.shape[0], state2d.shape[1], ptr(s_in), ptr(out), ptr(kr), ptr(g), ptr(ks),
                                      ptr(rh), float(dE), float(dt), int(rhs_only),
                                      int(torch.cuda.current_stream(dev).cuda_stream)), "qp_euler_collision")
    return out.cpu().numpy()


def apply_scattering_step(state: np.ndarray, K_s: np.ndarray, rho_bins: np.ndarray, dE: float, dt: float) -> None:
    """One forward-Euler step of fixed-bath scattering, in place on state[NE, n] (solver.py:551-580)."""
    state[:, :] = _euler_call(state, None, None, K_s, rho_bins, dE, dt, False)


def apply_recombination_step(state: np.ndarray, K_r: np.ndarray, G_therm: np.ndarray, dE: float, dt: float) -> None:
    """One forward-Euler step of recombination + thermal generation, in place (solver.py:583-605)."""
    state[:, :] = _euler_call(state, K_r, G_therm, None, None, dE, dt, False)


def _collision_rhs(n: np.ndarray, K_r, K_s, rho_bins, G_therm, dE: float) -> np.ndarray:
    """dn/dt of one pixel from recombination (if K_r and G_therm) and scattering (if K_s and rho) (solver.py:608-637)."""
    use_r = K_r is not None and G_therm is not None
    use_s = K_s is not None and rho_bins is not None
    if not (use_r or use_s):
        return np.zeros_like(n)
    return _euler_call(np.asarray(n, dtype=float)[:, None], K_r if use_r else None, G_therm if use_r else None,
                       K_s if use_s else None, rho_bins if use_s else None, dE, 0.0, True)[:, 0]


def _mask_to_index(mask: np.ndarray):
    """index_map[ny, nx] (-1 outside) and interior (row, col) list in argwhere order (solver.py:53-58)."""
    mask = np.asarray(mask, dtype=bool)
    index_map = -np.ones(mask.shape, dtype=int)
    index_map[mask] = np.arange(int(mask.sum()))
    return index_map, [tuple(map(int, rc)) for rc in np.argwhere(mask)]


def _assemble_csr(geom, D):
    """CSR matrix and source vector of the 5-point operator described by a CompiledGeometry (D scalar or packed [n])."""
    from scipy import sparse
    mask = geom.mask
    n = int(mask.sum())
    index = -np.ones(mask.shape, dtype=np.int64)
    index[mask] = np.arange(n)
    Dg = np.zeros(mask.shape)
    Dg[mask] = D
    inv_dx2 = 1.0 / (geom.dx * geom.dx)
    rows, cols, vals = [], [], []
    diag = -(geom.ex + geom.ey) * Dg * inv_dx2
    for bit, (dr, dc) in ((1, (0, -1)), (2, (0, 1)), (4, (-1, 0)), (8, (1, 0))):
        r, c = np.nonzero((geom.flags & bit) > 0)
        dp, dq = Dg[r, c], Dg[r + dr, c + dc]
        w = 2.0 * dp * dq / np.maximum(dp + dq, 1e-30) * inv_dx2
        rows.append(index[r, c])
        cols.append(index[r + dr, c + dc])
        vals.append(w)
        np.subtract.at(diag, (r, c), w)
    r, c = np.nonzero(mask)
    rows.append(index[r, c])
    cols.append(index[r, c])
    vals.append(diag[r, c])
    L = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    return L, ((geom.sx + geom.sy) * Dg * inv_dx2)[mask], index


def build_laplacian_with_boundaries(mask, edges, edge_conditions, dx):
    """(L csr [n, n] in 1/dx^2 units, source [n], index_map) -- host-side equivalent of solver.py:152-212.

    The GPU path never forms this matrix; the function exists for callers that inspect the operator.
    """
    geom = compile_geometry(np.asarray(mask, dtype=bool), edges, edge_conditions, dx)
    L, src, index = _assemble_csr(geom, 1.0)
    index_map = np.where(geom.mask, index, -1).astype(int)
    return L, src, index_map


def build_variable_diffusion_laplacian(mask, edges, edge_conditions, dx, D_spatial):
    """(L_D csr, source) with harmonic-mean face diffusivities (host-side equivalent of solver.py:235-321)."""
    geom = compile_geometry(np.asarray(mask, dtype=bool), edges, edge_conditions, dx)
    L, src, _ = _assemble_csr(geom, np.asarray(D_spatial, dtype=float))
    return L, src


def apply_collision_step_fischer_catelani_uniform(state, phonon_state, K_r0, K_s0, rho_bins, omega_idx_diff,
                                                  omega_idx_sum, diff_sign, dE, dt, *, enable_recombination,
                                                  enable_scattering, update_phonons=True, device=None) -> None:
    """One coupled collision step with one kernel set for all pixels, in place (solver.py:794-831)."""
    _collision_step_host(state, phonon_state, None if K_r0 is None else np.asarray(K_r0)[None],
                         None if K_s0 is None else np.asarray(K_s0)[None], np.asarray(rho_bins)[None], omega_idx_diff,
                         omega_idx_sum, diff_sign, dE, dt, enable_recombination, enable_scattering, update_phonons,
                         device=device)


def apply_collision_step_fischer_catelani_nonuniform(state, phonon_state, K_r0_all, K_s0_all, rho_all, omega_idx_diff,
                                                     omega_idx_sum, diff_sign, dE, dt, *, enable_recombination,
                                                     enable_scattering, update_phonons=True, device=None) -> None:
    """Per-pixel kernels [n, NE, NE] / [n, NE]; de-duplicated into classes before upload (solver.py:834-875)."""
    rho_all = np.asarray(rho_all, dtype=float)
    if rho_all.shape[0] != state.shape[1]:
        raise ValueError("rho_all shape does not match quasiparticle state.")
    n = rho_all.shape[0]
    key = [rho_all.reshape(n, -1)]
    if K_r0_all is not None:
        key.append(np.asarray(K_r0_all, dtype=float).reshape(n, -1))
    if K_s0_all is not None:
        key.append(np.asarray(K_s0_all, dtype=float).reshape(n, -1))
    _, first, cls = np.unique(np.concatenate(key, axis=1), axis=0, return_index=True, return_inverse=True)
    cls = np.asarray(cls).reshape(-1)
    _collision_step_host(state, phonon_state, None if K_r0_all is None else np.asarray(K_r0_all)[first],
                         None if K_s0_all is None else np.asarray(K_s0_all)[first], rho_all[first], omega_idx_diff,
                         omega_idx_sum, diff_sign, dE, dt, enable_recombination, enable_scattering, update_phonons,
                         cls=cls, device=device)
