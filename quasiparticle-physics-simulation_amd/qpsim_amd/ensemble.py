"""Ensembles of independent runs of one geometry: ``run_2d_crank_nicolson_ensemble``.

M runs that share geometry, time stepping, energy grid and physics tables but differ in their initial state, generation,
bath temperature or diffusion coefficient are batched on one device: the planes are laid out [bin][member][cell], so the
diffusion plan sees NE * M fields and the collision kernels M * ncell pixels, and one launch serves every member.  The
Pauli guard is reduced per member on the device (``qp_pauli_stats_members`` and the ``*_guarded_members`` collision calls),
so every member warns and raises exactly as its lone run would, its messages prefixed ``member m: ``.

Parameter sweeps: ``sweep={"tau_0": [...], "T_c": [...], ...}`` (keys of ``SWEEP_KEYS``, one value per member) varies the
collision physics over the members.  Every member then has its own K^r_0 / K^s_0 / rho tables on the device (built on the
host exactly as its lone run builds them); with NE = 4 ... 16 and a member cell count that is a multiple of 64 the register
collision kernels - single pass and double half-step - read the table of the wave's member, bit-equal to the lone tables;
with NE = 30, 32, 40, 50 (the default 50 included) and a member cell count that is a multiple of 256 every block of the
one-pass collision kernel stages the tables of its member, bit-equal as well; other shapes and sizes run the
one-wave-per-pixel kernel through a member class map.  Outside NE = 4 ... 16 a step pair takes two calls instead of the
pair pass.  A sweep whose members all end up with the same tables runs exactly as the call without ``sweep``.

Rounding: members are bit-equal to their lone ``run_2d_crank_nicolson`` call with ``diffusion_scheme="adi"`` when both use
the same ADI tile family (``QPSIM_FINE_TILES``) and the same step form (``QPSIM_ADI_FUSED``: a batch of at least 4 Mi
cells takes the one-pass steps, which round the interface rows differently, while a smaller lone member does not), within
2e-13 relative otherwise, and within 1e-12 relative with ``cn_exact`` (the iteration's stop test is global over the batch).

Time traces (``trace_out=[]`` of the ensemble call, ``trace_regions`` / ``trace_every`` in the common arguments): one
reduction launch per sample serves all members of a batch.  A member's trace is bit-equal to its lone run's where its state
is (the conditions above) and the device grid holds an even number of cells; with an odd count every second member plane
starts on an odd element, pairs its cells differently, and the sums agree to rounding.

Coarse frames (``coarse_out=[]`` of the ensemble call, ``coarse_bin`` / ``coarse_every`` in the common arguments): one block
reduction launch per sample serves all members of a batch.  A member's coarse frames are bit-equal to its lone run's
wherever its state is (the conditions above), whatever the parity of the cell count.

Collision rate traces (``rates_out=[]`` of the ensemble call, ``rates_regions`` / ``rates_every`` in the common arguments):
one ``qp_collision_rates`` call per sample serves all members of a batch, with a sweep every member through its own tables.
A member's rates are bit-equal to its lone run's wherever its state and phonons are, whatever the parity of the cell count.

Phonon rate traces (``phonon_rates_out=[]`` of the ensemble call, ``phonon_rates_regions`` / ``phonon_rates_every`` in the
common arguments): one ``qp_phonon_rates`` call per sample, under the same rules and with the same bit-equality.

Boundary outflow traces (``flux_out=[]`` of the ensemble call, ``flux_surfaces`` / ``flux_every`` in the common arguments):
one ``qp_boundary_flux`` call per sample serves all members of a batch, member m with the coefficients of its own fields.
Which thread adds which face depends on the face list alone, so a member's outflow is bit-equal to its lone run's wherever
its state is, whatever the parity of the cell count.
"""
from __future__ import annotations

import inspect
import warnings

import numpy as np

from . import device_expr
from . import solver as S
from .distributed import shard_members
from .engine import Engine
from .timeloop import EnergyRun, Outputs, Schedule, energy_loop

__all__ = ["run_2d_crank_nicolson_ensemble", "PER_MEMBER_KEYS", "SWEEP_KEYS", "member_arguments", "plan_batches",
           "generation_amounts", "last_run_stats"]

# keys a member may set for itself; everything else is shared by the ensemble
PER_MEMBER_KEYS = ("initial_field", "energy_weights", "initial_condition_spec", "external_generation", "bath_temperature",
                   "diffusion_coefficient", "phonon_history_out", "progress_callback")
# shared keys that ``sweep=`` may vary over the members (one value per member): the collision physics
SWEEP_KEYS = ("tau_0", "tau_s", "tau_r", "T_c", "dynes_gamma")
_STATS: dict = {}


def last_run_stats() -> dict:
    """Counters of the last ensemble call on this process: batches, pair passes, guarded single calls."""
    return dict(_STATS)


def _checked_sweep(sweep, nmembers: int, common: dict) -> dict:
    """``sweep`` as {key: list of ``nmembers`` values}.  ``ValueError`` naming the key for an unknown key, a list of the
    wrong length, a key that ``common`` sets to something else than every swept value, or a sweep next to 'precomputed' /
    'gap_expression'."""
    if sweep is None:
        return {}
    if not isinstance(sweep, dict):
        raise TypeError("sweep must be a dict of {key: one value per member}")
    shared_pre = common.get("precomputed") is not None or str(common.get("gap_expression", "") or "").strip()
    out = {}
    for key, values in sweep.items():
        if key not in SWEEP_KEYS:
            raise ValueError(f"sweep: '{key}' cannot be swept (sweep keys: {', '.join(SWEEP_KEYS)})")
        if isinstance(values, (str, bytes)) or not hasattr(values, "__len__"):
            raise ValueError(f"sweep: '{key}' needs a sequence of {nmembers} values, one per member")
        values = list(values)
        if len(values) != nmembers:
            raise ValueError(f"sweep: '{key}' has {len(values)} values for {nmembers} members")
        if shared_pre:
            raise ValueError(f"'{key}' cannot be swept together with 'precomputed' or 'gap_expression' (the precomputed "
                             "arrays are built from one value)")
        if key in common and any(v != common[key] for v in values):
            raise ValueError(f"sweep: '{key}' is also set in the common arguments to {common[key]!r}, which differs from "
                             "its swept values; give it in one place")
        out[key] = values
    return out


def member_arguments(members: list[dict], common: dict, sweep: dict | None = None) -> list[dict]:
    """Complete keyword sets of ``run_2d_crank_nicolson`` per member (defaults applied, ``sweep[key][m]`` substituted for
    member m).  Raises ``ValueError`` naming the key when a member sets a shared key, varies D / bath temperature where the
    auto-precompute would depend on it, or the sweep is malformed (``_checked_sweep``).  A swept key may also stand in
    ``common`` only with the value every member sweeps to; any other value there is refused as a conflict."""
    sig = inspect.signature(S.run_2d_crank_nicolson)
    members = list(members)
    sweep = _checked_sweep(sweep, len(members), common)
    out = []
    for m, over in enumerate(members):
        if not isinstance(over, dict):
            raise TypeError(f"member {m}: expected a dict of per-member keyword arguments")
        for key in over:
            if key not in PER_MEMBER_KEYS:
                raise ValueError(f"member {m}: '{key}' is shared by all members of an ensemble and cannot be set per "
                                 f"member (per-member keys: {', '.join(PER_MEMBER_KEYS)})")
        kw = dict(common, **over)
        kw.update({key: values[m] for key, values in sweep.items()})
        try:
            bound = sig.bind(**kw)
        except TypeError as exc:
            raise TypeError(f"member {m}: {exc}") from None
        bound.apply_defaults()
        out.append(dict(bound.arguments))
    shared_pre = common.get("precomputed") is not None or str(common.get("gap_expression", "") or "").strip()
    if shared_pre:
        for key in ("diffusion_coefficient", "bath_temperature"):
            if any(key in over for over in members):
                raise ValueError(f"'{key}' cannot be set per member together with 'precomputed' or 'gap_expression' "
                                 "(the precomputed arrays are built from one value)")
    return out


def plan_batches(member_ids: list[int], bytes_per_member: float, free_bytes: float | None,
                 max_members_per_batch: int | None) -> list[list[int]]:
    """Consecutive batches of ``member_ids``: at most ``max_members_per_batch`` members each, and (when ``free_bytes`` is
    known) no more than fit into 80 % of it."""
    cap = max(1, len(member_ids)) if max_members_per_batch is None else int(max_members_per_batch)
    if cap < 1:
        raise ValueError("max_members_per_batch must be at least 1")
    if free_bytes is not None and bytes_per_member > 0:
        cap = min(cap, max(1, int(0.8 * free_bytes // bytes_per_member)))
    return [member_ids[i:i + cap] for i in range(0, len(member_ids), cap)]


def generation_amounts(specs, t_start: float, dt_of_step: float) -> list:
    """Per member dt g_ext of a step starting at ``t_start``: a number for constant / pulse / no generation, None for a
    custom expression (evaluated on the host)."""
    return [S._generation_amount(spec, t_start, dt_of_step) for spec in specs]


def _bytes_per_member(kw: dict, plans=()) -> float:
    """Device bytes one member needs: state planes (x2), phonon planes, diffusion / exact-CN work planes and its share of
    the buffer of every sampler (``plans``: the time-trace / coarse-frame plans of the call), as the buffer check counts it."""
    mask = np.asarray(kw["mask"], dtype=bool)
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    ncell = (rows[-1] - rows[0] + 1) * (cols[-1] - cols[0] + 1) if rows.size else 1
    ne = int(kw["num_energy_bins"]) if kw["energy_gap"] > 0.0 else 1
    nw = 3 * ne
    sched = Schedule(kw["total_time"], kw["dt"], 1)
    return 8.0 * ncell * (8 * ne + 3 * nw + 8) + sum(S._sample_buffer_bytes(plan, sched, 1, ne) for plan in plans)


def run_2d_crank_nicolson_ensemble(members: list[dict], *, sweep: dict | None = None, errors: str = "raise",
                                   max_members_per_batch: int | None = None, process_group=None,
                                   trace_out: list | None = None, coarse_out: list | None = None,
                                   rates_out: list | None = None, phonon_rates_out: list | None = None,
                                   flux_out: list | None = None, **common) -> list:
    """Run ``len(members)`` independent problems batched on the device.

    ``common`` takes the keyword arguments of ``run_2d_crank_nicolson``; ``members[m]`` overrides only the keys of
    ``PER_MEMBER_KEYS``.  ``sweep`` maps keys of ``SWEEP_KEYS`` (tau_0, tau_s, tau_r, T_c, dynes_gamma) to one value per
    member: member m runs as its lone call with ``sweep[key][m]`` in place of the common value (``tau_s`` / ``tau_r``
    default from that member's ``tau_0``; its ``dynes_gamma`` also shapes its initial state and its Pauli guard).  A swept
    key must not be set to another value in ``common``, and a sweep cannot be combined with ``precomputed`` or
    ``gap_expression``.  The register collision kernels serve per-member tables for ``num_energy_bins`` 4 ... 16 when the
    member's device grid holds a multiple of 64 cells, the one-pass kernel for 30, 32, 40 and 50 (the default) when it holds
    a multiple of 256; other sizes and grids run the one-wave-per-pixel kernel.
    Entry m is the 6-tuple member m's lone call returns (its ``phonon_history_out`` filled the same
    way), or - with ``errors="return"`` - the ``ValueError`` its Pauli guard raised (the other members finish).  With
    ``errors="raise"`` the first violation (earliest step, then lowest member) raises ``ValueError("member m: ...")``.
    Members run in consecutive batches when they do not all fit on the device (``max_members_per_batch`` caps a batch).
    With an initialised ``process_group`` of world size > 1, rank r runs ``shard_members(M, world, r)`` on its current
    device and every rank returns the full list.
    Time traces: ``trace_regions`` / ``trace_every`` are shared keys of ``common``; the sink is the list ``trace_out`` of
    THIS call (never a member key), cleared at entry and filled on normal return with one dict per member as the lone
    call fills its ``trace_out`` (None for a member that failed under ``errors="return"``).  One reduction launch per sample
    serves all members of a batch.
    Coarse frames: ``coarse_bin`` / ``coarse_every`` are shared keys of ``common`` and the sink is the list ``coarse_out`` of
    this call, handled exactly as ``trace_out`` is (one dict per member as the lone call fills its ``coarse_out``, None for
    a failed member); one block reduction launch per sample serves all members of a batch.
    Collision rate traces: ``rates_regions`` / ``rates_every`` are shared keys of ``common`` and the sink is the list
    ``rates_out`` of this call, handled exactly as ``trace_out`` is; one ``qp_collision_rates`` call per sample serves all
    members of a batch, with a sweep each member through its own tables.
    Phonon rate traces: ``phonon_rates_regions`` / ``phonon_rates_every`` are shared keys of ``common`` and the sink is the
    list ``phonon_rates_out`` of this call, handled exactly as ``rates_out`` is (one ``qp_phonon_rates`` call per sample).
    Boundary outflow traces: ``flux_surfaces`` / ``flux_every`` are shared keys of ``common`` and the sink is the list
    ``flux_out`` of this call, filled as ``trace_out`` is (one dict per member as the lone call fills its ``flux_out``, None
    for a failed member) but cleared only once every argument has been checked; one ``qp_boundary_flux`` call per sample
    serves all members of a batch, each with its own diffusion coefficients."""
    if errors not in ("raise", "return"):
        raise ValueError("errors must be 'raise' or 'return'")
    kws = member_arguments(list(members), common, sweep)
    for sink in (trace_out, coarse_out, rates_out, phonon_rates_out):
        if sink is not None:
            sink.clear()
    # per kind of sampler that is on (plan, sink of this call, {member: what its lone run's sink would receive})
    sampling: list = []
    if kws:                        # refuse bad trace / coarse-frame arguments before any device is touched
        a = kws[0]
        sampling = [(plan, sink, {}) for plan, sink in S._sampling_plans(
            np.asarray(a["mask"], dtype=bool), trace_out, a["trace_regions"], a["trace_every"], coarse_out, a["coarse_bin"],
            a["coarse_every"], rates_out, a["rates_regions"], a["rates_every"], a, phonon_rates_out,
            a["phonon_rates_regions"], a["phonon_rates_every"], flux_out, a["flux_surfaces"], a["flux_every"])]
    elif flux_out is not None:
        flux_out.clear()
    _STATS.clear()
    _STATS.update(batches=0, pair_passes=0, guarded_calls=0)
    device_expr.reset_run_stats()
    if not kws:
        return []
    world, rank = 1, 0
    if process_group is not None:
        import torch.distributed as dist
        if dist.is_initialized():
            world, rank = dist.get_world_size(process_group), dist.get_rank(process_group)
    mine = shard_members(len(kws), world, rank) if world > 1 else list(range(len(kws)))
    free = None
    if mine:
        from .engine import require_gpu
        torch = require_gpu()
        dev = kws[0].get("device")
        dev = torch.device("cuda", torch.cuda.current_device()) if (dev is None or world > 1) else torch.device(dev)
        free = float(torch.cuda.mem_get_info(dev)[0])
    batches = plan_batches(mine, _bytes_per_member(kws[0], [plan for plan, _, _ in sampling]), free, max_members_per_batch)
    # one batch on one process raises at once; otherwise every batch finishes and the earliest violation is raised after
    eager = errors == "raise" and world == 1 and len(batches) == 1
    results: dict[int, object] = {}
    for batch in batches:
        res = _run_batch([kws[m] for m in batch], batch, "raise" if eager else "return", None if world == 1 else dev,
                         sampling)
        results.update(zip(batch, res))
    out = [results.get(m) for m in range(len(kws))]
    if world > 1:
        import torch.distributed as dist
        local = [(m, results[m], kws[m]["phonon_history_out"], [got.get(m) for _, _, got in sampling]) for m in mine]
        gathered = [None] * world
        dist.all_gather_object(gathered, local, group=process_group)
        for part in gathered:
            for m, res, ph, sampled in part:
                out[m] = res
                for (_, _, got), value in zip(sampling, sampled):
                    got[m] = value
                target = kws[m]["phonon_history_out"]
                if target is not None and ph is not None and target is not ph:
                    target.clear()
                    target.update(ph)
    if errors == "raise":
        failures = [(getattr(r, "step", 0), m, r) for m, r in enumerate(out) if isinstance(r, Exception)]
        if failures:
            raise min(failures, key=lambda f: f[:2])[2]
    for _, sink, got in sampling:
        sink.extend(got.get(m) for m in range(len(kws)))
    return out


def _run_batch(kws: list[dict], ids: list[int], errors: str, device=None, sampling=()) -> list:
    import torch
    dev = kws[0]["device"] if device is None else device
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
    with torch.cuda.device(dev):
        _STATS["batches"] += 1
        return _run_batch_on_device(kws, ids, errors, dev, sampling)


def _prefixed(m: int, fn, *args):
    try:
        return fn(*args)
    except (ValueError, TypeError) as exc:
        raise type(exc)(f"member {m}: {exc}") from exc


def _run_batch_on_device(kws, ids, errors, device, sampling=()):
    """One batch; the dict of every entry of ``sampling`` (per kind of sampler: plan, sink, {member id: dict}) receives
    what each member's ``trace_out`` / ``coarse_out`` would, None for a member that failed."""
    a = kws[0]
    checked = [_prefixed(ids[j], S._checked_run_arguments, k["mask"], k["initial_field"], k["diffusion_coefficient"],
                         k["dt"], k["total_time"], k["store_every"], k["enable_diffusion"], k["enable_recombination"],
                         k["enable_scattering"], k["tau_0"], k["tau_s"], k["tau_r"], k["external_generation"],
                         k["phonon_history_out"]) for j, k in enumerate(kws)]
    mask, _, store_every, n, _, _ = checked[0]
    inits = [c[1] for c in checked]
    geom = S._run_geometry(mask, a["edges"], a["edge_conditions"], a["dx"], a["enable_diffusion"])
    sched = Schedule(a["total_time"], a["dt"], store_every)
    energy = a["energy_gap"] > 0.0
    nplanes = a["num_energy_bins"] if energy else 1
    for plan, _, _ in sampling:
        S._check_sample_buffer(plan, sched, len(kws), nplanes)
    eng = Engine(geom, device=device)
    eng.pin_stream()
    flags = eng.d_flags.reshape(-1).repeat(len(kws))     # [member][cell]
    out = Outputs(mask, a["dx"], [k["progress_callback"] for k in kws])
    samplers = tuple(plan.sampler(eng, mask, sched, len(kws), nplanes) for plan, _, _ in sampling)
    if not energy:
        results = S._run_scalar(eng, sched, out, inits, [k["diffusion_coefficient"] for k in kws], a["enable_diffusion"],
                                [k["bath_temperature"] for k in kws], [k["phonon_history_out"] for k in kws],
                                a["diffusion_scheme"], a["cn_rtol"], samplers)
    else:
        results = _run_energy_batch(eng, sched, out, kws, ids, errors, inits, n, flags, [(c[4], c[5]) for c in checked],
                                    samplers)
    if sampling:
        E_bins, dE = (S.build_energy_grid(a["energy_gap"], a["energy_min_factor"], a["energy_max_factor"], nplanes)
                      if energy else (None, None))
    for (plan, _, got), sampler in zip(sampling, samplers):
        rows = sampler.fetch()
        for j, res in enumerate(results):
            got[ids[j]] = None if isinstance(res, Exception) else plan.result(sampler.times, rows[:, j], E_bins, a["dx"], dE)
    return results


def table_parameters(kws: list[dict], taus: list[tuple]) -> list[tuple]:
    """Per member what its collision tables depend on beyond the shared energy grid: (dynes_gamma, tau_r, tau_s, T_c), with
    the entries of a disabled process blanked (they reach no table).  ``taus``: (tau_s, tau_r) as resolved per member."""
    out = []
    for k, (tau_s, tau_r) in zip(kws, taus):
        en_r, en_s = bool(k["enable_recombination"]), bool(k["enable_scattering"])
        out.append((k["dynes_gamma"], tau_r if en_r else None, tau_s if en_s else None,
                    k["T_c"] if (en_r or en_s) else None))
    return out


class _MembersRun(EnergyRun):
    """M problems over planes [bin][member][cell], driven by the ``*_members`` library calls: the guard is reduced per member
    and every member warns / fails for itself.  ``ctab``, ``floor``, ``physics`` = (recombination, scattering, phonon
    update), ``flags``, ``generations``, ``ids``, ``errors``, ``verdict`` and ``quiet_below`` are set by the caller."""

    def __init__(self, *args):
        super().__init__(*args)
        self.members = self.out.members
        self.warned = [False] * self.members
        self.failed: list = [None] * self.members
        self.step = 0              # generate() is called once per step: the step its status tickets belong to
        self.status: list = []

    def _generate_on_device(self, custom: list, t: float, dt_step: float) -> list:
        """Launches the device evaluator for the members of ``custom`` whose expression it serves at this step - one launch
        per distinct program, members with the same body, words and slots sharing it - and returns the members left to the
        host path."""
        gens, launches, host = self.generations, {}, []
        for m in custom:
            launch = gens[m].device_step(t)
            if launch is None:
                host.append(m)
                continue
            key = (gens[m].program.body, launch[0].tobytes(), launch[1].tobytes())
            launches.setdefault(key, launch + ([],))[2].append(m)
        if launches:
            self.status.append((self.step, self.eng.add_generation_expr(
                self.state, gens[custom[0]].window, list(launches.values()), dt_step, self.members, self.flags)))
        device_expr.count_steps(device=len(custom) - len(host), host=len(host))
        return host

    def generate(self, t: float, dt_step: float) -> None:
        gens, eng, M = self.generations, self.eng, self.members
        self.step += 1
        if not any(g.active for g in gens):
            return
        amounts = generation_amounts([g.spec for g in gens], t, dt_step)
        custom = self._generate_on_device([m for m, x in enumerate(amounts) if x is None], t, dt_step)
        if custom:                                               # custom expressions evaluated on the host
            n = int(np.sum(self.out.mask))
            g = np.zeros((self.state.shape[0] // M, M, n))
            for m in custom:
                g_ext = gens[m].rates(t)
                if g_ext is not None:
                    g[:, m] = g_ext
            eng.add_scaled(self.state, eng.upload_packed(g.reshape(-1, n)), dt_step)
        consts = [0.0 if x is None else x for x in amounts]
        if any(g.constant for g in gens) or any(x != 0.0 for x in consts):
            eng.add_constant_members(self.state, consts, eng.ncell, M, self.flags)

    def pair_amount(self, t_next: float, dt_next: float):
        # one scalar generation amount inside the pair kernel: only when every member adds the same
        nxt = generation_amounts([g.spec for g in self.generations], t_next, dt_next)
        return nxt[0] if all(x is not None and x == nxt[0] for x in nxt) else None

    def collide(self, dt_col: float, guarded: bool):
        eng = self.eng
        if not guarded:
            return eng.collide(self.ctab, self.state, self.state_alt, self.phonon, self.dE, dt_col, *self.physics,
                               ncell=self.ncell, flags=self.flags)
        _STATS["guarded_calls"] += 1
        return eng.collide_guarded_members(self.ctab, self.state, self.state_alt, self.phonon, self.dE, dt_col,
                                           *self.physics, self.floor, eng.ncell, self.members, self.flags)

    def collide_pair(self, dt_a: float, dt_b: float, amount: float):
        _STATS["pair_passes"] += 1
        return self.eng.collide_pair_guarded_members(self.ctab, self.state, self.state_alt, self.phonon, self.dE, dt_a, dt_b,
                                                     amount, *self.physics, self.floor, self.eng.ncell, self.members,
                                                     self.flags)

    def guard_launch(self):
        return self.eng.pauli_stats_members_launch(self.state, self.ctab, self.floor, self.eng.ncell, self.members,
                                                   self.flags)

    def guard_check(self, ticket, step: int, t: float) -> None:
        S._check_generation_status(self.eng, self.status, step)
        for m, stats in enumerate(self.eng.pauli_stats_members_result(ticket)):
            # no forbidden density and no occupation above the lower threshold: the member has nothing to report
            if self.failed[m] is not None or (stats[2] is None and not stats[0] > self.quiet_below):
                continue
            error, warning, self.warned[m] = self.verdict(stats, step, t, self.warned[m])
            if error is not None:
                self.failed[m] = ValueError(f"member {self.ids[m]}: {error}")
                self.failed[m].step = step
                if self.errors == "raise":
                    raise self.failed[m]
            elif warning is not None:
                # guard_check <- guard_flush <- energy_loop <- _run_energy_batch <- _run_batch_on_device <- _run_batch <-
                # run_2d_crank_nicolson_ensemble <- the caller
                warnings.warn(f"member {self.ids[m]}: {warning}", stacklevel=8)


def _run_energy_batch(eng, sched, out, kws, ids, errors, inits, n, flags, taus, samplers=()):
    """Energy-resolved mode for M members: the setup of ``run_2d_crank_nicolson`` over [bin][member][cell] planes."""
    a, M, mask = kws[0], len(kws), out.mask
    tau_s_eff, tau_r_eff = taus[0]
    tparams = table_parameters(kws, taus)
    if all(p == tparams[0] for p in tparams):                    # one table set serves every member (no sweep, or all equal)
        tparams = None
    ncm = eng.ncell
    gap, NE = a["energy_gap"], a["num_energy_bins"]
    E_bins, dE = S.build_energy_grid(gap, a["energy_min_factor"], a["energy_max_factor"], NE)
    precomputed = S._auto_precomputed(                           # one value of D and T_b (member_arguments checked)
        a["precomputed"], a["gap_expression"], mask, a["edges"], a["edge_conditions"],
        diffusion_coefficient=a["diffusion_coefficient"], dt=a["dt"], total_time=a["total_time"], mesh_size=a["dx"],
        energy_gap=gap, energy_min_factor=a["energy_min_factor"], energy_max_factor=a["energy_max_factor"],
        num_energy_bins=NE, dynes_gamma=a["dynes_gamma"], tau_0=a["tau_0"], tau_s=tau_s_eff, tau_r=tau_r_eff, T_c=a["T_c"],
        bath_temperature=a["bath_temperature"])
    nonuniform = precomputed is not None and not bool(precomputed.get("is_uniform", True))
    S.normalize_collision_solver_name(a["collision_solver"])
    en_r, en_s = a["enable_recombination"], a["enable_scattering"]
    diffuser = (S._energy_diffuser(eng, sched, a["diffusion_scheme"], a["cn_rtol"], E_bins, gap, precomputed,
                                   [k["diffusion_coefficient"] for k in kws]) if a["enable_diffusion"] else None)

    omega_bins, idx_diff, idx_sum, diff_sign = S._build_phonon_frequency_map(E_bins)
    nw = omega_bins.size
    ctab, rho_tab = S._collision_tables(eng, E_bins, gap, precomputed if nonuniform else None, n, a["dynes_gamma"],
                                        tau_r_eff, tau_s_eff, a["T_c"], en_r, en_s, idx_diff, idx_sum, diff_sign, members=M,
                                        member_params=tparams, member_ids=ids, pad_bins=a["collision_padded_bins"],
                                        wide_bins=a["collision_wide_bins"])
    phonon_host = np.stack([S._initial_phonon_state(mask, omega_bins, k["bath_temperature"], k["initial_condition_spec"])
                            for k in kws], axis=1).reshape(nw * M, n)
    state_host = np.stack([_prefixed(ids[m], S._initial_qp_state, mask, inits[m], E_bins, dE, gap, k["dynes_gamma"],
                                     k["energy_weights"], k["initial_condition_spec"]) for m, k in enumerate(kws)],
                          axis=1).reshape(NE * M, n)
    state = eng.upload_packed(state_host)                        # [NE * M, ncell] = [NE][M * ncell]
    histories = [k["phonon_history_out"] for k in kws]
    run = _MembersRun(eng, out, state, eng.empty(NE * M, ncm), eng.upload_packed(phonon_host), dE,
                      S._phonon_widths(eng, omega_bins, dE, histories))
    run.ctab, run.floor, run.physics = ctab, a["pauli_density_floor"], (en_r, en_s, not a["freeze_phonon_dynamics"])
    run.flags, run.generations = flags, [
        S._Generation(k["external_generation"], mask, E_bins, on_device=a["generation_on_device"]) for k in kws]
    run.ids, run.errors, run.samplers = ids, errors, samplers
    S._bind_rates(samplers, run)
    if diffuser is not None:
        S._bind_flux(samplers, diffuser)
    run.verdict = S._guard_rule(eng, mask, E_bins, a["enforce_pauli"], a["pauli_warn_threshold"], a["pauli_error_threshold"])
    run.quiet_below = min([v for v in (a["pauli_warn_threshold"], a["pauli_error_threshold"]) if v is not None],
                          default=float("inf"))

    collisions = bool(en_r or en_s)
    energy_loop(run, sched, diffuser, collisions=collisions,
                pair_ok=bool(collisions and a["enable_diffusion"] and Engine.pair_members_supported(ctab, ncm, M)),
                batch_diffusion=S._one_call_diffusion(diffuser, collisions, any(g.active for g in run.generations),
                                                      a["pauli_warn_threshold"], a["pauli_error_threshold"], rho_tab),
                guard_lag=eng.GUARD_LAG)

    results = []
    for m, history in enumerate(histories):
        if run.failed[m] is not None:
            results.append(run.failed[m])
            continue
        if history is not None:
            history.clear()
            history.update(S._dynamic_phonon_history(out, m, omega_bins))
        results.append((list(out.times), out.frames[m], out.mass[m], S._color_limits(out.frames[m]), out.energy_frames[m],
                        E_bins.copy()))
    return results
