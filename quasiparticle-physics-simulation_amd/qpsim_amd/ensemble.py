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
other shapes and larger NE run the one-wave-per-pixel kernel through a member class map and two calls instead of the pair
pass.  A sweep whose members all end up with the same tables runs exactly as the call without ``sweep``.

Rounding: members are bit-equal to their lone ``run_2d_crank_nicolson`` call with ``diffusion_scheme="adi"`` when both use
the same ADI tile family (``QPSIM_FINE_TILES``) and the same step form (``QPSIM_ADI_FUSED``: a batch of at least 4 Mi
cells takes the one-pass steps, which round the interface rows differently, while a smaller lone member does not), within
2e-13 relative otherwise, and within 1e-12 relative with ``cn_exact`` (the iteration's stop test is global over the batch).
"""
from __future__ import annotations

import inspect
import warnings

import numpy as np

from . import _hip
from . import solver as S
from . import tables as _tb
from .distributed import shard_members
from .engine import Engine, _ptr

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


def _bytes_per_member(kw: dict) -> float:
    """Device bytes one member needs: state planes (x2), phonon planes, diffusion / exact-CN work planes."""
    mask = np.asarray(kw["mask"], dtype=bool)
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    ncell = (rows[-1] - rows[0] + 1) * (cols[-1] - cols[0] + 1) if rows.size else 1
    ne = int(kw["num_energy_bins"]) if kw["energy_gap"] > 0.0 else 1
    nw = 3 * ne
    return 8.0 * ncell * (8 * ne + 3 * nw + 8)


def run_2d_crank_nicolson_ensemble(members: list[dict], *, sweep: dict | None = None, errors: str = "raise",
                                   max_members_per_batch: int | None = None, process_group=None, **common) -> list:
    """Run ``len(members)`` independent problems batched on the device.

    ``common`` takes the keyword arguments of ``run_2d_crank_nicolson``; ``members[m]`` overrides only the keys of
    ``PER_MEMBER_KEYS``.  ``sweep`` maps keys of ``SWEEP_KEYS`` (tau_0, tau_s, tau_r, T_c, dynes_gamma) to one value per
    member: member m runs as its lone call with ``sweep[key][m]`` in place of the common value (``tau_s`` / ``tau_r``
    default from that member's ``tau_0``; its ``dynes_gamma`` also shapes its initial state and its Pauli guard).  A swept
    key must not be set to another value in ``common``, and a sweep cannot be combined with ``precomputed`` or
    ``gap_expression``.  The register collision kernels serve per-member tables for ``num_energy_bins`` 4 ... 16 when the
    member's device grid holds a multiple of 64 cells; larger NE and other grids run the one-wave-per-pixel kernel.
    Entry m is the 6-tuple member m's lone call returns (its ``phonon_history_out`` filled the same
    way), or - with ``errors="return"`` - the ``ValueError`` its Pauli guard raised (the other members finish).  With
    ``errors="raise"`` the first violation (earliest step, then lowest member) raises ``ValueError("member m: ...")``.
    Members run in consecutive batches when they do not all fit on the device (``max_members_per_batch`` caps a batch).
    With an initialised ``process_group`` of world size > 1, rank r runs ``shard_members(M, world, r)`` on its current
    device and every rank returns the full list."""
    if errors not in ("raise", "return"):
        raise ValueError("errors must be 'raise' or 'return'")
    kws = member_arguments(list(members), common, sweep)
    _STATS.clear()
    _STATS.update(batches=0, pair_passes=0, guarded_calls=0)
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
    batches = plan_batches(mine, _bytes_per_member(kws[0]), free, max_members_per_batch)
    # one batch on one process raises at once; otherwise every batch finishes and the earliest violation is raised after
    eager = errors == "raise" and world == 1 and len(batches) == 1
    results: dict[int, object] = {}
    for batch in batches:
        res = _run_batch([kws[m] for m in batch], batch, "raise" if eager else "return", None if world == 1 else dev)
        results.update(zip(batch, res))
    out = [results.get(m) for m in range(len(kws))]
    if world > 1:
        import torch.distributed as dist
        local = [(m, results[m], kws[m]["phonon_history_out"]) for m in mine]
        gathered = [None] * world
        dist.all_gather_object(gathered, local, group=process_group)
        for part in gathered:
            for m, res, ph in part:
                out[m] = res
                target = kws[m]["phonon_history_out"]
                if target is not None and ph is not None and target is not ph:
                    target.clear()
                    target.update(ph)
    if errors == "raise":
        failures = [(getattr(r, "step", 0), m, r) for m, r in enumerate(out) if isinstance(r, Exception)]
        if failures:
            raise min(failures, key=lambda f: f[:2])[2]
    return out


def _run_batch(kws: list[dict], ids: list[int], errors: str, device=None) -> list:
    import torch
    dev = kws[0]["device"] if device is None else device
    dev = torch.device("cuda", torch.cuda.current_device()) if dev is None else torch.device(dev)
    with torch.cuda.device(dev):
        _STATS["batches"] += 1
        return _run_batch_on_device(kws, ids, errors, dev)


def _prefixed(m: int, fn, *args):
    try:
        return fn(*args)
    except (ValueError, TypeError) as exc:
        raise type(exc)(f"member {m}: {exc}") from exc


def _run_batch_on_device(kws, ids, errors, device):
    a = kws[0]
    M = len(kws)
    checked = [_prefixed(ids[j], S._checked_run_arguments, k["mask"], k["initial_field"], k["diffusion_coefficient"],
                         k["dt"], k["total_time"], k["store_every"], k["enable_diffusion"], k["enable_recombination"],
                         k["enable_scattering"], k["tau_0"], k["tau_s"], k["tau_r"], k["external_generation"],
                         k["phonon_history_out"]) for j, k in enumerate(kws)]
    mask, _, store_every, n, tau_s_eff, tau_r_eff = checked[0]
    inits = [c[1] for c in checked]
    geom = S._run_geometry(mask, a["edges"], a["edge_conditions"], a["dx"], a["enable_diffusion"])
    full_steps, rem, total_steps = S._step_plan(a["total_time"], a["dt"])
    eng = Engine(geom, device=device)
    eng.pin_stream()
    ncm = eng.ncell
    flags = eng.d_flags.reshape(-1).repeat(M)            # [member][cell]
    stored = lambda step: step % store_every == 0 or step == total_steps  # noqa: E731
    if not a["energy_gap"] > 0.0:
        return _run_scalar_batch(eng, kws, inits, mask, rem, full_steps, total_steps, stored)
    return _run_energy_batch(eng, kws, ids, errors, inits, mask, n, flags, [(c[4], c[5]) for c in checked], rem, full_steps,
                             total_steps, stored)


def _frames_async(eng, planes, mask):
    return S._device_frames_async(eng, planes, mask)


def _run_scalar_batch(eng, kws, inits, mask, rem, full_steps, total_steps, stored):
    """Scalar mode (energy_gap == 0) for M members: one [M, ncell] field set (solver._run_scalar per member)."""
    a, M = kws[0], len(kws)
    dx = a["dx"]
    u_host = np.stack([f[mask].astype(float) for f in inits])
    u = eng.upload_packed(u_host)
    diffuser = (S._Diffuser(eng, M, a["dt"], rem, a["diffusion_scheme"], a["cn_rtol"],
                            dcoef=[float(k["diffusion_coefficient"]) for k in kws]) if a["enable_diffusion"] else None)
    times = [0.0]
    frames = [[S.reconstruct_field(mask, u_host[m])] for m in range(M)]
    mass = [[float(np.sum(u_host[m]) * dx * dx)] for m in range(M)]
    for m, k in enumerate(kws):
        S._notify(k["progress_callback"], 0.0, frames[m][0])
    lazy = S._LazyOutputs()
    want_now = any(k["progress_callback"] is not None for k in kws)
    t = 0.0
    done = 0
    for step in range(1, total_steps + 1):
        t += rem if step > full_steps else a["dt"]
        if stored(step):
            if diffuser is not None:
                diffuser.advance(u, done + 1, step, full_steps)
            done = step
            times.append(float(t))
            kk = len(frames[0])
            for m in range(M):
                frames[m].append(None)
                mass[m].append(None)

            def put(arr, kk=kk):
                for m in range(M):
                    frames[m][kk] = arr[m]
                    mass[m][kk] = float(np.sum(arr[m][mask]) * dx * dx)

            ticket = _frames_async(eng, u, mask)
            if want_now:
                put(ticket.result())
                for m, k in enumerate(kws):
                    S._notify(k["progress_callback"], t, frames[m][kk])
            else:
                lazy.add(ticket, put)
    lazy.flush()
    out = []
    for m, k in enumerate(kws):
        ph = k["phonon_history_out"]
        if ph is not None:
            f, ef, bins, meta = S.build_fixed_phonon_history(mask=mask, times=times, bath_temperature=k["bath_temperature"],
                                                             phonon_energy_bins=None)
            ph.update({"phonon_frames": f, "phonon_energy_frames": ef, "phonon_energy_bins": bins, "phonon_metadata": meta})
        out.append((list(times), frames[m], mass[m], S._color_limits(frames[m]), None, None))
    return out


def table_parameters(kws: list[dict], taus: list[tuple]) -> list[tuple]:
    """Per member what its collision tables depend on beyond the shared energy grid: (dynes_gamma, tau_r, tau_s, T_c), with
    the entries of a disabled process blanked (they reach no table).  ``taus``: (tau_s, tau_r) as resolved per member."""
    out = []
    for k, (tau_s, tau_r) in zip(kws, taus):
        en_r, en_s = bool(k["enable_recombination"]), bool(k["enable_scattering"])
        out.append((k["dynes_gamma"], tau_r if en_r else None, tau_s if en_s else None,
                    k["T_c"] if (en_r or en_s) else None))
    return out


def _run_energy_batch(eng, kws, ids, errors, inits, mask, n, flags, taus, rem, full_steps, total_steps, stored):
    """Energy-resolved mode for M members: the time loop of ``run_2d_crank_nicolson`` over [bin][member][cell] planes."""
    a, M = kws[0], len(kws)
    tau_s_eff, tau_r_eff = taus[0]
    tparams = table_parameters(kws, taus)
    if all(p == tparams[0] for p in tparams):                    # one table set serves every member (no sweep, or all equal)
        tparams = None
    lib, ncm = eng.lib, eng.ncell
    dt, dx = a["dt"], a["dx"]
    gap, NE = a["energy_gap"], a["num_energy_bins"]
    E_bins, dE = S.build_energy_grid(gap, a["energy_min_factor"], a["energy_max_factor"], NE)
    precomputed = a["precomputed"]
    if precomputed is None and a["gap_expression"].strip():      # one value of D and T_b (member_arguments checked)
        from .models import SimulationParameters
        from .precompute import precompute_arrays
        params = SimulationParameters(
            diffusion_coefficient=a["diffusion_coefficient"], dt=dt, total_time=a["total_time"], mesh_size=dx,
            energy_gap=gap, energy_min_factor=a["energy_min_factor"], energy_max_factor=a["energy_max_factor"],
            num_energy_bins=NE, dynes_gamma=a["dynes_gamma"], gap_expression=a["gap_expression"], tau_0=a["tau_0"],
            tau_s=tau_s_eff, tau_r=tau_r_eff, T_c=a["T_c"], bath_temperature=a["bath_temperature"])
        precomputed = precompute_arrays(mask, a["edges"], a["edge_conditions"], params, include_collision_kernels=False)
    has_pre = precomputed is not None
    nonuniform = has_pre and not bool(precomputed.get("is_uniform", True))
    S.normalize_collision_solver_name(a["collision_solver"])
    en_r, en_s = a["enable_recombination"], a["enable_scattering"]
    upd = not a["freeze_phonon_dynamics"]
    floor = a["pauli_density_floor"]

    diffuser = None
    if a["enable_diffusion"]:
        scheme, rtol = a["diffusion_scheme"], a["cn_rtol"]
        if has_pre:
            D_array = np.asarray(precomputed["D_array"], dtype=float)
        if nonuniform:                                           # field i * M + m is bin i of member m
            dfield = np.zeros((NE, ncm))
            dfield[:, eng.mask_flat] = D_array
            diffuser = S._Diffuser(eng, NE * M, dt, rem, scheme, rtol, dfield=np.repeat(dfield, M, axis=0))
        else:
            per_member = []
            for k in kws:
                if has_pre:
                    per_member.append([float(D_array[i, 0]) if D_array.ndim == 2 else float(D_array[i]) for i in range(NE)])
                else:
                    per_member.append([float(v) for v in _tb.diffusion_coefficients(E_bins, gap, k["diffusion_coefficient"])])
            diffuser = S._Diffuser(eng, NE * M, dt, rem, scheme, rtol,
                                   dcoef=[per_member[m][i] for i in range(NE) for m in range(M)])

    omega_bins, idx_diff, idx_sum, diff_sign = S._build_phonon_frequency_map(E_bins)
    nw = omega_bins.size
    ctab, rho_tab = S._collision_tables(eng, E_bins, gap, precomputed if nonuniform else None, n, a["dynes_gamma"],
                                        tau_r_eff, tau_s_eff, a["T_c"], en_r, en_s, idx_diff, idx_sum, diff_sign, members=M,
                                        member_params=tparams, member_ids=ids)
    phonon_host = np.stack([S._initial_phonon_state(mask, omega_bins, k["bath_temperature"], k["initial_condition_spec"])
                            for k in kws], axis=1).reshape(nw * M, n)
    state_host = np.stack([_prefixed(ids[m], S._initial_qp_state, mask, inits[m], E_bins, dE, gap, k["dynes_gamma"],
                                     k["energy_weights"], k["initial_condition_spec"]) for m, k in enumerate(kws)],
                          axis=1).reshape(NE * M, n)
    state = eng.upload_packed(state_host)                        # [NE * M, ncell] = [NE][M * ncell]
    state_alt = eng.empty(NE * M, ncm)
    phonon = eng.upload_packed(phonon_host)
    coords = np.argwhere(mask)
    cell_to_px = np.cumsum(eng.mask_flat) - 1
    warned = [False] * M
    failed: list = [None] * M
    pending_guard: list = []

    # a member whose step shows no forbidden density and no occupation above the lower threshold has nothing to report
    quiet_below = min([v for v in (a["pauli_warn_threshold"], a["pauli_error_threshold"]) if v is not None],
                      default=float("inf"))

    def check(step_idx, time_ns, stats) -> None:
        for m in range(M):
            if failed[m] is not None or (stats[m][2] is None and not stats[m][0] > quiet_below):
                continue
            error, warning, warned[m] = S._pauli_verdict(stats[m], step_idx, time_ns, E_bins, coords, cell_to_px, warned[m],
                                                         a["enforce_pauli"], a["pauli_warn_threshold"],
                                                         a["pauli_error_threshold"])
            if error is not None:
                failed[m] = ValueError(f"member {ids[m]}: {error}")
                failed[m].step = step_idx
                if errors == "raise":
                    raise failed[m]
            elif warning is not None:
                warnings.warn(f"member {ids[m]}: {warning}", stacklevel=4)

    def guard_launch(step_idx, time_ns) -> None:
        pending_guard.append((eng.pauli_stats_members_launch(state, ctab, floor, ncm, M, flags), step_idx, time_ns))

    def guard_flush(keep: int = 0) -> None:
        while len(pending_guard) > keep:
            ticket, step_idx, time_ns = pending_guard.pop(0)
            check(step_idx, time_ns, eng.pauli_stats_members_result(ticket))

    check(0, 0.0, eng.pauli_stats_members_result(eng.pauli_stats_members_launch(state, ctab, floor, ncm, M, flags)))

    want_ph = [k["phonon_history_out"] is not None for k in kws]
    ph_frames = [[] for _ in range(M)]
    ph_eframes = [[] for _ in range(M)]
    ph_w = (eng.torch.as_tensor(S.integration_widths_from_centers(omega_bins, fallback_width=dE), device=eng.device)
            if any(want_ph) else None)
    callbacks = [k["progress_callback"] for k in kws]
    lazy = S._LazyOutputs()

    def per_member_planes(arr, nplanes):
        arr = arr.reshape((nplanes, M) + arr.shape[1:])
        return [list(np.ascontiguousarray(arr[:, m])) for m in range(M)]

    def snapshot_phonons() -> None:
        kk = len(ph_frames[0])
        for m in range(M):
            ph_eframes[m].append(None)
            ph_frames[m].append(None)

        def put_e(arr, kk=kk):
            for m, planes in enumerate(per_member_planes(arr, nw)):
                ph_eframes[m][kk] = planes

        def put_sum(arr, kk=kk):
            for m in range(M):
                ph_frames[m][kk] = arr[m]

        lazy.add(_frames_async(eng, phonon, mask), put_e)
        summed = eng.empty(M * ncm)
        _hip.check(lib.qp_weighted_sum(_ptr(phonon), _ptr(ph_w), nw, M * ncm, _ptr(summed), eng.stream),
                     "qp_weighted_sum")
        lazy.add(_frames_async(eng, summed, mask), put_sum)

    times: list[float] = [0.0]
    frames = [[] for _ in range(M)]
    energy_frames = [[] for _ in range(M)]
    mass = [[] for _ in range(M)]

    def store(t_now: float) -> None:
        kk = len(frames[0])
        for m in range(M):
            frames[m].append(None)
            energy_frames[m].append(None)
            mass[m].append(None)
        integ = eng.empty(M * ncm)
        _hip.check(lib.qp_energy_integrate(_ptr(state), NE, M * ncm, float(dE), _ptr(integ), eng.stream),
                     "qp_energy_integrate")
        t_int = _frames_async(eng, integ, mask)

        def put_integrated(arr, kk=kk):
            for m in range(M):
                frames[m][kk] = arr[m]
                mass[m][kk] = float(np.sum(arr[m][mask]) * dx * dx)

        def put_energy(arr, kk=kk):
            for m, planes in enumerate(per_member_planes(arr, NE)):
                energy_frames[m][kk] = planes

        lazy.add(_frames_async(eng, state, mask), put_energy)
        if any(want_ph):
            snapshot_phonons()
        if any(cb is not None for cb in callbacks):
            put_integrated(t_int.result())
            for m, cb in enumerate(callbacks):
                S._notify(cb, t_now, frames[m][kk])
        else:
            lazy.add(t_int, put_integrated)

    store(0.0)

    collisions = bool(en_r or en_s)
    specs = [k["external_generation"] for k in kws]
    gen_active = [spec is not None and spec.mode != "none" for spec in specs]
    constant_mode = [g and spec.mode.strip().lower() == "constant" for g, spec in zip(gen_active, specs)]
    compiled: list = [None] * M

    def collide(dt_col, guard_step=None) -> bool:
        nonlocal state, state_alt
        if dt_col <= 0.0 or not collisions:
            return False
        if guard_step is None:
            eng.collide(ctab, state, state_alt, phonon, dE, dt_col, en_r, en_s, upd, ncell=M * ncm, flags=flags)
        else:
            ticket = eng.collide_guarded_members(ctab, state, state_alt, phonon, dE, dt_col, en_r, en_s, upd, floor, ncm, M,
                                                 flags)
            pending_guard.append((ticket, guard_step[0], guard_step[1]))
            _STATS["guarded_calls"] += 1
        state, state_alt = state_alt, state
        return guard_step is not None

    def generate(t_start, dt_step) -> None:
        amounts = generation_amounts(specs, t_start, dt_step)
        if any(x is None for x in amounts):                      # custom expressions: evaluated on the host
            g = np.zeros((NE, M, n))
            for m, x in enumerate(amounts):
                if x is None:
                    if compiled[m] is None:
                        compiled[m] = S._CustomGeneration(specs[m], mask)
                    g_ext = S.evaluate_external_generation(specs[m], E_bins, n, t_start, mask, _compiled=compiled[m])
                    if g_ext is not None:
                        g[:, m] = g_ext
            eng.add_scaled(state, eng.upload_packed(g.reshape(NE * M, n)), dt_step)
        consts = [0.0 if x is None else x for x in amounts]
        if any(constant_mode) or any(x != 0.0 for x in consts):
            eng.add_constant_members(state, consts, ncm, M, flags)

    batch_diffusion = (a["enable_diffusion"] and not collisions and not any(gen_active) and a["diffusion_scheme"] == "adi"
                       and a["pauli_error_threshold"] is None and a["pauli_warn_threshold"] is None
                       and float(np.min(rho_tab)) > 1e-30)
    pair_ok = bool(collisions and a["enable_diffusion"] and Engine.pair_members_supported(ctab, ncm, M))
    current_time = 0.0
    done = 0
    opened = False
    for step in range(1, total_steps + 1):                       # the lone loop, solver.run_2d_crank_nicolson
        final = step > full_steps
        dt_step = rem if final else dt
        if batch_diffusion:
            current_time += dt_step
            if stored(step):
                diffuser.advance(state, done + 1, step, full_steps)
                done = step
                times.append(float(current_time))
                store(current_time)
            continue
        if any(gen_active) and not opened:
            generate(current_time, dt_step)
        guarded = False
        if collisions and a["enable_diffusion"]:                 # Strang: C(dt/2) D(dt) C(dt/2)
            if not opened:
                collide(0.5 * dt_step)
            opened = False
            diffuser.step(state, final)
            nxt = None
            if pair_ok and step < total_steps and not stored(step) and dt_step > 0.0:
                dt_next = rem if step + 1 > full_steps else dt
                nxt = generation_amounts(specs, current_time + dt_step, dt_next)
                # one scalar generation amount inside the pair kernel: only when every member adds the same
                nxt = nxt[0] if all(x is not None and x == nxt[0] for x in nxt) else None
            if nxt is not None:
                ticket = eng.collide_pair_guarded_members(ctab, state, state_alt, phonon, dE, 0.5 * dt_step, 0.5 * dt_next,
                                                          nxt, en_r, en_s, upd, floor, ncm, M, flags)
                pending_guard.append((ticket, step, current_time + dt_step))
                _STATS["pair_passes"] += 1
                state, state_alt = state_alt, state
                guarded = opened = True
            else:
                guarded = collide(0.5 * dt_step, guard_step=(step, current_time + dt_step))
        else:
            diffuse_after = a["enable_diffusion"] and dt_step > 0.0
            guarded = collide(dt_step, guard_step=None if diffuse_after else (step, current_time + dt_step))
            if diffuse_after:
                diffuser.step(state, final)
        if not guarded:
            guard_launch(step, current_time + dt_step)
        guard_flush(keep=0 if stored(step) else eng.GUARD_LAG)
        current_time += dt_step
        if stored(step):
            times.append(float(current_time))
            store(current_time)
    guard_flush()
    lazy.flush()

    out = []
    for m, k in enumerate(kws):
        if failed[m] is not None:
            out.append(failed[m])
            continue
        ph = k["phonon_history_out"]
        if ph is not None:
            ph.clear()
            ph.update({
                "phonon_frames": ph_frames[m],
                "phonon_energy_frames": ph_eframes[m],
                "phonon_energy_bins": np.asarray(omega_bins, dtype=float).copy(),
                "phonon_metadata": {"mode": "dynamic_local_coupled", "field_units": "integrated_occupation",
                                    "energy_frame_units": "occupation"},
            })
        out.append((list(times), frames[m], mass[m], S._color_limits(frames[m]), energy_frames[m], E_bins.copy()))
    return out
