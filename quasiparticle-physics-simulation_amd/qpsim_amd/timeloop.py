"""The time loop of a run, written once for lone runs and ensembles (host only: no device library is imported here).

``energy_loop`` sequences an energy-resolved run - generation, the Strang order C(dt/2) D(dt) C(dt/2) with the fused closing
and opening half-step, the Pauli guard read ``guard_lag`` steps late, the short last step, the store points - and
``scalar_loop`` the legacy scalar mode.  What is issued to the device at each point is the business of a run object:
``solver._LoneRun`` (one problem, the plain library calls) and ``ensemble._MembersRun`` (M problems laid out
[bin][member][cell], the ``*_members`` calls) both derive from ``EnergyRun``, which holds what they share: the device planes,
the ``state`` / ``state_alt`` swap and the store point.  ``Outputs`` keeps the host-side results of M members; a lone run is
M = 1.

Samplers (opt-in; time traces and coarse frames are the two kinds): a ``Sampler`` has a cadence ``every`` and a device
buffer with one row per sample - t = 0, every ``every``-th step and the last (``Schedule.due`` / ``Schedule.rows``) - and at
each of its steps enqueues one reduction of the state into the next row: the region sums of every plane for a trace, the
b x b block sums of every plane for the coarse frames.  The buffer is fetched once, after the loop.  Both loops take a
tuple of samplers.  A step that is due for any of them is sequenced exactly like a stored one (no pair pass across it, the
stretch of diffusion steps ends there, the guard is read), so the state it sees is the state a run with ``store_every`` =
that cadence stores there; it downloads no frame.  Each sampler is called at the steps of its own cadence only, those due
at one step in the order of the tuple.  With an empty tuple no step is sampled and both loops issue exactly the calls they
issued before.
"""
from __future__ import annotations

import numpy as np


def _step_plan(total_time: float, dt: float) -> tuple[int, float, int]:
    """(full steps, remainder dt or 0, total steps) (solver.py:1085-1089)."""
    full = int(np.floor(total_time / dt + 1e-12))
    rem = float(total_time - full * dt)
    if rem < 1e-12:
        rem = 0.0
    return full, rem, full + (1 if rem > 0.0 else 0)


class Schedule:
    """Step sizes and store points of a run: ``full_steps`` steps of ``dt``, then one of ``rem`` if that is positive.
    ``due`` / ``rows`` serve any cadence ``every`` (None: none) of sampled steps: every ``every``-th and the last."""

    def __init__(self, total_time: float, dt: float, store_every: int):
        self.dt, self.store_every = dt, store_every
        self.full_steps, self.rem, self.total_steps = _step_plan(total_time, dt)

    def stored(self, step: int) -> bool:
        return step % self.store_every == 0 or step == self.total_steps

    def due(self, every: int | None, step: int) -> bool:
        return every is not None and (step % every == 0 or step == self.total_steps)

    def rows(self, every: int | None) -> int:
        """Samples of a cadence: t = 0 and every step that is due."""
        if every is None:
            return 0
        return 1 + self.total_steps // every + (1 if self.total_steps % every else 0)

    def dt_of(self, step: int) -> float:
        return self.rem if step > self.full_steps else self.dt


def _device_frames_async(eng, planes, mask: np.ndarray):
    """Device planes -> ticket for host [n, ny, nx] frames on the FULL mask, NaN outside the interior (reconstruct_field
    semantics).  Padding and, for a cropped engine grid, the embedding into the full frame are done on the device; the copy
    to the host runs on a side stream into pinned memory while the time loop goes on (``ticket.result()`` waits for it)."""
    if (eng.ny, eng.nx) == mask.shape:
        return eng.download_frames_async(planes)
    r0 = int(np.flatnonzero(mask.any(axis=1))[0])
    c0 = int(np.flatnonzero(mask.any(axis=0))[0])
    return eng.download_frames_async(planes, full_shape=mask.shape, offset=(r0, c0))


class _LazyOutputs:
    """Store points enqueue their downloads and go on; the host arrays are filled in when the copies have landed (when a
    staging slot is recycled, when a progress callback needs the frame, or before the run returns)."""

    def __init__(self):
        self._pending: list = []

    def add(self, ticket, consume) -> None:
        self._pending.append((ticket, consume))

    def flush(self) -> None:
        while self._pending:
            ticket, consume = self._pending.pop(0)
            consume(ticket.result())


def _notify(cb, t: float, frame: np.ndarray) -> None:
    if cb is None:
        return
    try:
        cb(float(t), np.array(frame, copy=True))
    except Exception:
        pass


class Outputs:
    """Host-side results of M members: stored times (shared) and per member the integrated frames, their mass, the
    per-bin frames and the phonon frames.  Downloads arrive as tickets of [planes * M, ny, nx] frames on the full mask."""

    def __init__(self, mask: np.ndarray, dx: float, callbacks: list):
        self.mask, self.dx, self.callbacks, self.members = mask, dx, callbacks, len(callbacks)
        self.notify_now = any(cb is not None for cb in callbacks)
        self.lazy = _LazyOutputs()
        self.times: list[float] = [0.0]
        self.frames, self.mass, self.energy_frames, self.phonon_frames, self.phonon_energy_frames = (
            [[] for _ in callbacks] for _ in range(5))

    def _slot(self, *series) -> int:
        k = len(series[0][0])
        for per_member in series:
            for entries in per_member:
                entries.append(None)
        return k

    def add_host_frames(self, t: float, frames: list, mass: list) -> None:
        """A store point whose frames are already on the host (the initial state of scalar mode)."""
        for m, cb in enumerate(self.callbacks):
            self.frames[m].append(frames[m])
            self.mass[m].append(mass[m])
            _notify(cb, t, frames[m])

    def add_integrated(self, t: float, ticket) -> None:
        """One integrated frame per member: filled in lazily unless a progress callback wants it now."""
        k = self._slot(self.frames, self.mass)

        def put(arr):
            for m in range(self.members):
                self.frames[m][k] = arr[m]
                # same summation order as the reference's packed sum
                self.mass[m][k] = float(np.sum(arr[m][self.mask]) * self.dx * self.dx)

        if not self.notify_now:
            self.lazy.add(ticket, put)
            return
        put(ticket.result())
        for m, cb in enumerate(self.callbacks):
            _notify(cb, t, self.frames[m][k])

    def add_planes(self, series, ticket) -> None:
        """[planes * M] frames laid out [plane][member] -> a list of planes per member."""
        k = self._slot(series)

        def put(arr):
            arr = arr.reshape((-1, self.members) + arr.shape[1:])
            for m in range(self.members):
                series[m][k] = list(np.ascontiguousarray(arr[:, m]))

        self.lazy.add(ticket, put)

    def add_frames(self, series, ticket) -> None:
        k = self._slot(series)
        self.lazy.add(ticket, lambda arr: [series[m].__setitem__(k, arr[m]) for m in range(self.members)])


class Sampler:
    """One cadence of sampled steps over M members: at every sample ``reduce(state, out_row)`` enqueues one device
    reduction of the planes [field][member][cell] into row k of a device buffer [rows, M, *row_shape]; nothing is read back
    before ``fetch()``.  A time trace reduces with ``Engine.region_sums`` into rows (regions, fields), the coarse frames with
    ``Engine.block_sums`` into rows (fields, cny, cnx), the boundary outflow with ``Engine.boundary_flux`` into rows
    (surfaces, fields)."""

    def __init__(self, eng, sched: Schedule, every: int, members: int, row_shape: tuple, reduce):
        self.sched, self.every, self.reduce = sched, every, reduce
        self.buffer = eng.empty(sched.rows(every), members, *row_shape)
        self.times: list[float] = []

    def due(self, step: int) -> bool:
        return self.sched.due(self.every, step)

    def sample(self, t: float, state) -> None:
        self.reduce(state, self.buffer[len(self.times)])
        self.times.append(float(t))

    def fetch(self) -> np.ndarray:
        """[samples taken, M, *row_shape] on the host (the one transfer of a sampler)."""
        return self.buffer[:len(self.times)].cpu().numpy()


def _sample(samplers, t: float, state) -> None:
    for sampler in samplers:
        sampler.sample(t, state)


def scalar_loop(sched: Schedule, diffuser, u, out: Outputs, eng, samplers=()) -> None:
    """Legacy scalar mode, energy_gap == 0 (solver.py:1540-1555): nothing happens between two store points (or steps due
    for one of ``samplers``) but diffusion steps, which ``diffuser.advance`` takes in one go."""
    t = 0.0
    done = 0
    _sample(samplers, 0.0, u)
    for step in range(1, sched.total_steps + 1):
        t += sched.dt_of(step)                        # same accumulation order as the reference
        stored = sched.stored(step)
        due = [s for s in samplers if s.due(step)]
        if stored or due:
            if diffuser is not None:
                diffuser.advance(u, done + 1, step, sched.full_steps)
            done = step
        if stored:
            out.times.append(float(t))
            out.add_integrated(t, _device_frames_async(eng, u, out.mask))
        _sample(due, t, u)
    out.lazy.flush()


class EnergyRun:
    """Device state of an energy-resolved run over planes [bin][member][cell], and the store point.  A subclass issues the
    calls that differ between a lone run and an ensemble:

    ``generate(t, dt)``                                external generation of the step starting at ``t``
    ``pair_amount(t_next, dt_next)``                   the one number the fused pass may add for the next step, or None
    ``collide(dt, guarded)``                           state -> state_alt; the guard ticket if ``guarded``
    ``collide_pair(dt_a, dt_b, amount)``               the fused closing + opening half-step; the guard ticket
    ``guard_launch()``                                 the guard of ``state`` on its own; its ticket
    ``guard_check(ticket, step, t)``                   reads a ticket; warns / raises with the step and time it belongs to

    ``samplers``: the ``Sampler`` s of the run, in the order they are called; empty (the default) without any.
    """
    samplers: tuple = ()

    def __init__(self, eng, out: Outputs, state, state_alt, phonon, dE: float, phonon_widths=None):
        self.eng, self.out = eng, out
        self.state, self.state_alt, self.phonon, self.dE = state, state_alt, phonon, dE
        self.ncell = eng.ncell * out.members
        self.phonon_widths = phonon_widths                       # on the device; None: phonon frames are not wanted

    def download(self, planes):
        return _device_frames_async(self.eng, planes, self.out.mask)

    def swap(self) -> None:
        self.state, self.state_alt = self.state_alt, self.state

    def store(self, t: float) -> None:                           # solver.py:1354-1374, 1480-1489
        # frames are formed on the device (energy integral, NaN padding), cross PCIe once on a side stream while the next
        # steps run, and are handed out as they are; only a progress callback forces the integrated frame now
        eng, out = self.eng, self.out
        integrated = self.download(eng.energy_integral(self.state, self.dE, ncell=self.ncell))
        out.add_planes(out.energy_frames, self.download(self.state))
        if self.phonon_widths is not None:
            out.add_planes(out.phonon_energy_frames, self.download(self.phonon))
            out.add_frames(out.phonon_frames, self.download(eng.weighted_sum(self.phonon, self.phonon_widths,
                                                                              ncell=self.ncell)))
        out.add_integrated(t, integrated)


def energy_loop(run: EnergyRun, sched: Schedule, diffuser, *, collisions: bool, pair_ok: bool, batch_diffusion: bool,
                guard_lag: int) -> None:
    """Energy-resolved mode (solver.py:1454-1494).  ``diffuser`` is None without diffusion.

    The guard of step k is enqueued right after the step and examined after step k + ``guard_lag`` has been enqueued (or
    before anything is stored / returned), so the device does not idle during the host round trip and the host never
    sleeps on an event.  Messages carry the step / time of the step that was checked, exactly as the reference's.
    ``batch_diffusion``: pure diffusion with a guard that cannot fire - the steps between two store points are one call.
    ``pair_ok``: Strang steps that follow one another without a store point in between run the closing half-step of step k
    and the opening half-step of step k + 1 as ONE pass over the state (``run.collide_pair``); ``opened`` says that the
    generation term and the first half-step of the step now starting were already applied by that pass.
    A step that is due for one of ``run.samplers`` ends a stretch exactly as a stored one does (``halt``) and enqueues the
    reductions of those samplers instead of a download."""
    pending: list = []
    samplers = run.samplers

    def guard_flush(keep: int = 0) -> None:
        while len(pending) > keep:
            run.guard_check(*pending.pop(0))

    def collide(dt_col: float, guard_step=None) -> bool:
        """One collision update; with ``guard_step = (step, time)`` the Pauli guard of that step is reduced by the same
        call (the collision is then the last operation of the step).  Returns True when the guard was enqueued."""
        if dt_col <= 0.0 or not collisions:
            return False
        ticket = run.collide(dt_col, guard_step is not None)
        run.swap()
        if guard_step is not None:
            pending.append((ticket,) + guard_step)
        return guard_step is not None

    pending.append((run.guard_launch(), 0, 0.0))
    guard_flush()
    run.store(0.0)
    _sample(samplers, 0.0, run.state)
    times = run.out.times
    t = 0.0
    done = 0
    opened = False
    for step in range(1, sched.total_steps + 1):
        final = step > sched.full_steps
        dt_step = sched.dt_of(step)
        stored = sched.stored(step)
        due = [s for s in samplers if s.due(step)]
        halt = stored or bool(due)
        if batch_diffusion:
            t += dt_step
            if halt:
                diffuser.advance(run.state, done + 1, step, sched.full_steps)
                done = step
            if stored:
                times.append(float(t))
                run.store(t)
            _sample(due, t, run.state)
            continue
        if not opened:
            run.generate(t, dt_step)
        if collisions and diffuser is not None:                  # Strang: C(dt/2) D(dt) C(dt/2)
            if not opened:
                collide(0.5 * dt_step)
            opened = False
            diffuser.step(run.state, final)
            amount = None
            if pair_ok and step < sched.total_steps and not halt and dt_step > 0.0:
                dt_next = sched.dt_of(step + 1)
                amount = run.pair_amount(t + dt_step, dt_next)
            if amount is not None:
                pending.append((run.collide_pair(0.5 * dt_step, 0.5 * dt_next, amount), step, t + dt_step))
                run.swap()
                guarded = opened = True
            else:
                guarded = collide(0.5 * dt_step, guard_step=(step, t + dt_step))
        else:
            diffuse_after = diffuser is not None and dt_step > 0.0
            guarded = collide(dt_step, guard_step=None if diffuse_after else (step, t + dt_step))
            if diffuse_after:
                diffuser.step(run.state, final)
        if not guarded:
            pending.append((run.guard_launch(), step, t + dt_step))
        guard_flush(keep=0 if halt else guard_lag)
        t += dt_step
        if stored:
            times.append(float(t))
            run.store(t)
        _sample(due, t, run.state)
    guard_flush()
    run.out.lazy.flush()
