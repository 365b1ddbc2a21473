"""Custom generation evaluated on the device: ``qp_add_generation_expr`` against the host hook and the host path, and
``generation_on_device=True`` against ``False`` through the public API (lone runs, ensembles, fallback, errors)."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

import generation_expr_cases as G
from test_device_expr_host import HAVE_X87, function_truth, power_truth, product_bound_and_error

pytestmark = pytest.mark.gpu
SENTINEL = 7.25


def _engine(dev_mask):
    from qpsim_amd.engine import CompiledGeometry, Engine, link_flags
    z = np.zeros(dev_mask.shape)
    return Engine(CompiledGeometry(dev_mask, 1.0, link_flags(dev_mask), z, z, z, z))


def _planes(eng, packed, members=1, fill=0.0):
    """[NE * members, ncell] device planes from packed [NE * members, n] values, holes = ``fill``."""
    full = np.full((packed.shape[0], eng.ncell), fill)
    full[:, eng.mask_flat] = packed
    return eng.torch.as_tensor(full, device=eng.device)


def device_values(body, params, mask, E, t, dt=1.0):
    """[NE, n] the kernel adds to a zero state with ``dt`` (1: the values themselves), the holes checked for the sentinel."""
    _, words, table = G.compiled(body, params, E, t)
    dev_mask, win = G.window(mask)
    eng = _engine(dev_mask)
    state = _planes(eng, np.zeros((len(E), int(mask.sum()))), fill=SENTINEL)
    status = eng.generation_status(eng.add_generation_expr(state, win, [(words, table, None)], dt, 1, eng.d_flags))
    out = state.cpu().numpy()
    assert np.all(out[:, ~eng.mask_flat] == SENTINEL)
    return out[:, eng.mask_flat], status[0]


@pytest.mark.parametrize("ne", [3, 12])
@pytest.mark.parametrize("grid", sorted(G.GRIDS))
def test_exact_class_kernel_is_bit_equal_to_the_host_hook(grid, ne):
    mask, E = G.GRIDS[grid], G.E_BINS[ne]
    for body, params in G.EXACT:
        for t in G.T_VALUES:
            got, _ = device_values(body, params, mask, E, t)
            hook = G.host_hook(body, params, mask, E, t)
            # 0 + 1 * g keeps every bit of g but the sign of a zero
            assert G.bits_equal(got + 0.0, hook + 0.0), (body, t)
            assert G.bits_equal(hook + 0.0, G.numpy_reference(body, params, mask, E, t) + 0.0), (body, t)


@pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")
@pytest.mark.parametrize("grid,ne", [("full_17x31", 3), ("framed_9x11", 12), ("full_6x10", 3)])
def test_approximate_class_kernel(grid, ne):
    mask, E = G.GRIDS[grid], G.E_BINS[ne]
    cases = [(f"{name}({arg})", function_truth(name, arg)) for name, arg, _ in G.APPROXIMATE]
    cases += [(body, power_truth(base, exponent)) for body, base, exponent in G.POWERS]
    misses = []
    for body, truth_of in cases:
        truth = truth_of(mask, E)
        k_dev = G.ulp_error(device_values(body, {}, mask, E, 0.0)[0], truth)
        k_np = G.ulp_error(G.numpy_reference(body, {}, mask, E, 0.0), truth)
        print(f"{body}: K_dev {k_dev:.3f} ulp, K_np {k_np:.3f} ulp")
        if not k_dev <= G.limit(k_np):
            misses.append((body, k_dev, k_np))
    assert not misses


@pytest.mark.skipif(not HAVE_X87, reason="np.longdouble is not the 80-bit extended format on this host")
def test_product_of_approximate_factors_kernel():
    error, bound = product_bound_and_error(lambda body, params, mask, E, t: device_values(body, params, mask, E, t)[0])
    print(f"product of {len(G.PRODUCT)} factors: {error:.3f} eps, bound {bound:.3f} eps")
    assert error <= bound


@pytest.mark.parametrize("shape", [(6, 10), (5, 13), (17, 31)])          # 60, 65, 527 cells per member
def test_update_form_is_the_host_paths(shape):
    """On a random non-zero state the kernel equals upload_packed + qp_add_scaled of the host path's g, bit for bit; three
    members of which the middle one is not listed (and must stay as it is)."""
    body, params, t, dt, ne, M = "1e-6*E/(1.0+x)+np.sqrt(x*y)*t", {}, 0.3, 0.137, 3, 3
    mask, E = np.ones(shape, dtype=bool), G.E_BINS[3]
    n = int(mask.sum())
    assert n in (60, 65, 527)
    _, words, table = G.compiled(body, params, E, t)
    eng = _engine(mask)
    start = np.random.default_rng(5).uniform(0.5, 2.0, (ne, M, n)) * 1e-4
    g = np.zeros((ne, M, n))
    g[:, 0] = g[:, 2] = G.numpy_reference(body, params, mask, E, t)
    flags = eng.d_flags.reshape(-1).repeat(M)
    on_device = eng.upload_packed(start.reshape(ne * M, n))
    status = eng.generation_status(eng.add_generation_expr(on_device, mask.shape + (0, 0), [(words, table, [0, 2])], dt, M,
                                                           flags))
    on_host = eng.upload_packed(start.reshape(ne * M, n))
    eng.add_scaled(on_host, eng.upload_packed(g.reshape(ne * M, n)), dt)
    got, ref = on_device.cpu().numpy().reshape(ne, M, n), on_host.cpu().numpy().reshape(ne, M, n)
    assert status == [(False, False)]
    assert np.array_equal(got[:, 1], start[:, 1]) and not np.array_equal(got[:, 0], start[:, 0])
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))


def test_status_bits():
    """One negative value, and one inf, in the last partial wave of a 527-cell plane: each sets exactly its word."""
    mask, E = G.GRIDS["full_17x31"], G.E_BINS[3]
    last = "(x>0.97)*(y>0.95)"                                   # true at row 16, col 30 only
    assert int(np.sum(G.numpy_reference(last + "*1.0", {}, mask, E, 0.0)[0])) == 1
    with np.errstate(all="ignore"):
        assert device_values(f"np.where({last}, 1.0, 2.0)", {}, mask, E, 0.0)[1] == (False, False)
        assert device_values(f"np.where({last}, -1.0, 2.0)", {}, mask, E, 0.0)[1] == (False, True)
        assert device_values(f"np.where({last}, 1.0/(x-x), 2.0)", {}, mask, E, 0.0)[1] == (True, False)
        assert device_values(f"np.where({last}, -1.0/(x-x), 2.0)", {}, mask, E, 0.0)[1] == (True, True)
        assert device_values(f"np.where({last}, np.sqrt(-x), 2.0)", {}, mask, E, 0.0)[1] == (True, False)


# ---------------------------------------------------------------------------------------------------------------- API
def _problem(mask, **over):
    from qpsim_amd.geometry import extract_edge_segments
    from qpsim_amd.models import BoundaryCondition
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BoundaryCondition("reflective") for e in edges}
    init = np.where(mask, 1e-4 * (1.0 + np.random.default_rng(1).random(mask.shape)), 0.0)
    kw = dict(mask=mask, edges=edges, edge_conditions=bcs, initial_field=init, diffusion_coefficient=6.0, dt=0.1,
              total_time=0.55, dx=1.0, store_every=2, energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0,
              num_energy_bins=4, enable_diffusion=True, enable_recombination=True, enable_scattering=True, T_c=1.2,
              bath_temperature=0.1)
    kw.update(over)
    return kw


def _custom(body, **params):
    from qpsim_amd.models import ExternalGenerationSpec
    return ExternalGenerationSpec(mode="custom", custom_body=body, custom_params=params)


SWITCHED = "1e-6*(1.0+x)*params['a']*(2.0 if t<0.25 else 0.5)+np.where(y<0.5, 1e-7, 0.0)*E/200.0"


def _same(a, b) -> bool:
    return G.bits_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float))


def _run_both(kw, runner=None):
    """Results and phonon histories of ``generation_on_device`` False and True, with the stats of each."""
    from qpsim_amd import device_expr
    from qpsim_amd.solver import run_2d_crank_nicolson
    out = {}
    for on in (False, True):
        history: dict = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = (runner or run_2d_crank_nicolson)(**kw, phonon_history_out=history, generation_on_device=on)
        out[on] = (res, history, device_expr.last_run_stats())
    return out


def _assert_runs_equal(off, on):
    (r0, h0, _), (r1, h1, _) = off, on
    assert r0[0] == r1[0] and _same(r0[2], r1[2]) and _same(r0[5], r1[5])
    assert _same(np.stack(r0[1]), np.stack(r1[1]))
    assert _same(np.stack([np.stack(f) for f in r0[4]]), np.stack([np.stack(f) for f in r1[4]]))
    assert _same(np.stack(h0["phonon_frames"]), np.stack(h1["phonon_frames"]))
    assert _same(np.stack([np.stack(f) for f in h0["phonon_energy_frames"]]),
                 np.stack([np.stack(f) for f in h1["phonon_energy_frames"]]))


@pytest.mark.parametrize("grid,scheme", [("full_8x16", "cn_exact"), ("framed_9x11", "cn_exact"), ("full_8x16", "adi")])
def test_lone_run_switch_on_equals_off(grid, scheme):
    mask = np.ones((8, 16), dtype=bool) if grid == "full_8x16" else G.GRIDS[grid]
    both = _run_both(_problem(mask, external_generation=_custom(SWITCHED, a=1.5), diffusion_scheme=scheme))
    _assert_runs_equal(both[False], both[True])
    assert both[True][2] == {"device_steps": 6, "host_steps": 0}
    assert both[False][2] == {"device_steps": 0, "host_steps": 6}
    assert len(both[True][0][0]) == 4                            # t = 0, 0.2, 0.4 and the short last step


def test_ensemble_switch_on_equals_off():
    from qpsim_amd import device_expr, ensemble
    from qpsim_amd.models import ExternalGenerationSpec
    mask = np.ones((8, 16), dtype=bool)
    kw = _problem(mask, diffusion_scheme="adi")
    members = [dict(external_generation=_custom(SWITCHED, a=1.5)),
               dict(external_generation=_custom("np.sqrt(x*y)*params['b']*t", b=2e-6)),
               dict(external_generation=ExternalGenerationSpec(mode="constant", rate=2e-6)),
               dict(external_generation=_custom(SWITCHED, a=1.5))]
    out = {}
    for on in (False, True):
        histories = [dict() for _ in members]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = ensemble.run_2d_crank_nicolson_ensemble(
                [dict(m, phonon_history_out=h) for m, h in zip(members, histories)], generation_on_device=on, **kw)
        out[on] = (res, histories, ensemble.last_run_stats(), device_expr.last_run_stats())
    assert out[False][2] == out[True][2]
    assert out[True][3] == {"device_steps": 18, "host_steps": 0} and out[False][3] == {"device_steps": 0, "host_steps": 18}
    for m in range(len(members)):
        _assert_runs_equal((out[False][0][m], out[False][1][m], None), (out[True][0][m], out[True][1][m], None))
    # the members with the same body and params computed the same thing, the others did not
    assert _same(np.stack(out[True][0][0][1]), np.stack(out[True][0][3][1]))
    assert not _same(np.stack(out[True][0][0][1]), np.stack(out[True][0][1][1]))


def test_refused_body_takes_the_host_path():
    both = _run_both(_problem(np.ones((8, 16), dtype=bool), external_generation=_custom("1e-6*(1.0+x//0.25)*t")))
    _assert_runs_equal(both[False], both[True])
    assert both[True][2] == {"device_steps": 0, "host_steps": 6} == both[False][2]


@pytest.mark.parametrize("body,message", [("1e-6*(0.5-x)", "produced negative values. Generation rates must be non-negative."),
                                          ("1.0/(x-x)", "produced non-finite values.")])
def test_errors_are_the_host_paths(body, message):
    from qpsim_amd.solver import run_2d_crank_nicolson
    kw = _problem(np.ones((8, 16), dtype=bool), external_generation=_custom(body))
    for on in (False, True):
        with pytest.raises(ValueError) as err, warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            run_2d_crank_nicolson(**kw, generation_on_device=on)
        assert str(err.value) == f"External generation mode 'custom' {message}"


def test_error_in_an_ensemble_is_unprefixed_whatever_errors_says():
    from qpsim_amd.ensemble import run_2d_crank_nicolson_ensemble
    kw = _problem(np.ones((8, 16), dtype=bool), diffusion_scheme="adi")
    members = [dict(external_generation=_custom("1e-6*x")), dict(external_generation=_custom("1e-6*(0.5-x)"))]
    for errors in ("raise", "return"):
        with pytest.raises(ValueError) as err, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run_2d_crank_nicolson_ensemble(members, errors=errors, generation_on_device=True, **kw)
        assert str(err.value).startswith("External generation mode 'custom' produced negative values.")


def test_late_error_arrives_before_anything_at_or_after_the_offending_step_is_handed_out():
    """Negative from t >= 0.3 on, store_every = 1, a progress callback.  The step that STARTS at t = 0.3 offends (the
    accumulated 0.1 + 0.1 + 0.1 is just above 0.3); the state before it is the store point of time 0.3, which the host path
    hands out as well.  The device path, whose check arrives with the guard of the offending step, must hand out exactly
    what the host path does: nothing that ends at or after the offending step (no time >= 0.4), the same callbacks."""
    from qpsim_amd.solver import run_2d_crank_nicolson
    seen = {False: [], True: []}
    for on in (False, True):
        kw = _problem(np.ones((8, 16), dtype=bool), total_time=1.0, store_every=1,
                      external_generation=_custom("1e-6*(1.0+x)*(1.0 if t<0.3 else -1.0)"),
                      progress_callback=lambda t, frame, on=on: seen[on].append(t))
        with pytest.raises(ValueError, match="produced negative values"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run_2d_crank_nicolson(**kw, generation_on_device=on)
    assert seen[True] == seen[False] and len(seen[True]) == 4    # t = 0, 0.1, 0.2, 0.3 (the last good state)
    assert max(seen[True]) < 0.3 + 1e-12
