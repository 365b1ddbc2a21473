"""Boundary outflow traces, host side (no GPU): the reference helper against the oracle's operator, the face compiler against
the helper, the argument checks of both public calls, the plan layout, the argument validation of the library and the
Crank-Nicolson balance on the oracle, whose measured closure error is the margin of the GPU test."""
from __future__ import annotations

import inspect
import math

import numpy as np
import pytest

import boundary_flux_ref as R
from oracle import qp_oracle as O
from qpsim_amd import engine as E
from qpsim_amd import ensemble as ENS
from qpsim_amd import solver as S
from qpsim_amd.geometry import extract_edge_segments
from qpsim_amd.models import BoundaryCondition, EdgeSegment

U = 2.0 ** -53
BC = BoundaryCondition
FIVE = [BC("absorbing"), BC("dirichlet", 0.7), BC("robin", 0.3, 0.2), BC("neumann", -0.05), BC("reflective"),
        BC("dirichlet", 2.5), BC("neumann", 0.04), BC("robin", 0.6, 0.0)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from qpsim_amd import _hip
    return _hip.load()


def split_edges(edges):
    """Every edge of more than one face cut into two edges (ids ``<id>a``, ``<id>b``): a rectangle gets eight edges."""
    out = []
    for e in edges:
        if len(e.faces) < 2:
            out.append(e)
            continue
        h = len(e.faces) // 2
        for tag, faces in (("a", e.faces[:h]), ("b", e.faces[h:])):
            out.append(EdgeSegment(e.edge_id + tag, e.x0, e.y0, e.x1, e.y1, e.normal, list(faces)))
    return out


def geometries():
    rect = np.ones((12, 9), dtype=bool)
    donut = np.ones((16, 16), dtype=bool)
    donut[6:10, 5:11] = False
    ragged = np.ones((10, 14), dtype=bool)
    ragged[:3, :4] = False
    ragged[7:, 10:] = False
    ragged[4:6, 6:8] = False
    rng = np.random.default_rng(11)
    return [("rect12x9", rect, split_edges(extract_edge_segments(rect)), 6.0),
            ("donut16", donut, extract_edge_segments(donut), 1.5),
            ("ragged10x14", ragged, extract_edge_segments(ragged), 0.5 + 1.5 * rng.random(ragged.shape))]


def compile_faces(mask, edges, bcs, dx, surfaces):
    dev_mask, dev_edges = S._crop_to_bounding_box(np.asarray(mask, dtype=bool), edges)
    return E.compile_boundary_faces(dev_mask, dev_edges, bcs, dx, surfaces)


def assert_faces_equal(got, want):
    """``got``: engine.BoundaryFaces; ``want``: the helper's list of face lists."""
    assert got.counts == [len(w) for w in want]
    assert got.face_cell.dtype == np.int32 and got.face_diag.dtype == np.float64 and got.face_src.dtype == np.float64
    for s, faces in enumerate(want):
        b, e = got.surface_begin[s], got.surface_begin[s + 1]
        cell, diag, src = R.face_arrays(faces)
        assert np.array_equal(got.face_cell[b:e], cell) and np.array_equal(got.face_diag[b:e], diag)
        assert np.array_equal(got.face_src[b:e], src)


def assert_chunks_sound(faces):
    rows = faces.chunks
    assert rows.dtype == np.int32 and rows.ndim == 2 and rows.shape[1] == 3
    covered = []
    for begin, count, s in rows.tolist():
        assert 1 <= count <= E.FLUX_CHUNK
        assert faces.surface_begin[s] <= begin and begin + count <= faces.surface_begin[s + 1]
        covered += list(range(begin, begin + count))
    assert covered == list(range(int(faces.surface_begin[-1])))
    assert rows[:, 2].tolist() == sorted(rows[:, 2].tolist())


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name,mask,edges,D", geometries(), ids=[g[0] for g in geometries()])
def test_the_helper_totals_the_boundary_part_of_the_oracle_operator(name, mask, edges, D):
    """Links between interior cells are symmetric and cancel in the sum over the cells: with the surfaces a partition of
    the faces, the helper's total is -dx^2 fsum(L u + src) of the oracle's ``assemble_sparse``, within 8 u dx^2
    sum_p sum_q |L_pq| |u_q| (six terms per row)."""
    dx = 0.5
    bcs = {e.edge_id: FIVE[k % len(FIVE)] for k, e in enumerate(edges)}
    assert {b.kind for b in bcs.values()} == {"absorbing", "dirichlet", "robin", "neumann", "reflective"}
    surfaces = [[e.edge_id] for e in edges]
    faces = R.walk_faces(mask, edges, bcs, dx, surfaces)
    L, src = O.assemble_sparse(O.build_grid_ops(mask, edges, bcs, dx), D)
    u = 0.2 + np.random.default_rng(5).random(int(mask.sum()))
    plane = R.grid_plane(mask, u)
    dplane = D if np.ndim(D) == 0 else R.grid_plane(mask, D[mask])
    all_terms = np.concatenate([R.terms(f, plane, dplane) for f in faces if f])
    total = math.fsum(all_terms.tolist())
    want = -dx * dx * math.fsum((L @ u + src).tolist())
    limit = 8 * U * dx * dx * float((abs(L) @ np.abs(u)).sum())
    print(f"{name}: total {total:.17g}, oracle {want:.17g}, difference / bound {abs(total - want) / limit:.3g}")
    assert all_terms.size > 20 and (all_terms < 0).any() and (all_terms > 0).any()
    assert abs(total - want) <= limit


# ------------------------------------------------------------------------------------------------ the face compiler
def test_compiled_faces_follow_the_order_and_the_owner_rule():
    """A face listed by two edges goes to the last one: its surfaces receive it, with that edge's terms."""
    mask = np.ones((6, 7), dtype=bool)
    edges = extract_edge_segments(mask)
    first = edges[0]
    edges = edges + [EdgeSegment("late", first.x0, first.y0, first.x1, first.y1, first.normal, list(first.faces[2:5]))]
    bcs = {e.edge_id: FIVE[k] for k, e in enumerate(edges[:4])}
    bcs["late"] = BC("dirichlet", 3.0)
    surfaces = [[first.edge_id], ["late"], [e.edge_id for e in edges]]
    want = R.walk_faces(mask, edges, bcs, 0.5, surfaces)
    got = compile_faces(mask, edges, bcs, 0.5, surfaces)
    assert_faces_equal(got, want)
    assert got.counts[0] == len(first.faces) - 3 and got.counts[1] == 3
    assert set(got.face_src[got.surface_begin[1]:got.surface_begin[2]].tolist()) == {6.0}
    for s in range(3):                                  # sorted by cell inside a surface
        cells = got.face_cell[got.surface_begin[s]:got.surface_begin[s + 1]]
        assert np.all(np.diff(cells) >= 0)
    assert_chunks_sound(got)


def test_compiled_faces_index_the_bounding_box_of_a_padded_mask():
    mask = np.zeros((11, 13), dtype=bool)
    mask[2:8, 3:10] = True
    mask[4, 5] = False
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: FIVE[k % len(FIVE)] for k, e in enumerate(edges)}
    surfaces = [[e.edge_id for e in edges[:3]], [e.edge_id for e in edges[3:]]]
    got = compile_faces(mask, edges, bcs, 2.0, surfaces)
    assert_faces_equal(got, R.walk_faces(mask, edges, bcs, 2.0, surfaces))
    assert int(got.face_cell.max()) < 6 * 7 and int(got.face_cell.min()) == 0
    # the same faces as the unpadded mask gives
    inner = np.ascontiguousarray(mask[2:8, 3:10])
    e2 = extract_edge_segments(inner)
    assert [e.edge_id for e in e2] == [e.edge_id for e in edges]
    same = compile_faces(inner, e2, bcs, 2.0, surfaces)
    assert np.array_equal(same.face_cell, got.face_cell) and np.array_equal(same.face_diag, got.face_diag)


def test_reflective_faces_are_dropped_and_overlapping_surfaces_share_faces():
    mask = np.ones((5, 8), dtype=bool)
    edges = extract_edge_segments(mask)
    ids = [e.edge_id for e in edges]
    bcs = dict(zip(ids, [BC("reflective"), BC("absorbing"), BC("neumann", 0.0), BC("robin", 0.5, 0.1)]))
    surfaces = [[ids[0]], [ids[0], ids[2]], [ids[1]], [ids[1], ids[3]], ids]
    got = compile_faces(mask, edges, bcs, 1.0, surfaces)
    want = R.walk_faces(mask, edges, bcs, 1.0, surfaces)
    assert_faces_equal(got, want)
    n1, n3 = len(edges[1].faces), len(edges[3].faces)
    assert got.counts == [0, 0, n1, n1 + n3, n1 + n3]
    assert_chunks_sound(got)
    assert not (got.chunks[:, 2] < 2).any()             # an empty surface has no chunk
    # no face at all: the arrays are empty, the offsets stay
    none = compile_faces(mask, edges, bcs, 1.0, [[ids[0]], [ids[2]]])
    assert none.face_cell.size == 0 and none.surface_begin.tolist() == [0, 0, 0] and none.chunks.shape == (0, 3)


def test_chunk_tables_at_the_chunk_edge():
    """Surfaces of 1, 1023, 1024, 1025 and 2049 faces and an empty one: chunks of QP_FLUX_CHUNK faces that never cross."""
    sizes = [1, 1023, 1024, 1025, 2049]
    n = sum(sizes)
    mask = np.ones((1, n), dtype=bool)
    edges = extract_edge_segments(mask)
    up = next(e for e in edges if e.normal == "up")
    assert len(up.faces) == n
    cut = np.cumsum([0] + sizes)
    pieces = [EdgeSegment(f"piece{k}", 0.0, 0.0, 0.0, 0.0, "up", list(up.faces[cut[k]:cut[k + 1]])) for k in range(5)]
    others = [e for e in edges if e is not up]
    all_edges = others + pieces
    bcs = {e.edge_id: BC("reflective") for e in others}
    bcs.update({p.edge_id: BC("absorbing") for p in pieces})
    surfaces = [[p.edge_id] for p in pieces[:2]] + [[others[0].edge_id]] + [[p.edge_id] for p in pieces[2:]]
    got = compile_faces(mask, all_edges, bcs, 1.0, surfaces)
    assert got.counts == [1, 1023, 0, 1024, 1025, 2049]
    assert_faces_equal(got, R.walk_faces(mask, all_edges, bcs, 1.0, surfaces))
    assert_chunks_sound(got)
    b = got.surface_begin.tolist()
    assert got.chunks.tolist() == [[b[0], 1, 0], [b[1], 1023, 1], [b[3], 1024, 3], [b[4], 1024, 4], [b[4] + 1024, 1, 4],
                                   [b[5], 1024, 5], [b[5] + 1024, 1024, 5], [b[5] + 2048, 1, 5]]
    assert E.FLUX_CHUNK == 1024 and np.array_equal(E.flux_chunks(got.surface_begin), got.chunks)


def test_a_grid_beyond_int32_cells_is_refused():
    huge = np.broadcast_to(np.ones((1, 1), dtype=bool), (2 ** 16, 2 ** 15))          # a view: no memory behind it
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        E.compile_boundary_faces(huge, [], {}, 1.0, [[]])


# ------------------------------------------------------------------------------------------------ arguments
def _small(**kw):
    mask = np.ones((3, 4), dtype=bool)
    edges = extract_edge_segments(mask)
    base = dict(mask=mask, edges=edges, edge_conditions={e.edge_id: BC("absorbing") for e in edges},
                initial_field=np.ones(mask.shape), diffusion_coefficient=1.0, dt=0.1, total_time=0.75, dx=1.0,
                energy_gap=180.0, energy_min_factor=1.0, energy_max_factor=3.0, num_energy_bins=8)
    base.update(kw)
    return base


def test_the_three_parameters_and_their_defaults():
    """Fails on a tree without the feature: the keywords do not exist."""
    params = inspect.signature(S.run_2d_crank_nicolson).parameters
    assert [params[k].default for k in ("flux_out", "flux_surfaces", "flux_every")] == [None, None, 1]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("flux_out", "flux_surfaces", "flux_every"))
    sink = inspect.signature(ENS.run_2d_crank_nicolson_ensemble).parameters["flux_out"]
    assert sink.default is None and sink.kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("kw,match", [
    (dict(flux_out={}, flux_every=0), "flux_every"),
    (dict(flux_every=-1), "flux_every"),
    (dict(flux_every=True), "flux_every"),
    (dict(flux_out={}, flux_every=1.5), "flux_every"),
    (dict(flux_surfaces={"a": ["edge_0001"]}), "flux_surfaces needs flux_out"),
    (dict(flux_out={}, flux_surfaces={"a": ["edge_0001", "edge_9999"]}), r"flux_surfaces\['a'\].*edge_9999"),
    (dict(flux_out={}, flux_surfaces={"a": ["edge_0001"], "b": []}), r"flux_surfaces\['b'\] is empty"),
    (dict(flux_out={}, flux_surfaces={f"s{k}": ["edge_0001"] for k in range(65)}), "flux_surfaces.*1 to 64.*65"),
    (dict(flux_out={}, flux_surfaces={}), "flux_surfaces.*1 to 64"),
    (dict(flux_out={}, enable_diffusion=False), "flux_out.*enable_diffusion"),
    # 100001 samples x 64 surfaces x 8 planes x 8 B = 391 MiB
    (dict(flux_out={}, flux_surfaces={f"s{k}": ["edge_0001"] for k in range(64)}, dt=1e-5, total_time=1.0),
     "flux_every.*256 MiB.*larger flux_every"),
])
def test_bad_flux_arguments_are_refused_before_a_sink_is_cleared_or_a_device_is_needed(lib, kw, match):
    kw = dict(kw)
    sink = kw.get("flux_out")
    if sink is not None:
        sink["stale"] = True
    other = {"stale": True}
    with pytest.raises(ValueError, match=match):
        S.run_2d_crank_nicolson(**_small(**kw), trace_out=other)
    if "larger flux_every" not in match:           # the buffer check needs the schedule: it comes after the plans
        assert other == {"stale": True} and (sink is None or sink == {"stale": True})


def test_flux_keys_are_shared_by_all_members_and_the_sink_outlives_a_bad_argument(lib):
    common = _small()
    for key, value in (("flux_surfaces", {"a": ["edge_0001"]}), ("flux_every", 2), ("flux_out", {})):
        with pytest.raises(ValueError, match=f"member 1: '{key}' is shared by all members"):
            ENS.member_arguments([{}, {key: value}], common)
    kws = ENS.member_arguments([{}, {}], dict(common, flux_every=4))
    assert [k["flux_every"] for k in kws] == [4, 4] and kws[0]["flux_surfaces"] is None and kws[0]["flux_out"] is None
    with pytest.raises(ValueError, match="flux_surfaces needs flux_out"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], flux_surfaces={"a": ["edge_0001"]}, **common)
    sink = ["stale"]
    with pytest.raises(ValueError, match="flux_every"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], flux_out=sink, flux_every=0, **common)
    assert sink == ["stale"]
    with pytest.raises(ValueError, match="flux_out.*enable_diffusion"):
        ENS.run_2d_crank_nicolson_ensemble([{}, {}], flux_out=sink, **dict(common, enable_diffusion=False))
    assert sink == ["stale"]
    assert ENS.run_2d_crank_nicolson_ensemble([], flux_out=sink) == [] and sink == []


def test_a_block_plan_of_a_decomposed_run_is_refused():
    """``Engine.boundary_flux`` takes the ``DiffusionOperator`` of its own engine and nothing else (no device is needed
    for the refusal)."""
    eng = object.__new__(E.Engine)
    with pytest.raises(ValueError, match="domain-decomposed"):
        E.Engine.boundary_flux(eng, {}, object(), None, 1, None)


def test_the_plan_has_the_method_set_of_the_other_plans_and_comes_fifth(lib):
    from qpsim_amd.timeloop import Schedule
    a = _small(enable_recombination=True, enable_scattering=True)
    mask = a["mask"]
    ones = np.ones(mask.shape, dtype=bool)
    sinks = [{}, {}, {}, {}, {}]
    ids = [e.edge_id for e in a["edges"]]
    plans = S._sampling_plans(mask, sinks[0], None, 1, sinks[1], 2, 1, sinks[2], {"a": ones}, 3, a, sinks[3], None, 1,
                              sinks[4], {"left": ids[:1], "rest": ids[1:]}, 3)
    assert [type(p).__name__ for p, _ in plans] == ["_TracePlan", "_CoarsePlan", "_RatesPlan", "_PhononRatesPlan",
                                                    "_FluxPlan"]
    assert [sink is s for (_, sink), s in zip(plans, sinks)] == [True] * 5
    plan = plans[4][0]
    for name in ("every", "row_shape", "sampler", "result", "too_large"):
        assert hasattr(plan, name)
    assert plan.every == 3 and plan.row_shape(8) == (2, 8) and plan.names == ["left", "rest"]
    assert plan.counts == [len(a["edges"][0].faces), sum(len(e.faces) for e in a["edges"][1:])]
    sched = Schedule(0.75, 0.1, 1)
    assert S._sample_buffer_bytes(plan, sched, 5, 8) == 8 * sched.rows(3) * 5 * 2 * 8
    kw = ENS.member_arguments([{}], dict(a, flux_every=3))[0]
    assert ENS._bytes_per_member(kw, [plan]) - ENS._bytes_per_member(kw) == 8 * sched.rows(3) * 2 * 8
    rows = np.arange(2 * 2 * 8, dtype=float).reshape(2, 2, 8)
    got = plan.result([0.0, 0.3], rows, np.linspace(180.0, 540.0, 8), 0.5, 2.0)
    assert sorted(got) == ["energy_bins", "faces", "number_outflow", "outflow", "surfaces", "times"]
    assert got["surfaces"] == ["left", "rest"] and got["faces"] == plan.counts and got["outflow"].shape == (2, 2, 8)
    assert np.array_equal(got["number_outflow"], 2.0 * rows.sum(axis=-1))
    scalar = plan.result([0.0], rows[:1, :, :1], None, 0.5, None)
    assert scalar["energy_bins"] is None and np.array_equal(scalar["number_outflow"], rows[:1, :, 0])
    # None: one surface "all" made of every edge
    alone = S._sampling_plans(mask, None, None, 1, None, 8, 1, None, None, 1, a, None, None, 1, {}, None, 1)
    assert len(alone) == 1 and alone[0][0].names == ["all"] and alone[0][0].counts == [2 * (3 + 4)]
    # without a sink the call plans exactly what it planned before
    assert S._sampling_plans(mask, None, None, 1, None, 8, 1) == []
    assert S._sampling_plans(mask, None, None, 1, None, 8, 1, None, None, 1, a, None, None, 1, None, None, 1) == []


# ------------------------------------------------------------------------------------------------ the library, no GPU
def test_workspace_formula(lib):
    """Fails on a tree without the feature: the symbols do not exist."""
    ws = lib.qp_boundary_flux_workspace_bytes
    assert ws(4, 3, 7) == 8 * 4 * 3 * 7 and ws(1, 1, 0) == 8 and ws(13, 1, 1) == 8 * 13
    assert ws(0, 1, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 1, -1) == 0 and ws(256, 256, 1) == 0


def test_the_call_validates_before_any_launch(lib):
    begin = np.array([0, 3, 3, 2000], dtype=np.int32)
    chunks = np.array([[0, 3, 0], [3, 1024, 2], [1027, 973, 2]], dtype=np.int32)
    ok = dict(state=8, dcoef=8, dfield=0, nplane=2, ncm=100, members=1, cell=8, diag=8, src=8, nface=2000, begin=begin,
              nsurface=3, chunks=chunks, chunks_dev=8, nchunk=3, ws=8, out=8)

    def call(**bad):
        a = dict(ok, **bad)
        host = lambda v: 0 if v is None else np.ascontiguousarray(v, dtype=np.int32).ctypes.data  # noqa: E731
        tables = [np.ascontiguousarray(a[k], dtype=np.int32) if a[k] is not None else None for k in ("begin", "chunks")]
        return lib.qp_boundary_flux(a["state"], a["dcoef"], a["dfield"], a["nplane"], a["ncm"], a["members"], a["cell"],
                                    a["diag"], a["src"], a["nface"], host(tables[0]), a["nsurface"], host(tables[1]),
                                    a["chunks_dev"], a["nchunk"], a["ws"], a["out"], 0)

    def rows(*r):
        return np.array(r, dtype=np.int32)

    for bad in (dict(state=0), dict(ws=0), dict(out=0), dict(begin=None), dict(cell=0), dict(diag=0), dict(src=0),
                dict(chunks=None), dict(chunks_dev=0), dict(dcoef=0), dict(dfield=8), dict(nplane=0), dict(ncm=0),
                dict(members=0), dict(ncm=2 ** 31), dict(nplane=300, members=300), dict(nface=-1), dict(nchunk=-1),
                dict(nchunk=0), dict(nsurface=0), dict(nsurface=65),
                dict(begin=[0, 3, 3, 1999]), dict(begin=[1, 3, 3, 2000]), dict(begin=[0, 3, 2, 2000]),
                dict(chunks=rows([0, 3, 0], [3, 1025, 2], [1028, 972, 2])),        # above QP_FLUX_CHUNK
                dict(chunks=rows([0, 3, 0], [3, 0, 2], [1027, 973, 2])),           # empty
                dict(chunks=rows([0, 4, 0], [4, 1023, 2], [1027, 973, 2])),        # crosses surface 0 -> 1
                dict(chunks=rows([0, 3, 0], [3, 1024, 1], [1027, 973, 2])),        # in a surface that is empty
                dict(chunks=rows([0, 3, 0], [3, 1024, 2], [1027, 974, 2])),        # past the last face
                dict(chunks=rows([0, 3, 0], [1027, 973, 2], [3, 1024, 2])),        # out of order
                dict(chunks=rows([3, 1024, 2], [0, 3, 0], [1027, 973, 2])),
                dict(chunks=rows([0, 3, 0], [3, 1024, 2], [1000, 973, 2])),        # overlapping
                dict(chunks=rows([0, 3, 3], [3, 1024, 2], [1027, 973, 2])),        # surface out of range
                dict(chunks=rows([0, 3, -1], [3, 1024, 2], [1027, 973, 2]))):
        assert call(**bad) == -1, bad
        assert b"qp_boundary_flux" in lib.qp_last_error()
    assert call(nsurface=65) == -1 and b"1 to 64" in lib.qp_last_error()
    assert call(chunks=rows([0, 4, 0], [4, 1023, 2], [1027, 973, 2])) == -1 and b"crosses" in lib.qp_last_error()


# ------------------------------------------------------------------------------------------------ the CN balance
def test_crank_nicolson_closes_the_number_balance_on_the_oracle():
    """The outflow is affine in u, so the trapezoidal rule of the unsplit CN step integrates it exactly:
    mass_k - mass_{k+1} = dt (F_k + F_{k+1}) / 2 with mass = dx^2 sum u and F the total outflow.  What is left is the
    rounding of the sparse solve and of the sums; in units of u * mass_k it is recorded as ``R.CN_CLOSURE_UNITS``, from
    which the GPU test takes its margin (measured here: 2.06 units at worst over the six steps, see the printed lines)."""
    case = R.balance_case()
    mask, dx, dt, D = (case[k] for k in ("mask", "dx", "dt", "D"))
    edges = extract_edge_segments(mask)
    bcs = {e.edge_id: BC(*kind) for e, kind in zip(edges, case["kinds"])}
    assert {b.kind for b in bcs.values()} == {"absorbing", "dirichlet", "robin", "neumann"}
    faces = R.walk_faces(mask, edges, bcs, dx, [[e.edge_id for e in edges]])[0]
    stepper = O.CNStepper(O.build_grid_ops(mask, edges, bcs, dx), D, dt)
    u = case["u0"][mask].astype(float)
    worst = 0.0
    for k in range(6):
        nxt = stepper.step(u)
        mass0, mass1 = (dx * dx * math.fsum(v.tolist()) for v in (u, nxt))
        f0, f1 = (R.outflow(faces, R.grid_plane(mask, v), D)[0] for v in (u, nxt))
        err = mass0 - mass1 - dt * (f0 + f1) / 2
        units = abs(err) / (U * mass0)
        print(f"step {k + 1}: mass {mass0:.17g} -> {mass1:.17g}, outflow {f0:.6g} -> {f1:.6g}, closure {err:.3g} "
              f"= {units:.3g} u mass")
        worst = max(worst, units)
        assert (mass0 - mass1) > 1e6 * U * mass0        # the balance is not trivially closed
        u = nxt
    print(f"worst closure error: {worst:.3g} u mass (recorded margin: {R.CN_CLOSURE_UNITS})")
    assert worst <= R.CN_CLOSURE_UNITS
