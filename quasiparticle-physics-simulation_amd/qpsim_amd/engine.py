"""Device-side engine: geometry compilation, resident state and kernel sequencing.

Host code here is plumbing only (PyTorch-ROCm tensors for device memory and streams, ctypes calls
into ``libqpsim_hip.so``).  All arithmetic of the time loop runs in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import math
import os

import numpy as np

from . import _hip
from . import collision_tables
from .collision_tables import (antidiagonal_major, diagonal_major, onepass_tables, structured_bin_maps,  # noqa: F401
                               tag_merged_bins)
from .models import BoundaryCondition, EdgeSegment

FLAG_XM, FLAG_XP, FLAG_YM, FLAG_YP, FLAG_ACTIVE = 1, 2, 4, 8, 16
_DIRECTIONS = ("up", "down", "left", "right")  # the reference's face walk order (solver.py:25-30)


class BoundaryAssignmentError(ValueError):
    """A boundary face or edge has no boundary condition (reference solver.py:21)."""


def _torch():
    import torch
    return torch


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("qpsim_amd needs a HIP device (torch.cuda.is_available() is False); "
                           "there is no CPU fallback for the time loop.")
    return torch


# --------------------------------------------------------------------------------------------------------- #
# geometry compilation (host, vectorised): mask + edges + edge_conditions -> per-cell operator tables
# --------------------------------------------------------------------------------------------------------- #
@dataclass
class CompiledGeometry:
    mask: np.ndarray      # [ny, nx] bool
    dx: float
    flags: np.ndarray     # [ny, nx] uint8
    ex: np.ndarray        # [ny, nx] f64, BC diagonal terms of x-faces in 1/dx^2 units
    ey: np.ndarray
    sx: np.ndarray        # BC sources in 1/dx^2 units
    sy: np.ndarray

    @property
    def is_full_rectangle(self) -> bool:
        return bool(self.mask.all())


def _face_terms(bc: BoundaryCondition, dx: float) -> tuple[float, float]:
    """(diagonal, source) contribution of one boundary face in units of 1/dx^2 (solver.py:112-149)."""
    kind = bc.normalized_kind()
    if kind == "reflective":
        return 0.0, 0.0
    if kind == "absorbing":
        return 2.0, 0.0
    if kind == "dirichlet":
        return 2.0, 2.0 * float(bc.value or 0.0)
    if kind == "neumann":
        return 0.0, float(bc.value or 0.0) * dx
    if kind == "robin":
        return float(bc.value or 0.0) * dx, float(bc.aux_value or 0.0) * dx
    raise BoundaryAssignmentError(f"Unsupported boundary kind: {bc.kind}")


def link_flags(mask: np.ndarray) -> np.ndarray:
    m = np.asarray(mask, dtype=bool)
    pad = np.zeros((m.shape[0] + 2, m.shape[1] + 2), dtype=bool)
    pad[1:-1, 1:-1] = m
    f = np.zeros(m.shape, dtype=np.uint8)
    f |= (m & pad[1:-1, :-2]).astype(np.uint8) * FLAG_XM
    f |= (m & pad[1:-1, 2:]).astype(np.uint8) * FLAG_XP
    f |= (m & pad[:-2, 1:-1]).astype(np.uint8) * FLAG_YM
    f |= (m & pad[2:, 1:-1]).astype(np.uint8) * FLAG_YP
    f |= m.astype(np.uint8) * FLAG_ACTIVE
    return f


def compile_geometry(mask: np.ndarray, edges: list[EdgeSegment], edge_conditions: dict[str, BoundaryCondition],
                     dx: float) -> CompiledGeometry:
    """Per-cell link flags and boundary terms; same checks / errors as solver.py:152-212."""
    if dx <= 0:
        raise ValueError("dx must be positive.")
    mask = np.asarray(mask, dtype=bool)
    if mask.ndim != 2:
        raise ValueError("mask must be 2D.")
    if not mask.any():
        raise ValueError("Geometry mask has no interior points.")
    ny, nx = mask.shape
    # BC index per face; later edges overwrite earlier ones, edges without a BC are skipped (solver.py:37-50)
    bc_list: list[tuple[float, float]] = []
    face_bc = {d: np.full((ny, nx), -1, dtype=np.int32) for d in _DIRECTIONS}
    for edge in edges:
        bc = edge_conditions.get(edge.edge_id)
        if bc is None:
            continue
        bc.validate()
        bc_list.append(_face_terms(bc, dx))
        k = len(bc_list) - 1
        for d in _DIRECTIONS:
            rc = [(f.row, f.col) for f in edge.faces if f.direction == d]
            if rc:
                rows, cols = np.asarray(rc, dtype=np.int64).T
                face_bc[d][rows, cols] = k
    missing = [e.edge_id for e in edges if e.edge_id not in edge_conditions]
    if missing:
        raise BoundaryAssignmentError(
            f"All edges must be assigned boundary conditions before simulation. Missing: {len(missing)}")

    flags = link_flags(mask)
    link_of = {"up": FLAG_YM, "down": FLAG_YP, "left": FLAG_XM, "right": FLAG_XP}
    diag = np.asarray([t[0] for t in bc_list] + [0.0])
    src = np.asarray([t[1] for t in bc_list] + [0.0])
    ex = np.zeros((ny, nx))
    ey = np.zeros((ny, nx))
    sx = np.zeros((ny, nx))
    sy = np.zeros((ny, nx))
    unassigned = np.zeros((ny, nx), dtype=np.int8)  # 1 + index of first direction lacking a BC
    for order, d in reversed(list(enumerate(_DIRECTIONS))):
        boundary = mask & ((flags & link_of[d]) == 0)
        k = face_bc[d]
        bad = boundary & (k < 0)
        unassigned[bad] = order + 1
        kk = np.where(boundary & (k >= 0), k, len(bc_list))
        if d in ("left", "right"):
            ex += diag[kk]
            sx += src[kk]
        else:
            ey += diag[kk]
            sy += src[kk]
    if unassigned.any():
        r, c = (int(v) for v in np.argwhere(unassigned > 0)[0])
        d = _DIRECTIONS[int(unassigned[r, c]) - 1]
        raise BoundaryAssignmentError(f"Missing boundary condition for face at cell ({r}, {c}) direction '{d}'.")
    return CompiledGeometry(mask, float(dx), flags, ex, ey, sx, sy)


def pack_region_bits(regions, grid_mask: np.ndarray, offset=(0, 0)) -> np.ndarray:
    """Up to 8 boolean regions given on a full frame -> one uint8 plane on the grid of ``grid_mask`` (the window of the full
    frame at ``offset``: the solver crops padded geometries onto their bounding box).  Bit r of a cell is set when the cell
    lies in region r AND inside the mask, so a kernel that reads the bits needs no flags.  Host only."""
    grid_mask = np.asarray(grid_mask, dtype=bool)
    regions = list(regions)
    if not 1 <= len(regions) <= 8:
        raise ValueError("1 to 8 regions fit into one plane of region bits")
    ny, nx = grid_mask.shape
    r0, c0 = int(offset[0]), int(offset[1])
    bits = np.zeros((ny, nx), dtype=np.uint8)
    for r, region in enumerate(regions):
        region = np.asarray(region, dtype=bool)
        window = region[r0:r0 + ny, c0:c0 + nx]
        if region.ndim != 2 or window.shape != (ny, nx):
            raise ValueError(f"region {r} of shape {region.shape} does not cover the {ny} x {nx} grid at offset ({r0}, {c0})")
        bits |= (window & grid_mask).astype(np.uint8) << r
    return bits


FLUX_CHUNK = 1024          # QP_FLUX_CHUNK of include/qpsim_hip.h: faces per block of ``qp_boundary_flux``
FLUX_SURFACES = 64         # surfaces per call: one lane of the second stage each


@dataclass
class BoundaryFaces:
    """The non-reflective boundary faces of a grid, grouped by surface (``compile_boundary_faces``): surface s owns the faces
    ``surface_begin[s] : surface_begin[s + 1]`` of the flat arrays, sorted by cell index (faces of one cell in the
    reference's walk order up, down, left, right); ``chunks`` [nchunk, 3] = (first face, faces, surface) cuts every surface
    into chunks of at most ``FLUX_CHUNK`` faces that never cross a surface."""
    face_cell: np.ndarray        # [nface] int32, r * nx + c on the grid of the mask
    face_diag: np.ndarray        # [nface] f64, 1/dx^2 units
    face_src: np.ndarray         # [nface] f64
    surface_begin: np.ndarray    # [nsurface + 1] int32
    chunks: np.ndarray           # [nchunk, 3] int32

    @property
    def counts(self) -> list:
        return [int(v) for v in np.diff(self.surface_begin)]


def flux_chunks(surface_begin, chunk: int = FLUX_CHUNK) -> np.ndarray:
    """The chunk table [nchunk, 3] int32 = (first face, faces, surface) of surfaces that own the faces
    ``surface_begin[s] : surface_begin[s + 1]``: every surface cut into chunks of ``chunk`` faces, the last one shorter; an
    empty surface has no chunk."""
    rows = [(b, min(chunk, int(e) - b), s)
            for s, (b0, e) in enumerate(zip(surface_begin[:-1], surface_begin[1:])) for b in range(int(b0), int(e), chunk)]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def compile_boundary_faces(mask: np.ndarray, edges: list[EdgeSegment], edge_conditions: dict[str, BoundaryCondition],
                           dx: float, surfaces) -> BoundaryFaces:
    """Flat face arrays of ``surfaces`` (a sequence of lists of edge ids; surfaces may overlap) on the grid of ``mask`` (the
    device grid: the bounding box of the run's mask, ``edges`` cropped with it).  A boundary face belongs to the edge whose
    boundary condition ``compile_geometry`` applies to it - the last edge that lists it - and goes to every surface naming
    that edge with the ``_face_terms`` of its condition; faces whose terms are both zero (reflective, zero-flux Neumann)
    are dropped, so their cells are never loaded.  Host only, vectorised apart from the loops over edges and surfaces."""
    mask = np.asarray(mask, dtype=bool)
    ny, nx = mask.shape
    if ny * nx > 2 ** 31 - 1:
        raise ValueError(f"a grid of {ny} x {nx} cells is too large for boundary faces (at most 2^31 - 1 cells)")
    owner = {d: np.full((ny, nx), -1, dtype=np.int32) for d in _DIRECTIONS}
    terms = np.zeros((len(edges), 2))
    for k, edge in enumerate(edges):
        bc = edge_conditions.get(edge.edge_id)
        if bc is None:
            continue
        terms[k] = _face_terms(bc, dx)
        for d in _DIRECTIONS:
            rc = [(f.row, f.col) for f in edge.faces if f.direction == d]
            if rc:
                rows, cols = np.asarray(rc, dtype=np.int64).T
                owner[d][rows, cols] = k
    flags = link_flags(mask)
    link_of = {"up": FLAG_YM, "down": FLAG_YP, "left": FLAG_XM, "right": FLAG_XP}
    cell, walk, own = [], [], []
    for order, d in enumerate(_DIRECTIONS):
        r, c = np.nonzero(mask & ((flags & link_of[d]) == 0) & (owner[d] >= 0))
        cell.append(r * nx + c)
        walk.append(np.full(r.size, order))
        own.append(owner[d][r, c])
    cell, walk, own = np.concatenate(cell), np.concatenate(walk), np.concatenate(own)
    live = (terms[own, 0] != 0.0) | (terms[own, 1] != 0.0)
    cell, walk, own = cell[live], walk[live], own[live]
    first = np.lexsort((walk, cell))
    cell, own = cell[first], own[first]
    position = {}
    for k, edge in enumerate(edges):
        position.setdefault(edge.edge_id, []).append(k)
    picked, begin = [], [0]
    for ids in surfaces:
        wanted = np.zeros(len(edges) + 1, dtype=bool)
        for edge_id in ids:
            wanted[position.get(edge_id, [])] = True
        picked.append(np.flatnonzero(wanted[own]))
        begin.append(begin[-1] + picked[-1].size)
    if begin[-1] > 2 ** 31 - 1:
        raise ValueError(f"{begin[-1]} boundary faces over all surfaces are too many (at most 2^31 - 1)")
    sel = np.concatenate(picked) if picked else np.zeros(0, dtype=np.int64)
    surface_begin = np.asarray(begin, dtype=np.int32)
    return BoundaryFaces(cell[sel].astype(np.int32), np.ascontiguousarray(terms[own[sel], 0]),
                         np.ascontiguousarray(terms[own[sel], 1]), surface_begin, flux_chunks(surface_begin))


COARSE_BINS = (2, 4, 8, 16, 32, 64)      # block edges of coarse frames (``qp_block_sums``)


class CoarseLayout:
    """Where the b x b blocks of coarse frames lie (``coarse_layout``): ``shape`` (cy, cx) of the full coarse frame,
    ``cells`` [cy, cx] in-mask cells per block, ``origin`` (r0, c0) of the mask's bounding box, ``offset`` (oy, ox) of the
    device cell (0, 0) inside its block, ``window`` (wy, wx, cny, cnx): the rows / columns of the full coarse frame that
    the device output [cny, cnx] occupies."""

    def __init__(self, bin, shape, cells, origin, offset, window):
        self.bin, self.shape, self.cells, self.origin, self.offset, self.window = bin, shape, cells, origin, offset, window


def coarse_layout(mask: np.ndarray, bin: int) -> CoarseLayout:
    """Blocks of ``bin`` x ``bin`` cells aligned to the origin of the full frame of ``mask``, and the part of them that the
    device grid (the bounding box of the mask) touches.  Host only."""
    mask = np.asarray(mask, dtype=bool)
    b = int(bin)
    if mask.ndim != 2 or not mask.any():
        raise ValueError("coarse_layout needs a 2-D mask with at least one interior cell")
    H, W = mask.shape
    cy, cx = -(-H // b), -(-W // b)
    padded = np.zeros((cy * b, cx * b), dtype=np.int64)
    padded[:H, :W] = mask
    cells = padded.reshape(cy, b, cx, b).sum(axis=(1, 3))
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    r0, c0 = int(rows[0]), int(cols[0])
    ny, nx = int(rows[-1]) - r0 + 1, int(cols[-1]) - c0 + 1
    oy, ox = r0 % b, c0 % b
    window = (r0 // b, c0 // b, -(-(oy + ny) // b), -(-(ox + nx) // b))
    return CoarseLayout(b, (cy, cx), cells, (r0, c0), (oy, ox), window)


# --------------------------------------------------------------------------------------------------------- #
# device engine
# --------------------------------------------------------------------------------------------------------- #
_TINY = float(np.finfo(np.float64).tiny)


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def rect_side_terms(geom: CompiledGeometry):
    """(bc_diag[4], bc_src[4]) in left, right, up, down order if the geometry is a full rectangle whose four
    sides each carry one boundary condition; None otherwise (then only the general kernels apply)."""
    if not geom.is_full_rectangle:
        return None
    ny, nx = geom.mask.shape

    def side(arr, sl):
        vals = arr[sl]
        return float(vals.flat[0]) if np.all(vals == vals.flat[0]) else None

    if nx > 1:
        xs = [side(geom.ex, (slice(None), 0)), side(geom.ex, (slice(None), -1)),
              side(geom.sx, (slice(None), 0)), side(geom.sx, (slice(None), -1))]
    else:  # one column: both x-faces sit on the same cell; only their sum enters
        xs = [side(geom.ex, (slice(None), 0)), 0.0, side(geom.sx, (slice(None), 0)), 0.0]
    if ny > 1:
        ys = [side(geom.ey, (0, slice(None))), side(geom.ey, (-1, slice(None))),
              side(geom.sy, (0, slice(None))), side(geom.sy, (-1, slice(None)))]
    else:
        ys = [side(geom.ey, (0, slice(None))), 0.0, side(geom.sy, (0, slice(None))), 0.0]
    if any(v is None for v in xs + ys):
        return None
    return [xs[0], xs[1], ys[0], ys[1]], [xs[2], xs[3], ys[2], ys[3]]


class RectPlan:
    """Owner of a ``qp_adi_rect_plan`` (device tables + work planes of the fast full-rectangle ADI path)."""

    def __init__(self, lib, ny, nx, nfield, r, dcoef, bc_diag, bc_src, force_banded: bool = False, block=None):
        """``block = (gny, gnx, j0, i0)`` makes this the plan of one block of a decomposed gny x gnx grid."""
        self._lib = lib
        self._h = C.POINTER(_hip.RectPlan)()
        dc = (C.c_double * nfield)(*[float(v) for v in dcoef])
        bd = (C.c_double * 4)(*bc_diag)
        bs = (C.c_double * 4)(*bc_src)
        gny, gnx, j0, i0 = (ny, nx, 0, 0) if block is None else block
        _hip.check(lib.qp_adi_rect_plan_create_block(ny, nx, nfield, float(r), dc, bd, bs, int(bool(force_banded)),
                                                     int(gny), int(gnx), int(j0), int(i0), C.byref(self._h)),
                   "qp_adi_rect_plan_create_block")
        self.decoupled = (bool(lib.qp_adi_rect_plan_decoupled(self._h, 0)), bool(lib.qp_adi_rect_plan_decoupled(self._h, 1)))
        self.fine = bool(lib.qp_adi_rect_plan_fine(self._h))      # 32-cell chunks (qp_adi_fine.inc) instead of 64 x 64 tiles

    @classmethod
    def peaceman_rachford(cls, lib, ny, nx, nfield, r, dcoef, bc_diag, p: float, share: "RectPlan | None" = None):
        """Plan of one Peaceman-Rachford iteration with parameter ``p`` (``qp_adi_rect_plan_create_pr``); ``share`` lends its
        work plane (keep it alive as long as the borrower)."""
        self = cls.__new__(cls)
        self._lib = lib
        self._h = C.POINTER(_hip.RectPlan)()
        self._lender = share
        dc = (C.c_double * nfield)(*[float(v) for v in dcoef])
        bd = (C.c_double * 4)(*bc_diag)
        _hip.check(lib.qp_adi_rect_plan_create_pr(ny, nx, nfield, float(r), dc, bd, float(p),
                                                  share.handle if share is not None else None, C.byref(self._h)),
                   "qp_adi_rect_plan_create_pr")
        self.decoupled = (bool(lib.qp_adi_rect_plan_decoupled(self._h, 0)), bool(lib.qp_adi_rect_plan_decoupled(self._h, 1)))
        self.fine, self.p = bool(lib.qp_adi_rect_plan_fine(self._h)), float(p)
        return self

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.qp_adi_rect_plan_destroy(self._h)
            self._h = C.POINTER(_hip.RectPlan)()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _jacobi_dn(u: float, m: float) -> tuple[float, float]:
    """(dn(u | m), K(m)) by the arithmetic-geometric mean (Abramowitz & Stegun 16.4, 17.6), parameter m = k^2 < 1."""
    a, b, c = [1.0], [math.sqrt(1.0 - m)], [math.sqrt(m)]
    while abs(c[-1]) > 1e-17 and len(a) < 40:
        a.append(0.5 * (a[-1] + b[-1]))
        b.append(math.sqrt(a[-2] * b[-1]))
        c.append(0.5 * (a[-2] - b[-2]))
    n = len(a) - 1
    K = math.pi / (2.0 * a[n])
    phi = [0.0] * (n + 1)
    phi[n] = (2.0 ** n) * a[n] * u
    for k in range(n, 0, -1):
        phi[k - 1] = 0.5 * (phi[k] + math.asin(c[k] * math.sin(phi[k]) / a[k]))
    if n == 0:
        return 1.0, K
    return math.cos(phi[0]) / math.cos(phi[1] - phi[0]), K


def peaceman_rachford_cycle(alpha: float, beta: float, J: int):
    """Jordan's optimal cyclic parameters of J Peaceman-Rachford iterations for commuting H, V with spectra in
    [alpha, beta], p_j = beta dn((2j-1) K / (2J), k), k^2 = 1 - (alpha/beta)^2, and the worst-case factor
    max_{h,v} prod_j |(h - p_j)/(h + p_j)| |(v - p_j)/(v + p_j)| of the cycle (evaluated on 4000 points of the interval)."""
    alpha, beta = float(alpha), float(max(beta, alpha * (1.0 + 1e-9)))
    m = 1.0 - (alpha / beta) ** 2
    K = _jacobi_dn(0.0, m)[1]
    ps = [beta * _jacobi_dn((2 * j - 1) * K / (2.0 * J), m)[0] for j in range(1, J + 1)]
    h = np.geomspace(alpha, beta, 4000)
    f = np.ones_like(h)
    for p in ps:
        f *= np.abs((h - p) / (h + p))
    return ps, float(f.max()) ** 2


def peaceman_rachford_parameters(alpha: float, beta: float, reduction: float, jmax: int = 24):
    """The shortest cycle (``peaceman_rachford_cycle``) whose worst-case factor is <= ``reduction`` (or the cycle of
    ``jmax`` iterations when none is).  Returns (parameters, worst-case factor)."""
    best = None
    for J in range(1, jmax + 1):
        best = peaceman_rachford_cycle(alpha, beta, J)
        if best[1] <= reduction:
            break
    return best


class TilePlan:
    """Owner of a ``qp_adi_tile_plan`` (tiled ADI path for masked grids with one diffusivity per field)."""

    def __init__(self, lib, geom: CompiledGeometry, nfield, r, dcoef=None, dfield_dev=None):
        """``dcoef``: one diffusivity per field (host values) or ``dfield_dev``: device tensor [nfield, ncell]."""
        self._lib = lib
        self._h = C.POINTER(_hip.TilePlan)()
        ny, nx = geom.mask.shape
        host = [np.ascontiguousarray(geom.flags, dtype=np.uint8)] + [
            np.ascontiguousarray(a, dtype=np.float64) for a in (geom.ex, geom.ey, geom.sx, geom.sy)]
        if dfield_dev is None:
            dc = (C.c_double * nfield)(*[float(v) for v in dcoef])
            _hip.check(lib.qp_adi_tile_plan_create(ny, nx, nfield, float(r), dc, *[a.ctypes.data for a in host],
                                                   C.byref(self._h)), "qp_adi_tile_plan_create")
        else:
            _hip.check(lib.qp_adi_tile_plan_create_var(ny, nx, nfield, float(r), int(dfield_dev.data_ptr()),
                                                       *[a.ctypes.data for a in host], C.byref(self._h)),
                       "qp_adi_tile_plan_create_var")
        counts = (C.c_int32 * 3)()
        far = C.c_double()
        _hip.check(lib.qp_adi_tile_plan_info(self._h, counts, C.byref(far)), "qp_adi_tile_plan_info")
        self.tile_counts = {"empty": counts[0], "clean": counts[1], "general": counts[2]}
        self.far_coupling = far.value

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.qp_adi_tile_plan_destroy(self._h)
            self._h = C.POINTER(_hip.TilePlan)()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DiffusionOperator:
    """(I - r L_x), (I - r L_y) and friends for one time step size on a batch of fields."""

    def __init__(self, engine: "Engine", nfield: int, dt: float, dcoef=None, dfield=None, allow_fast: bool = True,
                 force_banded: bool = False, allow_tile: bool = True):
        torch = engine.torch
        self.engine = engine
        self.nfield = int(nfield)
        self.dt = float(dt)
        self.r = 0.5 * self.dt / (engine.geom.dx * engine.geom.dx)
        self.dcoef = None if dcoef is None else torch.as_tensor(np.asarray(dcoef, dtype=np.float64), device=engine.device)
        self.dfield = None if dfield is None else torch.as_tensor(
            np.ascontiguousarray(dfield, dtype=np.float64), device=engine.device)
        if (self.dcoef is None) == (self.dfield is None):
            raise ValueError("give exactly one of dcoef / dfield")
        g = engine
        self.desc = _hip.GridDesc.make(g.ny, g.nx, self.nfield, _ptr(g.d_flags), _ptr(g.d_ex), _ptr(g.d_ey), _ptr(g.d_sx),
                                  _ptr(g.d_sy), _ptr(self.dcoef), _ptr(self.dfield))
        # full rectangle + one D per field + one BC per side -> tiled partition-method kernels
        self.rect = None
        sides = rect_side_terms(engine.geom) if (allow_fast and dcoef is not None) else None
        self._sides = sides
        self._pr_cycles: dict = {}
        if sides is not None and self.dt > 0.0:
            with torch.cuda.device(engine.device):
                self.rect = RectPlan(engine.lib, g.ny, g.nx, self.nfield, self.r, np.asarray(dcoef, dtype=float),
                                     sides[0], sides[1], force_banded=force_banded)
        # any other geometry with one D per field -> tiled kernels driven by per-cell codes, unless r*D is too large for
        # 64-cell chunks to decouple (then the per-line kernels below remain)
        self.tile = None
        self.tile_refused = None
        if self.rect is None and allow_fast and allow_tile and self.dt > 0.0:
            with torch.cuda.device(engine.device):
                try:
                    if dcoef is not None:
                        self.tile = TilePlan(engine.lib, engine.geom, self.nfield, self.r, np.asarray(dcoef, dtype=float))
                    else:
                        self.tile = TilePlan(engine.lib, engine.geom, self.nfield, self.r, dfield_dev=self.dfield)
                except _hip.QPHipError as exc:
                    if exc.status != -3:      # QP_ERR_UNSUPPORTED
                        raise
                    self.tile_refused = str(exc)


def _pr_bounds(op: "DiffusionOperator"):
    """(alpha, beta) holding the spectra of H = I/2 - r D Lx and V = I/2 - r D Ly of ``op``, or None when the operator has no
    Peaceman-Rachford cycle: not a full rectangle with one D per field and one BC per side (Lx, Ly would not commute), or a
    boundary diagonal term below zero (H, V no longer bounded below by 1/2)."""
    if (op.rect is None or op._sides is None or min(op._sides[0]) < 0.0 or os.environ.get("QPSIM_CN_PR", "1") == "0"):
        return None
    amax = op.r * float(op.dcoef.max().item())
    if amax <= 0.0:
        return None
    emax = max(op._sides[0])
    return 0.5, 0.5 + amax * max(4.0, 2.0 + emax, 2.0 * emax)      # Gershgorin; 2 e: a direction one cell thick


def _pr_cycle(op: "DiffusionOperator", J: int):
    """The plans of the J-iteration Peaceman-Rachford cycle of ``op`` (cached, at most four cycles), or None."""
    if J in op._pr_cycles:
        return op._pr_cycles[J]
    cycle = None
    bounds = _pr_bounds(op)
    eng = op.engine
    if bounds is not None:
        ps, _ = peaceman_rachford_cycle(bounds[0], bounds[1], int(J))
        dc = op.dcoef.cpu().numpy()
        try:
            with eng.torch.cuda.device(eng.device):
                plans = []
                for p in ps:
                    plans.append(RectPlan.peaceman_rachford(eng.lib, eng.ny, eng.nx, op.nfield, op.r, dc, op._sides[0], p,
                                                            share=plans[0] if plans else None))
            cycle = plans
        except _hip.QPHipError as exc:
            if exc.status != -3:      # QP_ERR_UNSUPPORTED
                raise
    while len(op._pr_cycles) >= 4:      # the cycle length moves one iteration at a time: a few neighbouring lengths stay built
        op._pr_cycles.pop(next(iter(op._pr_cycles)))
    op._pr_cycles[J] = cycle
    return cycle


def _pr_initial_length(op: "DiffusionOperator", reduction: float):
    bounds = _pr_bounds(op)
    if bounds is None:
        return None
    return len(peaceman_rachford_parameters(bounds[0], bounds[1], reduction)[0])


class FrameTicket:
    """Handle of one asynchronous frame download (``Engine.download_frames_async``)."""

    def __init__(self, slot, done_event, numel: int, shape):
        self._slot, self._done, self._numel, self._shape = slot, done_event, numel, shape
        self._frames = None

    def result(self) -> np.ndarray:
        if self._frames is None:
            self._done.synchronize()
            self._frames = self._slot["host"][:self._numel].numpy().reshape(self._shape).copy()
            if self._slot["ticket"] is self:
                self._slot["ticket"] = None
            self._slot = None
        return self._frames


class Engine:
    """Owns the device copies of one geometry and sequences the kernels on torch's current stream."""

    def __init__(self, geom: CompiledGeometry, device: str | int | None = None):
        torch = require_gpu()
        self.torch = torch
        self.lib = _hip.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.geom = geom
        self.ny, self.nx = geom.mask.shape
        self.ncell = self.ny * self.nx
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.device)  # noqa: E731
        self.d_flags = up(geom.flags, np.uint8)
        self.d_ex, self.d_ey = up(geom.ex, np.float64), up(geom.ey, np.float64)
        self.d_sx, self.d_sy = up(geom.sx, np.float64), up(geom.sy, np.float64)
        self.mask_flat = geom.mask.reshape(-1)
        self._full_mask = bool(self.mask_flat.all())
        self._interior_idx = None
        self._ws = torch.empty(int(self.lib.qp_pauli_workspace_bytes()), dtype=torch.uint8, device=self.device)
        # results of the reductions: [max occupation, spare | first-max index, first forbidden index] in ONE 32-byte buffer,
        # so that a guard ticket is one device-to-host copy (a copy is ~4.7 us on the stream: 2 % of a 1024^2 NE = 12 step)
        self._red_buf = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._red_vals = self._red_buf[:2].view(torch.float64)
        self._red_idx = self._red_buf[2:]
        self._scratch = {}
        self._pinned_stream = None
        # made at their first use: download staging rings, guard workspace, pinned guard read-back slots (lone: a ring;
        # ensembles: result buffer + ring per ensemble size), device vectors of per-member generation amounts, staging / status
        # ring of the device-evaluated custom generation
        self._dl_slots = None
        self._guard_ws = None
        self._guard_slots = None
        self._mguard: dict = {}
        self._amount_vectors: dict = {}
        self._gen_slots = None

    # -- plumbing -------------------------------------------------------------------------------------------
    @property
    def stream(self) -> int:
        """hipStream_t of torch's current stream; `pin_stream()` caches it for the duration of a time loop (the lookup costs
        ~4 us and a step of a small problem issues dozens of launches)."""
        if self._pinned_stream is not None:
            return self._pinned_stream
        return int(self.torch.cuda.current_stream(self.device).cuda_stream)

    def pin_stream(self, on: bool = True) -> None:
        self._pinned_stream = int(self.torch.cuda.current_stream(self.device).cuda_stream) if on else None

    def empty(self, *shape):
        return self.torch.empty(*shape, dtype=self.torch.float64, device=self.device)

    def scratch(self, key: str, numel: int):
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < numel:
            buf = self.empty(int(numel))
            self._scratch[key] = buf
        return buf

    def upload_packed(self, packed: np.ndarray):
        """[nfield, n_interior] host array (reference layout) -> [nfield, ncell] device planes, holes = 0."""
        packed = self.torch.as_tensor(np.ascontiguousarray(packed, dtype=np.float64), device=self.device)
        if self._full_mask:
            return packed
        full = self.torch.zeros((packed.shape[0], self.ncell), dtype=self.torch.float64, device=self.device)
        full[:, self._interior_index()] = packed          # scatter on the device: the host only sends the packed values
        return full

    def download_packed(self, planes) -> np.ndarray:
        if self._full_mask:
            return planes.detach().cpu().numpy()
        return planes.detach()[:, self._interior_index()].cpu().numpy()

    def _interior_index(self):
        if self._interior_idx is None:
            self._interior_idx = self.torch.as_tensor(np.flatnonzero(self.mask_flat), device=self.device)
        return self._interior_idx

    def download_frames(self, planes, scale: float = 1.0, full_shape=None, offset=(0, 0)) -> np.ndarray:
        """[nfield, ncell] device planes -> host [nfield, ny, nx] frames, NaN outside the mask (reconstruct_field), times
        `scale`; the padding happens on the device, the host only receives.  With ``full_shape`` the engine grid is the
        window at ``offset`` of a larger all-NaN frame (the solver crops padded geometries onto their bounding box)."""
        return self.download_frames_async(planes, scale, full_shape, offset).result()

    def download_frames_async(self, planes, scale: float = 1.0, full_shape=None, offset=(0, 0)) -> "FrameTicket":
        """Same frames, but the call only ENQUEUES: the NaN padding runs on the compute stream into a staging buffer, the
        device-to-host copy runs on a side stream into pinned memory, and the compute stream goes on with the next time
        step.  ``ticket.result()`` waits for that copy and returns the frames as a fresh NumPy array.  A small ring of
        staging / pinned buffer pairs is reused (one ring for single planes, one for plane sets); taking a slot whose
        previous ticket is still open completes that ticket first (its copy has had a whole store interval to finish)."""
        torch = self.torch
        planes = planes.reshape(-1, self.ncell)
        n = planes.shape[0]
        shape = (n, self.ny, self.nx) if full_shape is None else (n,) + tuple(full_shape)
        numel = int(np.prod(shape))
        if self._dl_slots is None:
            self._dl_stream = torch.cuda.Stream(device=self.device)
            # Two rings: a store point of a full-physics run enqueues up to four downloads (integrated frame, state, phonon
            # planes, phonon sum) - two of one plane, two of NE / Nw planes.  Each ring holds two store points' worth of its
            # size class, so a slot is recycled only after a whole store interval (and small frames do not grow to the
            # size of the state: 2 x 2 large staging pairs instead of 3 of everything).
            self._dl_slots = {cls: [{"dev": None, "host": None, "ticket": None} for _ in range(4)] for cls in ("small", "large")}
            self._dl_next = {"small": 0, "large": 0}
        ring_name = "small" if n <= 1 else "large"
        ring = self._dl_slots[ring_name]
        slot = ring[self._dl_next[ring_name]]
        self._dl_next[ring_name] = (self._dl_next[ring_name] + 1) % len(ring)
        if slot["ticket"] is not None:
            slot["ticket"].result()                    # frees the slot (keeps the frames inside the ticket)
        if slot["dev"] is None or slot["dev"].numel() < numel:
            slot["dev"] = self.empty(numel)
            slot["host"] = torch.empty(numel, dtype=torch.float64).pin_memory()
        stage = slot["dev"][:numel]
        compute = torch.cuda.current_stream(self.device)
        embed = full_shape is not None and tuple(full_shape) != (self.ny, self.nx)
        pad_out = self.scratch("nan_pad", n * self.ncell)[:n * self.ncell] if embed else stage
        _hip.check(self.lib.qp_nan_pad(_ptr(self.d_flags), self.ncell, n, _ptr(planes), float(scale), _ptr(pad_out),
                                       self.stream), "qp_nan_pad")
        if embed:
            full = stage.view(shape)
            full.fill_(float("nan"))
            full[:, offset[0]:offset[0] + self.ny, offset[1]:offset[1] + self.nx] = pad_out.view(n, self.ny, self.nx)
        ready = torch.cuda.Event()
        ready.record(compute)
        self._dl_stream.wait_event(ready)
        with torch.cuda.stream(self._dl_stream):
            slot["host"][:numel].copy_(stage, non_blocking=True)
        done = torch.cuda.Event()
        done.record(self._dl_stream)
        ticket = FrameTicket(slot, done, numel, shape)
        slot["ticket"] = ticket
        return ticket

    def masked_sum(self, plane) -> float:
        """Sum of one plane over the cells inside the mask (holes hold 0 by invariant)."""
        return float(plane.sum().item())

    # -- diffusion --------------------------------------------------------------------------------------------
    def stencil(self, op: DiffusionOperator, u, out, c0, cx, cy, cs, rin=None, cr=0.0, norm_out=None, norms_out=None):
        """out = c0 u + cx rLx u + cy rLy u + cs rD S + cr rin; with ``norm_out`` (device scalar) also max |out|, with
        ``norms_out`` (``nfield`` device values) max |out| of every field.  Full rectangles with one boundary condition per
        side use the plan's own operator (no per-cell geometry arrays); other geometries the general kernel (boundary terms
        read only at boundary cells); the norms are formed in the same pass."""
        if norms_out is not None:
            if op.rect is not None:
                _hip.check(self.lib.qp_adi_rect_combine_norms(op.rect.handle, _ptr(u), _ptr(rin), _ptr(out), c0, cx, cy, cs,
                                                              cr, _ptr(self._ws), _ptr(norms_out), self.stream),
                           "qp_adi_rect_combine_norms")
            else:
                _hip.check(self.lib.qp_stencil_combine_norms(C.byref(op.desc), op.r, _ptr(u), _ptr(rin), _ptr(out), c0, cx,
                                                             cy, cs, cr, _ptr(self._ws), _ptr(norms_out), self.stream),
                           "qp_stencil_combine_norms")
            return
        if op.rect is not None:
            _hip.check(self.lib.qp_adi_rect_combine(op.rect.handle, _ptr(u), _ptr(rin), _ptr(out), c0, cx, cy, cs, cr,
                                                    _ptr(self._ws) if norm_out is not None else 0, _ptr(norm_out),
                                                    self.stream), "qp_adi_rect_combine")
            return
        _hip.check(self.lib.qp_stencil_combine_norm(C.byref(op.desc), op.r, _ptr(u), _ptr(rin), _ptr(out), c0, cx, cy, cs,
                                                    cr, _ptr(self._ws) if norm_out is not None else 0, _ptr(norm_out),
                                                    self.stream), "qp_stencil_combine")

    def sweep(self, op: DiffusionOperator, direction: int, rhs, x):
        scr = self.scratch("thomas", 2 * op.nfield * self.ncell)
        _hip.check(self.lib.qp_implicit_sweep(C.byref(op.desc), op.r, direction, _ptr(rhs), _ptr(x), _ptr(scr),
                                              self.stream), "qp_implicit_sweep")

    def adi_steps(self, op: DiffusionOperator, u, nsteps: int = 1):
        """`nsteps` consecutive Peaceman-Rachford steps in place (fast path carries the state between steps)."""
        if op.rect is not None:
            _hip.check(self.lib.qp_adi_rect_steps(op.rect.handle, _ptr(u), int(nsteps), self.stream), "qp_adi_rect_steps")
            return u
        if op.tile is not None:
            _hip.check(self.lib.qp_adi_tile_steps(op.tile.handle, _ptr(u), int(nsteps), self.stream), "qp_adi_tile_steps")
            return u
        for _ in range(int(nsteps)):
            self.adi_step(op, u)
        return u

    def adi_step(self, op: DiffusionOperator, u, out=None):
        """Peaceman-Rachford step: (I-rLx)u* = (I+rLy)u + rS; (I-rLy)u' = (I+rLx)u* + rS.  In place unless `out`."""
        if op.rect is not None or op.tile is not None:
            if out is not None:
                out.copy_(u)
                u = out
            return self.adi_steps(op, u, 1)
        n = op.nfield * self.ncell
        t1 = self.scratch("adi_t1", n).view(op.nfield, self.ncell)
        t2 = self.scratch("adi_t2", n).view(op.nfield, self.ncell)
        self.stencil(op, u, t1, 1.0, 0.0, 1.0, 1.0)
        self.sweep(op, 0, t1, t1)
        self.stencil(op, t1, t2, 1.0, 1.0, 0.0, 1.0)
        res = u if out is None else out
        self.sweep(op, 1, t2, res)
        return res

    def _precondition(self, op: DiffusionOperator, res) -> None:
        """res <- (I - rLy)^-1 (I - rLx)^-1 res: the ADI factorisation applied as preconditioner."""
        if op.rect is not None:
            _hip.check(self.lib.qp_adi_rect_solve(op.rect.handle, _ptr(res), self.stream), "qp_adi_rect_solve")
        elif op.tile is not None:
            _hip.check(self.lib.qp_adi_tile_solve(op.tile.handle, _ptr(res), self.stream), "qp_adi_tile_solve")
        else:
            self.sweep(op, 0, res, res)
            self.sweep(op, 1, res, res)

    def cn_contraction_bound(self, op: DiffusionOperator) -> float:
        """Upper estimate of the contraction factor of the plain ADI-preconditioned Richardson iteration,
        (a lx / (1 + a lx)) (a ly / (1 + a ly)) with a = r max D and l = the Gershgorin bound of -L_dir (4 + boundary term)."""
        cached = getattr(op, "_cn_rho", None)
        if cached is not None:
            return cached
        dmax = float(op.dcoef.max().item()) if op.dcoef is not None else float(op.dfield.max().item())
        a = op.r * dmax
        lx = a * (4.0 + float(self.geom.ex.max())) if self.nx > 1 else a * float(self.geom.ex.max())
        ly = a * (4.0 + float(self.geom.ey.max())) if self.ny > 1 else a * float(self.geom.ey.max())
        op._cn_rho = (lx / (1.0 + lx)) * (ly / (1.0 + ly))
        return op._cn_rho

    # contraction bound from which the Chebyshev semi-iteration replaces plain Richardson: at rho = 0.3 (r D = 0.3, the
    # physical step sizes) it converges like 0.09^k instead of 0.3^k - 6 instead of 12 iterations on rough data
    CHEBYSHEV_FROM = 0.02

    def cn_exact_step(self, op: DiffusionOperator, u, rtol: float = 1e-13, max_iter: int = 2000):
        """Unsplit CN step (I - rL)u' = (I + rL)u + 2rS by ADI-preconditioned iteration, in place.

        The ADI factorisation M = (I-rLx)(I-rLy) differs from A = I - rL by r^2 Lx Ly, so
        v <- v + M^-1 (R - A v) contracts with factor rho(Tx Ty) < 1 (Tx = (I-rLx)^-1 rLx).  The starting
        guess is the ADI step itself; on strips with reflective side walls it is already exact and no iteration runs.
        Whenever the contraction bound rho = (a lx / (1 + a lx)) (a ly / (1 + a ly)) exceeds CHEBYSHEV_FROM, the same
        residual / preconditioner kernels are driven by the Chebyshev semi-iteration on the interval [1 - rho, 1] that
        holds the spectrum of M^-1 A (half the iterations at r D = 0.3, a tenth at r D = 10); if the residual ever grows
        (non-commuting Lx, Ly on an exotic mask) the plain iteration takes over for that operator.
        Raises ``RuntimeError`` when ``rtol`` is not reached within ``max_iter`` iterations - the reference's SuperLU solve
        is exact for any dt, so a silent partial solve would not be a drop-in.  Returns the number of iterations.
        """
        n = op.nfield * self.ncell
        R = self.scratch("cn_R", n).view(op.nfield, self.ncell)
        res = self.scratch("cn_res", n).view(op.nfield, self.ncell)
        v = self.scratch("cn_v", n).view(op.nfield, self.ncell)
        # [max |R_k|, max |(R - A v)_k|] of every plane k, read back in one transfer per look: the iteration is accepted
        # plane by plane (`_cn_plane_error`) - energy planes differ by many decades, and maxima over the whole batch would
        # never look at a plane far below the largest one
        nf = op.nfield
        norms = self.scratch("cn_norms", 2 * nf)[:2 * nf]
        self.stencil(op, u, R, 1.0, 1.0, 1.0, 2.0, norms_out=norms[:nf])
        rho = self.cn_contraction_bound(op)
        # Full rectangles (commuting Lx, Ly): one cycle of Peaceman-Rachford iterations with Jordan's parameters on the
        # spectrum of I/2 - r D L_dir - 8 plane transfers per iteration against 13 of the preconditioned iteration below and
        # a larger reduction per iteration (r D = 0.3: x45 against x11).  The residual is checked afterwards; whatever is
        # left (worst-case bound missed, e.g. rounding at very small rtol) is polished by the iteration below.
        # The cycle length follows the data.  It starts at the length whose worst-case factor is 100 rtol (the old field is
        # an O(r D) guess), drops by one iteration whenever a cycle ended 30 times below the tolerance (smooth physical
        # fields need 5-6 iterations where random data needs 8 at r D = 0.3) and grows by one when a cycle missed it -
        # after which shorter cycles are not tried again for 8, 16, 32 ... steps (doubling with every miss).
        J = None
        if rho > self.CHEBYSHEV_FROM:
            J = getattr(op, "_pr_J", None)
            if J is None:
                J = op._pr_J = _pr_initial_length(op, max(100.0 * rtol, 1e-15))
                op._pr_hold, op._pr_backoff = 0, 8
        cycle = _pr_cycle(op, J) if J is not None else None
        if cycle is not None:
            # in place on u (the right-hand side R is already formed): no copies when the cycle suffices
            handles = (C.POINTER(_hip.RectPlan) * len(cycle))(*[plan.handle for plan in cycle])
            _hip.check(self.lib.qp_adi_rect_pr_cycle(handles, len(cycle), _ptr(u), _ptr(R), self.stream),
                       "qp_adi_rect_pr_cycle")
            # the check needs the NORM of the residual only (its plane is formed again by the polishing loop if the check
            # fails): no output plane
            self.stencil(op, u, None, -1.0, 1.0, 1.0, 0.0, rin=R, cr=1.0, norms_out=norms[nf:])
            err = self._cn_plane_error(norms)
            if err <= rtol:
                if op._pr_hold > 0:
                    op._pr_hold -= 1
                elif err <= rtol / 30.0 and J > 2:
                    op._pr_J = J - 1
                return len(cycle)
            op._pr_J, op._pr_hold = min(J + 1, 24), op._pr_backoff
            op._pr_backoff = min(2 * op._pr_backoff, 512)
            v.copy_(u)
        else:
            v.copy_(u)
            self.adi_step(op, v)
        if rho > self.CHEBYSHEV_FROM and not getattr(op, "_cn_plain", False):
            its = self._cn_chebyshev(op, R, res, v, norms, rho, rtol, max_iter)
            if its >= 0:
                u.copy_(v)
                return its
            op._cn_plain = True       # residual grew: spectrum outside the assumed interval; v holds the best iterate
            its = -its
        else:
            its = 0
        # The iteration count hardly changes from one step to the next (same operator, smooth data), and looking at
        # the residual costs a device-to-host round trip: the count of the previous call runs blind, then every
        # iteration is checked.  (Running an iteration more than strictly needed only lowers the residual further.)
        blind = its + getattr(op, "_cn_its", 0)
        first = its
        while True:
            look = its >= blind or its >= max_iter
            self.stencil(op, v, res, -1.0, 1.0, 1.0, 0.0, rin=R, cr=1.0, norms_out=norms[nf:] if look else None)
            if look:
                err = self._cn_plane_error(norms)
                if err <= rtol:
                    break
                if its >= max_iter:
                    raise RuntimeError(
                        f"exact-CN iteration did not reach rtol={rtol:g} in {max_iter} iterations (residual "
                        f"{err:.3g} of its plane, estimated contraction factor {rho:.4f}); the step is too stiff "
                        "(r D = dt D / (2 dx^2) very large) - reduce dt or use diffusion_scheme='adi'.")
            self._precondition(op, res)
            _hip.check(self.lib.qp_axpy(n, 1.0, _ptr(res), _ptr(v), self.stream), "qp_axpy")
            its += 1
        # next call: one iteration fewer runs blind when this one was already far below the tolerance at its first look
        done = its - first
        op._cn_its = done - 1 if (its == blind and done > 0 and err <= 0.01 * rtol) else done
        u.copy_(v)
        return its

    def _cn_chebyshev(self, op: DiffusionOperator, R, res, v, norms, rho: float, rtol: float, max_iter: int) -> int:
        """Chebyshev semi-iteration on M^-1 A (spectrum in [1 - rho, 1]) from the iterate in ``v``.  Returns the iteration
        count, or minus the count when the residual grew (the caller continues with the plain iteration)."""
        n = op.nfield * self.ncell
        d = self.scratch("cn_d", n)
        lmin, lmax = 1.0 - rho, 1.0
        theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        sigma = theta / delta
        rk = 1.0 / sigma
        blind = getattr(op, "_cn_cheb_its", 0)
        best = float("inf")
        its = 0
        while True:
            look = its >= blind or its >= max_iter
            self.stencil(op, v, res, -1.0, 1.0, 1.0, 0.0, rin=R, cr=1.0, norms_out=norms[op.nfield:] if look else None)
            if look:
                err = self._cn_plane_error(norms)
                if err <= rtol:
                    break
                if err > 10.0 * best:
                    return -max(its, 1)
                best = min(best, err)
                if its >= max_iter:
                    raise RuntimeError(
                        f"exact-CN (Chebyshev) iteration did not reach rtol={rtol:g} in {max_iter} iterations (residual "
                        f"{err:.3g} of its plane, contraction bound {rho:.6f}); reduce dt or use "
                        "diffusion_scheme='adi'.")
            self._precondition(op, res)
            if its == 0:
                c1, c2 = 1.0 / theta, 0.0
            else:
                rn = 1.0 / (2.0 * sigma - rk)
                c1, c2 = 2.0 * rn / delta, rn * rk
                rk = rn
            _hip.check(self.lib.qp_cheb_update(n, c1, _ptr(res), c2, _ptr(d), _ptr(v), self.stream), "qp_cheb_update")
            its += 1
        op._cn_cheb_its = its - 1 if (its == blind and its > 0 and err <= 0.01 * rtol) else its
        return its

    @staticmethod
    def _cn_plane_error(norms) -> float:
        """max_k (max |res_k| / max |R_k|) from ``norms`` = [max |R_k| ..., max |res_k| ...] on the device (one transfer):
        the residual of the exact-CN iteration relative to its own plane.  A plane whose right-hand side is zero must have
        a zero residual (inf otherwise).  A residual below the smallest normal number (2.2e-308) counts as zero, whatever
        the plane's own scale: a plane whose right-hand side lies below about 2.2e-308 / rtol (2e-295 at the default rtol)
        is in effect not held to rtol - subnormal arithmetic cannot express that ratio.  A non-finite right-hand side or
        residual raises."""
        h = norms.tolist()      # plain floats: a look costs the transfer, not array arithmetic (one plane is the common case)
        nf = len(h) // 2
        worst = 0.0
        for scale, err in zip(h[:nf], h[nf:]):
            if not (math.isfinite(err) and math.isfinite(scale)):
                raise FloatingPointError("exact-CN iteration diverged (non-finite right-hand side or residual)")
            if err >= _TINY:
                worst = max(worst, err / scale if scale > 0.0 else math.inf)
        return worst

    def _absmax_into(self, a, out) -> None:
        _hip.check(self.lib.qp_absmax(_ptr(a), a.numel(), _ptr(self._ws), _ptr(out), self.stream), "qp_absmax")

    def absmax(self, a) -> float:
        _hip.check(self.lib.qp_absmax(_ptr(a), a.numel(), _ptr(self._ws), _ptr(self._red_vals), self.stream), "qp_absmax")
        return float(self._red_vals[0].item())

    # -- collisions, generation, reductions -------------------------------------------------------------------
    def make_collision_tables(self, kr0, ks0, rho, idx_diff, idx_sum, sign, cls_packed=None, allow_fast=True,
                              kernel: str = "auto", gap_params: dict | None = None, members: int = 1,
                              member_classes: bool = False, pad_bins: bool = False, wide_bins: bool = False):
        """Upload per-gap-class tables ([C,NE,NE], [C,NE]) and maps; returns an opaque handle.

        ``kernel``: "auto" | "generic" | "wave" | "wave_unstructured" forces a collision kernel (tests, A/B timing).
        ``gap_params`` (gap classes only): ``dict(E=E_bins, gaps=class_gaps, tau_r=, tau_s=, T_c=)`` - lets the register
        kernel form K^r_0, K^s_0 per pixel from gap-independent tables (they are separable in the gap).
        ``members`` > 1: the class map is repeated over an ensemble laid out [member][cell] (same tables for every member).
        ``member_classes``: the C tables are one set per ensemble member instead (``QP_COLL_MEMBER_CLASSES``: ``members``
        = C, class m = the cells of member m).  The register kernels read them for NE = 4 ... 16 when a member's cell count
        is a multiple of 64, the one-pass kernel for NE = 30, 32, 40, 50 when it is a multiple of 256 (the handle then
        carries ``ks0_diag`` / ``kr0_anti2`` per member and reports ``kernel == "register"``); other shapes and sizes run
        the one-wave-per-pixel kernel through the class map.
        ``pad_bins`` (opt-in, ``QP_COLL_PAD_BINS``): a size NE = 17 ... 49 without a kernel of its own
        (``qp_collision_padded_ceiling(NE) != 0``) with structured symmetric maps and one class or member classes runs the
        one-pass kernel of the next instantiated size on its live bins; every array keeps the live size.  Sizes with their
        own kernel, NE >= 51 and gap classes plan exactly as without it.
        ``wide_bins`` (opt-in, ``QP_COLL_WIDE_BINS``): NE = 65 ... 128 with at most 512 phonon bins and symmetric tables
        (``qp_collision_wide_available``) runs the two-bins-per-lane wave kernel instead of the generic kernel, for one
        class, gap classes and member classes alike: ``kernel == "wave"``, ``fast``, and no ``2 nw ncell`` accumulator
        planes are allocated.  Every other size plans exactly as without it.

        Every rule is ``collision_tables.plan_collision_tables`` (host only); this method uploads its arrays and fills the
        struct.  ``handle["kernel"]`` is the family the table set can reach (``collision_tables.CollisionPlan``)."""
        plan = collision_tables.plan_collision_tables(self.lib, self.ncell, self.mask_flat, kr0, ks0, rho, idx_diff, idx_sum,
                                                      sign, cls_packed, allow_fast, kernel, gap_params, members,
                                                      member_classes, pad_bins, wide_bins)
        h = {name: None if a is None else self.torch.as_tensor(a, device=self.device) for name, a in plan.arrays.items()}
        h.update(ne=plan.ne, nclass=plan.nclass, nw=plan.nw, merged_slots=plan.merged_slots, symmetric=plan.symmetric,
                 member_classes=plan.member_classes, kernel=plan.kernel, fast=plan.fast, pair=plan.pair,
                 struct=plan.struct({name: _ptr(t) for name, t in h.items()}))
        return h

    def collision_scratch(self, tables, nc: int, en_r, en_s, update_phonons):
        """What a collision call over ``nc`` pixels needs beside its planes (``collision_tables.scratch_planes``): the phonon
        accumulator planes of the kernels that are not ``fast``, the merged-bin stash of the register kernels, or None."""
        planes = collision_tables.scratch_planes(tables, en_r, en_s, update_phonons)
        return self.scratch("coll_acc", 2 * planes * nc) if planes else None

    def _guard_workspace(self, nc: int, min_bytes: int = 0):
        """The workspace of a guarded collision call over ``nc`` pixels (at least ``min_bytes``), grown when too small.  One
        buffer serves the lone ``*_guarded`` calls and, through ``_members_ws``, the ``*_members`` calls and the per-member
        guard: it only ever grows, and every user runs on the engine's one stream, one call after the other."""
        nbytes = max(int(self.lib.qp_collision_guard_workspace_bytes(nc)), int(min_bytes))
        if self._guard_ws is None or self._guard_ws.numel() < nbytes:
            self._guard_ws = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.device)
        return self._guard_ws

    def collide(self, tables, state, state_out, phonon, dE, dt, en_r, en_s, update_phonons, ncell: int | None = None,
                flags=None):
        """One collision update; ``ncell`` / ``flags`` override the engine's grid (ensembles: members x cells)."""
        nc = self.ncell if ncell is None else int(ncell)
        acc = self.collision_scratch(tables, nc, en_r, en_s, update_phonons)
        _hip.check(self.lib.qp_collision_step(C.byref(tables["struct"]), _ptr(self.d_flags if flags is None else flags), nc, _ptr(state),
                                              _ptr(state_out), _ptr(phonon), _ptr(acc), float(dE), float(dt),
                                              int(bool(en_r)), int(bool(en_s)), int(bool(update_phonons)), self.stream),
                   "qp_collision_step")

    def collide_guarded(self, tables, state, state_out, phonon, dE, dt, en_r, en_s, update_phonons, floor: float,
                        ncell: int | None = None, flags=None):
        """``collide`` + the Pauli-guard reduction of ``state_out`` in one library call (``qp_collision_step_guarded``): the
        single-pass register kernels reduce the statistics of the new densities while they are still in registers.
        Returns a ticket for ``pauli_stats_result`` (asynchronous read-back, as ``pauli_stats_launch``)."""
        nc = self.ncell if ncell is None else int(ncell)
        acc = self.collision_scratch(tables, nc, en_r, en_s, update_phonons)
        ws = self._guard_workspace(nc)
        hv, hi, ev = self._guard_slot()
        _hip.check(self.lib.qp_collision_step_guarded(
            C.byref(tables["struct"]), _ptr(self.d_flags if flags is None else flags), nc, _ptr(state), _ptr(state_out),
            _ptr(phonon), _ptr(acc), float(dE), float(dt), int(bool(en_r)), int(bool(en_s)), int(bool(update_phonons)),
            float(floor), _ptr(ws), _ptr(self._red_vals), _ptr(self._red_idx), self.stream), "qp_collision_step_guarded")
        self._guard_copy(hv)
        ev.record(self.torch.cuda.current_stream(self.device))
        return hv, hi, ev, nc, tables["ne"]

    def collide_pair_guarded(self, tables, state, state_out, phonon, dE, dt_first, dt_second, gen_amount, en_r, en_s,
                             update_phonons, floor: float, ncell: int | None = None, flags=None):
        """The closing collision half-step of one Strang step, its Pauli guard, the constant / pulse generation term of the
        next step and that step's opening half-step as ONE pass over the state (``qp_collision_double_step_guarded``; only
        call when ``tables["pair"]``).  Returns the guard ticket of the step that closes (as ``collide_guarded``)."""
        nc = self.ncell if ncell is None else int(ncell)
        ws = self._guard_workspace(nc)
        hv, hi, ev = self._guard_slot()
        _hip.check(self.lib.qp_collision_double_step_guarded(
            C.byref(tables["struct"]), _ptr(self.d_flags if flags is None else flags), nc, _ptr(state), _ptr(state_out),
            _ptr(phonon), float(dE), float(dt_first), float(dt_second), float(gen_amount), int(bool(en_r)), int(bool(en_s)),
            int(bool(update_phonons)), float(floor), _ptr(ws), _ptr(self._red_vals), _ptr(self._red_idx), self.stream),
            "qp_collision_double_step_guarded")
        self._guard_copy(hv)
        ev.record(self.torch.cuda.current_stream(self.device))
        return hv, hi, ev, nc, tables["ne"]

    GUARD_LAG = 3       # guard tickets a time loop may keep outstanding (GUARD_LAG + 1 pinned read-back slots)

    def _guard_slot(self):
        """Next pinned read-back slot of the guard.  A time loop looks at the guard of step k only after step k + GUARD_LAG
        has been enqueued, so the device always has queued work while the host reads (measured: lags 1, 3 and 6 give the
        same 0.067 / 0.084 / 0.455 ms per coupled NE = 12 step at 64^2 / 256^2 / 1024^2 - the loop is not host-bound)."""
        torch = self.torch
        if self._guard_slots is None:
            self._guard_slots, self._guard_host = [], {}
            for _ in range(self.GUARD_LAG + 1):
                buf = torch.empty(4, dtype=torch.int64).pin_memory()          # host image of _red_buf
                hv, hi = buf[:2].view(torch.float64), buf[2:]
                self._guard_host[hv.data_ptr()] = buf
                self._guard_slots.append((hv, hi, torch.cuda.Event()))
            self._guard_next = 0
        slot = self._guard_slots[self._guard_next]
        self._guard_next = (self._guard_next + 1) % len(self._guard_slots)
        return slot

    def _guard_copy(self, hv) -> None:
        """Asynchronous read-back of the reduction results into the pinned slot whose value view is ``hv`` (one copy)."""
        self._guard_host[hv.data_ptr()].copy_(self._red_buf, non_blocking=True)

    def add_constant(self, state, amount: float):
        _hip.check(self.lib.qp_add_constant(_ptr(self.d_flags), self.ncell, state.shape[0], _ptr(state), float(amount),
                                            self.stream), "qp_add_constant")

    def add_scaled(self, state, g, scale: float):
        _hip.check(self.lib.qp_add_scaled(state.numel(), _ptr(state), _ptr(g), float(scale), self.stream), "qp_add_scaled")

    def _generation_slot(self, nbytes: int, nlaunch: int):
        """Next slot of the generation ring, GUARD_LAG + 1 beside the guard's: a pinned staging buffer with its device
        image for the slot tables and member lists of a step, the two status words per launch on the device with their
        pinned read-back image, and the event recorded behind that read-back.  A time loop reads the status of step k
        before it enqueues step k + GUARD_LAG + 1, so a slot is free when its turn comes again (its event is waited for
        all the same)."""
        torch = self.torch
        if self._gen_slots is None:
            self._gen_slots = [{"host": None, "dev": None, "status_host": None, "status_dev": None,
                                "event": torch.cuda.Event(), "open": False} for _ in range(self.GUARD_LAG + 1)]
            self._gen_next = 0
        slot = self._gen_slots[self._gen_next]
        self._gen_next = (self._gen_next + 1) % len(self._gen_slots)
        if slot["open"]:
            slot["event"].synchronize()
        if slot["host"] is None or slot["host"].numel() < nbytes:
            slot["host"] = torch.empty(max(nbytes, 1024), dtype=torch.uint8).pin_memory()
            slot["dev"] = torch.empty(max(nbytes, 1024), dtype=torch.uint8, device=self.device)
        if slot["status_host"] is None or slot["status_host"].numel() < 2 * nlaunch:
            slot["status_host"] = torch.zeros(2 * nlaunch, dtype=torch.int32).pin_memory()
            slot["status_dev"] = torch.zeros(2 * nlaunch, dtype=torch.int32, device=self.device)
        return slot

    def add_generation_expr(self, state, window, launches, dt: float, members: int, flags):
        """state[bin][m][c] += dt * g on the interior cells of the listed members, g evaluated by ``qp_add_generation_expr``
        (custom generation in the device subset, ``device_expr``).  ``launches``: ``(words, slot table [NE, nslot], member
        list or None for all)`` per distinct program; ``window`` = (ny_full, nx_full, row0, col0) places the engine grid in
        the full mask whose pixel centres are x, y.  The tables and lists go up in one asynchronous copy from pinned
        memory; the status words of all launches come back in one, as the guard's do.  Returns a ticket for
        ``generation_status``."""
        members = int(members)
        ne = state.numel() // (self.ncell * members)
        offsets, nbytes = [], 0
        for words, table, listed in launches:
            ids = None if listed is None else np.asarray(listed, dtype=np.int32)
            offsets.append((nbytes, ids, nbytes + table.nbytes))
            nbytes += table.nbytes + (0 if ids is None else 8 * ((ids.nbytes + 7) // 8))
        slot = self._generation_slot(nbytes, len(launches))
        staging = slot["host"].numpy()
        for (words, table, _), (at, ids, ids_at) in zip(launches, offsets):
            staging[at:at + table.nbytes] = np.ascontiguousarray(table, dtype=np.float64).reshape(-1).view(np.uint8)
            if ids is not None:
                staging[ids_at:ids_at + ids.nbytes] = ids.view(np.uint8)
        if nbytes:
            slot["dev"][:nbytes].copy_(slot["host"][:nbytes], non_blocking=True)
        base, status = _ptr(slot["dev"]), _ptr(slot["status_dev"])
        ny_full, nx_full, row0, col0 = (int(v) for v in window)
        for k, ((words, table, _), (at, ids, ids_at)) in enumerate(zip(launches, offsets)):
            words = np.ascontiguousarray(words, dtype=np.uint32)
            prog = _hip.GenerationProgram.make(self.ny, self.nx, ny_full, nx_full, row0, col0, ne, table.shape[1], words.size,
                                               words.ctypes.data, base + at if table.shape[1] else 0)
            _hip.check(self.lib.qp_add_generation_expr(C.byref(prog), _ptr(flags), members, 0 if ids is None else base + ids_at,
                                                       members if ids is None else ids.size, _ptr(state), float(dt),
                                                       status + 8 * k, self.stream), "qp_add_generation_expr")
        n = 2 * len(launches)
        slot["status_host"][:n].copy_(slot["status_dev"][:n], non_blocking=True)
        slot["event"].record(self.torch.cuda.current_stream(self.device))
        slot["open"] = True
        return slot, len(launches)

    def generation_status(self, ticket) -> list:
        """[(a value was not finite, a value was negative)] per launch of an ``add_generation_expr`` ticket."""
        slot, nlaunch = ticket
        slot["event"].synchronize()
        slot["open"] = False
        words = slot["status_host"][:2 * nlaunch].numpy()
        return [(bool(words[2 * k]), bool(words[2 * k + 1])) for k in range(nlaunch)]

    def pauli_stats(self, state, tables, floor: float):
        """(max occupation, (energy index, cell index), forbidden (energy, cell) or None)."""
        return self.pauli_stats_result(self.pauli_stats_launch(state, tables, floor))

    def pauli_stats_launch(self, state, tables, floor: float, ncell: int | None = None, flags=None):
        """Enqueue the Pauli-guard reduction and an asynchronous read-back into pinned memory; returns a ticket for
        ``pauli_stats_result``.  GUARD_LAG + 1 tickets may be outstanding, so a time loop can enqueue the next steps
        before it looks at an earlier step's guard and the GPU never waits for the host round trip."""
        torch = self.torch
        hv, hi, ev = self._guard_slot()
        nc = self.ncell if ncell is None else int(ncell)
        _hip.check(self.lib.qp_pauli_stats(_ptr(state), _ptr(tables["rho"]), _ptr(tables["cls"]),
                                           _ptr(self.d_flags if flags is None else flags), tables["ne"], tables["nclass"],
                                           nc, float(floor), _ptr(self._ws), _ptr(self._red_vals), _ptr(self._red_idx),
                                           self.stream), "qp_pauli_stats")
        self._guard_copy(hv)
        ev.record(torch.cuda.current_stream(self.device))
        return hv, hi, ev, nc, tables["ne"]

    def pauli_stats_result(self, ticket):
        hv, hi, ev, nc, ne = ticket
        ev.synchronize()
        mx = float(hv[0])
        i0, i1 = int(hi[0]), int(hi[1])
        i0 = min(max(i0, 0), nc * int(ne) - 1)
        top = (i0 // nc, i0 % nc)
        forb = None if i1 < 0 else (i1 // nc, i1 % nc)
        return mx, top, forb

    # -- ensembles: `members` problems of this geometry laid out [bin][member][cell]; the guard is reduced per member ----
    def _members_guard_buffers(self, members: int):
        """Device result buffer [vals | argmax, forbidden per member] (members x 24 bytes: one read-back copy per ticket) and
        its ring of GUARD_LAG + 1 pinned host images, per ensemble size."""
        torch = self.torch
        cache = self._mguard
        if members not in cache:
            dev = torch.zeros(3 * members, dtype=torch.int64, device=self.device)
            ring = [(torch.empty(3 * members, dtype=torch.int64).pin_memory(), torch.cuda.Event())
                    for _ in range(self.GUARD_LAG + 1)]
            cache[members] = {"dev": dev, "ring": ring, "next": 0}
        return cache[members]

    def _members_ws(self, ncell_member: int, members: int):
        return self._guard_workspace(ncell_member * members,
                                     self.lib.qp_pauli_members_workspace_bytes(ncell_member, members))

    def _members_launch(self, tables, ncell_member: int, members: int, call):
        """Runs ``call(ws, out_vals, out_idx)`` and enqueues the asynchronous read-back of its per-member results."""
        b = self._members_guard_buffers(members)
        host, ev = b["ring"][b["next"]]
        b["next"] = (b["next"] + 1) % len(b["ring"])
        dev = b["dev"]
        call(self._members_ws(ncell_member, members), _ptr(dev[:members]), _ptr(dev[members:]))
        host.copy_(dev, non_blocking=True)
        ev.record(self.torch.cuda.current_stream(self.device))
        return host, ev, int(ncell_member), int(members), int(tables["ne"])

    def pauli_stats_members_launch(self, state, tables, floor: float, ncell_member: int, members: int, flags):
        """Per-member Pauli guard (``qp_pauli_stats_members``) + read-back; ticket for ``pauli_stats_members_result``."""
        def call(ws, vals, idx):
            _hip.check(self.lib.qp_pauli_stats_members(_ptr(state), _ptr(tables["rho"]), _ptr(tables["cls"]), _ptr(flags),
                                                       tables["ne"], tables["nclass"], int(ncell_member), int(members),
                                                       float(floor), _ptr(ws), vals, idx, self.stream),
                       "qp_pauli_stats_members")
        return self._members_launch(tables, ncell_member, members, call)

    def pauli_stats_members_result(self, ticket):
        """[(max occupation, (energy index, member cell index), forbidden (energy, cell) or None)] per member, each as
        ``pauli_stats_result`` of that member's lone run."""
        host, ev, ncm, members, ne = ticket
        ev.synchronize()
        vals = host[:members].view(self.torch.float64).numpy().copy()
        idx = host[members:].numpy().copy()
        out = []
        for m in range(members):
            i0, i1 = int(idx[2 * m]), int(idx[2 * m + 1])
            i0 = min(max(i0, 0), ncm * ne - 1)
            out.append((float(vals[m]), (i0 // ncm, i0 % ncm), None if i1 < 0 else (i1 // ncm, i1 % ncm)))
        return out

    def collide_guarded_members(self, tables, state, state_out, phonon, dE, dt, en_r, en_s, update_phonons, floor: float,
                                ncell_member: int, members: int, flags):
        """``collide_guarded`` over an ensemble with the guard reduced per member (``qp_collision_step_guarded_members``)."""
        nc = int(ncell_member) * int(members)
        acc = self.collision_scratch(tables, nc, en_r, en_s, update_phonons)

        def call(ws, vals, idx):
            _hip.check(self.lib.qp_collision_step_guarded_members(
                C.byref(tables["struct"]), _ptr(flags), nc, _ptr(state), _ptr(state_out), _ptr(phonon), _ptr(acc),
                float(dE), float(dt), int(bool(en_r)), int(bool(en_s)), int(bool(update_phonons)), float(floor), _ptr(ws),
                int(ncell_member), int(members), vals, idx, self.stream), "qp_collision_step_guarded_members")
        return self._members_launch(tables, ncell_member, members, call)

    @staticmethod
    def pair_members_supported(tables, ncell_member: int, members: int) -> bool:
        """Whether ``qp_collision_double_step_guarded_members`` accepts this ensemble (else two calls per step pair)."""
        return collision_tables.pair_members_supported(tables, ncell_member, members)

    def collide_pair_guarded_members(self, tables, state, state_out, phonon, dE, dt_first, dt_second, gen_amount, en_r,
                                     en_s, update_phonons, floor: float, ncell_member: int, members: int, flags):
        """``collide_pair_guarded`` over an ensemble, guard per member (only when ``pair_members_supported``)."""
        nc = int(ncell_member) * int(members)

        def call(ws, vals, idx):
            _hip.check(self.lib.qp_collision_double_step_guarded_members(
                C.byref(tables["struct"]), _ptr(flags), nc, _ptr(state), _ptr(state_out), _ptr(phonon), float(dE),
                float(dt_first), float(dt_second), float(gen_amount), int(bool(en_r)), int(bool(en_s)),
                int(bool(update_phonons)), float(floor), _ptr(ws), int(ncell_member), int(members), vals, idx, self.stream),
                "qp_collision_double_step_guarded_members")
        return self._members_launch(tables, ncell_member, members, call)

    def add_constant_members(self, state, amounts: tuple, ncell_member: int, members: int, flags):
        """state[f][m * ncell_member + c] += amounts[m] on interior cells.  The device vectors are cached by value: constant
        and pulse generation take few distinct per-member patterns, so no step uploads synchronously."""
        key = tuple(float(a) for a in amounts)
        vec = self._amount_vectors.get(key)
        if vec is None:
            vec = self._amount_vectors[key] = self.upload_vector(key)
        nfield = state.numel() // (int(ncell_member) * int(members))
        _hip.check(self.lib.qp_add_constant_members(_ptr(flags), int(ncell_member), int(members), int(nfield), _ptr(state),
                                                    _ptr(vec), self.stream), "qp_add_constant_members")

    def energy_integral(self, state, dE: float, ncell: int | None = None):
        """dE * sum over the bins of ``state`` [NE, ncell]; ``ncell`` overrides the engine's grid (members x cells)."""
        nc = self.ncell if ncell is None else int(ncell)
        out = self.empty(nc)
        _hip.check(self.lib.qp_energy_integrate(_ptr(state), state.numel() // nc, nc, float(dE), _ptr(out), self.stream),
                   "qp_energy_integrate")
        return out

    def region_bits(self, regions, offset=(0, 0)):
        """``pack_region_bits`` of up to 8 boolean full-frame regions on this engine's grid (the window of the full frame at
        ``offset``), on the device as a uint8 plane [ncell]."""
        return self.torch.as_tensor(pack_region_bits(regions, self.geom.mask, offset).reshape(-1), device=self.device)

    def region_sums(self, state, bits, members: int, out_row) -> None:
        """out_row[m][r][f] = sum over the cells of region r of state[f][m][cell] (``qp_region_sums``), ``state`` laid out
        [field][member][cell] and ``out_row`` one [members, regions, fields] row of a caller-owned device buffer.  Enqueues
        two kernels and nothing else: the sums stay on the device until the caller fetches its buffer."""
        members, nregion, nfield = int(members), int(out_row.shape[-2]), int(out_row.shape[-1])
        if state.numel() != nfield * members * self.ncell or not out_row.is_contiguous():
            raise ValueError("region_sums: out_row must be a contiguous [members, regions, fields] row matching the state")
        nbytes = int(self.lib.qp_region_sums_workspace_bytes(nfield, self.ncell, members, nregion))
        ws = self.scratch("region_sums", (nbytes + 7) // 8)
        _hip.check(self.lib.qp_region_sums(_ptr(state), _ptr(bits), nfield, self.ncell, members, nregion, _ptr(ws),
                                           _ptr(out_row), self.stream), "qp_region_sums")

    def collision_rates(self, tables, state, phonon, bits, members: int, dE: float, en_r, en_s, out_row) -> None:
        """out_row[m][r][ch][i] = sum over the cells of region r of channel ch (scattering in / out, recombination, pair
        breaking) of bin i (``qp_collision_rates``), ``state`` [NE][member][cell] and ``phonon`` [NW][member][cell] only
        read, ``out_row`` one [members, regions, 4, NE] row of a caller-owned device buffer.  Enqueues two kernels and
        nothing else.  The kernel reads row j of the tables for the pairs (lane, j): tables that are not symmetric are
        refused here, on the host."""
        self._rates("collision_rates", int(tables["ne"]), "[members, regions, 4, NE] row matching the state", tables, state,
                    phonon, bits, members, dE, en_r, en_s, out_row)

    def phonon_rates(self, tables, state, phonon, bits, members: int, dE: float, en_r, en_s, out_row) -> None:
        """out_row[m][r][ch][w] = sum over the cells of region r of channel ch (emission by scattering, absorption by
        scattering, emission by recombination, absorption by pair breaking) of phonon bin w (``qp_phonon_rates``), ``state``
        [NE][member][cell] and ``phonon`` [NW][member][cell] only read, ``out_row`` one [members, regions, 4, NW] row of a
        caller-owned device buffer.  Enqueues two kernels and nothing else.  The kernel adds the pairs of a bin without
        atomics, which needs the |i - j| / i + j structure of the bin maps and symmetric tables: a table set without
        ``diag_bin`` (forced to ``"wave_unstructured"``) or without symmetry is refused here, on the host."""
        if tables["diag_bin"] is None:
            raise ValueError("phonon_rates: the bin maps must have the |i - j| / i + j structure (diag_bin); unstructured "
                             "maps are not served")
        self._rates("phonon_rates", int(tables["nw"]), "[members, regions, 4, NW] row matching the planes", tables, state,
                    phonon, bits, members, dE, en_r, en_s, out_row)

    def _rates(self, name: str, count: int, row: str, tables, state, phonon, bits, members, dE, en_r, en_s, out_row):
        """``collision_rates`` / ``phonon_rates`` (``name``) from the symmetry check on: the shapes against ``count`` values
        per region and channel (``row``: how the message describes ``out_row``), the workspace of ``qp_<name>_workspace_bytes`` in the scratch ``name``, the call."""
        members, nregion, ne, nw = int(members), int(out_row.shape[-3]), int(tables["ne"]), int(tables["nw"])
        if not tables["symmetric"]:
            raise ValueError(f"{name}: kr0 / ks0 / idx_diff / idx_sum must be symmetric and sign antisymmetric")
        if (state.numel() != ne * members * self.ncell or phonon.numel() != nw * members * self.ncell
                or tuple(out_row.shape[-2:]) != (4, count) or not out_row.is_contiguous()):
            raise ValueError(f"{name}: out_row must be a contiguous {row}")
        nbytes = int(getattr(self.lib, f"qp_{name}_workspace_bytes")(count, self.ncell, members, nregion))
        ws = self.scratch(name, max((nbytes + 7) // 8, 1))
        _hip.check(getattr(self.lib, f"qp_{name}")(C.byref(tables["struct"]), _ptr(bits), self.ncell, members, nregion,
                                                   _ptr(state), _ptr(phonon), float(dE), int(bool(en_r)), int(bool(en_s)),
                                                   _ptr(ws), _ptr(out_row), self.stream), f"qp_{name}")

    def block_sums(self, state, members: int, bin: int, oy: int, ox: int, out_row) -> None:
        """out_row[m][f][cy][cx] = sum of state[f][m][cell] over the active cells of one ``bin`` x ``bin`` block
        (``qp_block_sums``; ``(oy, ox)`` as ``coarse_layout`` gives them), ``state`` laid out [field][member][cell] and
        ``out_row`` one [members, fields, cny, cnx] row of a caller-owned device buffer.  Enqueues one kernel on the compute
        stream and nothing else: the sums stay on the device until the caller fetches its buffer."""
        members, nfield = int(members), int(out_row.shape[1])
        cny, cnx = -(-(oy + self.ny) // bin), -(-(ox + self.nx) // bin)
        if (state.numel() != nfield * members * self.ncell or tuple(out_row.shape) != (members, nfield, cny, cnx)
                or not out_row.is_contiguous()):
            raise ValueError("block_sums: out_row must be a contiguous [members, fields, cny, cnx] row matching the state")
        _hip.check(self.lib.qp_block_sums(_ptr(state), _ptr(self.d_flags), nfield, self.ny, self.nx, members, int(bin),
                                          int(oy), int(ox), _ptr(out_row), self.stream), "qp_block_sums")

    def upload_boundary_faces(self, faces: BoundaryFaces) -> dict:
        """The face arrays and the chunk table of ``faces`` on the device, next to the host tables ``qp_boundary_flux``
        validates on every call: the one upload of a run, handed to ``boundary_flux``."""
        if faces.face_cell.size and not (0 <= int(faces.face_cell.min()) and int(faces.face_cell.max()) < self.ncell):
            raise ValueError("boundary faces: a cell index lies outside the engine's grid")
        if int(faces.surface_begin[-1]) != faces.face_cell.size or not 1 <= faces.surface_begin.size - 1 <= FLUX_SURFACES:
            raise ValueError(f"boundary faces: 1 to {FLUX_SURFACES} surfaces whose offsets end at the face count")
        up = lambda a, dt: self.torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.device)  # noqa: E731
        return {"cell": up(faces.face_cell, np.int32), "diag": up(faces.face_diag, np.float64),
                "src": up(faces.face_src, np.float64), "chunks": up(faces.chunks, np.int32),
                "chunks_host": np.ascontiguousarray(faces.chunks, dtype=np.int32),
                "surface_begin": np.ascontiguousarray(faces.surface_begin, dtype=np.int32),
                "nface": int(faces.face_cell.size), "nchunk": int(faces.chunks.shape[0]),
                "nsurface": int(faces.surface_begin.size - 1)}

    def boundary_flux(self, faces: dict, op: DiffusionOperator, state, members: int, out_row) -> None:
        """out_row[m][s][i] = sum over the faces of surface s of D (diag u - src) on plane i of member m
        (``qp_boundary_flux``): ``faces`` from ``upload_boundary_faces``, ``state`` laid out [plane][member][cell] and only
        read, D the coefficients ``op`` already holds on the device (``dcoef`` per field or ``dfield`` per field and cell,
        field = plane * members + member), ``out_row`` one [members, surfaces, planes] row of a caller-owned device buffer.
        Enqueues two kernels and nothing else.  ``op`` must be a ``DiffusionOperator`` of this engine: the block plans of a
        domain-decomposed run are not served."""
        if not isinstance(op, DiffusionOperator) or op.engine is not self:
            raise ValueError("boundary_flux: op must be the DiffusionOperator of this engine's grid; the blocks of a "
                             "domain-decomposed run are not served")
        members, nsurface, nplane = int(members), int(out_row.shape[-2]), int(out_row.shape[-1])
        nfield = nplane * members
        held = op.dcoef.numel() == nfield if op.dfield is None else op.dfield.numel() == nfield * self.ncell
        if (state.numel() != nfield * self.ncell or op.nfield != nfield or not held or tuple(out_row.shape) != (members, faces["nsurface"], nplane) or not out_row.is_contiguous()):
            raise ValueError("boundary_flux: out_row must be a contiguous [members, surfaces, planes] row matching the "
                             "state, the faces and the operator's fields")
        nbytes = int(self.lib.qp_boundary_flux_workspace_bytes(nplane, members, faces["nchunk"]))
        ws = self.scratch("boundary_flux", max((nbytes + 7) // 8, 1))
        _hip.check(self.lib.qp_boundary_flux(_ptr(state), _ptr(op.dcoef), _ptr(op.dfield), nplane, self.ncell, members,
                                             _ptr(faces["cell"]), _ptr(faces["diag"]), _ptr(faces["src"]), faces["nface"],
                                             faces["surface_begin"].ctypes.data, nsurface, faces["chunks_host"].ctypes.data,
                                             _ptr(faces["chunks"]), faces["nchunk"], _ptr(ws), _ptr(out_row), self.stream),
                   "qp_boundary_flux")

    def weighted_sum(self, planes, weights, ncell: int | None = None):
        """sum_k weights[k] planes[k]; ``weights`` on the host or already on the device, ``ncell`` as ``energy_integral``."""
        nc = self.ncell if ncell is None else int(ncell)
        out = self.empty(nc)
        w = weights if self.torch.is_tensor(weights) else self.upload_vector(weights)
        _hip.check(self.lib.qp_weighted_sum(_ptr(planes), _ptr(w), planes.numel() // nc, nc, _ptr(out), self.stream),
                   "qp_weighted_sum")
        return out

    def upload_vector(self, values):
        return self.torch.as_tensor(np.asarray(values, dtype=np.float64), device=self.device)
