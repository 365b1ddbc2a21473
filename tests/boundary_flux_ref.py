"""Reference for the boundary outflow traces (test-only, imports nothing of the product).

A plain-Python walk over the boundary faces of a mask gives ``(surface, cell, diag, src)`` from its own copy of the table of
boundary kinds and the rule that the last edge listing a face owns it; NumPy forms the terms with the three roundings of the
definition, ``D * (diag * u - src)``; ``math.fsum`` takes the sums.
"""
from __future__ import annotations

import math

import numpy as np

WALK = ("up", "down", "left", "right")
_NEIGHBOUR = {"up": (-1, 0), "down": (1, 0), "left": (0, -1), "right": (0, 1)}


def face_terms(bc, dx: float) -> tuple[float, float]:
    """(diag, src) of one boundary face in 1/dx^2 units."""
    kind = str(bc.kind).strip().lower()
    value = float(bc.value or 0.0)
    aux = float(getattr(bc, "aux_value", None) or 0.0)
    return {"reflective": (0.0, 0.0), "absorbing": (2.0, 0.0), "dirichlet": (2.0, 2.0 * value),
            "neumann": (0.0, value * dx), "robin": (value * dx, aux * dx)}[kind]


def bounding_box(mask: np.ndarray) -> tuple[int, int, int, int]:
    """(r0, c0, ny, nx) of the interior cells: the device grid."""
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return int(rows[0]), int(cols[0]), int(rows[-1] - rows[0] + 1), int(cols[-1] - cols[0] + 1)


def walk_faces(mask, edges, edge_conditions, dx: float, surfaces) -> list:
    """Per surface (``surfaces``: a sequence of lists of edge ids) the list of ``(cell, diag, src)`` of its faces, cell =
    r * nx + c on the bounding box of the mask, sorted by cell and, within a cell, in the order up, down, left, right.
    Faces whose terms are both zero are left out."""
    mask = np.asarray(mask, dtype=bool)
    ny_full, nx_full = mask.shape
    r0, c0, _, nx = bounding_box(mask)
    owner = {}
    for edge in edges:                                 # the last edge listing a face wins
        if edge.edge_id in edge_conditions:
            for f in edge.faces:
                owner[(int(f.row), int(f.col), f.direction)] = edge.edge_id
    out = [[] for _ in surfaces]
    surfaces = [set(ids) for ids in surfaces]
    for r in range(ny_full):
        for c in range(nx_full):
            if not mask[r, c]:
                continue
            for direction in WALK:
                dr, dc = _NEIGHBOUR[direction]
                rr, cc = r + dr, c + dc
                if 0 <= rr < ny_full and 0 <= cc < nx_full and mask[rr, cc]:
                    continue
                edge_id = owner.get((r, c, direction))
                if edge_id is None:
                    continue
                diag, src = face_terms(edge_conditions[edge_id], dx)
                if diag == 0.0 and src == 0.0:
                    continue
                for s, ids in enumerate(surfaces):
                    if edge_id in ids:
                        out[s].append(((r - r0) * nx + (c - c0), diag, src))
    return out


def face_arrays(faces: list):
    """(cell int64, diag, src) arrays of one surface's face list."""
    cell = np.array([f[0] for f in faces], dtype=np.int64)
    return cell, np.array([f[1] for f in faces], dtype=float), np.array([f[2] for f in faces], dtype=float)


def terms(faces: list, u: np.ndarray, D) -> np.ndarray:
    """The outflow terms of one surface on the plane ``u`` [ncell of the bounding box]; ``D`` a number or a plane like u.
    Three roundings: the product, the difference, the product."""
    cell, diag, src = face_arrays(faces)
    d = np.asarray(D, dtype=float)
    d = d.reshape(-1)[cell] if d.ndim else np.full(cell.size, float(d))
    t = diag * np.asarray(u, dtype=float).reshape(-1)[cell]
    t = t - src
    return d * t


def outflow(faces: list, u: np.ndarray, D) -> tuple[float, float]:
    """(fsum of the terms, fsum of their magnitudes) of one surface on one plane."""
    t = terms(faces, u, D)
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())


def bound(nfaces: int, magnitude: float) -> float:
    """What a sum of ``nfaces`` terms taken in any order may differ from ``fsum`` by (first order in 2^-53)."""
    return max(nfaces - 1, 0) * 2.0 ** -53 * magnitude


def grid_plane(mask: np.ndarray, packed: np.ndarray) -> np.ndarray:
    """Packed interior values [..., n] -> planes [..., ncell] on the bounding box of the mask, 0 in the holes."""
    mask = np.asarray(mask, dtype=bool)
    r0, c0, ny, nx = bounding_box(mask)
    box = mask[r0:r0 + ny, c0:c0 + nx]
    packed = np.asarray(packed, dtype=float)
    out = np.zeros(packed.shape[:-1] + (ny * nx,))
    out[..., box.reshape(-1)] = packed
    return out


def frame_plane(mask: np.ndarray, frame: np.ndarray) -> np.ndarray:
    """A stored [ny, nx] frame (NaN outside the mask) -> plane on the bounding box, 0 in the holes."""
    return grid_plane(mask, np.asarray(frame)[np.asarray(mask, dtype=bool)])


# The worst closure error of the Crank-Nicolson number balance on the oracle, in units of 2^-53 * mass_k, as
# tests/test_boundary_flux_host.py measures it on ``balance_case`` (rounded up); the GPU test takes four times this.
CN_CLOSURE_UNITS = 2.1


def balance_case() -> dict:
    """The 24 x 20 rectangle of the balance tests: one boundary kind per side as (kind, value, aux_value) in the order of
    the rectangle's four edges, a rough positive initial field, dx, dt and one D."""
    mask = np.ones((24, 20), dtype=bool)
    u0 = 1.0 + np.random.default_rng(3).random(mask.shape)
    kinds = [("absorbing", None, None), ("dirichlet", 0.7, None), ("robin", 0.3, 0.2), ("neumann", -0.05, None)]
    return dict(mask=mask, u0=u0, kinds=kinds, dx=0.5, dt=0.1, D=6.0)
