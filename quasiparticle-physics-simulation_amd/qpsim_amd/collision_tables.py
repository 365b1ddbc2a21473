"""Collision tables planned on the host: table layouts, flag bits, kernel family, scratch and pair rules.

Pure NumPy plus the library's ``*_available`` queries, none of which touches a device: ``Engine.make_collision_tables``
uploads what ``plan_collision_tables`` returns, array by array, and fills ``qp_collision_tables`` with the addresses.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from . import _hip
from .tables import KB_UEV_PER_K

# the device arrays of ``qp_collision_tables`` in declaration order (``flags`` sits between anti_bin and gap_sq)
ARRAY_NAMES = ("kr0", "ks0", "rho", "idx_diff", "idx_sum", "sign", "cls", "diag_bin", "anti_bin",
               "gap_sq", "kr_amp", "ks_amp", "pair_inv", "ks0_diag", "kr0_anti2")


def structured_bin_maps(idx_diff, idx_sum, sign, allow_shared: bool = False):
    """(diag_bin[NE], anti_bin[2NE-1]) if idx_diff[i][j] depends only on |i-j|, idx_sum[i][j] only on i+j and sign is
    sign(i-j); None otherwise.  Unless ``allow_shared``, None is also returned when a phonon bin is fed by both a
    diagonal (k >= 1) and an anti-diagonal (merged bins, e.g. when 2 E_min / dE is an integer)."""
    idx_diff, idx_sum, sign = np.asarray(idx_diff), np.asarray(idx_sum), np.asarray(sign)
    ne = idx_diff.shape[0]
    if ne < 2:
        return None
    i, j = np.indices((ne, ne))
    diag = idx_diff[np.arange(ne), 0]            # k = i - 0
    anti = np.concatenate([idx_sum[0, :], idx_sum[1:, -1]])   # m = 0..2ne-2
    if not (np.array_equal(idx_diff, diag[np.abs(i - j)]) and np.array_equal(idx_sum, anti[i + j])
            and np.array_equal(sign, np.sign(i - j))):
        return None
    if np.unique(diag[1:]).size != ne - 1 or np.unique(anti).size != anti.size:
        return None
    used = np.concatenate([diag[1:], anti])
    if not allow_shared and np.unique(used).size != used.size:
        return None
    return diag.astype(np.int32), anti.astype(np.int32)


def diagonal_major(table: np.ndarray) -> np.ndarray:
    """[..., ne, ne] -> [..., ne, ne] with out[k, i] = table[i, i - k] for k <= i < ne, 0 elsewhere: row k holds diagonal k
    (the pairs with E_i - E_j = k dE) indexed by the higher bin - what a sweep along that diagonal reads is contiguous."""
    t = np.asarray(table, dtype=np.float64)
    ne = t.shape[-1]
    out = np.zeros_like(t)
    for k in range(ne):
        i = np.arange(k, ne)
        out[..., k, i] = t[..., i, i - k]
    return out


def antidiagonal_major(table: np.ndarray, scale: float = 1.0) -> np.ndarray:
    """[..., ne, ne] -> [..., 2 ne - 1, ne] with out[m, i] = scale * table[i, m - i] for 0 <= m - i < ne, 0 elsewhere: row m
    holds anti-diagonal m (the pairs with E_i + E_j fixed) indexed by one of its bins."""
    t = np.asarray(table, dtype=np.float64)
    ne = t.shape[-1]
    out = np.zeros(t.shape[:-2] + (2 * ne - 1, ne))
    for m in range(2 * ne - 1):
        i = np.arange(max(0, m - ne + 1), min(ne, m + 1))
        out[..., m, i] = scale * t[..., i, m - i]
    return out


def onepass_tables(ks0, kr0, nclass: int, ne: int):
    """(ks0_diag, kr0_anti2) of the one-pass collision kernel (qpsim_hip.h): ``diagonal_major(ks0)`` [nclass, ne, ne] and
    ``antidiagonal_major(kr0, 2.0)`` [nclass, 2 ne - 1, ne], one image per table - the image of class m is that of its table
    alone, so a member's slice is what a lone call uploads.  None for a table that is None."""
    ksd = None if ks0 is None else diagonal_major(np.asarray(ks0, dtype=np.float64).reshape(nclass, ne, ne))
    kra = None if kr0 is None else antidiagonal_major(np.asarray(kr0, dtype=np.float64).reshape(nclass, ne, ne), 2.0)
    return ksd, kra


def tag_merged_bins(diag, anti):
    """(diag, anti, n_merged): entries of a phonon bin fed by both a diagonal k >= 1 and an anti-diagonal m get
    (slot + 1) << 16 added, slot numbering the merged bins (what the register collision kernels expect, qpsim_hip.h)."""
    diag, anti = np.array(diag, dtype=np.int32), np.array(anti, dtype=np.int32)
    where = {int(b): m for m, b in enumerate(anti)}
    slots = 0
    for k in range(1, diag.size):
        m = where.get(int(diag[k]))
        if m is not None:
            tag = (slots + 1) << 16
            diag[k] |= tag
            anti[m] |= tag
            slots += 1
    return diag, anti, slots


@dataclass
class CollisionPlan:
    """What ``plan_collision_tables`` decided: the arrays to upload and the scalars of the handle.

    ``kernel`` is the family the table set can reach - "register" (the register, one-pass, member-table and gap-class
    kernels), "wave" (one wave per pixel; with ``wide_bins`` at NE = 65 ... 128 its two-bins-per-lane form) or "generic" -
    not the kernel of a particular call.  With member tables a call
    whose members are not wave-aligned (64 cells; one-pass sizes: block-aligned, 256) takes the class-map kernels;
    ``qp_collision_route`` answers for a particular call.  ``fast``: no phonon accumulator planes are needed; ``pair``:
    two consecutive half-steps can run as one pass (``qp_collision_double_step_guarded``)."""
    arrays: dict          # ARRAY_NAMES -> None or a C-contiguous array in the dtype that is uploaded
    ne: int
    nw: int
    nclass: int
    flag_bits: int
    merged_slots: int
    symmetric: bool
    member_classes: bool
    kernel: str
    fast: bool
    pair: bool

    def struct(self, address: dict) -> "_hip.CollisionTables":
        """``qp_collision_tables`` with ``address[name]`` for every array (0 where the array is None)."""
        p = [0 if self.arrays[name] is None else int(address[name]) for name in ARRAY_NAMES]
        return _hip.CollisionTables.make(self.ne, self.nw, self.nclass, *p[:9], self.flag_bits, *p[9:])


def plan_collision_tables(lib, ncell: int, mask_flat, kr0, ks0, rho, idx_diff, idx_sum, sign, cls_packed=None,
                          allow_fast=True, kernel: str = "auto", gap_params: dict | None = None, members: int = 1,
                          member_classes: bool = False, pad_bins: bool = False,
                          wide_bins: bool = False) -> CollisionPlan:
    """Tables of ``Engine.make_collision_tables`` (which documents the arguments) for an engine of ``ncell`` cells with
    interior ``mask_flat``, on the host.  ``lib`` answers the ``qp_collision_*_available`` queries."""
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    rho = np.atleast_2d(np.asarray(rho, dtype=np.float64))
    nclass, ne = rho.shape
    arrays = dict.fromkeys(ARRAY_NAMES)
    arrays.update(kr0=f64(None if kr0 is None else np.asarray(kr0).reshape(nclass, ne, ne)),
                  ks0=f64(None if ks0 is None else np.asarray(ks0).reshape(nclass, ne, ne)),
                  rho=f64(rho), idx_diff=i32(idx_diff), idx_sum=i32(idx_sum),
                  sign=np.ascontiguousarray(sign, dtype=np.int8))
    nw = int(max(np.max(idx_diff), np.max(idx_sum))) + 1
    # 1. class map: one class per member, or the gap classes scattered over the mask and repeated per member
    if member_classes:
        if nclass != int(members):
            raise ValueError("member classes need one table set per member")
        arrays["cls"] = i32(np.repeat(np.arange(nclass, dtype=np.int32), ncell))
        gap_params = None
        if kernel == "auto" and os.environ.get("QPSIM_MEMBER_TABLES", "1") == "0":      # A/B timing: class-map kernels
            kernel = "wave"
    elif nclass > 1:
        if cls_packed is None:
            raise ValueError("cls is required for more than one gap class")
        full = np.zeros(ncell, dtype=np.int32)
        full[mask_flat] = np.asarray(cls_packed, dtype=np.int32)
        arrays["cls"] = i32(np.tile(full, int(members)))
    # 2. bin-map structure
    merged_slots = 0
    structure = structured_bin_maps(idx_diff, idx_sum, sign, allow_shared=True)
    shared = structure is not None and structured_bin_maps(idx_diff, idx_sum, sign) is None
    if structure is not None and kernel != "wave_unstructured":
        diag, anti = (np.array(a, dtype=np.int32) for a in structure)
        if shared:
            # a phonon bin fed by diagonal k AND anti-diagonal m: both table entries carry (slot + 1) << 16 so that the
            # register kernels park the diagonal's sums in scratch slot `slot` until the anti-diagonal finalises the bin
            diag, anti, merged_slots = tag_merged_bins(diag, anti)
        arrays["diag_bin"], arrays["anti_bin"] = i32(diag), i32(anti)
    # 3. symmetry and flag bits.  The register and wave kernels visit each unordered pair once (K^r_0, K^s_0 and the bin
    # maps of the reference are symmetric, sign antisymmetric: solver.py:463-490, 668-683); caller-supplied tables of the
    # step API that are not run the generic kernel, which reads (i, j) and (j, i) separately
    sym = lambda a: a is None or np.array_equal(np.asarray(a), np.swapaxes(np.asarray(a), -1, -2))  # noqa: E731
    symmetric = bool(sym(kr0 if kr0 is None else np.asarray(kr0).reshape(nclass, ne, ne))
                     and sym(ks0 if ks0 is None else np.asarray(ks0).reshape(nclass, ne, ne))
                     and sym(idx_diff) and sym(idx_sum)
                     and np.array_equal(np.asarray(sign), -np.asarray(sign).T))
    if (not allow_fast or not symmetric) and kernel == "auto":
        kernel = "generic"
    flag_bits = ({"auto": 0, "generic": 1, "wave": 2, "wave_unstructured": 2}[kernel] | (4 if shared else 0)
                 | (8 if member_classes else 0))
    if kernel == "wave_unstructured":
        kernel = "wave"
    # 4. gap classes: K^r_0, K^s_0 are separable in the gap, so the register kernel forms them per pixel
    classes_ok = False
    if (nclass > 1 and gap_params is not None and structure is not None
            and bool(lib.qp_collision_register_kernel_classes(ne))):
        E = np.asarray(gap_params["E"], dtype=np.float64)
        kTc = KB_UEV_PER_K * float(gap_params["T_c"])
        psum, pdiff = E[:, None] + E[None, :], E[:, None] - E[None, :]
        arrays["pair_inv"] = f64(1.0 / np.maximum(E[:, None] * E[None, :], 1e-30))
        arrays["gap_sq"] = f64(np.asarray(gap_params["gaps"], dtype=np.float64) ** 2)
        if kr0 is not None:
            arrays["kr_amp"] = f64((1.0 / float(gap_params["tau_r"])) * (psum / kTc) ** 2 / kTc)
        if ks0 is not None:
            ksa = (1.0 / float(gap_params["tau_s"])) * pdiff ** 2 / kTc ** 3
            np.fill_diagonal(ksa, 0.0)
            arrays["ks_amp"] = f64(ksa)
        classes_ok = True
    # 5. kernel family.  Member classes: the register kernels' member-table form where it exists, decided per call by the
    # member's cell count (the merged-bin stash is sized for it either way) ...
    members_ok = bool(member_classes and lib.qp_collision_member_tables_available(ne))
    # ... and at the one-pass sizes that kernel, whose 256-pixel blocks each stage the tables of one member
    # (``pad_bins``: also at the sizes the one-pass kernel of a larger size serves, QP_COLL_PAD_BINS)
    ceiling = int(lib.qp_collision_padded_ceiling(ne)) if pad_bins else 0
    members_onepass = bool(member_classes and kernel == "auto" and structure is not None and symmetric
                           and ncell % 256 == 0 and (lib.qp_collision_onepass_available(ne) or ceiling))
    # padded bins: a size without a kernel of its own, one class or member classes; everything else plans as without it
    padded = bool(ceiling and kernel == "auto" and structure is not None and symmetric
                  and (members_onepass if member_classes else nclass == 1))
    if padded:
        flag_bits |= 16
    wave_ok = ne <= 64 and nw <= 192
    # wide bins (opt-in, QP_COLL_WIDE_BINS): NE = 65 ... 128 on the two-bins-per-lane wave kernel, any class map, no
    # accumulator planes; every other size plans as without it
    if (wide_bins and kernel in ("auto", "wave") and symmetric and not wave_ok
            and bool(lib.qp_collision_wide_available(ne, nw))):
        flag_bits |= 32
        wave_ok = True
    label = ("generic" if (kernel == "generic" or not wave_ok) else
             "register" if padded or (kernel == "auto" and structure is not None
                                      and ((members_ok or members_onepass) if member_classes
                                           else (nclass == 1 or classes_ok))
                                      and bool(lib.qp_collision_register_kernel_available(ne))) else "wave")
    # 6. one-pass kernel (ne = 30, 32, 40, 50, or padded bins): the kernel tables once more in (anti)diagonal-major order
    # (qpsim_hip.h), at the live size; member classes: one image per member
    if (label == "register" and (nclass == 1 or members_onepass) and symmetric
            and (padded or bool(lib.qp_collision_onepass_available(ne)))):
        ksd, kra = onepass_tables(ks0, kr0, nclass, ne)
        arrays["ks0_diag"] = f64(ksd if nclass > 1 or ksd is None else ksd[0])
        arrays["kr0_anti2"] = f64(kra if nclass > 1 or kra is None else kra[0])
    # 7. consecutive half-steps of neighbouring Strang steps in one pass (qp_collision_double_step_guarded)
    pair = bool(label == "register" and (nclass == 1 or members_ok) and structure is not None and not shared
                and symmetric
                and kernel == "auto" and lib.qp_collision_pair_available(ne)
                and os.environ.get("QPSIM_COLL_PAIR", "1") != "0")
    return CollisionPlan(arrays=arrays, ne=ne, nw=nw, nclass=nclass, flag_bits=flag_bits, merged_slots=merged_slots,
                         symmetric=symmetric, member_classes=bool(member_classes), kernel=label,
                         fast=label != "generic", pair=pair)


def _field(tables, name: str):
    return tables[name] if isinstance(tables, dict) else getattr(tables, name)


def scratch_planes(tables, en_r, en_s, update_phonons) -> int:
    """Planes of ``ph_scratch`` (2 x planes x pixels doubles) a collision call with these tables (plan or handle) must pass:
    ``nw`` phonon accumulator planes for the kernels that are not ``fast``, ``merged_slots`` for the merged-bin stash of the
    register kernels, else 0.  A register table set with merged bins that gets none falls to the one-wave-per-pixel
    kernel."""
    planes = 0
    if update_phonons and (en_r or en_s) and not _field(tables, "fast"):
        planes = _field(tables, "nw")
    if _field(tables, "kernel") == "register" and _field(tables, "merged_slots") and update_phonons and en_r and en_s:
        planes = _field(tables, "merged_slots")
    return planes


def pair_members_supported(tables, ncell_member: int, members: int) -> bool:
    """Whether ``qp_collision_double_step_guarded_members`` accepts this ensemble (else two calls per step pair)."""
    pair = tables.get("pair") if isinstance(tables, dict) else tables.pair
    return bool(pair) and ncell_member % 64 == 0 and ncell_member * members < (1 << 28)
