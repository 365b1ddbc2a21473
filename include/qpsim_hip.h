/*
 * qpsim_hip.h -- C ABI of libqpsim_hip.so: the MI355X (gfx950) kernels behind the time loop of
 * qpsim.solver.run_2d_crank_nicolson (reference: /root/reference/qpsim/solver.py, cited per entry).
 *
 * The reference is pure Python and has no FFI of its own; the boundary it exposes for this path is one
 * Python function plus the step helpers.  This header is the binding a maintainer of the reference would
 * call from Python (ctypes) in place of the NumPy/SciPy bodies cited below.
 *
 * Conventions
 *   - Plain C types only: device pointers (HIP global memory), sizes, scalars, and a hipStream_t passed as
 *     void*.  No torch types.  All real data is IEEE fp64.
 *   - Every call returns 0 on success or a negative qp_status code; qp_last_error() gives the message of the
 *     last failure on the calling thread.  Nothing throws across the boundary.
 *   - Calls only enqueue work on `stream`; they never allocate, free or synchronise (graph-capture safe),
 *     except the *_create / *_destroy plan calls.
 *   - Fields live on the FULL ny x nx grid, row-major, one contiguous "plane" of ncell = ny*nx doubles per
 *     field; cells outside the geometry mask are kept at 0.  A batch is `nfield` consecutive planes
 *     (energy bins, ensemble members x bins).  The reference packs only interior cells
 *     (solver.py:53-58,1281-1285); the host layer converts at the boundary.
 *
 * Geometry / operator encoding (shared by every field of a problem)
 *   flags[ncell] (uint8): bit0 link to x-1, bit1 link to x+1, bit2 link to y-1, bit3 link to y+1,
 *                         bit4 cell is interior.  A link exists when both cells are interior.
 *   ex, ey[ncell]: boundary-face diagonal terms of the x- / y-faces of the cell in units of 1/dx^2:
 *                  absorbing 2, dirichlet 2, robin beta*dx, reflective/neumann 0     (solver.py:112-149)
 *   sx, sy[ncell]: boundary-face source terms in units of 1/dx^2:
 *                  dirichlet 2g, neumann q*dx, robin gamma*dx                          (solver.py:112-149)
 *   Diffusion coefficient of field b: scalar dcoef[b] (uniform gap) or plane dfield[b*ncell + p]
 *   (non-uniform gap: harmonic-mean face values 2 Dp Dq / max(Dp+Dq, 1e-30), solver.py:235-321).
 *   With r = dt/(2 dx^2) the directional operators are
 *      (r Lx u)_p = r [ w-(u_{p-1}-u_p) + w+(u_{p+1}-u_p) - ex_p D_p u_p ],   source r D_p sx_p   (same in y).
 */
#ifndef QPSIM_HIP_H
#define QPSIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum qp_status {
  QP_OK = 0,
  QP_ERR_INVALID_ARGUMENT = -1,
  QP_ERR_LAUNCH = -2,
  QP_ERR_UNSUPPORTED = -3,
  QP_ERR_ALLOC = -4
} qp_status;

#define QP_FLAG_LINK_XM 1u
#define QP_FLAG_LINK_XP 2u
#define QP_FLAG_LINK_YM 4u
#define QP_FLAG_LINK_YP 8u
#define QP_FLAG_ACTIVE 16u

/* Library version (major*10000 + minor*100 + patch) and last error text of this thread. */
int qp_version(void);
const char* qp_last_error(void);
/* Identity of the build as one JSON object: {"version": .., "arch": "gfx950", "qp_abl": N, "source_hash": "16 hex digits"}.
 * qp_abl != 0 marks a timing-only ablation build (tools/ablate.sh) whose results are wrong by construction: bench.py
 * prints this object with every number and refuses to measure such a build. */
const char* qp_build_info(void);

/* Geometry + per-field diffusivity description passed to the general diffusion kernels. */
typedef struct qp_grid_desc {
  uint32_t struct_size;    /* sizeof(qp_grid_desc) as the CALLER compiled it; a mismatch is QP_ERR_INVALID_ARGUMENT */
  int32_t ny, nx;          /* grid extent; ncell = ny*nx */
  int32_t nfield;          /* planes in the batch */
  const uint8_t* flags;    /* [ncell] */
  const double* ex;        /* [ncell] */
  const double* ey;        /* [ncell] */
  const double* sx;        /* [ncell] */
  const double* sy;        /* [ncell] */
  const double* dcoef;     /* [nfield] uniform diffusivity per field, or NULL */
  const double* dfield;    /* [nfield*ncell] diffusivity planes, or NULL (exactly one of dcoef/dfield) */
} qp_grid_desc;

/*
 * out = c0*u + cx*(r Lx u) + cy*(r Ly u) + cs*(r D (sx+sy)) + cr*rin          (rin may be NULL when cr == 0)
 *
 * One pass of the 5-point operator of solver.py:152-212 / :235-321 split by direction.  With
 * (c0,cx,cy,cs,cr) = (1,0,1,1,0) it is the explicit half of the first ADI sweep, (1,1,1,2,0) the
 * Crank-Nicolson right-hand side B u + dt D source of solver.py:1440,1451,1554, and (-1,1,1,0,1) the residual
 * rin - (I - r L) u used by the exact-CN iteration.  r = dt/(2 dx^2).
 */
int qp_stencil_combine(const qp_grid_desc* g, double r, const double* u, const double* rin, double* out,
                       double c0, double cx, double cy, double cs, double cr, void* stream);
/* The same with norm_out[0] = max |out| formed in the same pass (NaN counts as +inf; workspace:
 * qp_pauli_workspace_bytes() bytes): the residual and its norm of the exact-CN iteration in one kernel.
 * ex, ey, sx, sy are read only at cells with a missing link - boundary terms belong to boundary faces. */
int qp_stencil_combine_norm(const qp_grid_desc* g, double r, const double* u, const double* rin, double* out,
                            double c0, double cx, double cy, double cs, double cr, void* workspace, double* norm_out,
                            void* stream);
/* The same with one norm per field: norms_out[f] = max |out| of field f, f < nfield (the blocks of the pass never leave
 * their field, so the per-plane norms cost no pass of their own).  The exact-CN iteration accepts plane by plane -
 * max_f (max |res_f| / max |R_f|) <= rtol - so that a plane many decades below the largest one is solved too (a residual
 * below DBL_MIN counts as zero there, so a plane whose right-hand side lies below about DBL_MIN / rtol, 2e-295 at 1e-13,
 * is in effect not held to rtol).  Any field count: beyond the 1024 partial slots of the workspace the pass and its
 * per-field finish run in launches of at most 1024 fields; qp_stencil_combine(_norm) stay one launch whose blocks stride
 * over the fields. */
int qp_stencil_combine_norms(const qp_grid_desc* g, double r, const double* u, const double* rin, double* out,
                             double c0, double cx, double cy, double cs, double cr, void* workspace, double* norms_out,
                             void* stream);

/*
 * Implicit sweep: solve (I - r L_dir) x = rhs along every grid line of every field (dir 0 = x, 1 = y).
 * Replaces `lu.solve(rhs)` of solver.py:1441,1452,1555 one direction at a time.  `scratch` holds
 * 2*nfield*ncell doubles.  rhs and x may alias.  General (masked / variable-D) path: Thomas per line.
 */
int qp_implicit_sweep(const qp_grid_desc* g, double r, int dir, const double* rhs, double* x, double* scratch,
                      void* stream);

/*
 * Collision tables for qp_collision_step (all device pointers).  Built on the host exactly as
 * solver.py:463-490 (kernels), :324-342 (rho), :668-683 (phonon bin maps); `cls` selects the per-pixel
 * gap class (solver.py:1203-1232 copies per-pixel tables; here only one table set per distinct gap is kept).
 */
typedef struct qp_collision_tables {
  uint32_t struct_size;    /* sizeof(qp_collision_tables) as the CALLER compiled it: a binding written against another
                            * revision of this header (fewer / more members) is rejected with QP_ERR_INVALID_ARGUMENT
                            * instead of being read past its end */
  int32_t ne;              /* quasiparticle energy bins */
  int32_t nw;              /* phonon bins */
  int32_t nclass;          /* distinct gap classes (1 = uniform) */
  const double* kr0;       /* [nclass][ne][ne] or NULL when recombination is off */
  const double* ks0;       /* [nclass][ne][ne] or NULL when scattering is off */
  const double* rho;       /* [nclass][ne] */
  const int32_t* idx_diff; /* [ne][ne] phonon bin of |Ei-Ej| */
  const int32_t* idx_sum;  /* [ne][ne] phonon bin of Ei+Ej */
  const int8_t* sign;      /* [ne][ne] sign(Ei-Ej) */
  const int32_t* cls;      /* [ncell] gap class per cell, or NULL when nclass == 1 */
  /* Optional structure hint (both or neither).  On the reference's uniform energy grid idx_diff[i][j] = diag_bin[|i-j|]
   * and idx_sum[i][j] = anti_bin[i+j], sign[i][j] = sign(i-j); pass the two arrays when the host has verified that.
   * If a phonon bin is shared between a diagonal k and an anti-diagonal m (merged bins, e.g. whenever 2 E_min / dE is an
   * integer) also set QP_COLL_SHARED_BINS and tag BOTH entries, diag_bin[k] and anti_bin[m], with (slot + 1) << 16 on top of
   * the bin index (slot = 0, 1, ... numbering the merged bins): the register-resident kernels then park the diagonal's sums
   * in ph_scratch[2 slot], ph_scratch[2 slot + 1] (planes of ncell doubles) until the anti-diagonal finalises the bin, so
   * ph_scratch must hold 2 * (number of merged bins) * ncell doubles when phonons are updated with both processes on. */
  const int32_t* diag_bin; /* [ne] or NULL */
  const int32_t* anti_bin; /* [2*ne-1] or NULL */
  /* Kernel selection.  Default (0): register-resident kernel when (diag_bin, nclass == 1,
   * qp_collision_register_kernel_available(ne)); otherwise, for
   * ne <= 64, one wave per pixel with lanes <-> energy bins (deterministic when diag_bin vouches for the bin-map structure,
   * LDS atomics otherwise); otherwise the generic one-thread-per-cell kernel.  The FORCE bits exist for tests. */
  uint32_t flags;
  /* Optional, for nclass > 1 (non-uniform gap): the reference's kernels are separable in the gap (solver.py:463-490),
   *   K^r_0 = kr_amp[i][j] (1 + gap^2 pair_inv[i][j]),   K^s_0 = ks_amp[i][j] max(1 - gap^2 pair_inv[i][j], 0),
   * with kr_amp = (1/tau_r) ((Ei+Ej)/kTc)^2 / kTc, ks_amp = (1/tau_s) (Ei-Ej)^2 / kTc^3 (zero diagonal),
   * pair_inv = 1 / max(Ei Ej, 1e-30).  When gap_sq[nclass] and pair_inv are given (kr_amp / ks_amp per enabled process),
   * the register-resident kernel serves gap classes too (qp_collision_register_kernel_classes(ne)): it forms K per pixel from these three shared tables
   * instead of reading per-class tables; at ne = 50 with at most 16 classes that is the one-pass kernel as well (the tables
   * staged in LDS, K formed per lane).  All NULL: gap classes run the one-wave-per-pixel kernel. */
  const double* gap_sq;
  const double* kr_amp;
  const double* ks_amp;
  const double* pair_inv;
  /* Optional, for the ONE-PASS register kernel (qp_collision_onepass_available(ne); one gap class): one launch that reads
   * the old quasiparticle planes once and sweeps the phonon planes once per target block, where ne >= 32 otherwise runs
   * three launches.  Its phonon phase
   * walks the pairs (anti)diagonal by (anti)diagonal and wants the kernel values of a diagonal contiguous:
   *   ks0_diag  [ne][ne]      ks0_diag [k*ne + i] =     ks0[i][i-k]   for k <= i < ne,      0 elsewhere (k = 0..ne-1)
   *   kr0_anti2 [2ne-1][ne]   kr0_anti2[m*ne + i] = 2 * kr0[i][m-i]   for 0 <= m-i < ne,    0 elsewhere (m = 0..2ne-2)
   * Each is needed only for an enabled process; both NULL is always valid (three-launch path). */
  const double* ks0_diag;
  const double* kr0_anti2;
} qp_collision_tables;
#define QP_COLL_FORCE_GENERIC 1u
#define QP_COLL_FORCE_WAVE 2u
#define QP_COLL_SHARED_BINS 4u
/* Member classes (ensemble parameter sweeps): class k owns the contiguous cells [k * ncell / nclass,
 * (k + 1) * ncell / nclass), kr0 / ks0 / rho hold one table per class and cls (required: the kernels without a member-table
 * form read it) agrees with that.  ncell % nclass != 0 or cls == NULL: QP_ERR_INVALID_ARGUMENT before any launch.  Where
 * qp_collision_member_tables_available(ne) is 1, (ncell / nclass) % 64 == 0, diag_bin / anti_bin are given and no FORCE bit
 * is set, the single-pass register kernel runs with every wave reading its own class's tables (bit-equal to one call per
 * class with that class's single table), and the double half-step call accepts the tables unless QP_COLL_SHARED_BINS is
 * set.  Where qp_collision_onepass_available(ne) is 1 (ne = 30, 32, 40, 50), (ncell / nclass) % 256 == 0 - the 256-cell
 * rule: a block of the one-pass kernel stages the tables of ONE class, so no block may straddle two - diag_bin / anti_bin are
 * given and no FORCE bit is set, the one-pass kernel runs with every block reading its own class's tables (bit-equal to one
 * call per class again).  It reads ks0_diag / kr0_anti2 with this flag, as [nclass][ne][ne] and [nclass][2ne-1][ne]: one
 * image per class, each built from that class's ks0 / kr0 exactly as for one class; the image of an enabled process is
 * required (there is no member form of the three-launch split kernels).  Everything else runs the one-wave-per-pixel or the
 * generic kernel through cls, and the double half-step call returns QP_ERR_UNSUPPORTED.  gap_sq / kr_amp / ks_amp /
 * pair_inv are not used with this flag. */
#define QP_COLL_MEMBER_CLASSES 8u
/* Padded bins (opt-in): where qp_collision_padded_ceiling(ne) = C != 0, diag_bin / anti_bin are given, no FORCE bit is set,
 * there is one class (or member classes under the 256-cell rule above) and the image of every effective process is present,
 * the one-pass kernel instantiated for C bins runs on the ne live bins.  `ne`, `nw` and every array keep describing the LIVE
 * size: ks0_diag / kr0_anti2 are the [ne][ne] / [2ne-1][ne] images (one per class with QP_COLL_MEMBER_CLASSES); the kernel
 * lays them into its C-sized LDS image itself and neither reads nor writes a state, phonon or scratch plane that the live
 * size does not have.  Sizes with a kernel of their own, ne <= 16, ne >= 51, gap classes and the double half-step call are
 * not affected by the flag. */
#define QP_COLL_PAD_BINS 16u
/* Wide bins (opt-in): where qp_collision_wide_available(ne, nw) is 1 (65 <= ne <= 128, nw <= 512) and QP_COLL_FORCE_GENERIC
 * is not set, a one-wave-per-pixel kernel with TWO energy bins per lane runs instead of the generic kernel: ph_scratch may
 * be NULL (the per-pixel phonon sums live in LDS), kr0 / ks0 / idx_diff / idx_sum must be symmetric and sign antisymmetric
 * (as for the wave kernel), any class map.  Deterministic when diag_bin vouches for the bin-map structure, LDS atomics
 * otherwise.  No fused Pauli guard; the double half-step call is not affected.  Sizes outside the query ignore the flag. */
#define QP_COLL_WIDE_BINS 32u

/*
 * One local coupled quasiparticle-phonon collision update of every interior cell
 * (solver.py:703-791 per pixel, :794-875 the pixel loops).  state_in [ne][ncell] and phonon [nw][ncell]
 * are read as the OLD values; the new quasiparticle density goes to state_out (must not alias state_in),
 * phonons are updated in place when update_phonons != 0.
 * ph_scratch: the generic one-thread-per-cell kernel (ne > 64 or QP_COLL_FORCE_GENERIC) needs 2*nw*ncell doubles of
 * accumulators when phonons are updated (not where QP_COLL_WIDE_BINS takes effect, see above); the register-resident kernels need 2*(merged bins)*ncell doubles only when
 * QP_COLL_SHARED_BINS is set and both processes update phonons (see diag_bin above); every other case takes NULL.
 * Cells whose flags lack QP_FLAG_ACTIVE are copied through unchanged.
 */
int qp_collision_step(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell, const double* state_in,
                      double* state_out, double* phonon, double* ph_scratch, double dE, double dt,
                      int enable_recombination, int enable_scattering, int update_phonons, void* stream);

/*
 * qp_collision_step followed by qp_pauli_stats on state_out (the guard of solver.py:1477 after the last collision of a step),
 * as ONE call: the single-pass register kernels (ne < 32) reduce the occupation statistics of the new densities while they
 * are still in registers - one partial per wave into guard_workspace, finished by two small launches - which saves the
 * separate pass over the ne planes (7 % of a 4096^2, ne = 12 coupled step).  Other kernels run the separate pass.
 * out_vals / out_idx as qp_pauli_stats (bit-identical results); guard_workspace: qp_collision_guard_workspace_bytes(ncell).
 */
int64_t qp_collision_guard_workspace_bytes(int64_t ncell);
int qp_collision_step_guarded(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell, const double* state_in,
                              double* state_out, double* phonon, double* ph_scratch, double dE, double dt,
                              int enable_recombination, int enable_scattering, int update_phonons, double density_floor,
                              void* guard_workspace, double* out_vals, int64_t* out_idx, void* stream);

/*
 * TWO consecutive collision half-steps in one pass over the state: under Strang splitting the closing half-step of step k
 * and the opening half-step of step k + 1 (solver.py:1469-1475) act on the same state with nothing between them but the
 * Pauli guard of step k (solver.py:1477) and the explicit generation term of step k + 1 (solver.py:1459-1464) - unless step
 * k is a store point.  Equivalent, bit for bit, to
 *     qp_collision_step_guarded(state_in -> tmp, dt_first);   tmp += gen_amount on interior cells;
 *     qp_collision_step(tmp -> state_out, dt_second)
 * but n and the phonon planes make one round trip through HBM instead of two (the intermediate state never leaves the
 * registers).  out_vals / out_idx: guard statistics of the INTERMEDIATE state (before the generation term), as
 * qp_pauli_stats.  gen_amount: dt_{k+1} * rate for constant / active pulse generation, 0 otherwise.
 * Returns QP_ERR_UNSUPPORTED (nothing launched, nothing written) when no fused kernel fits - qp_collision_pair_available(ne)
 * is 0, more than one gap class (other than member classes, see QP_COLL_MEMBER_CLASSES), merged phonon bins
 * (QP_COLL_SHARED_BINS), no diag_bin / anti_bin, a FORCE flag, no enabled
 * process: the caller then issues the two calls above.  guard_workspace: qp_collision_guard_workspace_bytes(ncell).
 */
int qp_collision_pair_available(int32_t ne);
int qp_collision_double_step_guarded(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell, const double* state_in,
                                     double* state_out, double* phonon, double dE, double dt_first, double dt_second,
                                     double gen_amount, int enable_recombination, int enable_scattering, int update_phonons,
                                     double density_floor, void* guard_workspace, double* out_vals, int64_t* out_idx,
                                     void* stream);

/* 1 when qp_collision_step has a register-resident kernel for `ne` energy bins (structured, unshared bin maps and one gap
 * class are the other conditions); other sizes <= 64 run the one-wave-per-pixel kernel, larger ones the generic kernel. */
int qp_collision_register_kernel_available(int32_t ne);
/* 1 when the one-pass kernel (ks0_diag / kr0_anti2 above) is instantiated for `ne` energy bins: ne = 30, 32, 40 and 50 (the
 * reference's default num_energy_bins, solver.py:1012). */
int qp_collision_onepass_available(int32_t ne);
/* 1 when the register-resident kernel also has its gap-class variant for `ne`: the sizes of
 * qp_collision_register_kernel_available (single pass for ne = 2 ... 16, 18, 20, 24, 30; three launches for 32, 40, 50). */
int qp_collision_register_kernel_classes(int32_t ne);
/* 1 when the single-pass and the double half-step register kernels are instantiated in their member-table form
 * (QP_COLL_MEMBER_CLASSES) for `ne`: ne = 4 ... 16. */
int qp_collision_member_tables_available(int32_t ne);
/* The size C of the one-pass kernel that serves `ne` live bins under QP_COLL_PAD_BINS: 30 for ne = 17, 19, 21-23, 25-29;
 * 32 for 31; 40 for 33-39; 50 for 41-49; 0 for every size with a one-pass or register kernel of its own, for ne <= 16 and
 * for ne >= 51. */
int qp_collision_padded_ceiling(int32_t ne);
/* 1 when the two-bins-per-lane wave kernel of QP_COLL_WIDE_BINS serves `ne` energy bins and `nw` phonon bins:
 * 65 <= ne <= 128 and 1 <= nw <= 512. */
int qp_collision_wide_available(int32_t ne, int32_t nw);

/* The kernel family qp_collision_step (and the step inside the guarded calls) runs for these tables, cell count and
 * switches; have_scratch: whether ph_scratch would be non-NULL.  Launches nothing and reads only the struct itself (its
 * pointers are tested for NULL, never followed).  Returns a QP_ROUTE_* value, or the negative status with which
 * qp_collision_step refuses the same tables.  QPSIM_COLL_ONEPASS=0 in the environment switches the one-pass routes off. */
typedef enum qp_collision_route_kind {
  QP_ROUTE_ONEPASS = 0,          /* one-pass kernel: one gap class, or one table per member class (ks0_diag / kr0_anti2) */
  QP_ROUTE_REGISTER = 1,         /* register kernel, one gap class (ne >= 32: three launches) */
  QP_ROUTE_REGISTER_MEMBERS = 2, /* register kernel with one table per member class */
  QP_ROUTE_ONEPASS_CLASSES = 3,  /* one-pass kernel, gap classes */
  QP_ROUTE_REGISTER_CLASSES = 4, /* register kernel, gap classes */
  QP_ROUTE_WAVE = 5,             /* one wave per pixel */
  QP_ROUTE_GENERIC = 6,          /* one thread per cell, any table */
  QP_ROUTE_COPY = 7,             /* no effective process at a register-kernel size: n' = max(n, 0) */
  QP_ROUTE_ONEPASS_PADDED,       /* (8) one-pass kernel of the ceiling size on fewer live bins; only with QP_COLL_PAD_BINS */
  QP_ROUTE_WAVE_WIDE             /* (9) one wave per pixel, two energy bins per lane (65 <= ne <= 128); only with QP_COLL_WIDE_BINS */
} qp_collision_route_kind;
int qp_collision_route(const qp_collision_tables* t, int64_t ncell, int enable_recombination, int enable_scattering,
                       int update_phonons, int have_scratch);

/*
 * Explicit fixed-bath collision helpers of the reference's step API (not on its time loop; API parity):
 * rhs = [g_therm - 2 n dE (K_r n)] (if kr) + [dE rho (1-f) (K_s^T n) - n dE ((K_s rho) (1-f))] (if ks), per cell;
 * out = rhs (rhs_only != 0: solver.py:608-637 _collision_rhs) or max(n + dt rhs, 0) (solver.py:551-605
 * apply_scattering_step / apply_recombination_step).  state_in, out: [ne][ncell], must not alias.
 */
int qp_euler_collision(int32_t ne, int64_t ncell, const double* state_in, double* out, const double* kr,
                       const double* g_therm, const double* ks, const double* rho, double dE, double dt, int rhs_only,
                       void* stream);

/*
 * state[f][p] += amount for every interior cell of `nfield` planes (constant / pulse external generation,
 * solver.py:910-916,1464), or state += scale * g[f][p] (custom generation evaluated on the host).
 */
int qp_add_constant(const uint8_t* flags, int64_t ncell, int32_t nfield, double* state, double amount, void* stream);
/* out[f][p] = scale * in[f][p] inside the mask, NaN outside: the NaN-padded [ny, nx] frames of reconstruct_field
 * (solver.py:215-218, store block :1479-1494) formed on the device, so a stored state crosses PCIe once, ready to hand out. */
int qp_nan_pad(const uint8_t* flags, int64_t ncell, int32_t nfield, const double* in, double scale, double* out,
               void* stream);
int qp_add_scaled(int64_t n, double* state, const double* g, double scale, void* stream);

/*
 * Custom generation g(E, x, y, t, params) evaluated on the device (replaces the host evaluation + upload of
 * solver.py:918-962 and the update of solver.py:1464 for expressions in the device subset).
 *
 * The host splits the expression: every sub-expression that names neither x nor y is evaluated on the host per step and
 * energy bin and arrives as slots[bin][slot]; what mixes x, y with slots arrives as a register program of `nword`
 * instruction words, each
 *     op | dst << 8 | a << 12 | b << 18 | c << 24          (op 8 bits, dst 4 bits, operands 6 bits)
 * with dst a register 0 .. QP_EXPR_MAX_REGS-1 and an operand one of: 0 .. 7 a register, QP_EXPR_X, QP_EXPR_Y, or
 * QP_EXPR_SLOT0 + k for slot k < nslot.  The value of the program is what its LAST word writes.  Registers are read only
 * after they were written (checked).  Arithmetic is IEEE fp64 without contraction: +, -, *, /, sqrt are correctly rounded,
 * MAX / MIN propagate NaN as np.maximum / np.minimum do, a comparison yields 0.0 or 1.0, WHERE takes a when c != 0,
 * HEAVISIDE(a, b) is np.heaviside; POW and the transcendental ops are the device math library's (not bit-equal to NumPy).
 * Coordinates are the pixel centres of the FULL mask, x = (col0 + col + 0.5) / nx_full, y = (row0 + row + 0.5) / ny_full
 * (one IEEE division each, solver.py:924-929); the ny x nx device grid is the window at (row0, col0) of that mask.
 */
enum {
  QP_EXPR_MAX_WORDS = 64, /* instruction words of a program */
  QP_EXPR_MAX_REGS = 8,   /* live temporaries */
  QP_EXPR_MAX_SLOTS = 16, /* host-evaluated values per energy bin */
  QP_EXPR_X = 8,
  QP_EXPR_Y = 9,
  QP_EXPR_SLOT0 = 16
};
typedef enum qp_expr_op {
  QP_OP_COPY = 0, QP_OP_NEG, QP_OP_ADD, QP_OP_SUB, QP_OP_MUL, QP_OP_DIV, QP_OP_POW, QP_OP_SQUARE, QP_OP_SQRT, QP_OP_RECIP,
  QP_OP_ABS, QP_OP_MAX, QP_OP_MIN, QP_OP_WHERE /* c ? a : b */, QP_OP_HEAVISIDE, QP_OP_LT, QP_OP_LE, QP_OP_GT, QP_OP_GE,
  QP_OP_EQ, QP_OP_NE, QP_OP_EXP, QP_OP_LOG, QP_OP_LOG10, QP_OP_SIN, QP_OP_COS, QP_OP_TAN, QP_OP_ASIN, QP_OP_ACOS,
  QP_OP_ATAN, QP_OP_SINH, QP_OP_COSH, QP_OP_TANH, QP_OP_COUNT
} qp_expr_op;
typedef struct qp_generation_program {
  uint32_t struct_size;    /* sizeof(qp_generation_program) as the CALLER compiled it */
  int32_t ny, nx;          /* device grid of one member; ncell_member = ny*nx */
  int32_t ny_full, nx_full; /* extent of the full mask that defines x, y */
  int32_t row0, col0;      /* position of the device grid inside the full mask */
  int32_t ne;              /* energy bins */
  int32_t nslot;           /* slots per bin, 0 .. QP_EXPR_MAX_SLOTS */
  int32_t nword;           /* 1 .. QP_EXPR_MAX_WORDS */
  const uint32_t* words;   /* [nword] HOST memory: validated by the call and passed to the kernel by value */
  const double* slots;     /* [ne][nslot] device memory (host memory for qp_expr_eval_host); NULL when nslot == 0 */
} qp_generation_program;
/*
 * state[bin][m][c] += dt * g(bin, c) for every interior cell c of the listed members m over planes laid out
 * [bin][member][cell] (`members` members of ny*nx cells; flags cover members * ncell_member cells as in
 * qp_add_constant_members).  member_ids: device array of `nlisted` member indices, or NULL for all members
 * (nlisted == members).  The update rounds as qp_add_scaled does on the g the program evaluates to.  Cells outside the mask
 * are neither evaluated nor written.  status: two device words, zeroed by the call on `stream` before the kernel runs;
 * the kernel ORs 1 into status[0] when a value it added was not finite and into status[1] when one was negative
 * (the checks of solver.py:895-902, left to the caller to read back).
 */
int qp_add_generation_expr(const qp_generation_program* prog, const uint8_t* flags, int64_t members,
                           const int32_t* member_ids, int64_t nlisted, double* state, double dt, uint32_t* status,
                           void* stream);
/* Test hook: the same evaluator function compiled for the host.  out[bin][row * nx + col] = g for EVERY cell of the
 * ny x nx grid (all pointers host memory, no flags, no update).  The product never calls it. */
int qp_expr_eval_host(const qp_generation_program* prog, double* out);

/*
 * Pauli-guard statistics over state[ne][ncell] (solver.py:967-996): occupation f = n / rho where rho > 1e-30.
 * out_vals[0] = max f, out_idx[0] = its linear index ie*ncell + p (first in C order on ties; a NaN occupation counts as
 * the maximum and the first NaN wins, as np.argmax does),
 * out_idx[1] = first linear index with rho <= 1e-30 and n > density_floor, or -1.
 * workspace: qp_pauli_workspace_bytes() bytes.  Results land in device memory (copy them back yourself).
 */
int64_t qp_pauli_workspace_bytes(void);
int qp_pauli_stats(const double* state, const double* rho, const int32_t* cls, const uint8_t* flags, int32_t ne,
                   int32_t nclass, int64_t ncell, double density_floor, void* workspace, double* out_vals,
                   int64_t* out_idx, void* stream);

/*
 * Ensembles: `members` independent problems of ncell_member cells each, laid out [bin][member][cell] (state[ne][members *
 * ncell_member]; flags and cls cover all members * ncell_member cells).
 * qp_pauli_stats_members: for every member m, out_vals[m], out_idx[2m], out_idx[2m+1] are what qp_pauli_stats returns on
 * member m's slice alone, bit for bit - indices member-local (ie * ncell_member + c), same tie and NaN rules.  Deterministic
 * (per-block partials that never straddle two members, one finishing block per member; no atomics).
 * workspace: qp_pauli_members_workspace_bytes(ncell_member, members) bytes.
 */
int64_t qp_pauli_members_workspace_bytes(int64_t ncell_member, int64_t members);
int qp_pauli_stats_members(const double* state, const double* rho, const int32_t* cls, const uint8_t* flags, int32_t ne,
                           int32_t nclass, int64_t ncell_member, int64_t members, double density_floor, void* workspace,
                           double* out_vals, int64_t* out_idx, void* stream);
/* state[f][m * ncell_member + c] += amounts[m] on interior cells (amounts: device array of `members` doubles); per member
 * bit-equal to qp_add_constant on that member's slice (generation with per-member rates or pulse windows). */
int qp_add_constant_members(const uint8_t* flags, int64_t ncell_member, int64_t members, int32_t nfield, double* state,
                            const double* amounts, void* stream);
/*
 * qp_collision_step_guarded / qp_collision_double_step_guarded with the guard reduced PER MEMBER (out_vals[members],
 * out_idx[2 * members] as qp_pauli_stats_members).  ncell = members * ncell_member.  When ncell_member % 64 == 0 every wave
 * partial of the fused guard belongs to one member and a finishing kernel groups them (no extra pass over the state);
 * otherwise, or when the kernel has no fused guard, the single-step call runs qp_pauli_stats_members on state_out.  The
 * double-step call returns QP_ERR_UNSUPPORTED (nothing launched) in those cases, since its intermediate state never exists
 * in memory, and wherever qp_collision_double_step_guarded would (incl. ncell >= 2^28).
 * guard_workspace: max(qp_collision_guard_workspace_bytes(ncell), qp_pauli_members_workspace_bytes(ncell_member, members)).
 */
int qp_collision_step_guarded_members(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                      const double* state_in, double* state_out, double* phonon, double* ph_scratch,
                                      double dE, double dt, int enable_recombination, int enable_scattering,
                                      int update_phonons, double density_floor, void* guard_workspace,
                                      int64_t ncell_member, int64_t members, double* out_vals, int64_t* out_idx,
                                      void* stream);
int qp_collision_double_step_guarded_members(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                             const double* state_in, double* state_out, double* phonon, double dE,
                                             double dt_first, double dt_second, double gen_amount, int enable_recombination,
                                             int enable_scattering, int update_phonons, double density_floor,
                                             void* guard_workspace, int64_t ncell_member, int64_t members,
                                             double* out_vals, int64_t* out_idx, void* stream);

/* out[p] = dE * sum_i state[i][p]  (energy integral of solver.py:1367,1480; sequential in i). */
int qp_energy_integrate(const double* state, int32_t ne, int64_t ncell, double dE, double* out, void* stream);

/*
 * Region sums (time traces; no reference counterpart: the reference has `mass` at store points only).
 * out[m][r][f] = sum of state[f][m][c] over the cells c of a member with bit r of region_bits[c] set, for nregion = 1 ... 8
 * regions that may overlap; region_bits[ncell_member] is shared by all members and read INSTEAD of flags (clear the bits of
 * cells outside the mask).  Every entry of out[members][nregion][nfield] is written; a region without cells gives 0.0.
 * Two launches: blocks reduce fixed chunks of one (field, member) plane into the workspace (registers, wave shuffles,
 * LDS), then one block per plane adds its chunk partials in index order.  The partition depends on the four sizes alone
 * and there are no atomics and no completion counters, so equal inputs give bitwise equal outputs whatever else runs.
 * 16-byte loads when `state` is 16-byte aligned (a plane that starts on an odd element takes one scalar cell first); any
 * 8-byte aligned `state` gives the same bits.  Bandwidth-bound: 8 B per cell and field, 1 B per cell of bits.
 * workspace: qp_region_sums_workspace_bytes(nfield, ncell_member, members, nregion) bytes (0 for sizes the call refuses).
 */
size_t qp_region_sums_workspace_bytes(int32_t nfield, int64_t ncell_member, int64_t members, int32_t nregion);
int qp_region_sums(const double* state, const uint8_t* region_bits, int32_t nfield, int64_t ncell_member, int64_t members,
                   int32_t nregion, void* workspace, double* out, void* stream);

/*
 * Collision rate traces (no reference counterpart on its time loop; the terms are those of solver.py:719-743).  Per cell
 * and energy bin i, with q = rho * max(1 - n / max(rho, 1e-30), 0) and N the phonon occupation of the pair's bin, four
 * non-negative channels in units of dn_i/dt:
 *   0 scattering_in    dE q_i sum_j Ks_eff[j][i] n_j        Ks_eff[a][b] = ks0[a][b] (1 + N_|a-b|) where E_a > E_b,
 *   1 scattering_out   n_i dE sum_j Ks_eff[i][j] q_j                       ks0[a][b] N_|a-b| where E_a < E_b, 0 where a == b
 *   2 recombination    n_i 2 dE sum_j kr0[i][j] (1 + N_{i+j}) n_j
 *   3 pair_breaking    2 dE q_i sum_j kr0[i][j] N_{i+j} q_j
 * out[m][r][ch][i] = sum of channel ch over the cells c of member m with bit r of region_bits[c] set (region_bits as in
 * qp_region_sums: one byte per cell of ONE member grid, holes carry no bit, so no flags plane is read).  Every entry of
 * out[members][nregion][4][ne] is written; the channels of a disabled process (or of a NULL kr0 / ks0) and a region without
 * cells are exactly 0.0.  state[ne][members * ncell_member] and phonon[nw][members * ncell_member] are only read, and not at
 * all in a group of 8 cells without a region bit: NaN outside every region reaches no sum, and such a group costs its wave
 * nothing (a call lasts as long as its busiest wave: DESIGN 6f).  Of the tables the call reads kr0, ks0, rho, idx_diff, idx_sum, sign and cls / nclass (cls covers all members *
 * ncell_member cells, as in the collision calls; with QP_COLL_MEMBER_CLASSES class k owns the cells of its members, which
 * cls says too); kr0 / ks0 / idx_diff / idx_sum must be symmetric and sign antisymmetric (row j serves the pairs (lane, j),
 * as in the one-wave-per-pixel kernel; the caller checks).  The route flags and the one-pass images are ignored.
 * Association: each sum runs over j = 0 ... ne-1 in order as fma(K * factor, x_j, sum) with factor 1 + N or N; the
 * prefactors are (dE q_i) sum, (n_i dE) sum, (n_i (2 dE)) sum, ((2 dE) q_i) sum.
 * Two launches, no atomics: a block of 4 waves owns one (chunk, member), a chunk being QP_RATES_CHUNK = 1024 consecutive
 * cells of a member grid; wave w owns cells [256 w, 256 w + 256) of the chunk and walks them in groups of 8 in index order,
 * lane <-> energy bin; the waves combine through LDS in wave order ((w0 + w1) + w2) + w3; the block writes nregion * 4 * ne
 * partials; the second launch adds the partials of each (member, region, channel, bin) in chunk order.  Which lane adds
 * which cell in which order depends on (ne, ncell_member, members, nregion) alone: equal inputs give bitwise equal
 * outputs, and member m of a batch gives the bits of a lone call on its planes whatever the parity of ncell_member.
 * workspace: qp_collision_rates_workspace_bytes = members * ceil(ncell_member / 1024) * nregion * 4 * ne * 8 bytes (0 for
 * sizes the call refuses).  QP_ERR_UNSUPPORTED where qp_collision_rates_available(ne, nw) is 0 (it is 1 for 2 <= ne <= 64
 * and 1 <= nw <= 191, and answers without a GPU) or nregion is outside 1 ... 8.
 */
#define QP_RATES_CHUNK 1024
int qp_collision_rates_available(int32_t ne, int32_t nw);
size_t qp_collision_rates_workspace_bytes(int32_t ne, int64_t ncell_member, int64_t members, int32_t nregion);
int qp_collision_rates(const qp_collision_tables* t, const uint8_t* region_bits, int64_t ncell_member, int64_t members,
                       int32_t nregion, const double* state, const double* phonon, double dE, int enable_recombination,
                       int enable_scattering, void* workspace, double* out, void* stream);

/*
 * Phonon rate traces (no reference counterpart on its time loop; the terms are those of solver.py:750-788).  Per cell and
 * phonon bin w, with q = rho * max(1 - n / max(rho, 1e-30), 0) and N_w the phonon occupation, four base sums
 *   E_w = dE sum n_i ks0[i][j] q_j   over the pairs with E_i > E_j and idx_diff[i][j] == w
 *   A_w = the same sum               over the pairs with E_i < E_j
 *   R_w = dE sum n_i kr0[i][j] n_j   over all (i, j), both orders and the diagonal, with idx_sum[i][j] == w
 *   B_w = dE sum q_i kr0[i][j] q_j   over the same pairs
 * (the phonon update is dN_w/dt = (E_w + R_w)(1 + N_w) - (A_w + B_w) N_w) and four non-negative channels in units of dN_w/dt:
 *   0 scattering_emission       E_w (1 + N_w)
 *   1 scattering_absorption     A_w N_w
 *   2 recombination_emission    R_w (1 + N_w)
 *   3 pair_breaking_absorption  B_w N_w
 * out[m][r][ch][w] = sum of channel ch over the cells c of member m with bit r of region_bits[c] set (region_bits as in
 * qp_region_sums and qp_collision_rates).  Every entry of out[members][nregion][4][nw] is written; the channels of a
 * disabled process (or of a NULL kr0 / ks0), of a bin no pair feeds and of a region without cells are exactly 0.0.
 * state[ne][members * ncell_member] and phonon[nw][members * ncell_member] are only read, and not at all in a group of
 * cells without a region bit (8, 4 or 2 consecutive cells, depending on nregion and nw); a cell without a bit inside
 * a group that is loaded is skipped as a whole: NaN outside every region reaches no sum.  Of the tables the call reads kr0, ks0, rho, idx_diff, idx_sum, sign and cls / nclass as
 * qp_collision_rates does, under the same symmetry condition (the caller checks), and requires diag_bin / anti_bin to be
 * non-NULL without reading them: they are the host's word that idx_diff depends on |i - j| alone, idx_sum on i + j alone,
 * and that distinct (anti)diagonals have distinct bins, which is what makes the per-bin sums race-free without atomics (a bin
 * shared by a diagonal and an anti-diagonal is fine: the four sums are separate arrays).  Unstructured maps return
 * QP_ERR_INVALID_ARGUMENT.  The route flags and the one-pass images are ignored.
 * Association: a pair term is (x_i * K) * y_j with (x, y) = (n, q), (n, n), (q, q), added to its bin's sum in the order
 * j = 0 ... ne-1 (the compiler may fuse the last product into the addition); a channel is (dE * sum) * (1 + N_w) or
 * (dE * sum) * N_w as rounded products.
 * Two launches, no atomics: the partition is that of qp_collision_rates - a block of 4 waves owns one (chunk, member) of
 * QP_RATES_CHUNK consecutive cells, wave w its cells [256 w, 256 w + 256) in index order, lane <-> energy bin while the pairs
 * are formed and lane <-> phonon bin (up to three per lane) when the channels are added; the waves combine through LDS in
 * wave order; the second launch adds the partials of each (member, region, channel, bin) in chunk order.  Equal inputs give
 * bitwise equal outputs, and member m of a batch gives the bits of a lone call on its planes whatever the parity of
 * ncell_member.
 * workspace: qp_phonon_rates_workspace_bytes = members * ceil(ncell_member / 1024) * nregion * 4 * nw * 8 bytes (0 for sizes
 * the call refuses).  QP_ERR_UNSUPPORTED where qp_phonon_rates_available(ne, nw) is 0 (it is 1 for 2 <= ne <= 64 and
 * 1 <= nw <= 191, and answers without a GPU) or nregion is outside 1 ... 8.
 */
int qp_phonon_rates_available(int32_t ne, int32_t nw);
size_t qp_phonon_rates_workspace_bytes(int32_t nw, int64_t ncell_member, int64_t members, int32_t nregion);
int qp_phonon_rates(const qp_collision_tables* t, const uint8_t* region_bits, int64_t ncell_member, int64_t members,
                    int32_t nregion, const double* state, const double* phonon, double dE, int enable_recombination,
                    int enable_scattering, void* workspace, double* out, void* stream);

/*
 * Boundary outflow (flux traces; no reference counterpart on its time loop: the terms are the boundary terms of
 * solver.py:112-149 as the operator applies them).  A boundary face k of interior cell c = face_cell[k] carries
 * (face_diag[k], face_src[k]) in 1/dx^2 units and adds D (-diag u_c + src) / dx^2 to du_c/dt; its outflow term is
 *   term_k = D * (diag_k * u_c - src_k)         three roundings: the product, the difference, the product - never an fma,
 * the bits of NumPy's D * (diag * u - src), with D = dcoef[f] or, when dfield is given, dfield[f][c] (the cell's own D, as
 * the reference scales boundary terms).  Exactly one of dcoef / dfield is non-NULL.  The planes are state[i][m][cell] as in
 * the time loop, f = i * members + m is the field index of the diffusion operator (dcoef[nplane * members],
 * dfield[nplane * members][ncell_member]), and
 *   out[m][s][i] = sum of term_k over the faces k of surface s         (positive: quasiparticles leave)
 * for nsurface = 1 ... 64 surfaces.  The face list is grouped by surface: surface s owns the faces
 * [surface_begin[s], surface_begin[s + 1]) (host array of nsurface + 1 offsets, ascending from 0 to nface; a surface may be
 * empty and gives +0.0).  The chunk table cuts the list into nchunk chunks, rows of three int32 (first face, faces,
 * surface) in ascending face order with 1 <= faces <= QP_FLUX_CHUNK and no chunk reaching outside its surface; the call
 * reads it on the host (chunks_host, validated before any launch) and on the device (chunks_dev, the same rows - the
 * caller's word).  face_cell, face_diag, face_src and chunks_dev are device arrays that a run uploads once; face_cell
 * entries must lie in [0, ncell_member) (the caller's word as well: the host cannot see them).  With nface = nchunk = 0
 * every entry of out is +0.0 and the face arrays may be NULL.
 * Two launches, no atomics, no completion counters: a block of 4 waves owns one (chunk, field); thread t takes the faces
 * t, t + 256, t + 512, t + 768 of the chunk (coalesced index and coefficient loads, the four gathers of u - and of D -
 * issued together), adds its four terms in that order (a face beyond the chunk enters as +0.0 through a select), the 64
 * lanes of a wave combine by shuffles from the upper half down, the waves through LDS as ((w0 + w1) + w2) + w3; the second
 * launch, one wave per field, lets lane s add the chunk partials of surface s in chunk order and write out[m][s][i] (hence
 * at most 64 surfaces).  Which thread adds which face depends on the face list alone - not on the plane, its alignment or
 * ncell_member - so equal inputs give bitwise equal outputs, and member m of a batch gives the bits of a lone call on its
 * planes.  Only cells on listed faces are loaded: NaN anywhere else reaches no sum.  A surface of very many chunks is added
 * by one lane in order (a known limit: masks with millions of boundary faces).
 * workspace: qp_boundary_flux_workspace_bytes = max(nplane * members * nchunk, 1) * 8 bytes (0 for sizes the call refuses).
 * QP_ERR_INVALID_ARGUMENT, before any launch, for NULL pointers, nsurface outside 1 ... 64, non-positive nplane /
 * ncell_member / members, ncell_member above 2^31 - 1, more than 65535 fields, offsets that do not ascend to nface, and a
 * chunk that is empty, exceeds QP_FLUX_CHUNK, is out of order or crosses a surface.
 */
#define QP_FLUX_CHUNK 1024
size_t qp_boundary_flux_workspace_bytes(int32_t nplane, int64_t members, int64_t nchunk);
int qp_boundary_flux(const double* state, const double* dcoef, const double* dfield, int32_t nplane, int64_t ncell_member,
                     int64_t members, const int32_t* face_cell, const double* face_diag, const double* face_src,
                     int64_t nface, const int32_t* surface_begin, int32_t nsurface, const int32_t* chunks_host,
                     const int32_t* chunks_dev, int64_t nchunk, void* workspace, double* out, void* stream);

/*
 * Block sums (coarse frames; stands in for the frame stores of solver.py:1479-1494, reduced over bin x bin blocks).
 * state[nfield][members][ny * nx] is the layout of the time loop, flags[ny * nx] the flag plane of ONE member grid (only
 * QP_FLAG_ACTIVE is read).  bin = 2, 4, 8, 16, 32 or 64 is the block edge; blocks are aligned to the origin of the full
 * frame and (oy, ox), 0 <= oy, ox < bin, is the position of device cell (0, 0) inside its block, so device cell (j, i)
 * belongs to block ((oy + j) / bin, (ox + i) / bin).  out[members][nfield][cny][cnx], cny = ceil((oy + ny) / bin), cnx =
 * ceil((ox + nx) / bin): every entry is written on every call, with the sum of the plane over the active cells of the
 * block (a select, never a product: NaN or Inf outside the mask reaches no sum); a block without an active cell gives +0.0.
 * One launch, no workspace, no LDS: a wave takes 64 frame columns (lane <-> column, 8-byte loads) and max(bin, 16) frame
 * rows; a lane adds its column over the rows of a block top to bottom, an xor butterfly over the aligned group of bin
 * lanes finishes the block, one lane stores it.  The partition depends on (ny, nx, oy, ox, bin) alone and there are no
 * atomics and no completion counters: equal inputs give bitwise equal outputs, and member m of a batch gives the bits of
 * a lone call on its slice whatever the parity of ny * nx.  Any 8-byte aligned `state` will do.  state and flags are
 * only read.  Bandwidth-bound: 8 B per cell and field, 1 B per cell and field of flags (served by the caches).
 */
int qp_block_sums(const double* state, const uint8_t* flags, int32_t nfield, int32_t ny, int32_t nx, int64_t members,
                  int32_t bin, int32_t oy, int32_t ox, double* out, void* stream);

/* out[p] = sum_i state[i][p] * weights[i]  (phonon integrated occupation, solver.py:1358). */
int qp_weighted_sum(const double* state, const double* weights, int32_t n, int64_t ncell, double* out, void* stream);

/* out_val[0] = max_p |a[p]| over n doubles (convergence check of the exact-CN iteration). workspace as above. */
int qp_absmax(const double* a, int64_t n, void* workspace, double* out_val, void* stream);

/* y[i] += alpha * x[i] */
int qp_axpy(int64_t n, double alpha, const double* x, double* y, void* stream);
/* d[i] = c1 * z[i] + c2 * d[i] (d is not read when c2 == 0: it may be uninitialised); v[i] += d[i]: direction and iterate
 * update of the Chebyshev-accelerated exact-CN iteration in one pass */
int qp_cheb_update(int64_t n, double c1, const double* z, double c2, double* d, double* v, void* stream);

/*
 * Fast CN-ADI path: full ny x nx rectangle, one diffusivity per field, one boundary condition per side.
 * Replaces, for that geometry class, the whole `rhs = B u + dt D source; u = lu.solve(rhs)` loop of
 * solver.py:1443-1452 / :1545-1555 by the Peaceman-Rachford factorisation of the same Crank-Nicolson step
 * (identical when ny == 1 or nx == 1; O(dt^3) splitting term per step otherwise).
 *
 *   r          dt / (2 dx^2)
 *   dcoef_host [nfield] diffusivities (HOST pointer; tables are built on the host at plan creation)
 *   bc_diag    [4] boundary diagonal terms of the left, right, up, down sides in 1/dx^2 units (see ex/ey above)
 *   bc_src     [4] boundary source terms of the same sides (see sx/sy above)
 *   force_banded  0: when the far couplings between 64-cell chunks underflow fp64 significance (< 1e-22, true for
 *              r*D <~ 1.5) the interface unknowns are solved as independent 2x2 systems inside the sweep kernels;
 *              otherwise, or when force_banded != 0, a banded reduced solve runs between the sweeps.
 *              qp_adi_rect_plan_decoupled(plan, dir) reports which one a direction uses (1 / 0).
 * The plan owns its device tables and work planes (hipMalloc at creation, the only allocating call).
 * qp_adi_rect_steps advances u [nfield][ny*nx] in place by `nsteps` consecutive diffusion steps; intermediate
 * fields are not materialised.  Steady-state traffic: one read + one write of the field per sweep (32 B per cell-update);
 * on fine-tile plans of >= 4 Mi cells a read-only reduce pass + one fused pass per step (24 B per cell-update, same
 * results bit for bit; QPSIM_ADI_FUSED=0 / 1 at plan creation forces the choice).
 */
typedef struct qp_adi_rect_plan qp_adi_rect_plan;
int qp_adi_rect_plan_create(int32_t ny, int32_t nx, int32_t nfield, double r, const double* dcoef_host,
                            const double* bc_diag, const double* bc_src, int32_t force_banded,
                            qp_adi_rect_plan** out);
int qp_adi_rect_plan_destroy(qp_adi_rect_plan* plan);
int qp_adi_rect_plan_decoupled(const qp_adi_rect_plan* plan, int32_t dir);
/* 1 when the plan runs its passes on fine tiles (lines cut into 32-cell chunks, one wave per 32 x 64 / 64 x 32 tile:
 * undecomposed grids whose extents are multiples of 64, r*D <~ 0.32 for every field, size rule or QPSIM_FINE_TILES=1),
 * 0 for the 64 x 64 tiles.  Same results to rounding (the dropped far couplings are < 1e-22 either way). */
int qp_adi_rect_plan_fine(const qp_adi_rect_plan* plan);
/* Peaceman-Rachford iteration for the UNSPLIT Crank-Nicolson system A u = b, A = I - r D (Lx + Ly) (the matrix the
 * reference factorises with SuperLU, solver.py:231,1155-1161), on full rectangles whose Lx and Ly commute:
 *   (H + p) u* = b - (V - p) u,   (V + p) u' = b - (H - p) u*,     H = I/2 - r D Lx,  V = I/2 - r D Ly.
 * qp_adi_rect_plan_create_pr builds the plan of ONE parameter p > 0 (tables of the sweeps with r D / (1/2 + p), explicit
 * operators with the shifted diagonal; boundary sources belong to b); it runs the fine tiles where the grid qualifies
 * (extents multiples of 64, r D / (1/2 + p) <~ 0.32) and the 64 x 64 tiles - any extents, banded reduced systems for
 * stiff steps - elsewhere.  `share` (may be NULL): another plan of the same shape whose work
 * plane is borrowed - a cycle of J parameters then holds one work plane, not J; destroy the lender last.
 * qp_adi_rect_pr_iteration overwrites u with the next iterate (three passes: 8 B read + 8 B read of b + 8 B written,
 * twice, and 8 + 8 B for the last solve, per cell).  With parameters spread over the spectrum of H and V, [1/2, 1/2 +
 * r D (4 + boundary term)], J = 5-7 iterations reduce the error by 1e-13 (the host chooses them: qpsim_amd/engine.py). */
int qp_adi_rect_plan_create_pr(int32_t ny, int32_t nx, int32_t nfield, double r, const double* dcoef_host,
                               const double* bc_diag, double p, qp_adi_rect_plan* share, qp_adi_rect_plan** out);
int qp_adi_rect_pr_iteration(qp_adi_rect_plan* plan, double* u, const double* b, void* stream);
/* One whole cycle, plans[0 .. nplans) in order, u overwritten with the last iterate.  When every plan runs the fine tiles
 * the iterations are carried (the y-pass of iteration j forms the right-hand side of iteration j + 1: two passes and
 * 6 plane transfers per iteration instead of three passes and 8); otherwise one qp_adi_rect_pr_iteration per plan. */
int qp_adi_rect_pr_cycle(qp_adi_rect_plan* const* plans, int32_t nplans, double* u, const double* b, void* stream);
int qp_adi_rect_steps(qp_adi_rect_plan* plan, double* u, int32_t nsteps, void* stream);
/* qp_stencil_combine for the plan's operator without per-cell geometry arrays (positions decide which side term applies):
 * out = c0 u + cx (a Lx u) + cy (a Ly u) + cs a S + cr rin on [nfield][ny*nx]; with norm_out non-NULL also
 * norm_out[0] = max |out| (workspace: qp_pauli_workspace_bytes() bytes), which saves the exact-CN iteration its
 * separate norm pass.  (1,1,1,2,0) = CN right-hand side, (-1,1,1,0,1) = residual rin - (I - a L) u.  `out` may be NULL when
 * norm_out is given: only the norm is formed (the residual CHECK after a Peaceman-Rachford cycle: one plane less to move). */
int qp_adi_rect_combine(qp_adi_rect_plan* plan, const double* u, const double* rin, double* out, double c0, double cx,
                        double cy, double cs, double cr, void* workspace, double* norm_out, void* stream);
/* The same with norms_out[f] = max |out| of field f, f < nfield (see qp_stencil_combine_norms; any field count, launches
 * of at most 1024 fields); `out` may be NULL. */
int qp_adi_rect_combine_norms(qp_adi_rect_plan* plan, const double* u, const double* rin, double* out, double c0, double cx,
                              double cy, double cs, double cr, void* workspace, double* norms_out, void* stream);
/* x[nfield][ny*nx] <- (I - a Ly)^-1 (I - a Lx)^-1 x in place: the ADI factorisation applied as the preconditioner of
 * the exact Crank-Nicolson iteration (replaces two qp_implicit_sweep calls on full rectangles). */
int qp_adi_rect_solve(qp_adi_rect_plan* plan, double* x, void* stream);

/*
 * Domain decomposition (one rank per GPU owns a ny x nx block at offset (j0, i0) of a gny x gnx grid; offsets and
 * interior block extents are multiples of 64).  Only the decoupled-interface regime is supported across ranks
 * (QP_ERR_UNSUPPORTED otherwise): the coupling between blocks is then the same 2x2 interface system as between
 * 64-cell chunks inside a block, and each sweep needs from each neighbour one row of reduced right-hand sides
 * (nfield x nlines doubles), the entry pass one row of the field.  The host sequences the phases and moves the rows
 * (RCCL send/recv); a time step that starts from a materialised field is
 *     [set_field_halo up/down] ENTRY [iface x] REDUCED_X SWEEP_X [iface y] REDUCED_Y SWEEP_Y_EXIT
 * and consecutive steps replace SWEEP_Y_EXIT by SWEEP_Y_CARRY [iface x] REDUCED_X SWEEP_X ...
 * qp_adi_rect_phase works on undecomposed plans too (it is what qp_adi_rect_steps calls).
 */
enum {
  QP_ADI_ENTRY = 0,         /* u -> rhs of the x-solve (needs field halo rows), reduced rhs for x */
  QP_ADI_REDUCED_X = 1,     /* banded reduced solve along x (no-op in the decoupled regime) */
  QP_ADI_SWEEP_X = 2,       /* x-solve, rhs of the y-solve, reduced rhs for y */
  QP_ADI_REDUCED_Y = 3,
  QP_ADI_SWEEP_Y_CARRY = 4, /* y-solve, rhs of the next step's x-solve, reduced rhs for x */
  QP_ADI_SWEEP_Y_EXIT = 5   /* y-solve, u' stored to u */
};
int qp_adi_rect_plan_create_block(int32_t ny, int32_t nx, int32_t nfield, double r, const double* dcoef_host,
                                  const double* bc_diag, const double* bc_src, int32_t force_banded, int32_t gny,
                                  int32_t gnx, int32_t j0, int32_t i0, qp_adi_rect_plan** out);
int qp_adi_rect_phase(qp_adi_rect_plan* plan, int32_t phase, double* u, void* stream);
/* dir 0: neighbours left (side 0) / right (side 1); dir 1: up / down.  op 0 packs the row the neighbour needs into
 * buf[nfield][nlines], op 1 stores the neighbour's row into the halo slot on that side. */
int qp_adi_rect_iface_halo(qp_adi_rect_plan* plan, int32_t dir, int32_t side, int32_t op, double* buf, void* stream);
/* rows[nfield][nx]: the field row just above (side 0) / below (side 1) the block, consumed by QP_ADI_ENTRY. */
int qp_adi_rect_set_field_halo(qp_adi_rect_plan* plan, int32_t side, const double* rows, void* stream);

/*
 * Halo refresh of the overlapped-halo decomposition (one rank per GPU holds its block + halos as u[nfield][ey][ex]):
 * copies `nrect` rectangular windows between u and ONE packed buffer in a single launch, so that a refresh is
 * pack -> one batch of RCCL send/recv on persistent buffers -> unpack, with no host synchronisation in between.
 *   rects  HOST array [nrect][4] = (row0, col0, rows, cols) of each window inside the ey x ex block, nrect <= 8
 *   buf    windows back to back in `rects` order, each stored [nfield][rows][cols]
 *   op     0: pack (u -> buf), 1: unpack (buf -> u)
 * The reference has no distributed path; this serves north_star's "RCCL halo exchange over xGMI".
 */
int qp_halo_pack(double* u, int32_t nfield, int32_t ey, int32_t ex, const int32_t* rects, int32_t nrect, int32_t op,
                 double* buf, void* stream);

/*
 * Tiled CN-ADI path for MASKED grids: any mask, any per-face boundary condition, one diffusivity per field
 * (qp_adi_tile_plan_create) or a diffusivity field per energy bin (qp_adi_tile_plan_create_var).
 * Replaces the same reference loop as the rectangle path (solver.py:1443-1452 / :1545-1555) on the geometries the
 * reference actually ships (strips with holes, donuts, GDS shapes: build_laplacian_with_boundaries solver.py:152-212).
 *   flags, ex, ey, sx, sy   HOST arrays [ny*nx] with the meaning of qp_grid_desc (the plan compresses them into 16-bit
 *              per-cell codes + a table of distinct boundary terms, classifies the 64 x 64 tiles as empty / clean /
 *              general and computes the chunk-interface coefficients on the device)
 * Returns QP_ERR_UNSUPPORTED when r*D is too large for 64-cell chunks to decouple (same 1e-22 criterion as the
 * rectangle path; r*D <~ 1.3) or when there are more than 1024 distinct boundary-term combinations: the caller then
 * uses qp_stencil_combine / qp_implicit_sweep.
 * qp_adi_tile_steps: `nsteps` Peaceman-Rachford steps in place on u[nfield][ny*nx]; cells outside the mask must be 0
 * and stay 0.  qp_adi_tile_solve: x <- (I - a Ly)^-1 (I - a Lx)^-1 x (preconditioner of the exact-CN iteration).
 * qp_adi_tile_plan_info: counts[3] = empty, clean, general tiles; far = largest coupling across a chunk.
 */
typedef struct qp_adi_tile_plan qp_adi_tile_plan;
int qp_adi_tile_plan_create(int32_t ny, int32_t nx, int32_t nfield, double r, const double* dcoef_host,
                            const uint8_t* flags, const double* ex, const double* ey, const double* sx, const double* sy,
                            qp_adi_tile_plan** out);
/* Same for spatially varying diffusivity (build_variable_diffusion_laplacian, solver.py:235-321: harmonic-mean face values,
 * boundary terms scaled by the cell's D): dfield is a DEVICE array [nfield][ny*nx] read once at plan creation (face weights
 * and r*D are stored per field in the layouts the sweeps read: 4 planes per field).  Every non-empty tile is "general". */
int qp_adi_tile_plan_create_var(int32_t ny, int32_t nx, int32_t nfield, double r, const double* dfield,
                                const uint8_t* flags, const double* ex, const double* ey, const double* sx,
                                const double* sy, qp_adi_tile_plan** out);
int qp_adi_tile_plan_destroy(qp_adi_tile_plan* plan);
int qp_adi_tile_plan_info(const qp_adi_tile_plan* plan, int32_t* counts, double* far);
int qp_adi_tile_steps(qp_adi_tile_plan* plan, double* u, int32_t nsteps, void* stream);
int qp_adi_tile_solve(qp_adi_tile_plan* plan, double* x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QPSIM_HIP_H */
