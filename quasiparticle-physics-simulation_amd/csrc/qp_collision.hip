// Local coupled quasiparticle-phonon collision update (reference solver.py:703-791), one thread per cell.
//
// Generic table-driven kernel: any NE, any phonon-bin map, per-cell gap classes.  State planes are
// [bin][cell], so every load/store of a plane element is coalesced across the wave.  The per-cell phonon
// accumulators a, b live in a scratch plane set [2][nw][ncell] (each thread only touches its own column).
#include <stdlib.h>

#include "qp_collision_dispatch.h"

namespace qp {

struct CollView {
  int ne, nw, nclass;
  const double* kr0;
  const double* ks0;
  const double* rho;
  const int32_t* idx_diff;
  const int32_t* idx_sum;
  const int8_t* sign;
  const int32_t* cls;
};

__global__ void __launch_bounds__(256) collision_generic_kernel(CollView t, const uint8_t* __restrict__ flags,
                                                                long ncell, const double* __restrict__ sin_,
                                                                double* __restrict__ sout, double* __restrict__ ph,
                                                                double* __restrict__ acc, double dE, double dt,
                                                                int en_r, int en_s, int upd_ph) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= ncell) return;
  const int NE = t.ne, NW = t.nw;
  if (!(flags[p] & QP_FLAG_ACTIVE)) {
    for (int i = 0; i < NE; ++i) sout[(long)i * ncell + p] = sin_[(long)i * ncell + p];
    return;
  }
  const int c = t.cls ? t.cls[p] : 0;
  const double* rho = t.rho + (long)c * NE;
  const double* kr = t.kr0 ? t.kr0 + (long)c * NE * NE : nullptr;
  const double* ks = t.ks0 ? t.ks0 + (long)c * NE * NE : nullptr;
  const bool use_r = en_r && kr;
  const bool use_s = en_s && ks;

  // ---- quasiparticle update: gain / loss rates from the OLD n and p ----
  for (int i = 0; i < NE; ++i) {
    const double ni = sin_[(long)i * ncell + p];
    const double rho_i = rho[i];
    const double qi = rho_i * fmax(1.0 - ni / fmax(rho_i, 1e-30), 0.0);
    double g_s = 0.0, l_s = 0.0, g_r = 0.0, l_r = 0.0;
    for (int j = 0; j < NE; ++j) {
      const double nj = sin_[(long)j * ncell + p];
      const double rho_j = rho[j];
      const double qj = rho_j * fmax(1.0 - nj / fmax(rho_j, 1e-30), 0.0);
      if (use_s && j != i) {
        // the reference's own maps are symmetric in (i, j); caller-supplied tables of the step API need not be
        const double pd_ij = ph[(long)t.idx_diff[i * NE + j] * ncell + p];
        const double pd_ji = ph[(long)t.idx_diff[j * NE + i] * ncell + p];
        const double np_ij = t.sign[i * NE + j] > 0 ? 1.0 + pd_ij : pd_ij;
        const double np_ji = t.sign[j * NE + i] > 0 ? 1.0 + pd_ji : pd_ji;
        g_s += ks[j * NE + i] * np_ji * nj;
        l_s += ks[i * NE + j] * np_ij * qj;
      }
      if (use_r) {
        const double ps = ph[(long)t.idx_sum[i * NE + j] * ncell + p];
        const double k = kr[i * NE + j];
        l_r += k * (1.0 + ps) * nj;
        g_r += k * ps * qj;
      }
    }
    const double gain = dE * qi * g_s + 2.0 * dE * qi * g_r;
    const double loss = dE * l_s + 2.0 * dE * l_r;
    sout[(long)i * ncell + p] = relax_update(ni, gain, loss, dt);
  }
  if (!upd_ph || !(en_r || en_s)) return;

  // ---- phonon update: bin the pair rates (bincount of solver.py:758-788) ----
  double* A = acc;
  double* B = acc + (long)NW * ncell;
  for (int w = 0; w < NW; ++w) {
    A[(long)w * ncell + p] = 0.0;
    B[(long)w * ncell + p] = 0.0;
  }
  for (int i = 0; i < NE; ++i) {
    const double ni = sin_[(long)i * ncell + p];
    const double rho_i = rho[i];
    const double qi = rho_i * fmax(1.0 - ni / fmax(rho_i, 1e-30), 0.0);
    for (int j = 0; j < NE; ++j) {
      const double nj = sin_[(long)j * ncell + p];
      const double rho_j = rho[j];
      const double qj = rho_j * fmax(1.0 - nj / fmax(rho_j, 1e-30), 0.0);
      if (use_s && j != i) {
        const long w = (long)t.idx_diff[i * NE + j] * ncell + p;
        const double base = dE * (ni * ks[i * NE + j] * qj);
        const int sg = t.sign[i * NE + j];
        if (sg > 0) {
          A[w] += base;
          B[w] += base;
        } else if (sg < 0) {
          B[w] -= base;
        }
      }
      if (use_r) {
        const long w = (long)t.idx_sum[i * NE + j] * ncell + p;
        const double k = kr[i * NE + j];
        const double rec = dE * (ni * k * nj);
        const double pb = dE * (qi * k * qj);
        A[w] += rec;
        B[w] += rec - pb;
      }
    }
  }
  for (int w = 0; w < NW; ++w) {
    const long o = (long)w * ncell + p;
    ph[o] = affine_update(ph[o], A[o], B[o], dt);
  }
}

// ---- which sizes have a launcher: generated from the lists the launchers themselves are generated from ---------------
#define QP_DEFINE_SUPPORTED(NAME, LISTS) \
  int NAME(int ne) {                     \
    switch (ne) {                        \
      LISTS return 1;                    \
      default: return 0;                 \
    }                                    \
  }
QP_DEFINE_SUPPORTED(collision_fast_supported, QP_DIAG_NE_LIST(QP_NE_CASE, _))
QP_DEFINE_SUPPORTED(collision_fast_classes_supported, QP_DIAGP_NE_LIST(QP_NE_CASE, _) QP_DIAGP_NE_LIST_EXT(QP_NE_CASE, _))
QP_DEFINE_SUPPORTED(collision_member_tables_supported, QP_MEMBER_NE_LIST(QP_NE_CASE, _))
QP_DEFINE_SUPPORTED(collision_pair_supported, QP_PAIR_NE_LIST(QP_NE_CASE, _))
QP_DEFINE_SUPPORTED(collision_onepass_supported, QP_ONEPASS_NE_LIST(QP_NE_CASE, _))
QP_DEFINE_SUPPORTED(collision_onepass_classes_supported, QP_ONEPASS_CLASSES_NE_LIST(QP_NE_CASE, _))

static bool onepass_enabled() {      // QPSIM_COLL_ONEPASS=0: the three-launch split kernels (A/B timing, tests)
  const char* e = getenv("QPSIM_COLL_ONEPASS");
  return !e || atoi(e) != 0;
}

// QP_COLL_WIDE_BINS takes effect: the route needs no ph_scratch (validate_step_tables asks the same question)
static bool wide_bins_ok(const qp_collision_tables& t) {
  return (t.flags & QP_COLL_WIDE_BINS) && !(t.flags & QP_COLL_FORCE_GENERIC) && qp_collision_wide_available(t.ne, t.nw);
}

// The whole rule for which kernel family serves a single collision step, first match wins.
Route collision_route(const qp_collision_tables& t, long ncell, bool en_r, bool en_s, bool upd, bool have_scratch) {
  const bool s = en_s && t.ks0, r = en_r && t.kr0;       // effective processes
  const bool member_classes = (t.flags & QP_COLL_MEMBER_CLASSES) && t.nclass > 1;
  const bool gap_classes = t.nclass > 1 && !member_classes;
  // merged bins (QP_COLL_SHARED_BINS): the register kernels park per-diagonal sums in ph_scratch (2 planes per merged bin);
  // without scratch only the variants that never write phonons qualify
  const bool shared_ok = !(t.flags & QP_COLL_SHARED_BINS) || have_scratch || !(upd && s && r);
  // every register-resident family: structured bin maps, no FORCE bit, 32-bit pixel offsets
  const bool reg = t.diag_bin && !(t.flags & (QP_COLL_FORCE_GENERIC | QP_COLL_FORCE_WAVE)) && shared_ok && ncell < (1L << 28);

  if (reg && t.nclass == 1) {
    // ne = 30, 32, 40, 50 with the diagonal-major tables of the enabled processes: one launch (instead of the three of the
    // split for ne >= 32)
    if (collision_onepass_supported(t.ne) && (s || r) && (!s || t.ks0_diag) && (!r || t.kr0_anti2) && onepass_enabled())
      return QP_ROUTE_ONEPASS;
    // no process enabled: relaxation with zero gain and loss, which the copy kernel does for any tables
    if (collision_fast_supported(t.ne)) return (s || r) ? QP_ROUTE_REGISTER : QP_ROUTE_COPY;
  }
  // one table per ensemble member: the register kernels that pick the wave's table, where no wave straddles two members;
  // every other member-class table runs the one-wave-per-pixel or generic kernel below through `cls`
  if (reg && member_classes && collision_member_tables_supported(t.ne) && (ncell / t.nclass) % 64 == 0 && (s || r))
    return QP_ROUTE_REGISTER_MEMBERS;
  // ... and at ne = 30, 32, 40, 50 the one-pass kernel, whose 256-pixel blocks stage the tables of their member: no block
  // may straddle two members, and the diagonal-major tables are one per member as well.  No member form of the split kernels
  if (reg && member_classes && collision_onepass_supported(t.ne) && (s || r) && (!s || t.ks0_diag) && (!r || t.kr0_anti2) &&
      onepass_enabled() && (ncell / t.nclass) % 256 == 0)
    return QP_ROUTE_ONEPASS;
  // padded bins (opt-in, QP_COLL_PAD_BINS): a size without a kernel of its own runs the one-pass kernel of its ceiling size
  // on the live bins; one class, or member classes under the same 256-cell rule.  Everything else falls through as without
  // the flag
  if ((t.flags & QP_COLL_PAD_BINS) && reg && (t.nclass == 1 || (member_classes && (ncell / t.nclass) % 256 == 0)) &&
      (s || r) && (!s || t.ks0_diag) && (!r || t.kr0_anti2) && qp_collision_padded_ceiling(t.ne) != 0 && onepass_enabled())
    return QP_ROUTE_ONEPASS_PADDED;
  // gap classes with the separable kernel tables: the one-pass kernel where it exists ...
  if (reg && gap_classes && t.cls && t.gap_sq && t.pair_inv) {
    if (collision_onepass_classes_supported(t.ne) && t.nclass <= kOnePassMaxClasses && (s || r) && (!s || t.ks_amp) &&
        (!r || t.kr_amp) && onepass_enabled())
      return QP_ROUTE_ONEPASS_CLASSES;
    // ... else the register kernels that form K per pixel; their processes are those with an amplitude table
    if ((!r || t.kr_amp) && (!s || t.ks_amp) && ((en_s && t.ks_amp) || (en_r && t.kr_amp)) &&
        collision_fast_classes_supported(t.ne))
      return QP_ROUTE_REGISTER_CLASSES;
  }
  // NE <= 64: one wave per pixel (any class map; LDS atomics unless the host vouched for the bin-map structure)
  if (!(t.flags & QP_COLL_FORCE_GENERIC) && t.ne <= 64 && t.nw <= 192) return QP_ROUTE_WAVE;
  // wide bins (opt-in, QP_COLL_WIDE_BINS): 65 <= NE <= 128 with two energy bins per lane; without the flag, and outside the
  // query's range, the generic kernel as ever
  if (wide_bins_ok(t)) return QP_ROUTE_WAVE_WIDE;
  return QP_ROUTE_GENERIC;
}

// The double half-step kernel: NE = 4 ... 16, one gap class or member tables, structured unmerged bin maps, a process.
PairRoute collision_pair_route(const qp_collision_tables& t, long ncell, bool s, bool r) {
  const bool memb = (t.flags & QP_COLL_MEMBER_CLASSES) && t.nclass > 1;
  if (!collision_pair_supported(t.ne) || (t.nclass != 1 && !memb) || !t.diag_bin || !t.anti_bin || !(s || r))
    return PairRoute::None;
  if ((t.flags & (QP_COLL_FORCE_GENERIC | QP_COLL_FORCE_WAVE | QP_COLL_SHARED_BINS)) || ncell >= (1L << 28))
    return PairRoute::None;
  if (!memb) return PairRoute::Shared;
  // one table per member: no wave may straddle two members
  const bool fits = collision_member_tables_supported(t.ne) && ncell % t.nclass == 0 && (ncell / t.nclass) % 64 == 0;
  return fits ? PairRoute::Members : PairRoute::None;
}

}  // namespace qp

// ---------------------------------------------------------------------------------------------------------
// Entry points.  `who` is the exported function the caller used: every message names it.
// ---------------------------------------------------------------------------------------------------------
#define QP_REQUIRE_AS(who, cond, msg)         \
  do {                                        \
    if (!(cond)) {                            \
      qp::set_error("%s: %s", who, msg);      \
      return QP_ERR_INVALID_ARGUMENT;         \
    }                                         \
  } while (0)

// What every collision entry point checks of its tables before it reads further.
static int validate_tables(const qp_collision_tables* t, int64_t ncell, const char* who) {
  QP_REQUIRE_AS(who, t != nullptr, "tables are NULL");
  if (t->struct_size != sizeof(qp_collision_tables)) {
    qp::set_error("%s: qp_collision_tables.struct_size is %u, this library expects %zu (binding built against another "
                  "header revision)", who, t->struct_size, sizeof(qp_collision_tables));
    return QP_ERR_INVALID_ARGUMENT;
  }
  QP_REQUIRE_AS(who, ncell > 0 && t->rho != nullptr, "ncell must be positive, rho non-NULL");
  // QP_COLL_MEMBER_CLASSES: the cells divide evenly among the classes, and the class map of the fallback kernels is there
  if (t->flags & QP_COLL_MEMBER_CLASSES) {
    if (t->nclass <= 0 || ncell % t->nclass != 0) {
      qp::set_error("%s: QP_COLL_MEMBER_CLASSES needs ncell (%lld) to be a multiple of nclass (%d)", who, (long long)ncell,
                    t->nclass);
      return QP_ERR_INVALID_ARGUMENT;
    }
    QP_REQUIRE_AS(who, t->cls, "QP_COLL_MEMBER_CLASSES needs cls (the kernels without member tables read it)");
  }
  return QP_OK;
}

// ... and what the single-step family (and the route query) asks on top: all its kernels walk the bin maps
static int validate_step_tables(const qp_collision_tables* t, int64_t ncell, int en_r, int en_s, int upd, bool have_scratch,
                                const char* who) {
  if (const int rc = validate_tables(t, ncell, who)) return rc;
  QP_REQUIRE_AS(who, t->ne > 0 && t->nw > 0 && t->nclass > 0, "ne, nw, nclass must be positive");
  QP_REQUIRE_AS(who, t->idx_diff && t->idx_sum && t->sign, "idx maps / sign must be non-NULL");
  QP_REQUIRE_AS(who, t->nclass == 1 || t->cls, "cls is required when nclass > 1");
  const bool no_scratch_ok = (!(t->flags & QP_COLL_FORCE_GENERIC) && t->ne <= 64 && t->nw <= 192) || qp::wide_bins_ok(*t);
  QP_REQUIRE_AS(who, !(upd && (en_r || en_s)) || have_scratch || no_scratch_ok,
                "ph_scratch is required when phonons are updated by the generic kernel");
  QP_REQUIRE_AS(who, (t->diag_bin == nullptr) == (t->anti_bin == nullptr), "diag_bin and anti_bin come together");
  return QP_OK;
}

extern "C" int qp_collision_route(const qp_collision_tables* t, int64_t ncell, int enable_recombination,
                                  int enable_scattering, int update_phonons, int have_scratch) {
  if (const int rc = validate_step_tables(t, ncell, enable_recombination, enable_scattering, update_phonons,
                                          have_scratch != 0, "qp_collision_route"))
    return rc;
  return qp::collision_route(*t, (long)ncell, enable_recombination, enable_scattering, update_phonons, have_scratch != 0);
}

// One collision step for the exported function `who`; *route_out (may be NULL) receives the route that ran.
static int collision_step_impl(const char* who, const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                               const double* state_in, double* state_out, double* phonon, double* ph_scratch, double dE,
                               double dt, int en_r, int en_s, int upd, qp::PauliPartial* guard, double guard_floor,
                               qp::Route* route_out, void* stream) {
  if (const int rc = validate_step_tables(t, ncell, en_r, en_s, upd, ph_scratch != nullptr, who)) return rc;
  QP_REQUIRE_AS(who, flags && state_in && state_out && phonon, "flags, state_in, state_out, phonon must be non-NULL");
  QP_REQUIRE_AS(who, state_in != state_out, "state_in and state_out must not alias");
  const qp::Route route = qp::collision_route(*t, (long)ncell, en_r, en_s, upd, ph_scratch != nullptr);
  if (route_out) *route_out = route;
  // the gap-class register kernels take their processes from the amplitude tables
  const bool classes = route == QP_ROUTE_REGISTER_CLASSES;
  const bool s = en_s && (classes ? t->ks_amp : t->ks0), r = en_r && (classes ? t->kr_amp : t->kr0);
  const qp::CollCall c{flags, (long)ncell, state_in, state_out, phonon, ph_scratch, dE, dt, 0.0, 0.0, s, r, upd && (s || r),
                       guard, guard_floor, (hipStream_t)stream};
  switch (route) {
    case QP_ROUTE_ONEPASS:
    case QP_ROUTE_ONEPASS_CLASSES:
    case QP_ROUTE_ONEPASS_PADDED:
      qp::collision_onepass_dispatch(route, *t, c);
      break;
    case QP_ROUTE_REGISTER:
    case QP_ROUTE_REGISTER_MEMBERS:
    case QP_ROUTE_REGISTER_CLASSES:
    case QP_ROUTE_COPY:
      qp::collision_fast_dispatch(route, *t, c);
      break;
    case QP_ROUTE_WAVE: {
      const qp::WaveCollView wv{t->ne, t->nw, t->nclass, t->kr0, t->ks0, t->rho, t->idx_diff, t->idx_sum, t->sign, t->cls,
                                t->diag_bin, t->anti_bin};
      qp::collision_wave_dispatch(wv, t->diag_bin != nullptr, c);
      break;
    }
    case QP_ROUTE_WAVE_WIDE: {
      const qp::WaveCollView wv{t->ne, t->nw, t->nclass, t->kr0, t->ks0, t->rho, t->idx_diff, t->idx_sum, t->sign, t->cls,
                                t->diag_bin, t->anti_bin};
      qp::collision_wave_wide_dispatch(wv, t->diag_bin != nullptr, c);
      break;
    }
    case QP_ROUTE_GENERIC: {    // the kernel tests the caller's switches itself (it also rewrites phonons with no table)
      const qp::CollView v{t->ne, t->nw, t->nclass, t->kr0, t->ks0, t->rho, t->idx_diff, t->idx_sum, t->sign, t->cls};
      hipLaunchKernelGGL(qp::collision_generic_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0,
                         (hipStream_t)stream, v, flags, (long)ncell, state_in, state_out, phonon, ph_scratch, dE, dt, en_r,
                         en_s, upd);
      break;
    }
  }
  return qp::check_launch(who);
}

extern "C" int qp_collision_step(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                 const double* state_in, double* state_out, double* phonon, double* ph_scratch,
                                 double dE, double dt, int enable_recombination, int enable_scattering,
                                 int update_phonons, void* stream) {
  return collision_step_impl("qp_collision_step", t, flags, ncell, state_in, state_out, phonon, ph_scratch, dE, dt,
                             enable_recombination, enable_scattering, update_phonons, nullptr, 0.0, nullptr, stream);
}

extern "C" int64_t qp_collision_guard_workspace_bytes(int64_t ncell) {
  // the register kernels launch ceil(ncell / 128) blocks of two waves and EVERY wave writes a partial (also the second wave
  // of a last block that holds <= 64 cells), so the count follows the launch geometry, not ceil(ncell / 64)
  const int64_t waves = 2 * ((ncell + 127) / 128) + qp::kGuardMergeBlocks;
  const int64_t fused = waves * (int64_t)sizeof(qp::PauliPartial);
  const int64_t plain = qp_pauli_workspace_bytes();
  return fused > plain ? fused : plain;
}

// ---------------------------------------------------------------------------------------------------------
// Explicit (forward-Euler) fixed-bath collision helpers of the reference's public step API
// (solver.py:551-580 apply_scattering_step, :583-605 apply_recombination_step, :608-637 _collision_rhs).
// They are not called by the reference's time loop; kept for API parity.  One thread per cell, generic NE.
// ---------------------------------------------------------------------------------------------------------
namespace qp {

__global__ void __launch_bounds__(256) euler_collision_kernel(int ne, long ncell, const double* __restrict__ sin_,
                                                              double* __restrict__ out, const double* __restrict__ kr,
                                                              const double* __restrict__ g_therm,
                                                              const double* __restrict__ ks,
                                                              const double* __restrict__ rho, double dE, double dt,
                                                              int rhs_only) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= ncell) return;
  for (int i = 0; i < ne; ++i) {
    const double ni = sin_[(long)i * ncell + p];
    double rhs = 0.0;
    if (kr && g_therm) {
      double acc = 0.0;
      for (int j = 0; j < ne; ++j) acc += kr[i * ne + j] * sin_[(long)j * ncell + p];
      rhs += g_therm[i] - 2.0 * ni * dE * acc;
    }
    if (ks && rho) {
      const double bi = fmax(1.0 - ni / fmax(rho[i], 1e-30), 0.0);
      double gin = 0.0, gout = 0.0;
      for (int j = 0; j < ne; ++j) {
        const double nj = sin_[(long)j * ncell + p];
        const double bj = fmax(1.0 - nj / fmax(rho[j], 1e-30), 0.0);
        gin += ks[j * ne + i] * nj;
        gout += ks[i * ne + j] * rho[j] * bj;
      }
      rhs += dE * rho[i] * bi * gin - ni * dE * gout;
    }
    out[(long)i * ncell + p] = rhs_only ? rhs : fmax(ni + dt * rhs, 0.0);
  }
}

}  // namespace qp

extern "C" int qp_euler_collision(int32_t ne, int64_t ncell, const double* state_in, double* out, const double* kr,
                                  const double* g_therm, const double* ks, const double* rho, double dE, double dt,
                                  int rhs_only, void* stream) {
  QP_REQUIRE(ne > 0 && ncell > 0 && state_in && out && state_in != out, "bad arguments (state_in and out must differ)");
  QP_REQUIRE((kr == nullptr) == (g_therm == nullptr), "kr and g_therm come together");
  QP_REQUIRE((ks == nullptr) == (rho == nullptr), "ks and rho come together");
  hipLaunchKernelGGL(qp::euler_collision_kernel, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (int)ne, (long)ncell, state_in, out, kr, g_therm, ks, rho, dE, dt, rhs_only);
  return qp::check_launch("qp_euler_collision");
}

// 1 when the register-resident collision kernel is instantiated for this number of energy bins
extern "C" int qp_collision_register_kernel_available(int32_t ne) { return qp::collision_fast_supported(ne); }

extern "C" int qp_collision_pair_available(int32_t ne) { return qp::collision_pair_supported(ne); }

// 1 when the single-pass and double half-step register kernels exist in their member-table form (QP_COLL_MEMBER_CLASSES)
extern "C" int qp_collision_member_tables_available(int32_t ne) { return qp::collision_member_tables_supported(ne); }

extern "C" int qp_collision_onepass_available(int32_t ne) { return qp::collision_onepass_supported(ne); }

// The one-pass kernel that serves `ne` live bins under QP_COLL_PAD_BINS: the smallest instantiated size above ne, for the
// sizes between 17 and 49 that have neither a one-pass nor a register kernel of their own
extern "C" int qp_collision_padded_ceiling(int32_t ne) {
  if (ne <= 16 || ne >= 50 || qp::collision_onepass_supported(ne) || qp::collision_fast_supported(ne)) return 0;
  return ne < 30 ? 30 : ne < 32 ? 32 : ne < 40 ? 40 : 50;
}

// The two-bins-per-lane wave kernel (QP_COLL_WIDE_BINS): lane l owns bins l and l + 64, and up to 8 phonon bins
extern "C" int qp_collision_wide_available(int32_t ne, int32_t nw) { return ne >= 65 && ne <= 128 && nw >= 1 && nw <= 512; }

// 1 when the gap-class variant (separable kernel tables, qp_collision_tables::gap_sq ...) exists as well
extern "C" int qp_collision_register_kernel_classes(int32_t ne) { return qp::collision_fast_classes_supported(ne); }

// ---------------------------------------------------------------------------------------------------------
// The guarded calls.  The register and pair kernels write one guard partial per wave of 64 consecutive pixels.  The plain
// calls reduce them all (pauli_finish).  The ensemble calls (`per_member`) reduce them per member (qp_pauli_stats_members
// semantics): with ncell_member % 64 == 0 no wave straddles two members, so one finishing block per member groups them
// (64 w / ncell_member) without another pass over the state.  The plain call is the case of one member that owns all cells.
// ---------------------------------------------------------------------------------------------------------
struct GuardOut {
  void* workspace;
  bool per_member;
  int64_t ncell_member, members;
  double* vals;
  int64_t* idx;
};

static int guard_out_ok(const GuardOut& g, int64_t ncell, const char* who) {
  QP_REQUIRE_AS(who, g.workspace && g.vals && g.idx, "guard_workspace, out_vals, out_idx must be non-NULL");
  if (g.per_member && (g.ncell_member <= 0 || g.members <= 0 || g.ncell_member * g.members != ncell)) {
    qp::set_error("%s: ncell (%lld) must equal ncell_member (%lld) * members (%lld)", who, (long long)ncell,
                  (long long)g.ncell_member, (long long)g.members);
    return QP_ERR_INVALID_ARGUMENT;
  }
  return QP_OK;
}

// finishes the reduction of the per-wave partials the collision kernel of this call has written (128-thread blocks)
static int guard_finish(const GuardOut& g, int64_t ncell, const char* who, void* stream) {
  auto* parts = (qp::PauliPartial*)g.workspace;
  if (g.per_member)
    qp::pauli_finish_members(parts + qp::kGuardMergeBlocks, (long)g.ncell_member, (long)g.members, g.vals, (long*)g.idx,
                             (hipStream_t)stream);
  else
    qp::pauli_finish(parts + qp::kGuardMergeBlocks, ((long)ncell + 127) / 128 * 2, parts, g.vals, (long*)g.idx,
                     (hipStream_t)stream);
  return qp::check_launch(who);
}

static int step_guarded_impl(const char* who, const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                             const double* state_in, double* state_out, double* phonon, double* ph_scratch, double dE,
                             double dt, int en_r, int en_s, int upd, double density_floor, const GuardOut& g, void* stream) {
  if (const int rc = guard_out_ok(g, ncell, who)) return rc;
  // a wave's partial belongs to one member only when the members are wave-aligned
  const bool aligned = !g.per_member || g.ncell_member % 64 == 0;
  qp::PauliPartial* const parts = aligned ? (qp::PauliPartial*)g.workspace + qp::kGuardMergeBlocks : nullptr;
  qp::Route route;
  if (const int rc = collision_step_impl(who, t, flags, ncell, state_in, state_out, phonon, ph_scratch, dE, dt, en_r, en_s,
                                         upd, parts, density_floor, &route, stream))
    return rc;
  if (parts && qp::route_writes_guard(route, t->ne)) return guard_finish(g, ncell, who, stream);
  // kernels without the fused epilogue (split kernels of NE >= 32, one-pass, copy, wave and generic kernels): separate pass
  if (g.per_member)
    return qp_pauli_stats_members(state_out, t->rho, t->cls, flags, t->ne, t->nclass, g.ncell_member, g.members,
                                  density_floor, g.workspace, g.vals, g.idx, stream);
  return qp_pauli_stats(state_out, t->rho, t->cls, flags, t->ne, t->nclass, ncell, density_floor, g.workspace, g.vals, g.idx,
                        stream);
}

static int double_step_guarded_impl(const char* who, const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                    const double* state_in, double* state_out, double* phonon, double dE, double dt_first,
                                    double dt_second, double gen_amount, int en_r, int en_s, int upd, double density_floor,
                                    const GuardOut& g, void* stream) {
  if (const int rc = validate_tables(t, ncell, who)) return rc;
  QP_REQUIRE_AS(who, flags && state_in && state_out && phonon && state_in != state_out,
                "flags, state_in, state_out (distinct), phonon");
  if (const int rc = guard_out_ok(g, ncell, who)) return rc;
  if (g.per_member && g.ncell_member % 64 != 0) {
    qp::set_error("%s: ncell_member (%lld) is not a multiple of 64", who, (long long)g.ncell_member);
    return QP_ERR_UNSUPPORTED;
  }
  const bool s = en_s && t->ks0, r = en_r && t->kr0;
  const qp::PairRoute route = qp::collision_pair_route(*t, (long)ncell, s, r);
  if (route == qp::PairRoute::None) {
    qp::set_error("%s: no fused double half-step kernel for these tables (ne = %d, ncell = %lld)", who, t->ne,
                  (long long)ncell);
    return QP_ERR_UNSUPPORTED;
  }
  const qp::CollCall c{flags, (long)ncell, state_in, state_out, phonon, nullptr, dE, dt_first, dt_second, gen_amount, s, r,
                       upd && (s || r), (qp::PauliPartial*)g.workspace + qp::kGuardMergeBlocks, density_floor,
                       (hipStream_t)stream};
  qp::collision_pair_dispatch(route, *t, c);
  return guard_finish(g, ncell, who, stream);
}

extern "C" int qp_collision_step_guarded(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                         const double* state_in, double* state_out, double* phonon, double* ph_scratch,
                                         double dE, double dt, int enable_recombination, int enable_scattering,
                                         int update_phonons, double density_floor, void* guard_workspace,
                                         double* out_vals, int64_t* out_idx, void* stream) {
  return step_guarded_impl("qp_collision_step_guarded", t, flags, ncell, state_in, state_out, phonon, ph_scratch, dE, dt,
                           enable_recombination, enable_scattering, update_phonons, density_floor,
                           {guard_workspace, false, ncell, 1, out_vals, out_idx}, stream);
}

extern "C" int qp_collision_step_guarded_members(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                                 const double* state_in, double* state_out, double* phonon,
                                                 double* ph_scratch, double dE, double dt, int enable_recombination,
                                                 int enable_scattering, int update_phonons, double density_floor,
                                                 void* guard_workspace, int64_t ncell_member, int64_t members,
                                                 double* out_vals, int64_t* out_idx, void* stream) {
  return step_guarded_impl("qp_collision_step_guarded_members", t, flags, ncell, state_in, state_out, phonon, ph_scratch, dE,
                           dt, enable_recombination, enable_scattering, update_phonons, density_floor,
                           {guard_workspace, true, ncell_member, members, out_vals, out_idx}, stream);
}

extern "C" int qp_collision_double_step_guarded(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                                const double* state_in, double* state_out, double* phonon, double dE,
                                                double dt_first, double dt_second, double gen_amount,
                                                int enable_recombination, int enable_scattering, int update_phonons,
                                                double density_floor, void* guard_workspace, double* out_vals,
                                                int64_t* out_idx, void* stream) {
  return double_step_guarded_impl("qp_collision_double_step_guarded", t, flags, ncell, state_in, state_out, phonon, dE,
                                  dt_first, dt_second, gen_amount, enable_recombination, enable_scattering, update_phonons,
                                  density_floor, {guard_workspace, false, ncell, 1, out_vals, out_idx}, stream);
}

extern "C" int qp_collision_double_step_guarded_members(const qp_collision_tables* t, const uint8_t* flags, int64_t ncell,
                                                        const double* state_in, double* state_out, double* phonon,
                                                        double dE, double dt_first, double dt_second, double gen_amount,
                                                        int enable_recombination, int enable_scattering, int update_phonons,
                                                        double density_floor, void* guard_workspace, int64_t ncell_member,
                                                        int64_t members, double* out_vals, int64_t* out_idx, void* stream) {
  return double_step_guarded_impl("qp_collision_double_step_guarded_members", t, flags, ncell, state_in, state_out, phonon,
                                  dE, dt_first, dt_second, gen_amount, enable_recombination, enable_scattering,
                                  update_phonons, density_floor,
                                  {guard_workspace, true, ncell_member, members, out_vals, out_idx}, stream);
}
