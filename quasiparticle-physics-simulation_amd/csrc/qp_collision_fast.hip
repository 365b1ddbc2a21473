// Dispatcher of the register-resident collision kernels (qp_collision_fast.inc) + the instantiations for NE <= 16.
// Larger NE live in qp_collision_fast_u*.hip, the member-table forms in qp_collision_fast_m*.hip; every NE of a list in
// qp_collision_dispatch.h has all process combinations.
#include <assert.h>

#include "qp_collision_fast.inc"

namespace qp {

// one gap class: the sizes of this unit (NE <= 16, which is QP_DIAGP_NE_LIST), the rest declared
QP_DIAGP_NE_LIST(QP_DEFINE_LAUNCHERS, diag)
QP_DIAG_NE_LIST(QP_DECLARE_LAUNCHERS, diag)

// gap classes (PARAM): the same sizes here, the rest declared
QP_DIAGP_NE_LIST(QP_DEFINE_LAUNCHERS, diagp)
QP_DIAGP_NE_LIST_EXT(QP_DECLARE_LAUNCHERS, diagp)

QP_MEMBER_NE_LIST(QP_DECLARE_LAUNCHERS, diagm)

QP_DEFINE_LOOKUP(diag, QP_DIAG_NE_LIST(QP_LOOKUP_CASE, diag))
QP_DEFINE_LOOKUP(diagp, QP_DIAGP_NE_LIST(QP_LOOKUP_CASE, diagp) QP_DIAGP_NE_LIST_EXT(QP_LOOKUP_CASE, diagp))
QP_DEFINE_LOOKUP(diagm, QP_MEMBER_NE_LIST(QP_LOOKUP_CASE, diagm))

__global__ void __launch_bounds__(256) collision_none_kernel(const uint8_t* __restrict__ flags, long ncell, long total,
                                                             const double* __restrict__ sin_, double* __restrict__ sout) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const double v = sin_[t];
  sout[t] = (flags[t % ncell] & QP_FLAG_ACTIVE) ? fmax(v, 0.0) : v;
}

// The register routes of collision_route.  The fused Pauli guard (c.guard, may be NULL) is written by the single-pass
// kernels, not by the split kernels of NE >= 32 or the copy: route_writes_guard.
void collision_fast_dispatch(Route route, const qp_collision_tables& t, const CollCall& c) {
  PauliPartial* const guard = t.ne < 32 ? c.guard : nullptr;
  coll_launcher_t fn = nullptr;
  CollFastViewM v{};
  switch (route) {
    case QP_ROUTE_COPY: {       // no process: relaxation with zero gain and loss, n' = max(n, 0) on active cells
      const long total = c.ncell * t.ne;
      hipLaunchKernelGGL(collision_none_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.stream, c.flags,
                         c.ncell, total, c.sin, c.sout);
      return;
    }
    case QP_ROUTE_REGISTER:
      v = {{t.kr0, t.ks0, t.rho, t.diag_bin, t.anti_bin, c.stash, nullptr, nullptr, nullptr, nullptr, nullptr, guard,
            c.guard_floor}, 0, 0};
      fn = find_diag(t.ne, c.s, c.r);
      break;
    case QP_ROUTE_REGISTER_CLASSES:     // `rho` is [nclass][ne]; kr_amp / ks_amp stand in for kr0 / ks0 (NULL = process off)
      v = {{nullptr, nullptr, t.rho, t.diag_bin, t.anti_bin, c.stash, t.cls, t.gap_sq, c.r ? t.kr_amp : nullptr,
            c.s ? t.ks_amp : nullptr, t.pair_inv, guard, c.guard_floor}, 0, 0};
      fn = find_diagp(t.ne, c.s, c.r);
      break;
    case QP_ROUTE_REGISTER_MEMBERS:     // kr0 / ks0 / rho hold `nclass` tables, class k owns the cells [k, k + 1) ncell / nclass
      v = {{t.kr0, t.ks0, t.rho, t.diag_bin, t.anti_bin, c.stash, nullptr, nullptr, nullptr, nullptr, nullptr, c.guard,
            c.guard_floor}, (unsigned)(c.ncell / t.nclass), (unsigned)t.nclass};
      fn = find_diagm(t.ne, c.s, c.r);
      break;
    default: break;
  }
  assert(fn && "collision_route chose a register route for a size without a launcher");
  fn(v, c);
}

}  // namespace qp
