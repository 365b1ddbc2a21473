// Dispatcher of the one-pass collision kernels (qp_collision_onepass.inc); the instantiations live in
// qp_collision_onepass_u*.hip (and _t*.hip: the trimmed kernels of the padded route), one (NE, process combination) per
// unit so that the build parallelises.
#include <assert.h>

#include "qp_collision_onepass.inc"

namespace qp {

QP_ONEPASS_NE_LIST(QP_DECLARE_LAUNCHERS, onepass)
QP_ONEPASS_NE_LIST(QP_DECLARE_LAUNCHERS, onepasst)
QP_ONEPASS_CLASSES_NE_LIST(QP_DECLARE_LAUNCHERS, onepassc_u0)
QP_ONEPASS_CLASSES_NE_LIST(QP_DECLARE_LAUNCHERS, onepassc_u1)

QP_DEFINE_LOOKUP(onepass, QP_ONEPASS_NE_LIST(QP_LOOKUP_CASE, onepass))
QP_DEFINE_LOOKUP(onepasst, QP_ONEPASS_NE_LIST(QP_LOOKUP_CASE, onepasst))
QP_DEFINE_LOOKUP(onepassc_u0, QP_ONEPASS_CLASSES_NE_LIST(QP_LOOKUP_CASE, onepassc_u0))
QP_DEFINE_LOOKUP(onepassc_u1, QP_ONEPASS_CLASSES_NE_LIST(QP_LOOKUP_CASE, onepassc_u1))

// The one-pass routes of collision_route.  Gap classes: the separable kernel tables (gap_sq, kr_amp, ks_amp, pair_inv)
// instead of kr0 / ks0 and their diagonal-major copies - the same kernel with K formed per lane.  Member tables
// (QP_COLL_MEMBER_CLASSES) are QP_ROUTE_ONEPASS with the member extent filled in: each block stages its member's set.
// QP_ROUTE_ONEPASS_PADDED is QP_ROUTE_ONEPASS with the launcher of the ceiling size and the live size in ne_live.
void collision_onepass_dispatch(Route route, const qp_collision_tables& t, const CollCall& c) {
  OnePassView v{};
  onepass_launcher_t fn = nullptr;
  if (route == QP_ROUTE_ONEPASS || route == QP_ROUTE_ONEPASS_PADDED) {
    v.base = CollFastView{t.kr0, t.ks0, t.rho, t.diag_bin, t.anti_bin, c.stash, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, 0.0};
    v.ksd = t.ks0_diag;
    v.kra2 = t.kr0_anti2;
    if ((t.flags & QP_COLL_MEMBER_CLASSES) && t.nclass > 1) {
      assert((c.ncell / t.nclass) % kOnePassThreads == 0 && "collision_route let a block straddle two members");
      v.member_blocks = (unsigned)(c.ncell / t.nclass / kOnePassThreads);
    }
    v.ne_live = t.ne;
    if (route == QP_ROUTE_ONEPASS) {
      fn = find_onepass(t.ne, c.s, c.r);
    } else {      // the kernel of the ceiling size; its guards start at the smallest live size that ceiling serves
      const int ceiling = qp_collision_padded_ceiling(t.ne);
      assert(t.ne >= onepass_trim_min(ceiling) && t.ne < ceiling && "live size outside the range of its ceiling's kernel");
      fn = find_onepasst(ceiling, c.s, c.r);
    }
  } else {
    v.base = CollFastView{nullptr, nullptr, t.rho, t.diag_bin, t.anti_bin, c.stash, t.cls, t.gap_sq,
                          c.r ? t.kr_amp : nullptr, c.s ? t.ks_amp : nullptr, t.pair_inv, nullptr, 0.0};
    v.nclass = t.nclass;
    fn = c.u ? find_onepassc_u1(t.ne, c.s, c.r) : find_onepassc_u0(t.ne, c.s, c.r);
  }
  assert(fn && "collision_route chose a one-pass route for a size without a launcher");
  fn(v, c);
}

}  // namespace qp
