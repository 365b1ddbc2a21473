// Instantiations + dispatcher of the double half-step collision kernel (qp_collision_pair.inc): NE = 4 ... 16.
#include <assert.h>

#include "qp_collision_pair.inc"

namespace qp {

QP_PAIR_NE_LIST(QP_DEFINE_LAUNCHERS, pair)

// the same sizes with per-member tables (QP_COLL_MEMBER_CLASSES), instantiated in qp_collision_pair_m*.hip
QP_MEMBER_NE_LIST(QP_DECLARE_LAUNCHERS, pairm)

QP_DEFINE_LOOKUP(pair, QP_PAIR_NE_LIST(QP_LOOKUP_CASE, pair))
QP_DEFINE_LOOKUP(pairm, QP_MEMBER_NE_LIST(QP_LOOKUP_CASE, pairm))

// route: collision_pair_route, not None.  Members: one table per member, each wave takes its member's.
void collision_pair_dispatch(PairRoute route, const qp_collision_tables& t, const CollCall& c) {
  const bool memb = route == PairRoute::Members;
  const CollFastViewM v{{t.kr0, t.ks0, t.rho, t.diag_bin, t.anti_bin, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         c.guard, c.guard_floor}, memb ? (unsigned)(c.ncell / t.nclass) : 0u, memb ? (unsigned)t.nclass : 0u};
  const auto fn = memb ? find_pairm(t.ne, c.s, c.r) : find_pair(t.ne, c.s, c.r);
  assert(fn && "collision_pair_route accepted a size without a launcher");
  fn(v, c);
}

}  // namespace qp
