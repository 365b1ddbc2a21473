// Double half-step collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 4, 5, 6, 7, 8, 9, 10, 11 (see
// qp_collision_pair.inc).
#include "qp_collision_pair.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(4, pairm)
QP_DEFINE_LAUNCHERS(5, pairm)
QP_DEFINE_LAUNCHERS(6, pairm)
QP_DEFINE_LAUNCHERS(7, pairm)
QP_DEFINE_LAUNCHERS(8, pairm)
QP_DEFINE_LAUNCHERS(9, pairm)
QP_DEFINE_LAUNCHERS(10, pairm)
QP_DEFINE_LAUNCHERS(11, pairm)
}  // namespace qp
