// Register collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 4, 5, 6, 7, 8, 9, 10, 11 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(4, diagm)
QP_DEFINE_LAUNCHERS(5, diagm)
QP_DEFINE_LAUNCHERS(6, diagm)
QP_DEFINE_LAUNCHERS(7, diagm)
QP_DEFINE_LAUNCHERS(8, diagm)
QP_DEFINE_LAUNCHERS(9, diagm)
QP_DEFINE_LAUNCHERS(10, diagm)
QP_DEFINE_LAUNCHERS(11, diagm)
}  // namespace qp
