// Register collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 12, 13, 14 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(12, diagm)
QP_DEFINE_LAUNCHERS(13, diagm)
QP_DEFINE_LAUNCHERS(14, diagm)
}  // namespace qp
