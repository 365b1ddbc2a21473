// Register collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 15, 16 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(15, diagm)
QP_DEFINE_LAUNCHERS(16, diagm)
}  // namespace qp
