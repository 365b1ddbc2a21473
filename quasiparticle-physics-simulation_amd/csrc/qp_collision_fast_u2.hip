// Register collision kernels, NE = 18, 20 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(18, diag)
QP_DEFINE_LAUNCHERS(20, diag)
QP_DEFINE_LAUNCHERS(18, diagp)
QP_DEFINE_LAUNCHERS(20, diagp)
}  // namespace qp
