// Register collision kernels, NE = 30, 32 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(30, diag)
QP_DEFINE_LAUNCHERS(32, diag)
QP_DEFINE_LAUNCHERS(30, diagp)
QP_DEFINE_LAUNCHERS(32, diagp)
}  // namespace qp
