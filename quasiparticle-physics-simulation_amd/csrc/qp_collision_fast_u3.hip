// Register collision kernels, NE = 24 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(24, diag)
QP_DEFINE_LAUNCHERS(24, diagp)
}  // namespace qp
