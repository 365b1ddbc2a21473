// Register collision kernels, NE = 40 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(40, diag)
QP_DEFINE_LAUNCHERS(40, diagp)
}  // namespace qp
