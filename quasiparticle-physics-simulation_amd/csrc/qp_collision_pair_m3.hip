// Double half-step collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 15, 16 (see
// qp_collision_pair.inc).
#include "qp_collision_pair.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(15, pairm)
QP_DEFINE_LAUNCHERS(16, pairm)
}  // namespace qp
