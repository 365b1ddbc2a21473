// Double half-step collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 12, 13, 14 (see
// qp_collision_pair.inc).
#include "qp_collision_pair.inc"

namespace qp {
QP_DEFINE_LAUNCHERS(12, pairm)
QP_DEFINE_LAUNCHERS(13, pairm)
QP_DEFINE_LAUNCHERS(14, pairm)
}  // namespace qp
