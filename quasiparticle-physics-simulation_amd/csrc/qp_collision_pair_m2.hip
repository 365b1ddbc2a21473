// Double half-step collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 12, 13, 14 (see
// qp_collision_pair.inc).
#include "qp_collision_pair.inc"

namespace qp {
QP_DEFINE_PAIRM(12)
QP_DEFINE_PAIRM(13)
QP_DEFINE_PAIRM(14)
}  // namespace qp
