// Double half-step collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 4, 5, 6, 7, 8, 9, 10, 11 (see
// qp_collision_pair.inc).
#include "qp_collision_pair.inc"

namespace qp {
QP_DEFINE_PAIRM(4)
QP_DEFINE_PAIRM(5)
QP_DEFINE_PAIRM(6)
QP_DEFINE_PAIRM(7)
QP_DEFINE_PAIRM(8)
QP_DEFINE_PAIRM(9)
QP_DEFINE_PAIRM(10)
QP_DEFINE_PAIRM(11)
}  // namespace qp
