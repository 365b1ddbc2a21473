// Register collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 12, 13, 14 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_DIAGM(12)
QP_DEFINE_DIAGM(13)
QP_DEFINE_DIAGM(14)
}  // namespace qp
