// Register collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 15, 16 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_DIAGM(15)
QP_DEFINE_DIAGM(16)
}  // namespace qp
