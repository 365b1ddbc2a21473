// Register collision kernels with per-member tables (QP_COLL_MEMBER_CLASSES), NE = 4, 5, 6, 7, 8, 9, 10, 11 (see qp_collision_fast.inc).
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_DIAGM(4)
QP_DEFINE_DIAGM(5)
QP_DEFINE_DIAGM(6)
QP_DEFINE_DIAGM(7)
QP_DEFINE_DIAGM(8)
QP_DEFINE_DIAGM(9)
QP_DEFINE_DIAGM(10)
QP_DEFINE_DIAGM(11)
}  // namespace qp
