// One-pass collision kernel, NE = 50, single-process combinations.
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(50, onepass, 0, 1, 14, 8, 2)
QP_DEFINE_LAUNCHER(50, onepass, 1, 0, 14, 8, 2)
}  // namespace qp
