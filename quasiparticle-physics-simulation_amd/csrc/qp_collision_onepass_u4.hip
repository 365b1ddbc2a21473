// One-pass collision kernel, NE = 32 (all process combinations).
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(32, onepass, 1, 1, 16, 8, 2)
QP_DEFINE_LAUNCHER(32, onepass, 0, 1, 16, 8, 2)
QP_DEFINE_LAUNCHER(32, onepass, 1, 0, 16, 8, 2)
}  // namespace qp
