// One-pass collision kernel, NE = 30 (all process combinations).  NE = 24 was measured too: 606 us per 1024^2 call against 506 us
// of the single-pass register kernel - not instantiated.
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(30, onepass, 1, 1, 16, 8, 2)
QP_DEFINE_LAUNCHER(30, onepass, 0, 1, 16, 8, 2)
QP_DEFINE_LAUNCHER(30, onepass, 1, 0, 16, 8, 2)
}  // namespace qp
