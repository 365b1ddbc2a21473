// Register collision kernels, NE = 50 (reference default), scattering + recombination.
#include "qp_collision_fast.inc"

namespace qp {
QP_DEFINE_LAUNCHER(50, diag, 1, 1)
}  // namespace qp
