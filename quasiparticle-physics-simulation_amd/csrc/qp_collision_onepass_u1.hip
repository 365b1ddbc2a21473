// One-pass collision kernel, NE = 50 (the reference's default), scattering + recombination.
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(50, onepass, 1, 1, 14, 8, 2)
}  // namespace qp
