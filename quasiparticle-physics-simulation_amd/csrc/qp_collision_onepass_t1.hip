// One-pass collision kernel with trimmed bins (TRIM): ceiling NE = 50, scattering + recombination; tiling of the NE = 50 kernel.
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(50, onepasst, 1, 1, 14, 8, 2)
}  // namespace qp
