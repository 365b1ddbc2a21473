// One-pass collision kernel with trimmed bins (TRIM): ceiling NE = 32, scattering only; tiling of the NE = 32 kernel.
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(32, onepasst, 1, 0, 16, 8, 2)
}  // namespace qp
