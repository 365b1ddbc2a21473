// One-pass collision kernel with trimmed bins (TRIM): ceiling NE = 40, scattering only; tiling of the NE = 40 kernel.
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(40, onepasst, 1, 0, 14, 8, 2)
}  // namespace qp
