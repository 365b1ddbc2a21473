// One-pass collision kernel with trimmed bins (TRIM): ceiling NE = 30, recombination only; tiling of the NE = 30 kernel.
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(30, onepasst, 0, 1, 16, 8, 2)
}  // namespace qp
