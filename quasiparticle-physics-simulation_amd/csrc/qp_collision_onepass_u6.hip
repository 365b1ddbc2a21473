// One-pass collision kernel, NE = 50, gap-class form (K per lane from the amplitude tables): scattering + recombination, phonons dynamic.
// Block / group sizes from a same-box A/B of nine variants (tools/exp_gap_variants.sh).
#include "qp_collision_onepass.inc"

namespace qp {
QP_DEFINE_LAUNCHER(50, onepassc_u1, 1, 1, 13, 6, 2, 4, 3, 8)
}  // namespace qp
