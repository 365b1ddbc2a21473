// Phonon rate traces: the four per-phonon-bin sums of the collision update (emission by scattering, absorption by
// scattering, emission by recombination, absorption by pair breaking), evaluated read-only and summed over the cells of up
// to 8 regions (qp_phonon_rates, include/qpsim_hip.h).
//
// The body stands in the frame of qp_rates_frame.h; its per-bin sums are those of collision_wave_kernel<false>
// (qp_collision_wave.hip): lane <-> energy bin in the j-loop, n_j and q_j broadcast with v_readlane, row j of the
// symmetric tables read from global memory, and four per-wave LDS arrays [4][NW] (E, A, R, B), cleared per pixel, that
// take the pair terms by a plain read-modify-write: for a fixed j the lanes of one instruction hit distinct bins (the host
// vouches for the |i-j| / i+j structure of the maps, diag_bin non-NULL; distinct diagonals and distinct anti-diagonals
// have distinct bins), emission and absorption go to different arrays, and so do scattering and recombination, which is
// what makes shared ("merged") bins safe.  Unstructured maps would need LDS atomics and are refused by the caller.
// After the j-loop the work moves to lane <-> phonon bin, BINS = ceil(NW / 64) bins per lane: the pixel's occupations are
// already there in registers (the frame loads the planes lane <-> phonon bin), so they are not staged through LDS.  Each
// lane forms the four channel values as rounded products, which the frame adds to its NR x 4 x BINS accumulators.
//
// Accumulators stay in registers in every instantiation (NR x BINS of 1, 2, 4, 8 x 1, 2, 3): per-wave LDS for the largest
// would need 4 waves x 8 x 4 x 191 doubles = 191 KiB, more than a CU has.  What shrinks instead is the group: PB pixels per
// group hold 2 PB (1 + BINS) registers of planes, and PB is 8, 4 or 2 depending on the instantiation (pixels_per_group).
#include "qp_rates_frame.h"

namespace qp {

namespace {

// pixels per group for NR x 4 x BINS accumulators per lane (2 registers each): 2 where accumulators + planes + the j-loop's
// working set would not fit the 256 architectural registers of a lane (<8, 3>), and 4 where that takes an instantiation
// from above 128 registers to below (<1, 3>, <2, 3>, <8, 1>: 4 waves per SIMD instead of 3, which is what lets the 4096
// waves of 1024^2 cells run in one residency of the device)
constexpr int pixels_per_group(int nr, int bins) {
  return nr * bins > 16 ? 2 : ((bins == 3 && nr <= 2) || (bins == 1 && nr == 8)) ? 4 : 8;
}

template <int NR_, int BINS>
struct PhononBody {
  static constexpr int NR = NR_, PB = pixels_per_group(NR_, BINS), PLANES = BINS, SLOTS = BINS;
  static __host__ __device__ int lds_per_wave(int nw) { return 4 * nw; }
  static __device__ int count(const RatesView& t) { return t.nw; }

  __device__ __forceinline__ void sums(const RatesLane& L, const RatesPixel& px, const double (&)[PLANES]) const {
    extern __shared__ double lds[];
    const RatesView& t = L.t;
    const int NE = t.ne, NW = t.nw, lane = L.lane;
    const bool on = lane < NE;
    const int o_E = L.o;                             // scattering, E_i > E_j
    const int o_A = o_E + NW;                        // scattering, E_i < E_j
    const int o_R = o_E + 2 * NW;                    // n K n
    const int o_B = o_E + 3 * NW;                    // q K q
    const double ni = px.ni, qi = px.qi;
    __builtin_amdgcn_wave_barrier();                 // the values of the wave's last pixel have been read
#pragma unroll
    for (int s = 0; s < BINS; ++s) {
      const int w = lane + 64 * s;
      if (w < NW) { lds[o_E + w] = 0.0; lds[o_A + w] = 0.0; lds[o_R + w] = 0.0; lds[o_B + w] = 0.0; }
    }
    __builtin_amdgcn_wave_barrier();      // LDS accesses of one wave execute in order: only code motion must be fenced
    for (int j = 0; j < NE; ++j) {
      const double nj = bcast(ni, j), qj = bcast(qi, j);
      const int row = on ? j * NE + lane : 0;
      if (L.use_s) {
        const double K = on ? px.ks[row] : 0.0;
        const int d = t.idx_diff[row];
        const int sg = on ? -(int)t.sign[row] : 0;                 // sign(E_lane - E_j)
        if (sg != 0) lds[(sg > 0 ? o_E : o_A) + d] += (ni * K) * qj;
      }
      if (L.use_r) {
        const double K = on ? px.kr[row] : 0.0;
        const int s = t.idx_sum[row];
        if (on) {
          lds[o_R + s] += (ni * K) * nj;
          lds[o_B + s] += (qi * K) * qj;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  __device__ __forceinline__ void values(const RatesLane& L, const RatesPixel&, const double (&N)[PLANES], int s,
                                         double (&v)[4]) const {
    extern __shared__ double lds[];
    const int NW = L.t.nw, w = L.lane + 64 * s;
    const bool live = w < NW;
    // Dead lanes read bin 0.  Where that select stands decides the registers and the j-loops the compiler makes of an
    // instantiation: with one bin per lane it is formed once, here (inside each load: a wait more per j in 7 of 8 j-loops,
    // 5 % at NE = 12); with more, inside each conditional load below (once: <2, 2>, <2, 3>, <8, 3> lose a wave per SIMD).
    // profiles/phonon_rates_resource_usage.txt has the figures of both forms.
    const int o_E = L.o + (BINS == 1 ? (live ? w : 0) : 0), o_A = o_E + NW, o_R = o_E + 2 * NW, o_B = o_E + 3 * NW;
    const auto bin = [&] { return BINS == 1 ? 0 : (live ? w : 0); };
    const double dE = L.dE, up = 1.0 + N[s];
    // rounded products: nothing contracts into the frame's accumulation
    v[0] = (live && L.use_s) ? __dmul_rn(__dmul_rn(dE, lds[o_E + bin()]), up) : 0.0;
    v[1] = (live && L.use_s) ? __dmul_rn(__dmul_rn(dE, lds[o_A + bin()]), N[s]) : 0.0;
    v[2] = (live && L.use_r) ? __dmul_rn(__dmul_rn(dE, lds[o_R + bin()]), up) : 0.0;
    v[3] = (live && L.use_r) ? __dmul_rn(__dmul_rn(dE, lds[o_B + bin()]), N[s]) : 0.0;
  }
};

}  // namespace

}  // namespace qp

extern "C" {

int qp_phonon_rates_available(int32_t ne, int32_t nw) {
  return ne >= 2 && ne <= 64 && nw >= 1 && nw <= 64 * qp::RMAXBINS - 1;
}

size_t qp_phonon_rates_workspace_bytes(int32_t nw, int64_t ncell_member, int64_t members, int32_t nregion) {
  if (nw < 1 || nw > 64 * qp::RMAXBINS - 1 || ncell_member < 1 || members < 1 || nregion < 1 || nregion > 8) return 0;
  return qp::rates_workspace_bytes(nw, ncell_member, members, nregion);
}

int qp_phonon_rates(const qp_collision_tables* t, const uint8_t* region_bits, int64_t ncell_member, int64_t members,
                    int32_t nregion, const double* state, const double* phonon, double dE, int enable_recombination,
                    int enable_scattering, void* workspace, double* out, void* stream) {
  const qp::RatesCall c{t, region_bits, ncell_member, members, nregion, state, phonon, dE, enable_recombination,
                        enable_scattering, workspace, out, stream};
  if (const int e = qp::rates_check_tables(__func__, c, qp_phonon_rates_available)) return e;
  QP_REQUIRE(t->diag_bin && t->anti_bin, "structured bin maps (diag_bin, anti_bin) are required: unstructured maps have no "
                                         "race-free per-bin sums");
  if (const int e = qp::rates_check_shape(__func__, c)) return e;
  qp::rates_ladder(nregion, [&](auto nr) {
    constexpr int NR = decltype(nr)::value;
    const int bins = (t->nw + 63) / 64;
    if (bins == 1) qp::rates_launch<qp::PhononBody<NR, 1>>(c);
    else if (bins == 2) qp::rates_launch<qp::PhononBody<NR, 2>>(c);
    else qp::rates_launch<qp::PhononBody<NR, 3>>(c);
  });
  qp::rates_finish(c, t->nw);
  return qp::check_launch("qp_phonon_rates");
}

}  // extern "C"
