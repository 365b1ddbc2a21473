// Phonon rate traces: the four per-phonon-bin sums of the collision update (emission by scattering, absorption by
// scattering, emission by recombination, absorption by pair breaking), evaluated read-only and summed over the cells of up
// to 8 regions (qp_phonon_rates, include/qpsim_hip.h).
//
// The partition, the region bits and the group skip are those of collision_rates_kernel (qp_collision_rates.hip); the
// per-bin sums are those of collision_wave_kernel<false> (qp_collision_wave.hip): one wave per run of pixels, lane <->
// energy bin in the j-loop, n_j and q_j broadcast with v_readlane, row j of the symmetric tables read from global memory,
// and four per-wave LDS arrays [4][NW] (E, A, R, B), cleared per pixel, that take the pair terms by a plain
// read-modify-write: for a fixed j the lanes of one instruction hit distinct bins (the host vouches for the |i-j| / i+j
// structure of the maps, diag_bin non-NULL; distinct diagonals and distinct anti-diagonals have distinct bins), emission
// and absorption go to different arrays, and so do scattering and recombination, which is what makes shared ("merged") bins
// safe.  Unstructured maps would need LDS atomics and are refused by the caller.
// After the j-loop the work moves to lane <-> phonon bin, BINS = ceil(NW / 64) bins per lane: the pixel's occupations are
// already there in registers (the planes are loaded lane <-> phonon bin), so they are not staged through LDS.  Each lane
// forms the four channel values as rounded products and adds them to its NR x 4 x BINS accumulators under a scalar branch
// on the pixel's region bits.
//
// Accumulators stay in registers in every instantiation (NR x BINS of 1, 2, 4, 8 x 1, 2, 3): per-wave LDS for the largest
// would need 4 waves x 8 x 4 x 191 doubles = 191 KiB, more than a CU has.  What shrinks instead is the group: PB pixels per
// group hold 2 PB (1 + BINS) registers of planes, and PB is 8, 4 or 2 depending on the instantiation (pixels_per_group).
// A lane adds the cells of its wave's run in index order whatever PB is, so PB is not part of the result.
//
// Fixed partition (determinism): block = (chunk of QP_RATES_CHUNK cells, member), wave w of the block owns the cells
// [RUN w, RUN w + RUN) of the chunk, walked in index order.  Cell indices are member-local.  The waves combine through LDS
// in wave order, the block stores nregion * 4 * nw partials, phonon_rates_final_kernel adds them in chunk order.  No
// atomics, no completion counters.
#include "qp_collision_dispatch.h"

namespace qp {

namespace {

constexpr int PWAVES = 4;                            // waves per block
constexpr int PCHUNK = QP_RATES_CHUNK;               // cells per block
constexpr int PRUN = PCHUNK / PWAVES;                // cells per wave
constexpr int PMAXBINS = 3;                          // phonon bins per lane: NW <= 3 * 64 - 1
static_assert(PRUN == 4 * 64, "the region bits of a run are held 4 cells per lane");

// pixels per group for NR x 4 x BINS accumulators per lane (2 registers each): 2 where accumulators + planes + the j-loop's
// working set would not fit the 256 architectural registers of a lane (<8, 3>), and 4 where that takes an instantiation
// from above 128 registers to below (<1, 3>, <2, 3>, <8, 1>: 4 waves per SIMD instead of 3, which is what lets the 4096
// waves of 1024^2 cells run in one residency of the device)
constexpr int pixels_per_group(int nr, int bins) {
  return nr * bins > 16 ? 2 : ((bins == 3 && nr <= 2) || (bins == 1 && nr == 8)) ? 4 : 8;
}

__device__ __forceinline__ double pbcast(double x, int srclane) {
  const unsigned long long u = __double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, srclane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), srclane);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

struct PhononRatesView {
  int ne, nw;
  const double* kr0;
  const double* ks0;
  const double* rho;
  const int32_t* idx_diff;
  const int32_t* idx_sum;
  const int8_t* sign;
  const int32_t* cls;
};

// LDS: [PWAVES][4][nw] per-bin sums of each wave's current pixel; after the pixel loops the same bytes serve the wave-order
// combine, [NR * 4 * BINS][64]
template <int NR, int BINS>
__global__ void __launch_bounds__(64 * PWAVES) phonon_rates_kernel(PhononRatesView t, const uint8_t* __restrict__ bits,
                                                                   long ncm, long members, int nregion, long nchunk,
                                                                   const double* __restrict__ state,
                                                                   const double* __restrict__ ph, double dE, int use_r,
                                                                   int use_s, double* __restrict__ part) {
  constexpr int PB = pixels_per_group(NR, BINS);
  static_assert(PRUN % PB == 0 && PB <= 8, "a wave's run is a whole number of groups");
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NE = t.ne, NW = t.nw, NN = NE * NE;
  const long chunk = blockIdx.x, m = blockIdx.y;
  const long ncell = ncm * members;                  // plane stride
  const long mbase = m * ncm;                        // first cell of the member in a plane
  const int o_E = wave * 4 * NW;                     // scattering, E_i > E_j
  const int o_A = o_E + NW;                          // scattering, E_i < E_j
  const int o_R = o_E + 2 * NW;                      // n K n
  const int o_B = o_E + 3 * NW;                      // q K q
  const bool on = lane < NE;
  const unsigned rmask = (1u << nregion) - 1u;

  double acc[NR][4][BINS];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
#pragma unroll
      for (int s = 0; s < BINS; ++s) acc[r][ch][s] = 0.0;

  // the region bits of the wave's whole run in one round trip: lane l holds the bytes of cells run0 + 4 l ... + 3 (0 past the
  // member's end)
  const long run0 = chunk * PCHUNK + (long)wave * PRUN;
  unsigned word = 0u;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long c = run0 + 4 * lane + b;
    if (c < ncm) word |= (unsigned)(bits[c] & rmask) << (8 * b);
  }
  for (int g = 0; g < PRUN / PB; ++g) {
    const long c0 = run0 + (long)g * PB;             // member-local index of the group's first pixel
    if (c0 >= ncm) break;
    // scalar: the bytes of the group's pixels from the lanes that hold them (0 past the member's end)
    unsigned byte[PB], any = 0u;
#pragma unroll
    for (int k = 0; k < PB; ++k) {
      const int px = g * PB + k;
      byte[k] = ((unsigned)__builtin_amdgcn_readlane(word, px >> 2) >> (8 * (px & 3))) & 0xffu;
      any |= byte[k];
    }
    if (any == 0u) continue;                         // no pixel of the group lies in a region: nothing is loaded
    const int npx = (int)min((long)PB, ncm - c0);

    const long p0 = mbase + c0;
    double n[PB], pb[BINS][PB];
#pragma unroll
    for (int k = 0; k < PB; ++k) n[k] = (on && k < npx) ? state[(long)lane * ncell + p0 + k] : 0.0;
#pragma unroll
    for (int s = 0; s < BINS; ++s) {
      const int w = lane + 64 * s;
#pragma unroll
      for (int k = 0; k < PB; ++k) pb[s][k] = (w < NW && k < npx) ? ph[(long)w * ncell + p0 + k] : 0.0;
    }

#pragma unroll
    for (int k = 0; k < PB; ++k) {
      const unsigned b = byte[k];
      if (b == 0u) continue;
      const int c = t.cls ? t.cls[p0 + k] : 0;
      const double rho_i = on ? t.rho[(long)c * NE + lane] : 0.0;
      const double* ks = use_s ? t.ks0 + (long)c * NN : nullptr;
      const double* kr = use_r ? t.kr0 + (long)c * NN : nullptr;
      const double ni = n[k];
      const double qi = rho_i * fmax(1.0 - ni / fmax(rho_i, 1e-30), 0.0);
#pragma unroll
      for (int s = 0; s < BINS; ++s) {
        const int w = lane + 64 * s;
        if (w < NW) { lds[o_E + w] = 0.0; lds[o_A + w] = 0.0; lds[o_R + w] = 0.0; lds[o_B + w] = 0.0; }
      }
      __builtin_amdgcn_wave_barrier();      // LDS accesses of one wave execute in order: only code motion must be fenced
      for (int j = 0; j < NE; ++j) {
        const double nj = pbcast(ni, j), qj = pbcast(qi, j);
        const int row = on ? j * NE + lane : 0;
        if (use_s) {
          const double K = on ? ks[row] : 0.0;
          const int d = t.idx_diff[row];
          const int sg = on ? -(int)t.sign[row] : 0;                 // sign(E_lane - E_j)
          if (sg != 0) lds[(sg > 0 ? o_E : o_A) + d] += (ni * K) * qj;
        }
        if (use_r) {
          const double K = on ? kr[row] : 0.0;
          const int s = t.idx_sum[row];
          if (on) {
            lds[o_R + s] += (ni * K) * nj;
            lds[o_B + s] += (qi * K) * qj;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s = 0; s < BINS; ++s) {
        const int w = lane + 64 * s;
        const bool live = w < NW;
        const double N = pb[s][k], up = 1.0 + N;
        double v[4];
        // rounded products: nothing contracts into the accumulation below
        v[0] = (live && use_s) ? __dmul_rn(__dmul_rn(dE, lds[o_E + (live ? w : 0)]), up) : 0.0;
        v[1] = (live && use_s) ? __dmul_rn(__dmul_rn(dE, lds[o_A + (live ? w : 0)]), N) : 0.0;
        v[2] = (live && use_r) ? __dmul_rn(__dmul_rn(dE, lds[o_R + (live ? w : 0)]), up) : 0.0;
        v[3] = (live && use_r) ? __dmul_rn(__dmul_rn(dE, lds[o_B + (live ? w : 0)]), N) : 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          if (b & (1u << r)) {               // scalar branch: the bits of a pixel are wave-uniform
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) acc[r][ch][s] += v[ch];
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }

  // waves combine in wave order: wave 0 holds ((w0 + w1) + w2) + w3.  The combine area overlays the per-bin sums, which
  // every wave has left by now.
  __syncthreads();
  for (int w = 1; w < PWAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
          for (int s = 0; s < BINS; ++s) lds[((r * 4 + ch) * BINS + s) * 64 + lane] = acc[r][ch][s];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
          for (int s = 0; s < BINS; ++s) acc[r][ch][s] += lds[((r * 4 + ch) * BINS + s) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    double* dst = part + (m * nchunk + chunk) * ((long)nregion * 4 * NW);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < nregion) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
          for (int s = 0; s < BINS; ++s) {
            const int w = lane + 64 * s;
            if (w < NW) dst[((long)r * 4 + ch) * NW + w] = acc[r][ch][s];
          }
      }
    }
  }
}

// out[m][e] = sum over chunks, in chunk order, of part[m][chunk][e], e < per = nregion * 4 * nw (a sibling of
// rates_final_kernel of qp_collision_rates.hip, which stays private to that file)
__global__ void __launch_bounds__(64) phonon_rates_final_kernel(const double* __restrict__ part, long nchunk, int per,
                                                                double* __restrict__ out) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const long m = blockIdx.y;
  if (e >= per) return;
  const double* src = part + m * nchunk * per + e;
  double s = 0.0;
  // the additions stay in chunk order; 32 loads are issued before the first of them
  constexpr int B = 32;
  long c = 0;
  for (; c + B <= nchunk; c += B) {
    double v[B];
#pragma unroll
    for (int k = 0; k < B; ++k) v[k] = src[(c + k) * per];
#pragma unroll
    for (int k = 0; k < B; ++k) s += v[k];
  }
  for (; c < nchunk; ++c) s += src[c * per];
  out[m * per + e] = s;
}

struct PhononRatesCall {
  PhononRatesView v;
  const uint8_t* bits;
  long ncm, members;
  int nregion;
  long nchunk;
  const double* state;
  const double* ph;
  double dE;
  int use_r, use_s;
  double* part;
  hipStream_t st;
};

template <int NR, int BINS>
void phonon_rates_launch(const PhononRatesCall& c) {
  const size_t sums = (size_t)PWAVES * 4 * c.v.nw, combine = (size_t)NR * 4 * BINS * 64;
  const size_t shmem = (sums > combine ? sums : combine) * sizeof(double);
  hipLaunchKernelGGL((phonon_rates_kernel<NR, BINS>), dim3((unsigned)c.nchunk, (unsigned)c.members), dim3(64 * PWAVES), shmem,
                     c.st, c.v, c.bits, c.ncm, c.members, c.nregion, c.nchunk, c.state, c.ph, c.dE, c.use_r, c.use_s, c.part);
}

template <int NR>
void phonon_rates_bins(const PhononRatesCall& c) {
  const int bins = (c.v.nw + 63) / 64;
  if (bins == 1) phonon_rates_launch<NR, 1>(c);
  else if (bins == 2) phonon_rates_launch<NR, 2>(c);
  else phonon_rates_launch<NR, 3>(c);
}

inline long phonon_rates_chunks(long ncm) { return (ncm + PCHUNK - 1) / PCHUNK; }

}  // namespace

}  // namespace qp

extern "C" {

int qp_phonon_rates_available(int32_t ne, int32_t nw) {
  return ne >= 2 && ne <= 64 && nw >= 1 && nw <= 64 * qp::PMAXBINS - 1;
}

size_t qp_phonon_rates_workspace_bytes(int32_t nw, int64_t ncell_member, int64_t members, int32_t nregion) {
  if (nw < 1 || nw > 64 * qp::PMAXBINS - 1 || ncell_member < 1 || members < 1 || nregion < 1 || nregion > 8) return 0;
  return (size_t)members * (size_t)qp::phonon_rates_chunks((long)ncell_member) * (size_t)nregion * 4 * (size_t)nw * sizeof(double);
}

int qp_phonon_rates(const qp_collision_tables* t, const uint8_t* region_bits, int64_t ncell_member, int64_t members,
                    int32_t nregion, const double* state, const double* phonon, double dE, int enable_recombination,
                    int enable_scattering, void* workspace, double* out, void* stream) {
  QP_REQUIRE(t != nullptr, "tables are NULL");
  if (t->struct_size != sizeof(qp_collision_tables)) {
    qp::set_error("%s: qp_collision_tables.struct_size is %u, this library expects %zu (binding built against another "
                  "header revision)", __func__, t->struct_size, sizeof(qp_collision_tables));
    return QP_ERR_INVALID_ARGUMENT;
  }
  QP_REQUIRE(region_bits && state && phonon && workspace && out, "NULL argument");
  QP_REQUIRE(ncell_member > 0 && members > 0, "ncell_member, members must be positive");
  QP_REQUIRE(t->ne > 0 && t->nw > 0 && t->nclass > 0, "ne, nw, nclass must be positive");
  if (!qp_phonon_rates_available(t->ne, t->nw)) {
    qp::set_error("%s: no kernel for ne = %d, nw = %d (2 <= ne <= 64, 1 <= nw <= 191)", __func__, t->ne, t->nw);
    return QP_ERR_UNSUPPORTED;
  }
  if (nregion < 1 || nregion > 8) {
    qp::set_error("%s: 1 to 8 regions per call, got %d", __func__, nregion);
    return QP_ERR_UNSUPPORTED;
  }
  QP_REQUIRE(t->rho && t->idx_diff && t->idx_sum && t->sign, "rho, idx maps and sign must be non-NULL");
  QP_REQUIRE(t->diag_bin && t->anti_bin, "structured bin maps (diag_bin, anti_bin) are required: unstructured maps have no "
                                         "race-free per-bin sums");
  QP_REQUIRE(t->nclass == 1 || t->cls, "cls is required when nclass > 1");
  if (t->flags & QP_COLL_MEMBER_CLASSES)
    QP_REQUIRE(members % t->nclass == 0, "QP_COLL_MEMBER_CLASSES needs members to be a multiple of nclass");
  QP_REQUIRE(members <= 65535, "at most 65535 members per call");
  const long nchunk = qp::phonon_rates_chunks((long)ncell_member);
  QP_REQUIRE(nchunk <= 0x7fffffffL, "ncell_member too large for one launch");
  const int use_r = enable_recombination && t->kr0, use_s = enable_scattering && t->ks0;
  const qp::PhononRatesCall c{{t->ne, t->nw, t->kr0, t->ks0, t->rho, t->idx_diff, t->idx_sum, t->sign, t->cls},
                              region_bits, (long)ncell_member, (long)members, (int)nregion, nchunk, state, phonon, dE,
                              use_r, use_s, (double*)workspace, (hipStream_t)stream};
  if (nregion == 1) qp::phonon_rates_bins<1>(c);
  else if (nregion == 2) qp::phonon_rates_bins<2>(c);
  else if (nregion <= 4) qp::phonon_rates_bins<4>(c);
  else qp::phonon_rates_bins<8>(c);
  const int per = nregion * 4 * t->nw;
  hipLaunchKernelGGL(qp::phonon_rates_final_kernel, dim3((unsigned)((per + 63) / 64), (unsigned)members), dim3(64), 0,
                     (hipStream_t)stream, (const double*)c.part, nchunk, per, out);
  return qp::check_launch("qp_phonon_rates");
}

}  // extern "C"
