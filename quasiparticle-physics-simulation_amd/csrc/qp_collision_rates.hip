// Collision rate traces: the four per-bin sums of the collision update (scattering in / out, recombination, pair breaking),
// evaluated read-only and summed over the cells of up to 8 regions (qp_collision_rates, include/qpsim_hip.h).
//
// A read-only sibling of collision_wave_kernel (qp_collision_wave.hip): one wave per run of pixels, lane <-> energy bin,
// n_j and q_j broadcast with v_readlane, row j of the symmetric tables read from global memory, the pixel's phonon
// occupations in NW doubles of LDS per wave.  The dead ends measured there (tables in LDS, ds_bpermute gathers, interleaved
// pixels) apply here unchanged.  What this kernel does not have: the A / B arrays with their read-modify-write, atomics,
// exponentials, stores of the planes.  What it adds: per lane NR x 4 accumulators (NR = nregion rounded up to 1, 2, 4, 8;
// 64 VGPRs at NR = 8) which take the channel values of a pixel under a scalar branch on the pixel's region bits - the
// bits are wave-uniform: the 256 bytes of a wave's run are read once, 4 per lane, and a pixel's byte is broadcast with
// v_readlane.  A group whose bits are all zero is left before its planes are loaded (one ballot per run tells which).
//
// Fixed partition (determinism): block = (chunk of QP_RATES_CHUNK cells, member), wave w of the block owns the cells
// [RUN w, RUN w + RUN) of the chunk, walked in groups of 8 in index order.  Cell indices are member-local, so the
// partition of a member does not depend on where its planes start.  The waves combine through LDS in wave order, the
// block stores nregion * 4 * ne partials, rates_final_kernel adds them in chunk order.  No atomics, no completion counters.
#include "qp_collision_dispatch.h"

namespace qp {

namespace {

constexpr int RPB = 8;                               // pixels per group: every lane reads 64 contiguous bytes of its planes
constexpr int RMAXBINS = 3;                          // phonon bins per lane: NW <= 3 * 64 - 1
constexpr int RWAVES = 4;                            // waves per block
constexpr int RCHUNK = QP_RATES_CHUNK;               // cells per block
constexpr int RRUN = RCHUNK / RWAVES;                // cells per wave
static_assert(RRUN % RPB == 0, "a wave's run is a whole number of groups");
static_assert(RRUN == 4 * 64 && RPB == 8, "the region bits of a run are held 4 cells per lane, a group in two lanes");

__device__ __forceinline__ double rbcast(double x, int srclane) {
  const unsigned long long u = __double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, srclane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), srclane);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

struct RatesView {
  int ne, nw;
  const double* kr0;
  const double* ks0;
  const double* rho;
  const int32_t* idx_diff;
  const int32_t* idx_sum;
  const int8_t* sign;
  const int32_t* cls;
};

// LDS: [RWAVES][nw] phonon occupations of each wave's current pixel, then [NR * 4][64] for the wave-order combine
template <int NR>
__global__ void __launch_bounds__(64 * RWAVES) collision_rates_kernel(RatesView t, const uint8_t* __restrict__ bits,
                                                                     long ncm, long members, int nregion, long nchunk,
                                                                     const double* __restrict__ state,
                                                                     const double* __restrict__ ph, double dE, int use_r,
                                                                     int use_s, double* __restrict__ part) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NE = t.ne, NW = t.nw, NN = NE * NE;
  const long chunk = blockIdx.x, m = blockIdx.y;
  const long ncell = ncm * members;                  // plane stride
  const long mbase = m * ncm;                        // first cell of the member in a plane
  const int o_P = wave * NW;
  const int o_C = RWAVES * NW;
  const bool on = lane < NE;
  const unsigned rmask = (1u << nregion) - 1u;
  const double dE2 = 2.0 * dE;

  double acc[NR][4];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) acc[r][ch] = 0.0;

  // the region bits of the wave's whole run in one round trip: lane l holds the bytes of cells run0 + 4 l ... + 3 (0 past the
  // member's end), so group g sits in lanes 2 g and 2 g + 1 and `nz` says which groups have a bit at all
  const long run0 = chunk * RCHUNK + (long)wave * RRUN;
  unsigned word = 0u;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long c = run0 + 4 * lane + b;
    if (c < ncm) word |= (unsigned)(bits[c] & rmask) << (8 * b);
  }
  const unsigned long long nz = __ballot(word != 0u);
  for (int g = 0; g < RRUN / RPB; ++g) {
    const long c0 = run0 + (long)g * RPB;            // member-local index of the group's first pixel
    if (c0 >= ncm) break;
    if (((nz >> (2 * g)) & 3ull) == 0ull) continue;  // no pixel of the group lies in a region: nothing is loaded
    const int npx = (int)min((long)RPB, ncm - c0);

    const long p0 = mbase + c0;
    double n[RPB], pb[RMAXBINS][RPB];
#pragma unroll
    for (int k = 0; k < RPB; ++k) n[k] = (on && k < npx) ? state[(long)lane * ncell + p0 + k] : 0.0;
#pragma unroll
    for (int s = 0; s < RMAXBINS; ++s) {
      const int w = lane + 64 * s;
#pragma unroll
      for (int k = 0; k < RPB; ++k) pb[s][k] = (w < NW && k < npx) ? ph[(long)w * ncell + p0 + k] : 0.0;
    }

#pragma unroll
    for (int k = 0; k < RPB; ++k) {
      // scalar: the pixel's byte of the lane that holds it (0 past the member's end)
      const unsigned b = ((unsigned)__builtin_amdgcn_readlane(word, 2 * g + (k >> 2)) >> (8 * (k & 3))) & 0xffu;
      if (b == 0u) continue;
      const int c = t.cls ? t.cls[p0 + k] : 0;
      const double rho_i = on ? t.rho[(long)c * NE + lane] : 0.0;
      const double* ks = use_s ? t.ks0 + (long)c * NN : nullptr;
      const double* kr = use_r ? t.kr0 + (long)c * NN : nullptr;
      const double ni = n[k];
      const double qi = rho_i * fmax(1.0 - ni / fmax(rho_i, 1e-30), 0.0);
#pragma unroll
      for (int s = 0; s < RMAXBINS; ++s) {
        const int w = lane + 64 * s;
        if (w < NW) lds[o_P + w] = pb[s][k];
      }
      __builtin_amdgcn_wave_barrier();      // LDS accesses of one wave execute in order: only code motion must be fenced
      double g_s = 0.0, l_s = 0.0, g_r = 0.0, l_r = 0.0;
      for (int j = 0; j < NE; ++j) {
        const double nj = rbcast(ni, j), qj = rbcast(qi, j);
        const int row = on ? j * NE + lane : 0;
        if (use_s) {
          const double K = on ? ks[row] : 0.0;
          const int d = t.idx_diff[row];
          const int sg = on ? -(int)t.sign[row] : 0;                 // sign(E_lane - E_j)
          const double P = lds[o_P + d];
          const double up = 1.0 + P;
          g_s = fma(K * (sg < 0 ? up : sg > 0 ? P : 0.0), nj, g_s);   // K^s_eff[j][i] n_j
          l_s = fma(K * (sg > 0 ? up : sg < 0 ? P : 0.0), qj, l_s);   // K^s_eff[i][j] q_j
        }
        if (use_r) {
          const double K = on ? kr[row] : 0.0;
          const int s = t.idx_sum[row];
          const double P = lds[o_P + s];
          l_r = fma(K * (1.0 + P), nj, l_r);
          g_r = fma(K * P, qj, g_r);
        }
      }
      __builtin_amdgcn_wave_barrier();
      double v[4];
      v[0] = __dmul_rn(__dmul_rn(dE, qi), g_s);      // rounded products: nothing contracts into the accumulation below
      v[1] = __dmul_rn(__dmul_rn(ni, dE), l_s);
      v[2] = __dmul_rn(__dmul_rn(ni, dE2), l_r);
      v[3] = __dmul_rn(__dmul_rn(dE2, qi), g_r);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (b & (1u << r)) {                 // scalar branch: the bits of a pixel are wave-uniform
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) acc[r][ch] += v[ch];
        }
      }
    }
  }

  // waves combine in wave order: wave 0 holds ((w0 + w1) + w2) + w3
  for (int w = 1; w < RWAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) lds[o_C + (r * 4 + ch) * 64 + lane] = acc[r][ch];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) acc[r][ch] += lds[o_C + (r * 4 + ch) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0 && on) {
    double* dst = part + (m * nchunk + chunk) * ((long)nregion * 4 * NE);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < nregion) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) dst[((long)r * 4 + ch) * NE + lane] = acc[r][ch];
      }
    }
  }
}

// out[m][e] = sum over chunks, in chunk order, of part[m][chunk][e], e < per = nregion * 4 * ne
__global__ void __launch_bounds__(64) rates_final_kernel(const double* __restrict__ part, long nchunk, int per,
                                                         double* __restrict__ out) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  const long m = blockIdx.y;
  if (e >= per) return;
  const double* src = part + m * nchunk * per + e;
  double s = 0.0;
  // the additions stay in chunk order; 32 loads are issued before the first of them (one round trip per 32 chunks instead
  // of one per chunk: few threads run here, so the chain of latencies is what this kernel costs)
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

template <int NR>
void rates_launch(const RatesView& v, const uint8_t* bits, long ncm, long members, int nregion, long nchunk,
                  const double* state, const double* ph, double dE, int use_r, int use_s, double* part, hipStream_t st) {
  const size_t shmem = ((size_t)RWAVES * v.nw + (size_t)NR * 4 * 64) * sizeof(double);
  hipLaunchKernelGGL(collision_rates_kernel<NR>, dim3((unsigned)nchunk, (unsigned)members), dim3(64 * RWAVES), shmem, st, v,
                     bits, ncm, members, nregion, nchunk, state, ph, dE, use_r, use_s, part);
}

inline long rates_chunks(long ncm) { return (ncm + RCHUNK - 1) / RCHUNK; }

}  // namespace

}  // namespace qp

extern "C" {

int qp_collision_rates_available(int32_t ne, int32_t nw) {
  return ne >= 2 && ne <= 64 && nw >= 1 && nw <= 64 * qp::RMAXBINS - 1;
}

size_t qp_collision_rates_workspace_bytes(int32_t ne, int64_t ncell_member, int64_t members, int32_t nregion) {
  if (ne < 2 || ne > 64 || ncell_member < 1 || members < 1 || nregion < 1 || nregion > 8) return 0;
  return (size_t)members * (size_t)qp::rates_chunks((long)ncell_member) * (size_t)nregion * 4 * (size_t)ne * sizeof(double);
}

int qp_collision_rates(const qp_collision_tables* t, const uint8_t* region_bits, int64_t ncell_member, int64_t members,
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
  if (!qp_collision_rates_available(t->ne, t->nw)) {
    qp::set_error("%s: no kernel for ne = %d, nw = %d (2 <= ne <= 64, 1 <= nw <= 191)", __func__, t->ne, t->nw);
    return QP_ERR_UNSUPPORTED;
  }
  if (nregion < 1 || nregion > 8) {
    qp::set_error("%s: 1 to 8 regions per call, got %d", __func__, nregion);
    return QP_ERR_UNSUPPORTED;
  }
  QP_REQUIRE(t->rho && t->idx_diff && t->idx_sum && t->sign, "rho, idx maps and sign must be non-NULL");
  QP_REQUIRE(t->nclass == 1 || t->cls, "cls is required when nclass > 1");
  if (t->flags & QP_COLL_MEMBER_CLASSES)
    QP_REQUIRE(members % t->nclass == 0, "QP_COLL_MEMBER_CLASSES needs members to be a multiple of nclass");
  QP_REQUIRE(members <= 65535, "at most 65535 members per call");
  const long nchunk = qp::rates_chunks((long)ncell_member);
  QP_REQUIRE(nchunk <= 0x7fffffffL, "ncell_member too large for one launch");
  const int use_r = enable_recombination && t->kr0, use_s = enable_scattering && t->ks0;
  const qp::RatesView v{t->ne, t->nw, t->kr0, t->ks0, t->rho, t->idx_diff, t->idx_sum, t->sign, t->cls};
  const hipStream_t st = (hipStream_t)stream;
  auto* part = (double*)workspace;
  const long ncm = (long)ncell_member, mem = (long)members;
  if (nregion == 1)
    qp::rates_launch<1>(v, region_bits, ncm, mem, 1, nchunk, state, phonon, dE, use_r, use_s, part, st);
  else if (nregion == 2)
    qp::rates_launch<2>(v, region_bits, ncm, mem, 2, nchunk, state, phonon, dE, use_r, use_s, part, st);
  else if (nregion <= 4)
    qp::rates_launch<4>(v, region_bits, ncm, mem, (int)nregion, nchunk, state, phonon, dE, use_r, use_s, part, st);
  else
    qp::rates_launch<8>(v, region_bits, ncm, mem, (int)nregion, nchunk, state, phonon, dE, use_r, use_s, part, st);
  const int per = nregion * 4 * t->ne;
  hipLaunchKernelGGL(qp::rates_final_kernel, dim3((unsigned)((per + 63) / 64), (unsigned)members), dim3(64), 0, st,
                     (const double*)part, nchunk, per, out);
  return qp::check_launch("qp_collision_rates");
}

}  // extern "C"
