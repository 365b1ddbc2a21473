// Collision rate traces: the four per-bin sums of the collision update (scattering in / out, recombination, pair breaking),
// evaluated read-only and summed over the cells of up to 8 regions (qp_collision_rates, include/qpsim_hip.h).
//
// The body is a read-only sibling of collision_wave_kernel (qp_collision_wave.hip) in the frame of qp_rates_frame.h: lane
// <-> energy bin, n_j and q_j broadcast with v_readlane, row j of the symmetric tables read from global memory, the
// pixel's phonon occupations in NW doubles of LDS per wave.  The dead ends measured there (tables in LDS, ds_bpermute
// gathers, interleaved pixels) apply here unchanged.  What this kernel does not have: the A / B arrays with their
// read-modify-write, atomics, exponentials, stores of the planes.  What the frame adds: per lane NR x 4 accumulators (NR =
// nregion rounded up to 1, 2, 4, 8; 64 VGPRs at NR = 8).  The lane loads RMAXBINS phonon planes under run-time guards, so
// the kernel is not specialised on the phonon bins per lane.
//
// This unit also holds the finish of both rate kernels (rates_final_kernel, rates_finish).
#include "qp_rates_frame.h"

namespace qp {

namespace {

template <int NR_>
struct CollisionBody {
  static constexpr int NR = NR_, PB = 8, PLANES = RMAXBINS, SLOTS = 1;   // PB 8: a lane reads 64 contiguous bytes of its planes
  static __host__ __device__ int lds_per_wave(int nw) { return nw; }
  static __device__ int count(const RatesView& t) { return t.ne; }

  double g_s, l_s, g_r, l_r;

  __device__ __forceinline__ void sums(const RatesLane& L, const RatesPixel& px, const double (&N)[PLANES]) {
    extern __shared__ double lds[];
    const RatesView& t = L.t;
    const int NE = t.ne, NW = t.nw, lane = L.lane, o_P = L.o;
    const bool on = lane < NE;
#pragma unroll
    for (int s = 0; s < PLANES; ++s) {
      const int w = lane + 64 * s;
      if (w < NW) lds[o_P + w] = N[s];
    }
    __builtin_amdgcn_wave_barrier();      // LDS accesses of one wave execute in order: only code motion must be fenced
    g_s = 0.0, l_s = 0.0, g_r = 0.0, l_r = 0.0;
    for (int j = 0; j < NE; ++j) {
      const double nj = bcast(px.ni, j), qj = bcast(px.qi, j);
      const int row = on ? j * NE + lane : 0;
      if (L.use_s) {
        const double K = on ? px.ks[row] : 0.0;
        const int d = t.idx_diff[row];
        const int sg = on ? -(int)t.sign[row] : 0;                 // sign(E_lane - E_j)
        const double P = lds[o_P + d];
        const double up = 1.0 + P;
        g_s = fma(K * (sg < 0 ? up : sg > 0 ? P : 0.0), nj, g_s);   // K^s_eff[j][i] n_j
        l_s = fma(K * (sg > 0 ? up : sg < 0 ? P : 0.0), qj, l_s);   // K^s_eff[i][j] q_j
      }
      if (L.use_r) {
        const double K = on ? px.kr[row] : 0.0;
        const int s = t.idx_sum[row];
        const double P = lds[o_P + s];
        l_r = fma(K * (1.0 + P), nj, l_r);
        g_r = fma(K * P, qj, g_r);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

  __device__ __forceinline__ void values(const RatesLane& L, const RatesPixel& px, const double (&)[PLANES], int,
                                         double (&v)[4]) const {
    const double dE = L.dE, dE2 = 2.0 * dE;
    v[0] = __dmul_rn(__dmul_rn(dE, px.qi), g_s);     // rounded products: nothing contracts into the frame's accumulation
    v[1] = __dmul_rn(__dmul_rn(px.ni, dE), l_s);
    v[2] = __dmul_rn(__dmul_rn(px.ni, dE2), l_r);
    v[3] = __dmul_rn(__dmul_rn(dE2, px.qi), g_r);
  }
};

// out[m][e] = sum over chunks, in chunk order, of part[m][chunk][e], e < per
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

}  // namespace

void rates_finish(const RatesCall& c, int count) {
  const int per = c.nregion * 4 * count;
  hipLaunchKernelGGL(rates_final_kernel, dim3((unsigned)((per + 63) / 64), (unsigned)c.members), dim3(64), 0,
                     (hipStream_t)c.stream, (const double*)c.workspace, rates_chunks((long)c.ncm), per, c.out);
}

}  // namespace qp

extern "C" {

int qp_collision_rates_available(int32_t ne, int32_t nw) {
  return ne >= 2 && ne <= 64 && nw >= 1 && nw <= 64 * qp::RMAXBINS - 1;
}

size_t qp_collision_rates_workspace_bytes(int32_t ne, int64_t ncell_member, int64_t members, int32_t nregion) {
  if (ne < 2 || ne > 64 || ncell_member < 1 || members < 1 || nregion < 1 || nregion > 8) return 0;
  return qp::rates_workspace_bytes(ne, ncell_member, members, nregion);
}

int qp_collision_rates(const qp_collision_tables* t, const uint8_t* region_bits, int64_t ncell_member, int64_t members,
                       int32_t nregion, const double* state, const double* phonon, double dE, int enable_recombination,
                       int enable_scattering, void* workspace, double* out, void* stream) {
  const qp::RatesCall c{t, region_bits, ncell_member, members, nregion, state, phonon, dE, enable_recombination,
                        enable_scattering, workspace, out, stream};
  if (const int e = qp::rates_check_tables(__func__, c, qp_collision_rates_available)) return e;
  if (const int e = qp::rates_check_shape(__func__, c)) return e;
  qp::rates_ladder(nregion, [&](auto nr) { qp::rates_launch<qp::CollisionBody<decltype(nr)::value>>(c); });
  qp::rates_finish(c, t->ne);
  return qp::check_launch("qp_collision_rates");
}

}  // extern "C"
