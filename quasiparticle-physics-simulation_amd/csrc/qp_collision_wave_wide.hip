// Collision update with one wave per pixel and TWO energy bins per lane (65 <= NE <= 128, NW <= 512; opt-in through
// QP_COLL_WIDE_BINS): the design of qp_collision_wave.hip carried past the 64 bins its lane <-> bin mapping allows.
//
// Lane l owns bin l (half 0, always live since NE > 64) and bin l + 64 (half 1, live when l + 64 < NE), and the phonon bins
// l, l + 64, ... l + 448.  The loop over the source bin j is written twice - j < 64 broadcasts from the half-0 registers,
// j >= 64 from the half-1 registers - so that the register v_readlane reads is fixed at compile time; inside, the two
// target halves are served one after the other with row index j NE + lane + 64 h, which makes every table row one coalesced
// read (the tables are symmetric, sign antisymmetric, as for the wave kernel).  The pixel's phonon occupations and per-bin
// sums live in LDS, 3 NW doubles per wave sized by the call's NW: no ph_scratch, where the generic kernel needs 2 NW planes.
//
// Per-bin sums without atomics (the host vouches for the |i-j| / i+j structure, diag_bin non-NULL): within one (j, half)
// instruction the lanes with E_i > E_j write A + d and the others B + d, d depends only on |i - j|, so the addresses are
// distinct; recombination writes s(i + j), distinct per lane.  The two halves are separate instructions of one wave, which
// LDS executes in order.  Dead lanes of half 1 never touch LDS.  Unstructured maps use LDS atomics (ds_add_f64).
// Every shared access is written as lds[integer index] (see qp_collision_wave.hip).
//
// A wave takes 4 consecutive pixels: n[2][4] and pb[8][4] are 40 doubles per lane, 154 registers, three waves per SIMD.
// With 8 pixels (80 doubles, 235 registers, two waves per SIMD) the kernel was 1.15 - 1.43 times slower at every size on
// MI355X (profiles/collision_wide_bins_ab.json, column b8).
#include "qp_collision_dispatch.h"

namespace qp {

namespace {

__device__ __forceinline__ double bcast2(double x, int srclane) {
  const unsigned long long u = __double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, srclane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), srclane);
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

constexpr int WIDE_PB = 4;        // pixels per wave
constexpr int WIDE_MAXBINS = 8;   // phonon bins per lane: NW <= 512
constexpr int WIDE_WAVES = 4;     // waves per block; they never synchronise with each other

// the sums of one target half's gain / loss terms
struct Rates {
  double g_s, l_s, g_r, l_r;
};

// The pair (i, j) of one live lane: i = the lane's bin of this half with old values ni / qi, row = j NE + i, nj / qj the
// broadcast values of bin j.  o_P / o_A / o_B as in the kernel.
template <bool ATOMIC>
__device__ __forceinline__ void wide_pair(const WaveCollView& t, const double* __restrict__ ks,
                                          const double* __restrict__ kr, int row, int o_P, int o_A, int o_B, bool do_ph,
                                          double dE, double ni, double qi, double nj, double qj, Rates& a) {
  extern __shared__ double lds[];
  if (ks) {
    const double K = ks[row];
    const int d = t.idx_diff[row];
    const int sg = -(int)t.sign[row];                            // sign(E_i - E_j)
    const double P = lds[o_P + d];
    a.g_s = fma(K * (sg < 0 ? 1.0 + P : P), nj, a.g_s);          // K^s_eff[j][i] n_j
    a.l_s = fma(K * (sg > 0 ? 1.0 + P : P), qj, a.l_s);          // K^s_eff[i][j] q_j
    if (do_ph && sg != 0) {
      const int slot = (sg > 0 ? o_A : o_B) + d;
      const double v = dE * (ni * K * qj);
      if (ATOMIC) atomicAdd(&lds[slot], v); else lds[slot] += v;
    }
  }
  if (kr) {
    const double K = kr[row];
    const int s = t.idx_sum[row];
    const double P = lds[o_P + s];
    a.l_r = fma(K * (1.0 + P), nj, a.l_r);
    a.g_r = fma(K * P, qj, a.g_r);
    if (do_ph) {
      const double va = dE * (ni * K * nj), vb = dE * (qi * K * qj);
      if (ATOMIC) { atomicAdd(&lds[o_A + s], va); atomicAdd(&lds[o_B + s], vb); }
      else { lds[o_A + s] += va; lds[o_B + s] += vb; }
    }
  }
}

}  // namespace

template <bool ATOMIC>
__global__ void __launch_bounds__(64 * WIDE_WAVES) collision_wave_wide_kernel(WaveCollView t, const uint8_t* __restrict__ flags,
                                                                             long ncell, const double* __restrict__ sin_,
                                                                             double* __restrict__ sout, double* __restrict__ ph,
                                                                             double dE, double dt, int en_r, int en_s,
                                                                             int upd_ph) {
  constexpr int PB = WIDE_PB;
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NE = t.ne, NW = t.nw, NN = NE * NE;
  const bool use_s = en_s && t.ks0, use_r = en_r && t.kr0;
  const bool do_ph = upd_ph && (use_s || use_r);
  const int o_P = wave * 3 * NW;        // phonon occupations of the current pixel
  const int o_A = o_P + NW;             // sum of "a" terms (emission, recombination)
  const int o_B = o_P + 2 * NW;         // sum of the negative "b" terms (absorption, pair breaking): b = A - B
  const long p0 = ((long)blockIdx.x * WIDE_WAVES + wave) * PB;
  if (p0 >= ncell) return;
  const int npx = (int)min((long)PB, ncell - p0);
  const int NE1 = NE - 64;              // live bins of half 1
  const bool on1 = lane < NE1;

  double n[2][PB], pb[WIDE_MAXBINS][PB];
#pragma unroll
  for (int k = 0; k < PB; ++k) {
    n[0][k] = (k < npx) ? sin_[(long)lane * ncell + p0 + k] : 0.0;
    n[1][k] = (on1 && k < npx) ? sin_[(long)(lane + 64) * ncell + p0 + k] : 0.0;
  }
#pragma unroll
  for (int s = 0; s < WIDE_MAXBINS; ++s) {
    const int w = lane + 64 * s;
#pragma unroll
    for (int k = 0; k < PB; ++k) pb[s][k] = (w < NW && k < npx) ? ph[(long)w * ncell + p0 + k] : 0.0;
  }

#pragma unroll
  for (int k = 0; k < PB; ++k) {
    if (k >= npx) break;
    if (!(flags[p0 + k] & QP_FLAG_ACTIVE)) continue;      // wave-uniform: holes pass through unchanged
    const int c = t.cls ? t.cls[p0 + k] : 0;
    const double* ks = use_s ? t.ks0 + (long)c * NN : nullptr;
    const double* kr = use_r ? t.kr0 + (long)c * NN : nullptr;
    const double rho0 = t.rho[(long)c * NE + lane];
    const double rho1 = on1 ? t.rho[(long)c * NE + lane + 64] : 0.0;
    const double ni0 = n[0][k], ni1 = n[1][k];
    const double qi0 = rho0 * fmax(1.0 - ni0 / fmax(rho0, 1e-30), 0.0);
    const double qi1 = rho1 * fmax(1.0 - ni1 / fmax(rho1, 1e-30), 0.0);
#pragma unroll
    for (int s = 0; s < WIDE_MAXBINS; ++s) {
      const int w = lane + 64 * s;
      if (w < NW) { lds[o_P + w] = pb[s][k]; lds[o_A + w] = 0.0; lds[o_B + w] = 0.0; }
    }
    __builtin_amdgcn_wave_barrier();      // LDS accesses of one wave execute in order: only code motion must be fenced
    Rates a0{0.0, 0.0, 0.0, 0.0}, a1{0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < 64; ++j) {        // source bins of half 0
      const double nj = bcast2(ni0, j), qj = bcast2(qi0, j);
      const int row = j * NE + lane;
      wide_pair<ATOMIC>(t, ks, kr, row, o_P, o_A, o_B, do_ph, dE, ni0, qi0, nj, qj, a0);
      if (on1) wide_pair<ATOMIC>(t, ks, kr, row + 64, o_P, o_A, o_B, do_ph, dE, ni1, qi1, nj, qj, a1);
    }
    for (int j = 0; j < NE1; ++j) {       // source bins of half 1
      const double nj = bcast2(ni1, j), qj = bcast2(qi1, j);
      const int row = (j + 64) * NE + lane;
      wide_pair<ATOMIC>(t, ks, kr, row, o_P, o_A, o_B, do_ph, dE, ni0, qi0, nj, qj, a0);
      if (on1) wide_pair<ATOMIC>(t, ks, kr, row + 64, o_P, o_A, o_B, do_ph, dE, ni1, qi1, nj, qj, a1);
    }
    n[0][k] = relax_update(ni0, dE * qi0 * a0.g_s + 2.0 * dE * qi0 * a0.g_r, dE * a0.l_s + 2.0 * dE * a0.l_r, dt);
    if (on1) n[1][k] = relax_update(ni1, dE * qi1 * a1.g_s + 2.0 * dE * qi1 * a1.g_r, dE * a1.l_s + 2.0 * dE * a1.l_r, dt);
    __builtin_amdgcn_wave_barrier();
    if (do_ph) {
#pragma unroll
      for (int s = 0; s < WIDE_MAXBINS; ++s) {
        const int w = lane + 64 * s;
        if (w < NW) pb[s][k] = affine_update(pb[s][k], lds[o_A + w], lds[o_A + w] - lds[o_B + w], dt);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }

#pragma unroll
  for (int k = 0; k < PB; ++k)
    if (k < npx) {
      sout[(long)lane * ncell + p0 + k] = n[0][k];
      if (on1) sout[(long)(lane + 64) * ncell + p0 + k] = n[1][k];
    }
  if (do_ph) {
#pragma unroll
    for (int s = 0; s < WIDE_MAXBINS; ++s) {
      const int w = lane + 64 * s;
      if (w < NW) {
#pragma unroll
        for (int k = 0; k < PB; ++k)
          if (k < npx) ph[(long)w * ncell + p0 + k] = pb[s][k];
      }
    }
  }
}

// the caller (collision_route) has checked the kernel's range: 65 <= ne <= 128, nw <= 64 WIDE_MAXBINS
void collision_wave_wide_dispatch(const WaveCollView& v, bool structured, const CollCall& c) {
  const unsigned blocks = (unsigned)((c.ncell + (long)WIDE_PB * WIDE_WAVES - 1) / ((long)WIDE_PB * WIDE_WAVES));
  const size_t shmem = (size_t)WIDE_WAVES * 3 * v.nw * sizeof(double);      // <= 48 KiB at nw = 512
  if (structured)
    hipLaunchKernelGGL(collision_wave_wide_kernel<false>, dim3(blocks), dim3(64 * WIDE_WAVES), shmem, c.stream, v, c.flags,
                       c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt, (int)c.r, (int)c.s, (int)c.u);
  else
    hipLaunchKernelGGL(collision_wave_wide_kernel<true>, dim3(blocks), dim3(64 * WIDE_WAVES), shmem, c.stream, v, c.flags,
                       c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt, (int)c.r, (int)c.s, (int)c.u);
}

}  // namespace qp
