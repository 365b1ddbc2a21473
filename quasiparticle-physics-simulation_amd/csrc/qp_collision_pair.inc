// Two consecutive collision half-steps in ONE pass over the state (small NE, one gap class, no merged phonon bins).
//
// Under Strang splitting a step is C(dt/2) D(dt) C(dt/2) (solver.py:1469-1475): the closing half-step of step k and the
// opening half-step of step k + 1 act on the same state with nothing between them but the Pauli guard of step k
// (solver.py:1477) and the explicit generation term of step k + 1 (solver.py:1459-1464) - unless step k is a store point.
// Run as two launches they read and write all NE + Nw planes twice (752 B per pixel and call at NE = 12, Nw = 35, where
// the kernel is balanced between HBM and the fp64 units).  Here the state makes ONE round trip:
//
//     n, P  --C(dt_a)-->  n', P'   [guard statistics of n']   n' += g   --C(dt_b)-->  n'', P''
//
// with n', P' never leaving the registers.  The arithmetic of each half is the single-pass kernel's, operation for
// operation (same pair order, same update formulas), so the result equals the two-launch sequence bit for bit.
// Register plan: n, q, gain, loss of all bins (4 NE doubles) + one occupation per DIAGONAL (NE - 1 doubles, indexed by
// diagonal - static after unrolling - not by bin).  The 2 NE - 1 anti-diagonal occupations do not stay in registers between
// the halves: the first half streams the old values in (a short prefetch queue) and parks each new value in LDS
// ([anti-diagonal][thread], 8 B per lane and value: 23.5 KB per 128-thread block at NE = 12), the second half reads them
// back one anti-diagonal ahead of its use.  That keeps the kernel at three waves per SIMD at NE = 12 (two with everything
// resident: 189 registers).
#pragma once
#include "qp_collision_fast.inc"

namespace qp {

// MEMB: per-member tables, selected per wave as in collision_diag_kernel.
template <int NE, bool USE_S, bool USE_R, bool UPD, bool MEMB = false>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu((NE <= 12 && UPD) ? 3 : 2)))
collision_pair_kernel(typename coll_view<MEMB>::type t, const uint8_t* __restrict__ flags, long ncell,
                      const double* __restrict__ sin_, double* __restrict__ sout, double* __restrict__ ph, double dE,
                      double dt_a, double dt_b, double gen_amount) {
  __shared__ double lds[(USE_R && UPD) ? (2 * NE - 1) * 128 : 1];
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  double gf = -__builtin_huge_val();
  long gt = 0x7fffffffffffffffL, gforb = -1;
  const bool in_grid = p < (unsigned long)ncell;
  unsigned long mb = 0;
  if constexpr (MEMB) mb = wave_member(p, t.ncell_member, t.members);      // all 64 lanes still active
  if (in_grid && !(flags[p] & QP_FLAG_ACTIVE)) {
#pragma unroll
    for (int i = 0; i < NE; ++i) (sout + (long)i * ncell)[p] = (sin_ + (long)i * ncell)[p];
  } else if (in_grid) {
    const cdtab_t rho = uniform_const<cdtab_t>(MEMB ? t.rho + mb * NE : t.rho);
    const cdtab_t ks = uniform_const<cdtab_t>(MEMB ? t.ks0 + mb * (NE * NE) : t.ks0);
    const cdtab_t kr = uniform_const<cdtab_t>(MEMB ? t.kr0 + mb * (NE * NE) : t.kr0);
    const citab_t dbin = uniform_const<citab_t>(t.diag_bin);
    const citab_t abin = uniform_const<citab_t>(t.anti_bin);
    const cdtab_t ec = exp_table();
    double n[NE], q[NE], ga[NE], la[NE];
    double Pd[USE_S ? NE : 1];
    constexpr int NA = 2 * NE - 1;
    constexpr int PFA = 3;             // prefetch depth of the streamed anti-diagonal occupations
    double* const park = lds + threadIdx.x;      // parked value of anti-diagonal m: park[m * 128]
    // frozen phonons: nothing changes between the halves and nothing is written - the occupations are loaded once and stay
    double Pa[(USE_R && !UPD) ? NA : 1];
    if (USE_R && !UPD) {
#pragma unroll
      for (int m = 0; m < NA; ++m) Pa[(USE_R && !UPD) ? m : 0] = QP_PLOAD(abin[m]);
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) n[i] = __builtin_nontemporal_load(&(sin_ + (long)i * ncell)[p]);
    if (USE_S) {
#pragma unroll
      for (int k = 1; k < NE; ++k) Pd[USE_S ? k : 0] = QP_PLOAD(dbin[k]);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const double dt = half == 0 ? dt_a : dt_b;
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const double r = rho[i];
        q[i] = r * fmax(1.0 - n[i] * rcp_nr(fmax(r, 1e-30)), 0.0);
        ga[i] = 0.0;
        la[i] = 0.0;
      }
      if (USE_S) {
#pragma unroll
        for (int k = 1; k < NE; ++k) {
          const cdtab_t ksk = pin_here(ks);
          const double P = Pd[USE_S ? k : 0];
          double em = 0.0, ab = 0.0;
#pragma unroll
          for (int j = 0; j + k < NE; ++j) {
            const int i = j + k;                    // E_i > E_j: (i -> j) emits, (j -> i) absorbs
            const double K = ksk[i * NE + j];
            const double t1 = K * P, t2 = K + t1;   // K P and K (1 + P)
            ga[i] = fma(t1, n[j], ga[i]);
            la[i] = fma(t2, q[j], la[i]);
            ga[j] = fma(t2, n[i], ga[j]);
            la[j] = fma(t1, q[i], la[j]);
            em = fma(n[i] * K, q[j], em);
            ab = fma(n[j] * K, q[i], ab);
          }
          if (UPD) {
            // pinned: the new occupation is only USED in the second half-step, and a pure computation may be sunk to its
            // use - all 34 exponential updates, each holding (P, em, ab) alive instead of one result (measured: 1.3 KB of
            // spills per lane, three times slower than two separate calls)
            Pd[USE_S ? k : 0] = affine_update_f(P, dE * em, dE * (em - ab), dt, ec);
            asm volatile("" : "+v"(Pd[USE_S ? k : 0]));
          }
          pin_array(ga);
          pin_array(la);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (USE_R) {
        // old occupations of the first half come from the planes, those of the second half from the LDS park (or, with
        // frozen phonons, from the planes again: they have not changed)
        const bool from_park = UPD && half == 1;
        double Pq[PFA];
#pragma unroll
        for (int m = 0; UPD && m < PFA && m < NA; ++m) Pq[m % PFA] = from_park ? park[m * 128] : QP_PLOAD(abin[m]);
#pragma unroll
        for (int m = 0; m < NA; ++m) {
          const cdtab_t krm = pin_here(kr);
          const double P = UPD ? Pq[m % PFA] : Pa[(USE_R && !UPD) ? m : 0];
          if (UPD && m + PFA < NA) Pq[m % PFA] = from_park ? park[(m + PFA) * 128] : QP_PLOAD(abin[m + PFA]);
          double rec = 0.0, pb = 0.0;
#pragma unroll
          for (int i = 0; i < NE; ++i) {
            const int j = m - i;
            if (j < 0 || j >= NE || j > i) continue;
            const double K2 = 2.0 * krm[i * NE + j];
            const double t1 = K2 * P, t2 = K2 + t1;
            if (i != j) {
              la[i] = fma(t2, n[j], la[i]);
              la[j] = fma(t2, n[i], la[j]);
              ga[i] = fma(t1, q[j], ga[i]);
              ga[j] = fma(t1, q[i], ga[j]);
              rec = fma(n[i] * K2, n[j], rec);
              pb = fma(q[i] * K2, q[j], pb);
            } else {
              la[i] = fma(t2, n[i], la[i]);
              ga[i] = fma(t1, q[i], ga[i]);
              rec = fma(0.5 * K2 * n[i], n[i], rec);
              pb = fma(0.5 * K2 * q[i], q[i], pb);
            }
          }
          if (UPD) {
            const double Pnew = affine_update_f(P, dE * rec, dE * (rec - pb), dt, ec);
            if (half == 0) park[m * 128] = Pnew;      // a store: cannot be sunk to the second half
            else __builtin_nontemporal_store(Pnew, &QP_PH(abin[m])[p]);
          }
          pin_array(ga);
          pin_array(la);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        n[i] = relax_update_f(n[i], dE * q[i] * ga[i], dE * la[i], dt, ec);
        asm volatile("" : "+v"(n[i]));
        __builtin_amdgcn_sched_barrier(0);
      }
      if (half == 0) {
        if (t.guard) {        // statistics of the state BETWEEN the two half-steps (the guard of the step that ends here)
#pragma unroll
          for (int i = 0; i < NE; ++i) {
            const double r = rho[i];
            const long lin = (long)i * ncell + p;
            double occ = 0.0;
            if (r > 1e-30) occ = n[i] / fmax(r, 1e-30);
            else if (n[i] > t.guard_floor && gforb < 0) gforb = lin;
            if (occ > gf) { gf = occ; gt = lin; }
          }
        }
        if (gen_amount != 0.0) {      // constant / pulse generation of the step that begins here (solver.py:1464)
#pragma unroll
          for (int i = 0; i < NE; ++i) n[i] += gen_amount;
        }
      }
    }
    // The plane addresses of the stores are formed again from an opaque copy of the cell index: otherwise the 35 + 12
    // 64-bit addresses of the loads at the top are kept alive through both half-steps for reuse here (92 registers - with
    // them the kernel spilled 1.3 KB per lane and ran three times slower than two separate calls).
    unsigned ps = p;
    asm volatile("" : "+v"(ps));
#pragma unroll
    for (int i = 0; i < NE; ++i) __builtin_nontemporal_store(n[i], &(sout + (long)i * ncell)[ps]);
    if (UPD) {
      const citab_t dbs = pin_here(dbin);
      if (USE_S) {
#pragma unroll
        for (int k = 1; k < NE; ++k) __builtin_nontemporal_store(Pd[USE_S ? k : 0], &(ph + (long)bin_of(dbs[k]) * ncell)[ps]);
      }
    }
  }
  if (t.guard) {        // every lane of the wave gets here
    guard_wave_reduce(gf, gt, gforb);
    if ((threadIdx.x & 63) == 0) {
      PauliPartial* dst = t.guard + ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
      dst->maxf = gf;
      dst->maxidx = gt;
      dst->forb = gforb;
    }
  }
}

// the launcher families of the double half-step kernel (qp_collision_dispatch.h): shared tables, member tables
template <int NE, bool S, bool R, bool MEMB = false>
static void launch_pair(const CollFastViewM& vm, const CollCall& c) {
  const typename coll_view<MEMB>::type& v = vm;      // without MEMB: the CollFastView part, the kernel's whole argument
  const unsigned blocks = (unsigned)((c.ncell + 127) / 128);
  if (c.u)
    hipLaunchKernelGGL((collision_pair_kernel<NE, S, R, true, MEMB>), dim3(blocks), dim3(128), 0, c.stream, v, c.flags,
                       c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt, c.dt_b, c.gen);
  else
    hipLaunchKernelGGL((collision_pair_kernel<NE, S, R, false, MEMB>), dim3(blocks), dim3(128), 0, c.stream, v, c.flags,
                       c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt, c.dt_b, c.gen);
}
template <int NE, bool S, bool R>
static void launch_pairm(const CollFastViewM& v, const CollCall& c) { launch_pair<NE, S, R, true>(v, c); }

}  // namespace qp
