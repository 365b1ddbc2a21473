// Register-resident collision kernels for uniform tables (one gap class); included by the instantiation units
// qp_collision_fast*.hip (one NE range each, so that the build parallelises).
//
// On the reference's uniform energy grid the phonon-bin maps have structure: idx_diff[i][j] depends only on |i-j| and
// idx_sum[i][j] only on i+j (solver.py:668-683 builds them from Ei-Ej and Ei+Ej).  The host verifies this and that no
// bin is shared between a diagonal and an anti-diagonal (no merged bins), then passes diag_bin[NE] / anti_bin[2NE-1].
// The pair loops are then walked diagonal by diagonal (scattering) and anti-diagonal by anti-diagonal (recombination):
// each needs ONE phonon occupation (one coalesced load), accumulates that bin's emission / absorption sums in two
// registers, and the bin is finalised and stored as soon as its (anti)diagonal is done - no per-cell accumulator planes,
// no indexed register arrays (everything is unrolled at compile time), tables arrive as scalar loads.
// K^s_0 and K^r_0 are symmetric, so each unordered pair is visited once.
#pragma once
#include "qp_collision_dispatch.h"

namespace qp {

typedef const double __attribute__((address_space(4))) * cdtab_t;
typedef const int __attribute__((address_space(4))) * citab_t;

template <typename T>
__device__ __forceinline__ T uniform_const(const void* p) {
  const unsigned long long a = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  return (T)(((unsigned long long)hi << 32) | lo);
}

// Returns the same wave-uniform pointer, but opaque to the optimiser: the scalar table loads made through it cannot be
// hoisted above this point.  Without it all NE^2 kernel values are loaded up-front, overflow the ~100 SGPRs and are
// parked in VGPRs (the register count then grows like 1.4 NE^2 and occupancy drops to one wave per SIMD).
template <typename T>
__device__ __forceinline__ T pin_here(T p) {
  asm volatile("" : "+s"(p));
  return p;
}

// Empty asm with the value as in/out operand: the value is "redefined" here, so every instruction that produced it
// must come before and every consumer after.  Volatile asms keep their relative order (and their order against
// stores and sched_barrier), which pure VALU instructions do not: without these pins the single huge basic block lets
// instruction selection sink most accumulator FMAs of every diagonal to the end, with their K*P products kept live.
template <int N>
__device__ __forceinline__ void pin_array(double (&a)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(a[i]));
}

struct CollFastView {
  const double* kr0;      // [NE][NE] or NULL
  const double* ks0;      // [NE][NE] or NULL
  const double* rho;      // [NE]
  const int* diag_bin;    // [NE]      phonon bin of |Ei - Ej| for |i-j| = k
  const int* anti_bin;    // [2NE-1]   phonon bin of Ei + Ej for i+j = m
  // Merged bins (a phonon bin fed by one diagonal AND one anti-diagonal, e.g. whenever 2 E_min / dE is an integer): both
  // tables carry (slot + 1) << 16 on top of the bin for such entries.  The diagonal pass then parks its two sums in
  // stash[2 slot], stash[2 slot + 1] (planes of ncell doubles, the caller's ph_scratch) instead of finalising the bin, and
  // the anti-diagonal pass - which still reads the OLD occupation - adds them before the one exponential update.
  double* stash;
  // Gap classes (non-uniform gap), PARAM kernels only: K^r_0 and K^s_0 are separable in the gap (solver.py:463-490),
  //   K^r_0 = kr_amp_ij (1 + gap^2 pair_inv_ij),   K^s_0 = ks_amp_ij max(1 - gap^2 pair_inv_ij, 0),
  // so one set of tables + the pixel's gap^2 replace per-class kernel tables; rho stays a per-class table (NE loads).
  const int32_t* cls;     // [ncell] class of each cell
  const double* gap_sq;   // [nclass]
  const double* kr_amp;   // [NE][NE] (1/tau_r) ((Ei+Ej)/kTc)^2 / kTc, or NULL
  const double* ks_amp;   // [NE][NE] (1/tau_s) (Ei-Ej)^2 / kTc^3, or NULL
  const double* pair_inv; // [NE][NE] 1 / max(Ei Ej, 1e-30)
  // Fused Pauli guard (single-pass kernels): when non-NULL every wave reduces the occupation statistics of the NEW
  // quasiparticle densities it has just formed (solver.py:967-996: max n/rho with its first linear index, first forbidden
  // index with rho <= 1e-30 and n > floor) and writes one PauliPartial at guard[wave index]; qp_collision_step_guarded
  // finishes the reduction.  Saves the separate pass over the NE planes after the last collision of a step.
  PauliPartial* guard;
  double guard_floor;
};

// Member classes (QP_COLL_MEMBER_CLASSES), the argument of the MEMB kernels: class m owns the cells [m ncell_member,
// (m + 1) ncell_member) and kr0 / ks0 / rho hold one table per class.  ncell_member is a multiple of 64, so a wave never
// straddles two members.  (A type of its own: the kernels without MEMB keep their argument block.)
struct CollFastViewM : CollFastView {
  unsigned ncell_member;
  unsigned members;
};
template <bool MEMB>
struct coll_view { typedef CollFastView type; };
template <>
struct coll_view<true> { typedef CollFastViewM type; };

// Member of the wave whose first lane holds pixel `p` (call with every lane active: the value is taken from lane 0).  Waves
// are 64 consecutive pixels starting at a multiple of 64 and ncell_member % 64 == 0, so every pixel of the wave that lies
// inside the grid belongs to this member; the clamp keeps the table base of a wave beyond the grid inside the allocation.
__device__ __forceinline__ unsigned wave_member(unsigned p, unsigned ncell_member, unsigned members) {
  const unsigned p0 = __builtin_amdgcn_readfirstlane(p);
  const unsigned m = p0 / ncell_member;
  return __builtin_amdgcn_readfirstlane(m < members - 1u ? m : members - 1u);
}

// butterfly over the 64 lanes of a wave (all lanes active): (f, t) -> np.argmax order, forb -> smallest index >= 0
__device__ __forceinline__ void guard_wave_reduce(double& f, long& t, long& forb) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const double of = __shfl_xor(f, m, 64);
    const long ot = (long)__shfl_xor((long long)t, m, 64);
    const long ofb = (long)__shfl_xor((long long)forb, m, 64);
    const bool on = of != of, fn = f != f;
    const bool take = (on || fn) ? (on && (!fn || ot < t)) : (of > f || (of == f && ot < t));
    if (take) { f = of; t = ot; }
    if (ofb >= 0 && (forb < 0 || ofb < forb)) forb = ofb;
  }
}

__device__ __forceinline__ int bin_of(int v) { return v & 0xffff; }
__device__ __forceinline__ int slot_of(int v) { return (v >> 16) - 1; }

// 1 / x by v_rcp_f64 (measured on gfx950: relative error <= 4.7e-8) + one cubically convergent step
// y (1 + e + e^2), e = 1 - x y (|x| between 1e-30 and 1e30 here): 4 instructions instead of the ~12 of the IEEE division
// sequence, result within 1-2 ulp (e^3 = 1e-22).  One pixel update contains NE + Nw + NE divisions.
__device__ __forceinline__ double rcp_nr(double x) {
  const double y = __builtin_amdgcn_rcp(x);
  const double e = fma(-x, y, 1.0);
  return fma(y, fma(e, e, e), y);
}

// exp(x) for x <= ~80 with the polynomial coefficients read from constant memory (scalar loads, SGPR operands).  The
// library exp() re-materialises ~19 literal halves into VGPRs at each of the NE + Nw call sites of an unrolled kernel
// (15 % of its instructions at NE = 12).  n = rint(x log2 e), r = x - n ln2 (two-step), e^r = 1 + r + r^2 q(r) with q the
// degree-9 interpolant of (e^r - 1 - r) / r^2 at the Chebyshev nodes of |r| <= 0.3468 (fitted in 80-bit arithmetic; with
// the coefficients rounded to double the polynomial is within 1.7e-17 of e^r - two Horner steps fewer than the Taylor
// series needs for the same bound), 2^n by ldexp (underflows to 0 for very negative x, which is what the updates need).
// With the updates' other operations the exponential is a third of a small-NE collision kernel's instructions: the
// shorter polynomial, 1 + r (1 + r q) as two fma and the three-fma reciprocal below took 5.5 % off the 4096^2 NE = 12
// double half-step pass in a same-box A/B.
static __constant__ double kExpC[24] = {
    1.4426950408889634,      6.93147180369123816490e-01, 1.90821492927058770002e-10,
    2.5100464382838972e-08, 2.7620138327857954e-07, 2.755726829438213e-06, 2.480152119183358e-05,
    0.0001984126986316285, 0.0013888888917279946, 0.008333333333330036, 0.041666666666624,
    0.16666666666666669, 0.5000000000000001,
    0.0, 0.0, 0.0,
    // [16..23]: phi_small, 1/10! ... 1/3!
    1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0};

// the table pointer made opaque once per kernel: otherwise the loads are folded back into literals
__device__ __forceinline__ cdtab_t exp_table() {
  cdtab_t c = (cdtab_t)kExpC;
  asm volatile("" : "+s"(c));
  return c;
}

__device__ __forceinline__ double exp_c(double x, cdtab_t c) {
  const double nf = __builtin_rint(x * c[0]);
  double r = fma(-nf, c[1], x);
  r = fma(-nf, c[2], r);
  // Horner steps q <- q r + c_k with c_k as the SGPR addend of a VOP3 v_fma_f64.  Left to the compiler each step becomes
  // two v_mov (c_k into a VGPR pair) + v_fmac, i.e. 22 extra instructions per exp.
  double q = c[3];
#pragma unroll
  for (int k = 4; k <= 12; ++k) {
    const double ck = c[k];
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(q) : "v"(q), "v"(r), "s"(ck));
  }
  const double e = fma(r, fma(r, q, 1.0), 1.0);
  return ldexp(e, (int)nf);
}

// phi(x) = (e^x - 1) / x for |x| < 1/8 by its Taylor series to x^9 / 10! (remainder 2.3e-17)
constexpr double kPhiSmall = 0.125;
__device__ __forceinline__ double phi_small(double x, cdtab_t c) {
  double q = c[16];
#pragma unroll
  for (int k = 17; k <= 23; ++k) {
    const double ck = c[k];
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(q) : "v"(q), "v"(x), "s"(ck));
  }
  q = fma(q, x, 0.5);
  return fma(q, x, 1.0);
}

// The exponential updates of the reference (solver.py:640-665 and :686-700), y' = max(e^x y + ((e^x - 1) / x) dt s, 0) with
// x = -rate dt.  With the time steps of the reference's configurations |x| is far below 1/8 in every bin, where
// phi(x) = (e^x - 1) / x is a 9-step Horner polynomial - no range reduction, 2^n or Newton-refined division.  The
// reference's own arithmetic is kept, though: it forms e^x in double and then e^x - 1, which for small |x| carries the
// rounding of e^x to the grid of spacing 2^-52 around 1 (a relative error of 1.1e-16 / |x| in the coefficient, 1e-10 at
// |x| = 1e-6); the closed form dt phi(x) does not, and differs from the reference's planes by up to 2e-10 on the parity
// inputs.  So the fast path reproduces that rounding: u = x phi(x), e = fl(1 + u) (what a correctly rounded exp returns),
// rho = (e - 1) - u (exact), and the reference's coefficient (e - 1) / rate = dt (phi + rho / x), where rho / x needs 1 / x
// only to the accuracy of a bare v_rcp_f64.  23 operations per update instead of 34 - 35; an update is where a small-NE
// kernel spends almost half of its instructions (47 of them against 144 pairs at NE = 12).  A wave in which any lane has a
// larger |x| (or a non-finite one) also runs the general form - e^x by exp_c, the reference's clip to +-80 - and every
// lane selects by ITS OWN x, so a pixel's result does not depend on which other pixels share its wave.  Multiply-adds are
// written as fma throughout: with the compiler free to contract, two instantiations could round differently.
__device__ __forceinline__ bool wave_none(bool pred) { return __builtin_amdgcn_ballot_w64(pred) == 0; }

// e = fl(e^x) and g = (e - 1) / x for |x| < kPhiSmall, x != 0 (x = 0: g is NaN, the callers' small-rate switch takes dt)
__device__ __forceinline__ void exp_small(double x, cdtab_t c, double& e, double& g) {
  const double phi = phi_small(x, c);
  const double u = x * phi;
  e = 1.0 + u;
  const double rho = (e - 1.0) - u;
  g = fma(rho, __builtin_amdgcn_rcp(x), phi);
}

// FAST = false: the general form only (the NE >= 30 kernels: 2.5 % slower with the fast path in a same-box A/B at NE = 50 -
// updates are a twelfth of their instructions, and 198 more branches and 8 more constants cost more than they save).
template <bool FAST = true>
__device__ __forceinline__ double relax_update_f(double n, double gain, double loss, double dt, cdtab_t ec) {
  const double mu = fmax(loss, 0.0);
  // mu - loss of the reference, written as max(-loss, 0): the callers pass loss = dE * la, and with the subtraction spelled
  // out the compiler contracts it to fma(-dE, la, mu) - not 0 but the rounding error of the product (half an ulp of the
  // loss), which times n reached P: an absolute error of 1e-16 n in n', 1e-11 of n' in a bin that a long step depletes.
  const double P = fmax(fma(fmax(-loss, 0.0), n, gain), 0.0);
  const double x = -mu * dt;
  // dt == 0 (wave-uniform; the reference returns the state unchanged): x = 0 with a finite rate, exp_small's g is NaN
  const bool small = FAST && fabs(x) < kPhiSmall, slow_rate = mu < 1e-14 || dt == 0.0;
  double fast = 0.0;
  if (FAST) {
    double decay, g;
    exp_small(x, ec, decay, g);
    fast = fmax(fma(decay, n, (slow_rate ? dt : dt * g) * P), 0.0);
    if (__builtin_expect(wave_none(!small), 1)) return fast;
  }
  const double decay_l = exp_c(x, ec);
  const double coeff = slow_rate ? dt : (1.0 - decay_l) * rcp_nr(fmax(mu, 1e-14));
  return small ? fast : fmax(fma(decay_l, n, coeff * P), 0.0);
}

template <bool FAST = true>
__device__ __forceinline__ double affine_update_f(double y, double a, double b, double dt, cdtab_t ec) {
  const double x = b * dt;
  const bool small = FAST && fabs(x) < kPhiSmall, tiny = fabs(b) < 1e-14 || dt == 0.0;
  double fast = 0.0;
  if (FAST) {
    double ex, g;
    exp_small(x, ec, ex, g);
    fast = fmax(fma(ex, y, (tiny ? dt : dt * g) * a), 0.0);
    if (__builtin_expect(wave_none(!small), 1)) return fast;
  }
  const double ex_l = exp_c(fmin(fmax(x, -80.0), 80.0), ec);
  const double coeff = tiny ? dt : (ex_l - 1.0) * rcp_nr(tiny ? 1.0 : b);
  return small ? fast : fmax(fma(ex_l, y, coeff * a), 0.0);
}

// plane of the phonon bin of table entry `v` (bin in the low 16 bits, see CollFastView::stash)
#define QP_PH(v) (ph + (long)bin_of(v) * ncell)
#define QP_PLOAD(v) __builtin_nontemporal_load(&QP_PH(v)[p])

// USE_S / USE_R / UPD are compile-time: with run-time flags the compiler clones and threads the unrolled body into
// flag-specific paths whose instructions it then interleaves across diagonals (several phonon values live at once).
// MEMB: per-member tables (CollFastViewM); the wave takes its member's rho / K^s_0 / K^r_0, everything else is the same.
template <int NE, bool USE_S, bool USE_R, bool UPD, bool PARAM = false, bool MEMB = false>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(NE <= 12 ? 4 : 1, 8)))
collision_diag_kernel(typename coll_view<MEMB>::type t, const uint8_t* __restrict__ flags,
                                                             long ncell, const double* __restrict__ sin_,
                                                             double* __restrict__ sout, double* __restrict__ ph,
                                                             double dE, double dt) {
  // p is kept as a 32-bit offset and every plane base is wave-uniform (host checks ncell < 2^28)
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  // statistics of this thread's pixel for the fused guard (neutral for threads without an active pixel)
  double gf = -__builtin_huge_val();
  long gt = 0x7fffffffffffffffL, gforb = -1;
  const bool in_grid = p < (unsigned long)ncell;
  // before the branches below, where all 64 lanes are still active
  unsigned long mb = 0;
  if constexpr (MEMB) mb = wave_member(p, t.ncell_member, t.members);
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
  const cdtab_t ksa = uniform_const<cdtab_t>(t.ks_amp);
  const cdtab_t kra = uniform_const<cdtab_t>(t.kr_amp);
  const cdtab_t pinv = uniform_const<cdtab_t>(t.pair_inv);
  const int cl = PARAM ? t.cls[p] : 0;
  const double g2 = PARAM ? t.gap_sq[cl] : 0.0;
  // prefetch distance of the phonon occupations: 4 (anti)diagonals when phonons are only read (one diagonal is ~10
  // pairs of work, far less than a memory round trip; c2: 94 -> 79 us); with the in-place phonon stores in the same
  // stream a deeper prefetch measured slower (c4: 655 -> 763 us), so 1 there
#ifndef QP_PF_UPD
#define QP_PF_UPD 1
#endif
  constexpr int PF = UPD ? QP_PF_UPD : 4;

  // (NE >= 32 never gets here: launch_register splits it into collision_range_kernel passes + collision_phonon_kernel.)
  double n[NE], q[NE], ga[NE], la[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    n[i] = __builtin_nontemporal_load(&(sin_ + (long)i * ncell)[p]);
    const double r = PARAM ? t.rho[(long)cl * NE + i] : rho[i];
    q[i] = r * fmax(1.0 - n[i] * rcp_nr(fmax(r, 1e-30)), 0.0);
    ga[i] = 0.0;
    la[i] = 0.0;
  }

  // One phonon occupation per (anti)diagonal, prefetched PF ahead.  The scheduling barriers keep the compiler from
  // hoisting every load / exp chain to the top (which costs ~60 live doubles and halves the occupancy); with them the
  // live set is n, q, ga, la plus one diagonal's temporaries.
  if (USE_S) {
    double Pq[PF];
#pragma unroll
    for (int k = 1; k <= PF && k < NE; ++k) Pq[k % PF] = QP_PLOAD(dbin[k]);
#pragma unroll
    for (int k = 1; k < NE; ++k) {
      const int entry = dbin[k];
      const cdtab_t ksk = pin_here(PARAM ? ksa : ks);
      const cdtab_t piv = pin_here(pinv);
      const double P = Pq[k % PF];
      if (k + PF < NE) Pq[k % PF] = QP_PLOAD(dbin[k + PF]);
      double em = 0.0, ab = 0.0;
#pragma unroll
      for (int j = 0; j + k < NE; ++j) {
        const int i = j + k;                    // E_i > E_j: (i -> j) emits, (j -> i) absorbs
        const double K = PARAM ? ksk[i * NE + j] * fmax(fma(-g2, piv[i * NE + j], 1.0), 0.0) : ksk[i * NE + j];
        const double t1 = K * P, t2 = K + t1;   // K P and K (1 + P)
        ga[i] = fma(t1, n[j], ga[i]);
        la[i] = fma(t2, q[j], la[i]);
        ga[j] = fma(t2, n[i], ga[j]);
        la[j] = fma(t1, q[i], la[j]);
        em = fma(n[i] * K, q[j], em);
        ab = fma(n[j] * K, q[i], ab);
      }
      if (UPD) {
        if (USE_R && slot_of(entry) >= 0) {     // merged bin (wave-uniform): finalised by its anti-diagonal
          (t.stash + (long)(2 * slot_of(entry)) * ncell)[p] = em;
          (t.stash + (long)(2 * slot_of(entry) + 1) * ncell)[p] = ab;
        } else {
          __builtin_nontemporal_store(affine_update_f(P, dE * em, dE * (em - ab), dt, ec), &QP_PH(entry)[p]);
        }
      }
      pin_array(ga);
      pin_array(la);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (USE_R) {
    double Pq[PF];
#pragma unroll
    for (int m = 0; m < PF && m < 2 * NE - 1; ++m) Pq[m % PF] = QP_PLOAD(abin[m]);
#pragma unroll
    for (int m = 0; m < 2 * NE - 1; ++m) {
      const int entry = abin[m];
      const cdtab_t krm = pin_here(PARAM ? kra : kr);
      const cdtab_t piv = pin_here(pinv);
      const double P = Pq[m % PF];
      if (m + PF < 2 * NE - 1) Pq[m % PF] = QP_PLOAD(abin[m + PF]);
      double rec = 0.0, pb = 0.0;
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int j = m - i;
        if (j < 0 || j >= NE || j > i) continue;
        const double K2 = 2.0 * (PARAM ? krm[i * NE + j] * fma(g2, piv[i * NE + j], 1.0) : krm[i * NE + j]);
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
        double a = dE * rec, b = dE * (rec - pb);
        if (USE_S && slot_of(entry) >= 0) {     // merged bin: add the sums its diagonal parked
          const double em = (t.stash + (long)(2 * slot_of(entry)) * ncell)[p];
          const double ab = (t.stash + (long)(2 * slot_of(entry) + 1) * ncell)[p];
          a = dE * (em + rec);
          b = dE * ((em - ab) + (rec - pb));
        }
        __builtin_nontemporal_store(affine_update_f(P, a, b, dt, ec), &QP_PH(entry)[p]);
      }
      pin_array(ga);
      pin_array(la);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    n[i] = relax_update_f(n[i], dE * q[i] * ga[i], dE * la[i], dt, ec);
    __builtin_nontemporal_store(n[i], &(sout + (long)i * ncell)[p]);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (t.guard) {        // wave-uniform: occupations of the new densities, bins in ascending order (first maximum wins)
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const double r = PARAM ? t.rho[(long)cl * NE + i] : rho[i];
      const long lin = (long)i * ncell + p;
      double occ = 0.0;
      if (r > 1e-30) occ = n[i] / fmax(r, 1e-30);
      else if (n[i] > t.guard_floor && gforb < 0) gforb = lin;
      if (occ > gf) { gf = occ; gt = lin; }
    }
  }
  }
  if (t.guard) {        // every lane of the wave gets here (no early exits above)
    guard_wave_reduce(gf, gt, gforb);
    if ((threadIdx.x & 63) == 0) {
      PauliPartial* dst = t.guard + ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
      dst->maxf = gf;
      dst->maxidx = gt;
      dst->forb = gforb;
    }
  }
}


// Phonon half of the update for NE >= 32, where the fused kernel no longer fits two waves per SIMD: only n stays resident
// (q is re-formed at each use), every (anti)diagonal accumulates its bin's emission / absorption sums and finalises the
// bin.  Runs AFTER the collision_range_kernel passes of the same call: those read the old phonon planes and write the new
// quasiparticle planes to `sout`, this one reads the old quasiparticle planes `sin_` and updates `ph`.
template <int NE, bool USE_S, bool USE_R, bool PARAM = false>
__global__ void __launch_bounds__(128) collision_phonon_kernel(CollFastView t, const uint8_t* __restrict__ flags, long ncell,
                                                               const double* __restrict__ sin_, double* __restrict__ ph,
                                                               double dE, double dt) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (unsigned long)ncell) return;
  if (!(flags[p] & QP_FLAG_ACTIVE)) return;
  const cdtab_t rho = uniform_const<cdtab_t>(t.rho);
  const cdtab_t ks = uniform_const<cdtab_t>(t.ks0);
  const cdtab_t kr = uniform_const<cdtab_t>(t.kr0);
  const citab_t dbin = uniform_const<citab_t>(t.diag_bin);
  const citab_t abin = uniform_const<citab_t>(t.anti_bin);
  const cdtab_t ec = exp_table();
  // Up to NE = 32, n and q = max(rho - n, 0) of all bins stay resident (4 NE registers, two waves per SIMD): a pair then
  // costs a multiply and an FMA per sum instead of re-forming q twice (-5 % per call at NE = 32).  Measured slower beyond
  // (NE = 40: 1571 -> 1641 us, NE = 50: 2325 -> 2587 us per call: the register file no longer holds both), so larger NE
  // re-form q = max(rho_i - n_i, 0) at each use with rho_i as a scalar operand.
  // Gap classes (PARAM): rho is a per-class table, i.e. a per-lane value - q has to be resident whatever NE (one wave per
  // SIMD beyond NE = 32), formed as in the single-pass kernel; K comes from the separable amplitude tables.
  constexpr bool QRES = NE <= 32 || PARAM;
  const cdtab_t ksa = uniform_const<cdtab_t>(t.ks_amp);
  const cdtab_t kra = uniform_const<cdtab_t>(t.kr_amp);
  const cdtab_t pinv = uniform_const<cdtab_t>(t.pair_inv);
  const int cl = PARAM ? t.cls[p] : 0;
  const double g2 = PARAM ? t.gap_sq[cl] : 0.0;
  double n[NE], q[QRES ? NE : 1];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    n[i] = __builtin_nontemporal_load(&(sin_ + (long)i * ncell)[p]);
    if (PARAM) {
      const double r = t.rho[(long)cl * NE + i];
      q[QRES ? i : 0] = r * fmax(1.0 - n[i] * rcp_nr(fmax(r, 1e-30)), 0.0);
    } else if (QRES) {
      q[QRES ? i : 0] = fmax(rho[i] - n[i], 0.0);
    }
  }
  const cdtab_t rhop = rho;
#define QP_Q(i) (QRES ? q[QRES ? (i) : 0] : fmax(rhop[i] - n[i], 0.0))
  if (USE_S) {
    double Pnext = NE > 1 ? QP_PLOAD(dbin[1]) : 0.0;
#pragma unroll
    for (int k = 1; k < NE; ++k) {
      const int entry = dbin[k];
      const cdtab_t ksk = pin_here(PARAM ? ksa : ks);
      const cdtab_t piv = pin_here(pinv);
      const double P = Pnext;
      if (k + 1 < NE) Pnext = QP_PLOAD(dbin[k + 1]);
      double em = 0.0, ab = 0.0;
#pragma unroll
      for (int j = 0; j + k < NE; ++j) {
        const int i = j + k;
        const double K = PARAM ? ksk[i * NE + j] * fmax(fma(-g2, piv[i * NE + j], 1.0), 0.0) : ksk[i * NE + j];
        em = fma(n[i] * K, QP_Q(j), em);
        ab = fma(n[j] * K, QP_Q(i), ab);
      }
      if (USE_R && slot_of(entry) >= 0) {
        (t.stash + (long)(2 * slot_of(entry)) * ncell)[p] = em;
        (t.stash + (long)(2 * slot_of(entry) + 1) * ncell)[p] = ab;
      } else {
        __builtin_nontemporal_store(affine_update_f<false>(P, dE * em, dE * (em - ab), dt, ec), &QP_PH(entry)[p]);
      }
      asm volatile("" : "+v"(Pnext));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (USE_R) {
    double Pnext = QP_PLOAD(abin[0]);
#pragma unroll
    for (int m = 0; m < 2 * NE - 1; ++m) {
      const int entry = abin[m];
      const cdtab_t krm = pin_here(PARAM ? kra : kr);
      const cdtab_t piv = pin_here(pinv);
      const double P = Pnext;
      if (m + 1 < 2 * NE - 1) Pnext = QP_PLOAD(abin[m + 1]);
      double rec = 0.0, pb = 0.0;
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int j = m - i;
        if (j < 0 || j >= NE || j > i) continue;
        const double K2 = (i != j ? 2.0 : 1.0) * (PARAM ? krm[i * NE + j] * fma(g2, piv[i * NE + j], 1.0) : krm[i * NE + j]);
        const double qi = QP_Q(i);
        rec = fma(n[i] * K2, n[j], rec);
        pb = fma(qi * K2, i != j ? QP_Q(j) : qi, pb);
      }
      double a = dE * rec, b = dE * (rec - pb);
      if (USE_S && slot_of(entry) >= 0) {
        const double em = (t.stash + (long)(2 * slot_of(entry)) * ncell)[p];
        const double ab = (t.stash + (long)(2 * slot_of(entry) + 1) * ncell)[p];
        a = dE * (em + rec);
        b = dE * ((em - ab) + (rec - pb));
      }
      __builtin_nontemporal_store(affine_update_f<false>(P, a, b, dt, ec), &QP_PH(entry)[p]);
      asm volatile("" : "+v"(Pnext));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef QP_Q
}

// Quasiparticle half of the update for target bins [LO, HI) only (phonons read, never written): NE >= 32 is done in
// NE / (HI - LO) such passes + collision_phonon_kernel.  n of all bins stays resident (2 NE registers), gain / loss only
// for the HI - LO targets, q is re-formed at each use as max(rho_i - n_i, 0) (two instructions, rho_i a scalar operand;
// differs from rho (1 - n / rho) by rounding only) - ~230 registers at NE = 50, HI - LO = 25, i.e. two waves per SIMD and
// no AGPR shuffling, where a single-pass kernel needs 455.  The pair loops are those of collision_diag_kernel with the
// updates of targets outside the range removed at compile time (pairs with no target in range vanish entirely).
template <int NE, bool USE_S, bool USE_R, int LO, int HI, bool PARAM = false>
__global__ void __launch_bounds__(128) collision_range_kernel(CollFastView t, const uint8_t* __restrict__ flags, long ncell,
                                                              const double* __restrict__ sin_, double* __restrict__ sout,
                                                              const double* __restrict__ ph, double dE, double dt) {
  constexpr int TB = HI - LO;
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (unsigned long)ncell) return;
  if (!(flags[p] & QP_FLAG_ACTIVE)) {
#pragma unroll
    for (int i = LO; i < HI; ++i) (sout + (long)i * ncell)[p] = (sin_ + (long)i * ncell)[p];
    return;
  }
  const cdtab_t rho = uniform_const<cdtab_t>(t.rho);
  const cdtab_t ks = uniform_const<cdtab_t>(t.ks0);
  const cdtab_t kr = uniform_const<cdtab_t>(t.kr0);
  const citab_t dbin = uniform_const<citab_t>(t.diag_bin);
  const citab_t abin = uniform_const<citab_t>(t.anti_bin);
  const cdtab_t ec = exp_table();
  // gap classes (PARAM): q resident (rho is per lane), K from the separable amplitude tables - see collision_phonon_kernel
  const cdtab_t ksa = uniform_const<cdtab_t>(t.ks_amp);
  const cdtab_t kra = uniform_const<cdtab_t>(t.kr_amp);
  const cdtab_t pinv = uniform_const<cdtab_t>(t.pair_inv);
  const int cl = PARAM ? t.cls[p] : 0;
  const double g2 = PARAM ? t.gap_sq[cl] : 0.0;
  double n[NE], ga[TB], la[TB];
  double q[PARAM ? NE : 1];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    n[i] = __builtin_nontemporal_load(&(sin_ + (long)i * ncell)[p]);
    if (PARAM) {
      const double r = t.rho[(long)cl * NE + i];
      q[PARAM ? i : 0] = r * fmax(1.0 - n[i] * rcp_nr(fmax(r, 1e-30)), 0.0);
    }
  }
#pragma unroll
  for (int i = 0; i < TB; ++i) { ga[i] = 0.0; la[i] = 0.0; }
#define QP_Q(i) (PARAM ? q[PARAM ? (i) : 0] : fmax(rhop[i] - n[i], 0.0))
#define QP_IN(i) ((i) >= LO && (i) < HI)
  if (USE_S) {
    double Pnext = NE > 1 ? QP_PLOAD(dbin[1]) : 0.0;
#pragma unroll
    for (int k = 1; k < NE; ++k) {
      const cdtab_t ksk = pin_here(PARAM ? ksa : ks);
      const cdtab_t piv = pin_here(pinv);
      const cdtab_t rhop = pin_here(rho);
      const double P = Pnext;
      if (k + 1 < NE) Pnext = QP_PLOAD(dbin[k + 1]);
#pragma unroll
      for (int j = 0; j + k < NE; ++j) {
        const int i = j + k;                    // E_i > E_j
        if (!QP_IN(i) && !QP_IN(j)) continue;
        const double K = PARAM ? ksk[i * NE + j] * fmax(fma(-g2, piv[i * NE + j], 1.0), 0.0) : ksk[i * NE + j];
        const double t1 = K * P, t2 = K + t1;
        if (QP_IN(i)) {
          ga[i - LO] = fma(t1, n[j], ga[i - LO]);
          la[i - LO] = fma(t2, QP_Q(j), la[i - LO]);
        }
        if (QP_IN(j)) {
          ga[j - LO] = fma(t2, n[i], ga[j - LO]);
          la[j - LO] = fma(t1, QP_Q(i), la[j - LO]);
        }
      }
      pin_array(ga);
      pin_array(la);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (USE_R) {
    double Pnext = QP_PLOAD(abin[0]);
#pragma unroll
    for (int m = 0; m < 2 * NE - 1; ++m) {
      const cdtab_t krm = pin_here(PARAM ? kra : kr);
      const cdtab_t piv = pin_here(pinv);
      const cdtab_t rhop = pin_here(rho);
      const double P = Pnext;
      if (m + 1 < 2 * NE - 1) Pnext = QP_PLOAD(abin[m + 1]);
#pragma unroll
      for (int i = 0; i < NE; ++i) {
        const int j = m - i;
        if (j < 0 || j >= NE || j > i) continue;
        if (!QP_IN(i) && !QP_IN(j)) continue;
        const double K2 = 2.0 * (PARAM ? krm[i * NE + j] * fma(g2, piv[i * NE + j], 1.0) : krm[i * NE + j]);
        const double t1 = K2 * P, t2 = K2 + t1;
        if (QP_IN(i)) {
          la[i - LO] = fma(t2, n[j], la[i - LO]);
          ga[i - LO] = fma(t1, QP_Q(j), ga[i - LO]);
        }
        if (i != j && QP_IN(j)) {
          la[j - LO] = fma(t2, n[i], la[j - LO]);
          ga[j - LO] = fma(t1, QP_Q(i), ga[j - LO]);
        }
      }
      pin_array(ga);
      pin_array(la);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int i = LO; i < HI; ++i) {
    const cdtab_t rhop = rho;
    __builtin_nontemporal_store(relax_update_f<false>(n[i], dE * QP_Q(i) * ga[i - LO], dE * la[i - LO], dt, ec),
                                &(sout + (long)i * ncell)[p]);
    __builtin_amdgcn_sched_barrier(0);
  }
#undef QP_Q
#undef QP_IN
}

// The launches of one (NE, S, R) of the register family: NE >= 32 as the split - the quasiparticle half in two target ranges
// (old P), then the phonon half (old n, old P) when phonons are dynamic - smaller NE as the single-pass kernel.  PARAM: the
// gap-class form of every kernel (q resident, K from the amplitude tables).  MEMB: member tables, single-pass sizes only.
// The kernels without MEMB are launched with the CollFastView part of the view, which is their whole argument.
template <int NE, bool S, bool R, bool PARAM, bool MEMB>
static void launch_register(const CollFastViewM& vm, const CollCall& c) {
  static_assert(!MEMB || NE < 32, "the split kernels have no member-table form");
  const typename coll_view<MEMB>::type& v = vm;
  const unsigned blocks = (unsigned)((c.ncell + 127) / 128);
  if constexpr (NE >= 32) {
    constexpr int MID = NE / 2;
    hipLaunchKernelGGL((collision_range_kernel<NE, S, R, 0, MID, PARAM>), dim3(blocks), dim3(128), 0, c.stream, v, c.flags,
                       c.ncell, c.sin, c.sout, (const double*)c.ph, c.dE, c.dt);
    hipLaunchKernelGGL((collision_range_kernel<NE, S, R, MID, NE, PARAM>), dim3(blocks), dim3(128), 0, c.stream, v, c.flags,
                       c.ncell, c.sin, c.sout, (const double*)c.ph, c.dE, c.dt);
    if (c.u)
      hipLaunchKernelGGL((collision_phonon_kernel<NE, S, R, PARAM>), dim3(blocks), dim3(128), 0, c.stream, v, c.flags,
                         c.ncell, c.sin, c.ph, c.dE, c.dt);
  } else if (c.u) {
    hipLaunchKernelGGL((collision_diag_kernel<NE, S, R, true, PARAM, MEMB>), dim3(blocks), dim3(128), 0, c.stream, v,
                       c.flags, c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt);
  } else {
    hipLaunchKernelGGL((collision_diag_kernel<NE, S, R, false, PARAM, MEMB>), dim3(blocks), dim3(128), 0, c.stream, v,
                       c.flags, c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt);
  }
}

// the launcher families of the register kernels (qp_collision_dispatch.h): one gap class, gap classes, member tables
template <int NE, bool S, bool R>
static void launch_diag(const CollFastViewM& v, const CollCall& c) { launch_register<NE, S, R, false, false>(v, c); }
template <int NE, bool S, bool R>
static void launch_diagp(const CollFastViewM& v, const CollCall& c) { launch_register<NE, S, R, true, false>(v, c); }
template <int NE, bool S, bool R>
static void launch_diagm(const CollFastViewM& v, const CollCall& c) { launch_register<NE, S, R, false, true>(v, c); }

}  // namespace qp
