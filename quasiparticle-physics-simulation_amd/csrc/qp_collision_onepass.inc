// One-pass collision kernel for the reference's default resolution (NE = 50, solver.py:1012): ONE launch where the split
// kernels of qp_collision_fast.inc need three that each re-read n and the phonon planes and execute 58 k VALU instructions
// per wave between them.
//
// Register plan (two waves per SIMD: 256 registers per lane; one pixel per lane).  The single-pass kernel of the small
// sizes keeps n, q, gain and loss of ALL bins resident - 4 NE doubles = 400 registers at NE = 50.  Here only the old
// densities n[NE] are resident throughout (100 registers) and the update runs in two phases:
//
//   phase 1  quasiparticles, one target block of TB bins at a time (gain / loss accumulators of the block: 4 TB
//            registers), PARTNER-major: for every partner bin j - its q_j = max(rho_j - n_j, 0) formed on the spot, once -
//            the TB targets i of the block receive their half of the pair's update,
//                 scattering      k = |i - j|:  t1 = K P_k, t2 = t1 + K;   i > j: gain_i += t1 n_j, loss_i += t2 q_j
//                                                                          i < j: gain_i += t2 n_j, loss_i += t1 q_j
//                 recombination   m = i + j:    t1 = K P_m, t2 = t1 + K;          loss_i += t2 n_j, gain_i += t1 q_j   (x 2)
//            i.e. 4 operations per ORDERED pair (4 NE^2 per process pair instead of the 3 NE^2 of a symmetric visit, the
//            price of never holding q or a second accumulator set), with K[j][lo .. lo + TB) one contiguous run of the
//            ordinary row-major tables (K is symmetric) and the phonon occupations in a window of TB registers that slides
//            by one (anti)diagonal per partner - a compile-time schedule, every index is static after unrolling.  Targets
//            are taken G at a time: their K P products, then their sums, then their updates - independent instructions in
//            a row (a back-to-back dependent fp64 instruction costs a wave about twice its issue time, and two waves do
//            not hide that).  The factor 2 of the recombination terms is applied by halving the scattering sums before and
//            doubling everything after (exact).  The block's new densities are stored and its registers reused.
//   phase 2  phonons: q[NE] is materialised (the accumulators are dead: n, q = 200 registers) and the (anti)diagonals are
//            walked as in collision_phonon_kernel - emission / absorption sums of one bin in two registers (summed in the
//            reference's order: see the comment there), the bin finalised and stored - with the kernel values of a
//            diagonal contiguous in the diagonal-major tables (qp_collision_tables::ks0_diag, kr0_anti2).
//
// Where the tables live.  With two waves on a SIMD that run the same straight-line code almost in lock-step, operand
// latency is the enemy.  Scalar loads return out of order, so every wait on one is a wait on all outstanding ones - a
// prefetch can never be further ahead than one wait interval, i.e. one partner step - and the 40 - 100 KB of tables do
// not live in the 16 KB scalar cache.  (Measured on the scalar-load variant of this kernel: 2.8 ms per 1024^2 call as
// written first; 2.0 ms with the operands travelling one step ahead in two alternating SGPR buffers and the row segments
// of a block touched into the scalar cache up front - its limit.)  So a 256-thread block stages the tables of a phase in
// LDS once (phase 1: ks0, kr0, rho and the byte offsets of the phonon planes, 41 KB; phase 2: ks0_diag, kr0_anti2, 60 KB;
// two blocks per CU) and every lane reads them from there with compile-time offsets: a broadcast ds_read per two values,
// ~100 cycles of deterministic latency, in-order returns, no scalar registers.
//
// Measured (MI355X, 1024^2, dynamic phonons; NE = 32 / 40 / 50 with TB = 16 / 14 / 14): 0.90 / 1.31 / 1.89 ms per call
// against 1.02 / 1.59 / 2.31 ms of the split kernels (NE = 50: 0.46 against 0.375 of the fp64 vector peak in algorithmic
// flops); 42 k VALU instructions per wave against 58 k,
// VALU busy in 69 % of the SIMD cycles.  What is left: (i) the 4 target blocks each sweep the phonon planes (loads of 8 B
// per lane from 148 planes 8 MB apart: 265 us of phase 1, and L2-miss traffic of 6.9 GB per call = 2.2 x the algorithmic
// 3.2 GB - no better than the split kernels' 6.4 GB); (ii) the ordered-pair visits (4 NE^2 instead of 3 NE^2 operations).
// Both go away only with all 50 accumulator pairs resident, which needs more than 256 registers.
#pragma once
#include "qp_collision_fast.inc"

namespace qp {

struct OnePassView {
  CollFastView base;       // kr0, ks0: row-major [NE][NE] (symmetric), rho, diag_bin, anti_bin, stash
  const double* ksd;       // [NE][NE]     ksd[k NE + i]  = ks0[i][i - k]      (phase 2)
  const double* kra2;      // [2NE-1][NE]  kra2[m NE + i] = 2 kr0[i][m - i]    (phase 2)
  int nclass;              // gap-class form (PARAM kernels): base.cls, gap_sq, kr_amp, ks_amp, pair_inv, rho[nclass][NE]
  unsigned member_blocks;  // member tables (the other kernels): blocks per ensemble member - block b stages table set
                           // b / member_blocks of kr0, ks0, rho, ksd, kra2; 0: one shared set
  int ne_live;             // TRIM kernels: the live size ne <= NE every table, bin map and plane count above belongs to
};

constexpr int kOnePassThreads = 256;

// TRIM kernels: the smallest live size the kernel of ceiling size `ne` is launched with - one above the next smaller
// instantiated size (qp_collision_padded_ceiling: 30 serves 17 ... 29, 32: 31, 40: 33 ... 39, 50: 41 ... 49).  Bins below it
// are live in every launch, so their guards fold away at compile time; the dispatcher holds the launch to the range.
__host__ __device__ constexpr int onepass_trim_min(int ne) { return ne == 30 ? 17 : ne == 32 ? 31 : ne == 40 ? 33 : ne == 50 ? 41 : ne; }

// compact (anti)diagonal-major order of the unordered pairs phase 2 visits: diagonal k >= 1 holds (i, i - k) for
// i = k .. NE-1, anti-diagonal m holds (i, m - i) for i = ceil(m / 2) .. min(m, NE-1)
__host__ __device__ constexpr int onepass_diag_start(int ne, int k) { return (k - 1) * ne - (k - 1) * k / 2; }
__host__ __device__ constexpr int onepass_anti_lo(int m) { return (m + 1) / 2; }
__host__ __device__ constexpr int onepass_anti_hi(int ne, int m) { return m < ne - 1 ? m : ne - 1; }
__host__ __device__ constexpr int onepass_anti_start(int ne, int m) {
  int s = 0;
  for (int x = 0; x < m; ++x) s += onepass_anti_hi(ne, x) - onepass_anti_lo(x) + 1;
  return s;
}

// LDS image of a phase (doubles): phase 1 [ks0 | kr0 | rho | diagonal plane offsets | anti-diagonal plane offsets],
// phase 2 [ks0_diag | kr0_anti2] + the same offsets behind them
// Gap classes (PARAM): the tables are the gap-independent amplitudes + pair_inv (CollFastView), K is formed per lane from
// the pixel's gap^2; phase 1 holds a third table (pair_inv) and rho of every class, phase 2 the four tables in the compact
// order above (40 KB at NE = 50 where padded (anti)diagonal-major images would take 120 KB).
template <int NE, bool PARAM = false>
struct OnePassLds {
  static constexpr int kPairsD = NE * (NE - 1) / 2, kPairsA = NE * (NE + 1) / 2;
  static constexpr int kKs = 0;
  static constexpr int kKr = NE * NE;
  static constexpr int kPi = 2 * NE * NE;                              // PARAM: pair_inv, row-major
  static constexpr int kRho = (PARAM ? 3 : 2) * NE * NE;               // PARAM: [kOnePassMaxClasses][NE]
  static constexpr int kOffD = kRho + (PARAM ? kOnePassMaxClasses * NE : NE + (NE & 1));   // [NE] byte offset of the plane of diagonal k
  static constexpr int kOffA = kOffD + NE + (NE & 1);                 // [2NE-1]    ... of anti-diagonal m
  static constexpr int kSize1 = kOffA + 2 * NE;
  static constexpr int kKsd = 0;
  static constexpr int kKra = PARAM ? kPairsD + (kPairsD & 1) : NE * NE;
  static constexpr int kPid = kKra + kPairsA + (kPairsA & 1);          // PARAM: pair_inv in the compact diagonal order
  static constexpr int kPia = kPid + kPairsD + (kPairsD & 1);          // PARAM: ... in the compact anti-diagonal order
  static constexpr int kOffD2 = PARAM ? kPia + kPairsA + (kPairsA & 1) : kKra + (2 * NE - 1) * NE + 1;   // kept even
  static constexpr int kOffA2 = kOffD2 + NE + (NE & 1);
  static constexpr int kSize2 = kOffA2 + 2 * NE;
  static constexpr int kSize = kSize1 > kSize2 ? kSize1 : kSize2;
  // phase-2 positions of the pair (i, i - k) / (i, m - i)
  static constexpr int diag_at(int k, int i) { return PARAM ? onepass_diag_start(NE, k) + (i - k) : k * NE + i; }
  static constexpr int anti_at(int m, int i) { return PARAM ? onepass_anti_start(NE, m) + (i - onepass_anti_lo(m)) : m * NE + i; }
};

// TRIM (padded bins, QP_ROUTE_ONEPASS_PADDED): the kernel of the ceiling size NE on ne = w.ne_live < NE live bins.  The
// caller's tables, bin maps and planes all have the live size; nothing is padded outside the kernel.
//   staging  the rows of ks0, kr0, rho, ksd, kra2 are read with stride ne (member stride ne ne, (2 ne - 1) ne) and laid into
//            the NE-strided LDS image, every other entry of the image is 0.0; the offset tables hold, for a diagonal
//            k >= ne or an anti-diagonal m > 2 ne - 2, the offset of the LAST LIVE one (diag_bin / anti_bin are not read
//            past their live extent, and a load through such an entry reads a plane that exists)
//   reads    n_i of a pad bin is loaded from plane ne - 1 (scalar min) and replaced by 0.0; with rho = 0 and K = 0 from the
//            image, q = 0 and every product a pad bin enters is an exact +0.0 added to a non-negative accumulator: the
//            sums over the live pairs keep their order and their bits.  The load streams (n planes, the Pk / Pm windows,
//            the Pq rings) stay unconditional - a guard per load would serialise them.  A pad (anti)diagonal's window value
//            is the clamped plane's, NOT zeroed: it only ever multiplies K = 0 of a pair whose target is a pad bin (the
//            partner steps j >= ne that would pair it with a live target are skipped) and that target is never stored;
//            a select at the load site would wait for the load in the step that issues it and undo the prefetch
//   skipped  target blocks with lo >= ne, partner steps j >= ne, diagonals k >= ne and anti-diagonals m > 2 ne - 2:
//            wave-uniform branches (ne is a kernel argument) around whole blocks / steps / diagonals - only where the
//            index can be a pad one, i.e. from onepass_trim_min(NE) on: everything below is the native code
//   writes   state_out planes >= ne (also of cells outside the mask), phonon planes and stash planes of pad (anti)diagonals
//            are never written: the stores sit behind the same branches
// TRIM = false compiles to what it compiled to without the flag: every addition is under a compile-time condition.
template <int NE, int TB, bool USE_S, bool USE_R, bool UPD, int PF, int WAVES, int G = 7, int G2 = 4, int PF2 = 12,
          bool PARAM = false, bool TRIM = false>
__global__ void __launch_bounds__(kOnePassThreads) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
collision_onepass_kernel(OnePassView w, const uint8_t* __restrict__ flags, long ncell, const double* __restrict__ sin_,
                         double* __restrict__ sout, double* __restrict__ ph, double dE, double dt) {
  using L = OnePassLds<NE, PARAM>;
  __shared__ double lds[L::kSize];
  const CollFastView& t = w.base;
  const long pg = (long)blockIdx.x * kOnePassThreads + threadIdx.x;
  const bool in_grid = pg < ncell;
  const unsigned p = (unsigned)(in_grid ? pg : ncell - 1);       // lanes past the end compute on the last cell, store nothing
  const bool live = in_grid && (flags[p] & QP_FLAG_ACTIVE);
  const cdtab_t ec = exp_table();
  // Member tables: all cells of a block belong to one ensemble member (the route sees to it), so the block stages that
  // member's tables and everything behind the staging loops is the kernel of a lone call - bit-equal results.  Scalar code.
  const long mb = (!PARAM && w.member_blocks) ? (long)(blockIdx.x / w.member_blocks) : 0L;
  static_assert(!(TRIM && PARAM), "gap classes are not trimmed");
  const int ne = TRIM ? w.ne_live : NE;      // live bins (wave-uniform; the constant NE unless TRIM)
  constexpr int LMIN = onepass_trim_min(NE);  // ne >= LMIN: a bin, partner or diagonal below it needs no run-time test
  constexpr int AMIN = 2 * LMIN - 2;          // ... and an anti-diagonal up to it neither

  // ---- stage the phase-1 tables ------------------------------------------------------------------------------------------
  {
    const int tid = threadIdx.x;
    if constexpr (TRIM) {      // live rows (stride ne) into the NE-strided image, zeros everywhere else
      const long mt = mb * (ne * ne);
      for (int e = tid; e < NE * NE; e += kOnePassThreads) {
        const int row = e / NE, col = e % NE;
        const bool in = row < ne && col < ne;
        if (USE_S) lds[L::kKs + e] = in ? t.ks0[mt + row * ne + col] : 0.0;
        if (USE_R) lds[L::kKr + e] = in ? t.kr0[mt + row * ne + col] : 0.0;
      }
      if (tid < NE) lds[L::kRho + tid] = tid < ne ? t.rho[mb * ne + tid] : 0.0;
    } else {
    const long mt = mb * (NE * NE);
    if (USE_S) for (int e = tid; e < NE * NE; e += kOnePassThreads) lds[L::kKs + e] = PARAM ? t.ks_amp[e] : t.ks0[mt + e];
    if (USE_R) for (int e = tid; e < NE * NE; e += kOnePassThreads) lds[L::kKr + e] = PARAM ? t.kr_amp[e] : t.kr0[mt + e];
    if (PARAM) {
      for (int e = tid; e < NE * NE; e += kOnePassThreads) lds[L::kPi + e] = t.pair_inv[e];
      for (int e = tid; e < w.nclass * NE; e += kOnePassThreads) lds[L::kRho + e] = t.rho[e];
    } else if (tid < NE) {
      lds[L::kRho + tid] = t.rho[mb * NE + tid];
    }
    }
    // byte offsets of the phonon planes as 64-bit integers in the same array (TRIM: a pad entry repeats the last live one)
    const int td = TRIM ? (tid < ne - 1 ? tid : ne - 1) : tid, ta = TRIM ? (tid < 2 * ne - 2 ? tid : 2 * ne - 2) : tid;
    if (USE_S && tid < NE) reinterpret_cast<long*>(lds)[L::kOffD + tid] = (long)bin_of(t.diag_bin[td]) * ncell * 8;
    if (USE_R && tid < 2 * NE - 1) reinterpret_cast<long*>(lds)[L::kOffA + tid] = (long)bin_of(t.anti_bin[ta]) * ncell * 8;
  }
  __syncthreads();

  double n[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int plane = (TRIM && i >= LMIN && i >= ne) ? ne - 1 : i;      // TRIM: a pad bin re-reads the last live plane
    n[i] = __builtin_nontemporal_load(&(sin_ + (long)plane * ncell)[p]);
  }
  if constexpr (TRIM) {       // pad bins: every load above read a live plane; the lane sees n = 0
#pragma unroll
    for (int i = LMIN; i < NE; ++i) n[i] = i < ne ? n[i] : 0.0;
  }
  if (in_grid && !live) {     // cells outside the mask pass through unchanged
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      if (TRIM && i >= LMIN && i >= ne) continue;      // (continue, not break: a run-time exit would keep the loop from unrolling)
      (sout + (long)i * ncell)[p] = n[i];
    }
  }
  const char* const lane_ph = reinterpret_cast<const char*>(ph + p);      // this lane's cell in plane 0
  // gap classes: the lane's row of the rho table and -gap^2 (K_s = amp max(1 - gap^2 pair_inv, 0), K_r = amp (1 + gap^2 pair_inv))
  const int cl = (PARAM && live) ? t.cls[p] : 0;
  const int rho_lane = L::kRho + cl * NE;
  const double g2 = PARAM ? t.gap_sq[cl] : 0.0, ng2 = -g2;
#define QP_LDS_D(idx) (lds[(idx)])
#define QP_RHO(j) (PARAM ? lds[rho_lane + (j)] : lds[L::kRho + (j)])
#define QP_PLANE_LOAD(off_index) \
  (*reinterpret_cast<const double*>(lane_ph + reinterpret_cast<const long*>(lds)[(off_index)]))

  if (live) {
  // ---- phase 1: quasiparticle gain / loss, one target block at a time, partner-major ----------------------------------
  constexpr int NB = (NE + TB - 1) / TB;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int lo = b * TB, hi = lo + TB < NE ? lo + TB : NE;
    if (TRIM && lo >= LMIN && lo >= ne) continue;   // the block holds pad bins only
    double ga[TB], la[TB];
#pragma unroll
    for (int x = 0; x < TB; ++x) { ga[x] = 0.0; la[x] = 0.0; }
    if (USE_S) {
      double Pk[NE];      // Pk[k]: live only while diagonal k is inside the sliding window (registers by liveness)
      // Window of live diagonals.  Partner j meets the block along k in [lo - j, hi - 1 - j] (targets above it) and
      // [j - hi + 1, j - lo] (targets below it).  A diagonal is loaded PF partners before its first use: all of
      // [max(lo, 1), hi) up front, then per partner step at most one diagonal on each side - lo - j' while the partner is
      // still below the block, j' - lo once it has passed the block's middle (before that, j' - lo is still live from the
      // other side: the two stretches of a small k touch).
#pragma unroll
      for (int k = (lo > 1 ? lo : 1); k < hi; ++k) Pk[k] = QP_PLANE_LOAD(L::kOffD + k);
#pragma unroll
      for (int j = -PF; j < NE; ++j) {
        {
          const int jn = j + PF;      // the partner PF steps ahead
          if (jn >= 1 && jn < NE) {
            if (jn < lo && lo - jn < NE) Pk[lo - jn] = QP_PLANE_LOAD(L::kOffD + lo - jn);
            if (jn > lo && jn - lo < NE && 2 * jn > hi + lo) Pk[jn - lo] = QP_PLANE_LOAD(L::kOffD + jn - lo);
          }
        }
        if (j < 0) continue;
        if (TRIM && j >= LMIN && j >= ne) continue;  // pad partners: zero contributions (the window loads above stay unconditional)
        const double nj = n[j];
        const double qj = fmax(QP_RHO(j) - nj, 0.0);
        // G targets at a time: their K P products, then their K (1 + P) sums, then the four updates of each - three
        // groups of independent instructions instead of a dependent chain per target
#pragma unroll
        for (int x0 = 0; x0 < TB; x0 += G) {
          double K[G], t1[G], t2[G];
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi || i == j) continue;
            K[g] = QP_LDS_D(L::kKs + j * NE + i);
            if (PARAM) t2[g] = fma(ng2, QP_LDS_D(L::kPi + j * NE + i), 1.0);
            else t1[g] = K[g] * Pk[i > j ? i - j : j - i];
          }
          if (PARAM) {      // (no pin between the fma and the max: a pinned value is re-canonicalised, one more instruction)
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const int x = x0 + g, i = lo + x;
              if (x >= TB || i >= hi || i == j) continue;
              t2[g] = fmax(t2[g], 0.0);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const int x = x0 + g, i = lo + x;
              if (x >= TB || i >= hi || i == j) continue;
              K[g] *= t2[g];
              asm volatile("" : "+v"(K[g]));
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const int x = x0 + g, i = lo + x;
              if (x >= TB || i >= hi || i == j) continue;
              t1[g] = K[g] * Pk[i > j ? i - j : j - i];
            }
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi || i == j) continue;
            asm volatile("" : "+v"(t1[g]));
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi || i == j) continue;
            t2[g] = t1[g] + K[g];
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi || i == j) continue;
            asm volatile("" : "+v"(t2[g]));
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi || i == j) continue;
            if (i > j) {                // (i -> j) emits
              ga[x] = fma(t1[g], nj, ga[x]);
              la[x] = fma(t2[g], qj, la[x]);
            } else {                    // (j -> i) emits into this bin
              ga[x] = fma(t2[g], nj, ga[x]);
              la[x] = fma(t1[g], qj, la[x]);
            }
          }
          if (PARAM) __builtin_amdgcn_sched_barrier(0);      // keeps the table reads of the next group behind this one
        }
        pin_array(ga);
        pin_array(la);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (USE_R) {
      if (USE_S) {
#pragma unroll
        for (int x = 0; x < TB; ++x) { ga[x] *= 0.5; la[x] *= 0.5; }
      }
      double Pm[2 * NE - 1];
      // partner j meets the block along the anti-diagonals [lo + j, hi - 1 + j]: one new one per partner step
#pragma unroll
      for (int m = lo; m < hi; ++m) Pm[m] = QP_PLANE_LOAD(L::kOffA + m);
#pragma unroll
      for (int j = -PF; j < NE; ++j) {
        {
          const int jn = j + PF;
          if (jn >= 1 && jn < NE) Pm[hi - 1 + jn] = QP_PLANE_LOAD(L::kOffA + hi - 1 + jn);
        }
        if (j < 0) continue;
        if (TRIM && j >= LMIN && j >= ne) continue;  // pad partners: zero contributions (the window loads above stay unconditional)
        const double nj = n[j];
        const double qj = fmax(QP_RHO(j) - nj, 0.0);
#pragma unroll
        for (int x0 = 0; x0 < TB; x0 += G) {
          double K[G], t1[G], t2[G];
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi) continue;
            K[g] = QP_LDS_D(L::kKr + j * NE + i);
            if (PARAM) t2[g] = fma(g2, QP_LDS_D(L::kPi + j * NE + i), 1.0);
            else t1[g] = K[g] * Pm[i + j];
          }
          if (PARAM) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const int x = x0 + g, i = lo + x;
              if (x >= TB || i >= hi) continue;
              asm volatile("" : "+v"(t2[g]));
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const int x = x0 + g, i = lo + x;
              if (x >= TB || i >= hi) continue;
              K[g] *= t2[g];
              asm volatile("" : "+v"(K[g]));
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
              const int x = x0 + g, i = lo + x;
              if (x >= TB || i >= hi) continue;
              t1[g] = K[g] * Pm[i + j];
            }
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi) continue;
            asm volatile("" : "+v"(t1[g]));
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi) continue;
            t2[g] = t1[g] + K[g];
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi) continue;
            asm volatile("" : "+v"(t2[g]));
          }
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const int x = x0 + g, i = lo + x;
            if (x >= TB || i >= hi) continue;
            la[x] = fma(t2[g], nj, la[x]);
            ga[x] = fma(t1[g], qj, ga[x]);
          }
          if (PARAM) __builtin_amdgcn_sched_barrier(0);
        }
        pin_array(ga);
        pin_array(la);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const double scale = USE_R ? 2.0 * dE : dE;
#pragma unroll
    for (int x = 0; x < TB; ++x) {
      const int i = lo + x;
      if (i >= hi) continue;
      if (TRIM && i >= LMIN && i >= ne) continue;    // pad targets are not stored
      const double qi = fmax(QP_RHO(i) - n[i], 0.0);
      __builtin_nontemporal_store(relax_update_f<false>(n[i], scale * qi * ga[x], scale * la[x], dt, ec),
                                  &(sout + (long)i * ncell)[p]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  }

  // ---- phase 2: phonon bins from the old n and q = max(rho - n, 0) -----------------------------------------------------
  if (UPD) {
    double q[NE];
    if (live) {
#pragma unroll
      for (int i = 0; i < NE; ++i) q[i] = fmax(QP_RHO(i) - n[i], 0.0);
    }
    __syncthreads();          // every wave is done with the phase-1 image
    {
      const int tid = threadIdx.x;
      if (PARAM) {      // gathered from the row-major amplitude tables into the compact (anti)diagonal order
        if (USE_S)
          for (int e = tid; e < NE * NE; e += kOnePassThreads) {
            const int k = e / NE, i = e % NE;
            if (k >= 1 && i >= k) {
              lds[L::kKsd + onepass_diag_start(NE, k) + (i - k)] = t.ks_amp[i * NE + (i - k)];
              lds[L::kPid + onepass_diag_start(NE, k) + (i - k)] = t.pair_inv[i * NE + (i - k)];
            }
          }
        if (USE_R)
          for (int e = tid; e < (2 * NE - 1) * NE; e += kOnePassThreads) {
            const int m = e / NE, i = e % NE;
            if (i >= onepass_anti_lo(m) && i <= onepass_anti_hi(NE, m)) {
              const int at = onepass_anti_start(NE, m) + (i - onepass_anti_lo(m));
              lds[L::kKra + at] = 2.0 * t.kr_amp[i * NE + (m - i)];
              lds[L::kPia + at] = t.pair_inv[i * NE + (m - i)];
            }
          }
      } else if constexpr (TRIM) {      // the live [ne][ne] / [2 ne - 1][ne] images into the NE-strided ones, zeros elsewhere
        if (USE_S)
          for (int e = tid; e < NE * NE; e += kOnePassThreads) {
            const int k = e / NE, i = e % NE;
            lds[L::kKsd + e] = (k < ne && i < ne) ? w.ksd[mb * (ne * ne) + k * ne + i] : 0.0;
          }
        if (USE_R)
          for (int e = tid; e < (2 * NE - 1) * NE; e += kOnePassThreads) {
            const int m = e / NE, i = e % NE;
            lds[L::kKra + e] = (m < 2 * ne - 1 && i < ne) ? w.kra2[mb * ((2 * ne - 1) * ne) + m * ne + i] : 0.0;
          }
      } else {
        if (USE_S) for (int e = tid; e < NE * NE; e += kOnePassThreads) lds[L::kKsd + e] = w.ksd[mb * (NE * NE) + e];
        if (USE_R)
          for (int e = tid; e < (2 * NE - 1) * NE; e += kOnePassThreads) lds[L::kKra + e] = w.kra2[mb * ((2 * NE - 1) * NE) + e];
      }
      const int td = TRIM ? (tid < ne - 1 ? tid : ne - 1) : tid, ta = TRIM ? (tid < 2 * ne - 2 ? tid : 2 * ne - 2) : tid;
      if (USE_S && tid < NE) reinterpret_cast<long*>(lds)[L::kOffD2 + tid] = (long)bin_of(t.diag_bin[td]) * ncell * 8;
      if (USE_R && tid < 2 * NE - 1) reinterpret_cast<long*>(lds)[L::kOffA2 + tid] = (long)bin_of(t.anti_bin[ta]) * ncell * 8;
    }
    __syncthreads();
    if (live) {
    const citab_t dbin = uniform_const<citab_t>(t.diag_bin);
    const citab_t abin = uniform_const<citab_t>(t.anti_bin);
#define QP_PLANE_PTR(off_index) \
  reinterpret_cast<double*>(const_cast<char*>(lane_ph) + reinterpret_cast<const long*>(lds)[(off_index)])
    if (USE_S) {
      double Pq[PF2];
#pragma unroll
      for (int k = 1; k <= PF2 && k < NE; ++k) Pq[k % PF2] = __builtin_nontemporal_load(QP_PLANE_PTR(L::kOffD2 + k));
#pragma unroll
      for (int k = 1; k < NE; ++k) {
        const double P = Pq[k % PF2];
        if (k + PF2 < NE) Pq[k % PF2] = __builtin_nontemporal_load(QP_PLANE_PTR(L::kOffD2 + k + PF2));
        if (TRIM && k >= LMIN && k >= ne) continue;  // pad diagonals: no pair, no plane, no stash slot (the ring above stays unconditional)
        const int entry = dbin[k];
        // G2 pairs at a time: their products first (independent instructions), then the sums - in the order of the
        // reference's bincount (ascending i): em - ab cancels to ~1e-5 of em near detailed balance, and (e^x - 1) / x
        // carries that amplification into the phonon planes; partial accumulators (another summation order) moved them
        // by 1.4e-10 against the oracle
        double em = 0.0, ab = 0.0;
#pragma unroll
        for (int j0 = 0; j0 + k < NE; j0 += G2) {
          double a[G2], c[G2];
#pragma unroll
          for (int g = 0; g < G2; ++g) {
            const int j = j0 + g, i = j + k;
            if (i >= NE) continue;
            double K = QP_LDS_D(L::kKsd + L::diag_at(k, i));
            if (PARAM) K *= fmax(fma(ng2, QP_LDS_D(L::kPid + L::diag_at(k, i)), 1.0), 0.0);
            a[g] = n[i] * K;
            c[g] = n[j] * K;
          }
#pragma unroll
          for (int g = 0; g < G2; ++g) {
            if (j0 + g + k >= NE) continue;
            asm volatile("" : "+v"(a[g]), "+v"(c[g]));
          }
#pragma unroll
          for (int g = 0; g < G2; ++g) {
            const int j = j0 + g, i = j + k;
            if (i >= NE) continue;
            em = fma(a[g], q[j], em);
            ab = fma(c[g], q[i], ab);
          }
        }
        if (USE_R && slot_of(entry) >= 0) {     // merged bin (wave-uniform): finalised by its anti-diagonal
          (t.stash + (long)(2 * slot_of(entry)) * ncell)[p] = em;
          (t.stash + (long)(2 * slot_of(entry) + 1) * ncell)[p] = ab;
        } else {
          __builtin_nontemporal_store(affine_update_f<false>(P, dE * em, dE * (em - ab), dt, ec), QP_PLANE_PTR(L::kOffD2 + k));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (USE_R) {
      double Pq[PF2];
#pragma unroll
      for (int m = 0; m < PF2 && m < 2 * NE - 1; ++m) Pq[m % PF2] = __builtin_nontemporal_load(QP_PLANE_PTR(L::kOffA2 + m));
#pragma unroll
      for (int m = 0; m < 2 * NE - 1; ++m) {
        const double P = Pq[m % PF2];
        if (m + PF2 < 2 * NE - 1) Pq[m % PF2] = __builtin_nontemporal_load(QP_PLANE_PTR(L::kOffA2 + m + PF2));
        if (TRIM && m > AMIN && m > 2 * ne - 2) continue;
        const int entry = abin[m];
        double rec = 0.0, pb = 0.0;
        // the pairs (i, j = m - i) with j <= i: i from ceil(m / 2) up to min(m, NE - 1)
        const int i_lo = (m + 1) / 2, i_hi = m < NE - 1 ? m : NE - 1;
#pragma unroll
        for (int i0 = i_lo; i0 <= i_hi; i0 += G2) {
          double a[G2], c[G2];
#pragma unroll
          for (int g = 0; g < G2; ++g) {
            const int i = i0 + g, j = m - i;
            if (i > i_hi) continue;
            // the table holds 2 K, the weight of an unordered pair i != j; the diagonal pair counts once
            double K2 = (i != j ? 1.0 : 0.5) * QP_LDS_D(L::kKra + L::anti_at(m, i));
            if (PARAM) K2 *= fma(g2, QP_LDS_D(L::kPia + L::anti_at(m, i)), 1.0);
            a[g] = n[i] * K2;
            c[g] = q[i] * K2;
          }
#pragma unroll
          for (int g = 0; g < G2; ++g) {
            if (i0 + g > i_hi) continue;
            asm volatile("" : "+v"(a[g]), "+v"(c[g]));
          }
#pragma unroll
          for (int g = 0; g < G2; ++g) {
            const int i = i0 + g, j = m - i;
            if (i > i_hi) continue;
            rec = fma(a[g], n[j], rec);
            pb = fma(c[g], q[j], pb);
          }
        }
        double a = dE * rec, bb = dE * (rec - pb);
        if (USE_S && slot_of(entry) >= 0) {     // merged bin: add the sums its diagonal parked
          const double em = (t.stash + (long)(2 * slot_of(entry)) * ncell)[p];
          const double ab = (t.stash + (long)(2 * slot_of(entry) + 1) * ncell)[p];
          a = dE * (em + rec);
          bb = dE * ((em - ab) + (rec - pb));
        }
        __builtin_nontemporal_store(affine_update_f<false>(P, a, bb, dt, ec), QP_PLANE_PTR(L::kOffA2 + m));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#undef QP_PLANE_PTR
    }
  }
#undef QP_PLANE_LOAD
#undef QP_RHO
#undef QP_LDS_D
}

// the launcher families of the one-pass kernel (qp_collision_dispatch.h).  One gap class: both phonon modes in one unit.
template <int NE, bool S, bool R, int TB, int PF, int WAVES>
static void launch_onepass(const OnePassView& v, const CollCall& c) {
  const unsigned blocks = (unsigned)((c.ncell + kOnePassThreads - 1) / kOnePassThreads);
  if (c.u)
    hipLaunchKernelGGL((collision_onepass_kernel<NE, TB, S, R, true, PF, WAVES>), dim3(blocks), dim3(kOnePassThreads), 0,
                       c.stream, v, c.flags, c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt);
  else
    hipLaunchKernelGGL((collision_onepass_kernel<NE, TB, S, R, false, PF, WAVES>), dim3(blocks), dim3(kOnePassThreads), 0,
                       c.stream, v, c.flags, c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt);
}
// Padded bins: the kernel of the ceiling size NE with TRIM, the live size in OnePassView::ne_live
typedef OnePassView view_onepasst;
// (the ceiling's tiling; at NE = 50 with both processes the native kernel sits at exactly 256 registers and the guards' few
// extra live values spilled 6 of them: its phase-2 prefetch ring is 10 deep instead of 12 - 253 registers, no scratch)
template <int NE, bool S, bool R, int TB, int PF, int WAVES>
static void launch_onepasst(const OnePassView& v, const CollCall& c) {
  const unsigned blocks = (unsigned)((c.ncell + kOnePassThreads - 1) / kOnePassThreads);
  constexpr int PF2 = (NE == 50 && S && R) ? 10 : 12;
  if (c.u)
    hipLaunchKernelGGL((collision_onepass_kernel<NE, TB, S, R, true, PF, WAVES, 7, 4, PF2, false, true>), dim3(blocks),
                       dim3(kOnePassThreads), 0, c.stream, v, c.flags, c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt);
  else
    hipLaunchKernelGGL((collision_onepass_kernel<NE, TB, S, R, false, PF, WAVES, 7, 4, 12, false, true>), dim3(blocks),
                       dim3(kOnePassThreads), 0, c.stream, v, c.flags, c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt);
}
// Gap-class form: one kernel per unit (each takes ~4 minutes to compile), so frozen (u0) and dynamic (u1) phonons are
// families of their own and the dispatcher chooses between them.
template <int NE, bool S, bool R, bool U, int TB, int PF, int WAVES, int G, int G2, int PF2>
static void launch_onepassc(const OnePassView& v, const CollCall& c) {
  const unsigned blocks = (unsigned)((c.ncell + kOnePassThreads - 1) / kOnePassThreads);
  hipLaunchKernelGGL((collision_onepass_kernel<NE, TB, S, R, U, PF, WAVES, G, G2, PF2, true>), dim3(blocks),
                     dim3(kOnePassThreads), 0, c.stream, v, c.flags, c.ncell, c.sin, c.sout, c.ph, c.dE, c.dt);
}
template <int NE, bool S, bool R, int... TILING>
static void launch_onepassc_u0(const OnePassView& v, const CollCall& c) { launch_onepassc<NE, S, R, false, TILING...>(v, c); }
template <int NE, bool S, bool R, int... TILING>
static void launch_onepassc_u1(const OnePassView& v, const CollCall& c) { launch_onepassc<NE, S, R, true, TILING...>(v, c); }

}  // namespace qp
