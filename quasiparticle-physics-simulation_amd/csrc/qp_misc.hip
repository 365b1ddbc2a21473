// Small elementwise / reduction kernels of the time loop: external generation, Pauli guard statistics,
// energy integrals, max-norm.
#include "qp_common.h"

namespace qp {

__global__ void __launch_bounds__(256) add_constant_kernel(const uint8_t* __restrict__ flags, long ncell,
                                                           int nfield, double* __restrict__ s, double amount) {
  const long total = ncell * nfield;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long p = t % ncell;
    if (flags[p] & QP_FLAG_ACTIVE) s[t] += amount;
  }
}

// out[f][p] = inside the mask ? scale * in[f][p] : NaN  (frames as the reference returns them, reconstruct_field)
__global__ void __launch_bounds__(256) nan_pad_kernel(const uint8_t* __restrict__ flags, long ncell, int nfield,
                                                      const double* __restrict__ in, double scale,
                                                      double* __restrict__ out) {
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < ncell; p += (long)gridDim.x * blockDim.x) {
    const bool on = flags[p] & QP_FLAG_ACTIVE;
    for (int f = 0; f < nfield; ++f) out[(long)f * ncell + p] = on ? scale * in[(long)f * ncell + p] : qnan;
  }
}

__global__ void __launch_bounds__(256) add_scaled_kernel(long n, double* __restrict__ s,
                                                         const double* __restrict__ g, double scale) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x)
    s[t] += scale * g[t];
}

__global__ void __launch_bounds__(256) energy_integrate_kernel(const double* __restrict__ s, int ne, long ncell,
                                                               double dE, double* __restrict__ out) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < ncell; p += (long)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int i = 0; i < ne; ++i) acc += s[(long)i * ncell + p];
    out[p] = acc * dE;
  }
}

__global__ void __launch_bounds__(256) weighted_sum_kernel(const double* __restrict__ s,
                                                           const double* __restrict__ w, int n, long ncell,
                                                           double* __restrict__ out) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < ncell; p += (long)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += s[(long)i * ncell + p] * w[i];
    out[p] = acc;
  }
}

// ---- reductions: per-block partials in workspace, finished by a single-block kernel -----------------------
constexpr int kRedBlocks = 1024;

// np.argmax order (solver.py:993): a NaN occupation is the maximum and the first NaN in C order wins; otherwise the
// largest value, the smallest linear index on ties
__device__ __forceinline__ bool pauli_better(double of, long ofi, double f, long fi) {
  const bool on = of != of, fn = f != f;
  if (on || fn) return on && (!fn || ofi < fi);
  return of > f || (of == f && ofi < fi);
}

__device__ __forceinline__ void pauli_merge(double& f, long& fi, long& forb, double of, long ofi, long oforb) {
  if (pauli_better(of, ofi, f, fi)) { f = of; fi = ofi; }
  if (oforb >= 0 && (forb < 0 || oforb < forb)) forb = oforb;
}

__device__ void pauli_block_reduce(double f, long fi, long forb, PauliPartial* dst) {
  __shared__ double sf[256];
  __shared__ long si[256];
  __shared__ long sb[256];
  const int t = threadIdx.x;
  sf[t] = f; si[t] = fi; sb[t] = forb;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) pauli_merge(sf[t], si[t], sb[t], sf[t + s], si[t + s], sb[t + s]);
    __syncthreads();
  }
  if (t == 0) { dst->maxf = sf[0]; dst->maxidx = si[0]; dst->forb = sb[0]; }
}

__global__ void __launch_bounds__(256) pauli_partial_kernel(const double* __restrict__ s,
                                                            const double* __restrict__ rho,
                                                            const int32_t* __restrict__ cls,
                                                            const uint8_t* __restrict__ flags, int ne, long ncell,
                                                            double floor_, PauliPartial* part) {
  // f defaults to 0 where rho <= 1e-30 (np.divide(..., where=rho_mask) into zeros, solver.py:987-992);
  // np.argmax returns the first maximum in C order, so ties resolve to the smallest linear index.
  double f = -__builtin_huge_val();
  long fi = 0x7fffffffffffffffL, forb = -1;
  // blockIdx.y strides over energy bins, blockIdx.x over cells: no 64-bit div / mod per element.  Four independent
  // cells per trip so that four loads are in flight per thread (the loop is latency-bound otherwise: ~1.9 TB/s).
  const long stride = (long)gridDim.x * blockDim.x;
  for (int i = blockIdx.y; i < ne; i += gridDim.y) {
    const double* si = s + (long)i * ncell;
    const double r0 = rho[i];
    for (long p0 = (long)blockIdx.x * blockDim.x + threadIdx.x; p0 < ncell; p0 += 4 * stride) {
      double nv[4];
      unsigned fl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long p = p0 + u * stride;
        const bool in = p < ncell;
        fl[u] = in ? flags[p] : 0u;
        nv[u] = in ? si[p] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!(fl[u] & QP_FLAG_ACTIVE)) continue;
        const long p = p0 + u * stride;
        const double r = cls ? rho[(long)cls[p] * ne + i] : r0;
        const double n = nv[u];
        const long t = (long)i * ncell + p;
        double occ = 0.0;
        if (r > 1e-30) occ = n / fmax(r, 1e-30);
        else if (n > floor_ && (forb < 0 || t < forb)) forb = t;
        if (pauli_better(occ, t, f, fi)) { f = occ; fi = t; }
      }
    }
  }
  pauli_block_reduce(f, fi, forb, part + (long)blockIdx.y * gridDim.x + blockIdx.x);
}

__global__ void __launch_bounds__(256) pauli_final_kernel(const PauliPartial* part, int nparts, double* out_vals,
                                                          long* out_idx) {
  double f = -__builtin_huge_val();
  long fi = 0x7fffffffffffffffL, forb = -1;
  for (int k = threadIdx.x; k < nparts; k += blockDim.x) pauli_merge(f, fi, forb, part[k].maxf, part[k].maxidx, part[k].forb);
  __shared__ PauliPartial res;
  pauli_block_reduce(f, fi, forb, &res);
  __syncthreads();
  if (threadIdx.x == 0) { out_vals[0] = res.maxf; out_idx[0] = res.maxidx; out_idx[1] = res.forb; }
}

// middle stage for the per-wave partials of the fused guard (collision kernels): block b reduces its contiguous share
__global__ void __launch_bounds__(256) pauli_merge_kernel(const PauliPartial* part, long nparts, PauliPartial* out) {
  double f = -__builtin_huge_val();
  long fi = 0x7fffffffffffffffL, forb = -1;
  const long per = (nparts + gridDim.x - 1) / gridDim.x;
  const long lo = (long)blockIdx.x * per, hi = lo + per < nparts ? lo + per : nparts;
  for (long k = lo + threadIdx.x; k < hi; k += blockDim.x) pauli_merge(f, fi, forb, part[k].maxf, part[k].maxidx, part[k].forb);
  pauli_block_reduce(f, fi, forb, out + blockIdx.x);
}

void pauli_finish(const PauliPartial* parts, long nparts, PauliPartial* scratch, double* out_vals, long* out_idx,
                  hipStream_t stream) {
  hipLaunchKernelGGL(pauli_merge_kernel, dim3(kGuardMergeBlocks), dim3(256), 0, stream, parts, nparts, scratch);
  hipLaunchKernelGGL(pauli_final_kernel, dim3(1), dim3(256), 0, stream, (const PauliPartial*)scratch, kGuardMergeBlocks,
                     out_vals, out_idx);
}

// ---- per-member Pauli guard (ensembles: state[ne][members * ncm], member m owns cells [m * ncm, (m + 1) * ncm)) --------
// Blocks never straddle two members: block x = m * bxm + b covers member m only.  Indices are formed member-local
// (ie * ncm + c) from the start, so the merge order equals member m's own C order and pauli_better picks the winner of
// qp_pauli_stats on that slice alone.
__global__ void __launch_bounds__(256) pauli_members_partial_kernel(const double* __restrict__ s,
                                                                    const double* __restrict__ rho,
                                                                    const int32_t* __restrict__ cls,
                                                                    const uint8_t* __restrict__ flags, int ne, long ncm,
                                                                    long members, int bxm, double floor_,
                                                                    PauliPartial* part) {
  const long m = blockIdx.x / bxm;
  const int b = blockIdx.x % bxm;
  const long ncell = ncm * members;
  double f = -__builtin_huge_val();
  long fi = 0x7fffffffffffffffL, forb = -1;
  const long stride = (long)bxm * blockDim.x;
  for (int i = blockIdx.y; i < ne; i += gridDim.y) {
    const double* si = s + (long)i * ncell + m * ncm;
    const uint8_t* fm = flags + m * ncm;
    const int32_t* cm = cls ? cls + m * ncm : nullptr;
    const double r0 = rho[i];
    for (long c = (long)b * blockDim.x + threadIdx.x; c < ncm; c += stride) {
      if (!(fm[c] & QP_FLAG_ACTIVE)) continue;
      const double r = cm ? rho[(long)cm[c] * ne + i] : r0;
      const double n = si[c];
      const long t = (long)i * ncm + c;
      double occ = 0.0;
      if (r > 1e-30) occ = n / fmax(r, 1e-30);
      else if (n > floor_ && (forb < 0 || t < forb)) forb = t;
      if (pauli_better(occ, t, f, fi)) { f = occ; fi = t; }
    }
  }
  pauli_block_reduce(f, fi, forb, part + (m * gridDim.y + blockIdx.y) * bxm + b);
}

// block m merges member m's `per` contiguous partials; `wave_ncell` > 0: the partials are the per-wave ones of the fused
// guard (global indices ie * ncell + p, converted here to member-local ie * ncm + c)
__global__ void __launch_bounds__(256) pauli_members_final_kernel(const PauliPartial* part, long per, long ncm,
                                                                  long wave_ncell, double* out_vals, long* out_idx) {
  const long m = blockIdx.x;
  double f = -__builtin_huge_val();
  long fi = 0x7fffffffffffffffL, forb = -1;
  for (long k = m * per + threadIdx.x; k < (m + 1) * per; k += blockDim.x)
    pauli_merge(f, fi, forb, part[k].maxf, part[k].maxidx, part[k].forb);
  __shared__ PauliPartial res;
  pauli_block_reduce(f, fi, forb, &res);
  __syncthreads();
  if (threadIdx.x == 0) {
    long mi = res.maxidx, fb = res.forb;
    if (wave_ncell > 0) {      // global linear index -> member-local (the pixel lies in member m by construction)
      if (mi >= 0 && mi != 0x7fffffffffffffffL) mi = (mi / wave_ncell) * ncm + (mi % wave_ncell - m * ncm);
      if (fb >= 0) fb = (fb / wave_ncell) * ncm + (fb % wave_ncell - m * ncm);
    }
    out_vals[m] = res.maxf;
    out_idx[2 * m] = mi;
    out_idx[2 * m + 1] = fb;
  }
}

void pauli_finish_members(const PauliPartial* parts, long ncell_member, long members, double* out_vals, long* out_idx,
                          hipStream_t stream) {
  hipLaunchKernelGGL(pauli_members_final_kernel, dim3((unsigned)members), dim3(256), 0, stream, parts, ncell_member / 64,
                     ncell_member, ncell_member * members, out_vals, out_idx);
}

// blocks per member of the standalone pass: ~2048 blocks in all, at most kRedBlocks per member
static inline long pauli_member_budget(long members) {
  long b = 2048 / (members > 0 ? members : 1);
  return b < 1 ? 1 : (b > kRedBlocks ? kRedBlocks : b);
}

__global__ void __launch_bounds__(256) add_constant_members_kernel(const uint8_t* __restrict__ flags, long ncm, long members,
                                                                   int nfield, double* __restrict__ s,
                                                                   const double* __restrict__ amounts) {
  const long ncell = ncm * members;
  const long total = ncell * nfield;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long p = t % ncell;
    if (flags[p] & QP_FLAG_ACTIVE) s[t] += amounts[p / ncm];
  }
}

// ---- region sums (time traces): out[m][r][f] = sum over the cells c of member m with bit r of bits[c] set of s[f][m][c] ----
// Stage 1: block (chunk, m, f) reduces cells [chunk * kRegionChunk, ...) of plane (f, m) to `nregion` partials.  Stage 2:
// block (m, f) adds the chunk partials of its plane in index order.  Which thread adds which cell, the shuffle tree, the
// order of the four wave sums and the order of the chunks depend on the sizes alone, so a result is reproducible bit for
// bit; nothing is accumulated across blocks in memory (no atomics, no completion counters).
constexpr int kRegionChunk = 8192;   // cells of one plane per stage-1 block: 16 pairs per thread, two rounds of 8 loads
constexpr int kRegionTile = 512;     // chunk partials (x nregion) that stage 2 holds in LDS per round

// A plane starts at element (f * members + m) * ncm of `s`: with an odd ncm every second plane starts on an odd element.
// The pairs of a chunk therefore start at its first EVEN element (one scalar head cell before them, at most one tail cell
// after them): 16-byte loads when `s` itself is 16-byte aligned (VEC), else the same pairs from two 8-byte loads - the
// additions and their order are the same either way.  NR = nregion rounded up to 1, 2, 4, 8.
template <int NR, bool VEC>
__global__ void __launch_bounds__(256) region_partial_kernel(const double* __restrict__ s, const uint8_t* __restrict__ bits,
                                                             long ncm, long members, int nregion, long nchunk,
                                                             double* __restrict__ part) {
  const long chunk = blockIdx.x, m = blockIdx.y, f = blockIdx.z;
  const long plane = f * members + m;
  const long c0 = chunk * kRegionChunk;
  const long left = ncm - c0;
  const int n = (int)(left < kRegionChunk ? left : kRegionChunk);      // 1 ... kRegionChunk cells
  const long e0 = plane * ncm + c0;
  const int head = (int)(e0 & 1);                                       // n >= 1, so head <= n
  const int npair = (n - head) >> 1;
  const int tail = n - head - 2 * npair;
  const double* p = s + e0 + head;
  const uint8_t* b = bits + c0 + head;
  double acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.0;
  auto add = [&](double v, unsigned bb) {
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] += ((bb >> r) & 1u) ? v : 0.0;
  };
  for (int i0 = threadIdx.x; i0 < npair; i0 += 8 * 256) {
    double2 v[8];
    unsigned bb[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * 256;
      const bool in = i < npair;
      if (VEC) v[u] = in ? reinterpret_cast<const double2*>(p)[i] : make_double2(0.0, 0.0);
      else v[u] = in ? make_double2(p[2 * i], p[2 * i + 1]) : make_double2(0.0, 0.0);
      bb[u] = in ? ((unsigned)b[2 * i] | ((unsigned)b[2 * i + 1] << 8)) : 0u;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      add(v[u].x, bb[u]);
      add(v[u].y, bb[u] >> 8);
    }
  }
  if (threadIdx.x == 0 && head) add(s[e0], bits[c0]);
  if (threadIdx.x == 1 && tail) add(s[e0 + n - 1], bits[c0 + n - 1]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] += __shfl_down(acc[r], off, 64);
  }
  __shared__ double sm[4][NR];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int r = 0; r < NR; ++r) sm[threadIdx.x >> 6][r] = acc[r];
  }
  __syncthreads();
  if ((int)threadIdx.x < nregion) {
    const int r = threadIdx.x;
    part[(plane * nchunk + chunk) * nregion + r] = ((sm[0][r] + sm[1][r]) + sm[2][r]) + sm[3][r];
  }
}

__global__ void __launch_bounds__(64) region_final_kernel(const double* __restrict__ part, long nchunk, int nregion,
                                                          long members, int nfield, double* __restrict__ out) {
  __shared__ double tile[kRegionTile * 8];
  const long m = blockIdx.x, f = blockIdx.y;
  const double* src = part + (f * members + m) * nchunk * nregion;
  double acc = 0.0;
  for (long k0 = 0; k0 < nchunk; k0 += kRegionTile) {
    const int nk = (int)(nchunk - k0 < kRegionTile ? nchunk - k0 : kRegionTile);
    for (int t = threadIdx.x; t < nk * nregion; t += 64) tile[t] = src[k0 * nregion + t];
    __syncthreads();
    if ((int)threadIdx.x < nregion)
      for (int k = 0; k < nk; ++k) acc += tile[k * nregion + threadIdx.x];
    __syncthreads();
  }
  if ((int)threadIdx.x < nregion) out[(m * nregion + threadIdx.x) * nfield + f] = acc;
}

static inline long region_chunks(long ncm) { return (ncm + kRegionChunk - 1) / kRegionChunk; }

template <int NR>
static void region_partial_launch(bool vec, dim3 grid, hipStream_t stream, const double* s, const uint8_t* bits, long ncm,
                                  long members, int nregion, long nchunk, double* part) {
  if (vec)
    hipLaunchKernelGGL((region_partial_kernel<NR, true>), grid, dim3(256), 0, stream, s, bits, ncm, members, nregion, nchunk,
                       part);
  else
    hipLaunchKernelGGL((region_partial_kernel<NR, false>), grid, dim3(256), 0, stream, s, bits, ncm, members, nregion, nchunk,
                       part);
}

// ---- block sums (coarse frames): out[m][f][cy][cx] = sum of s[f][m][j][i] over the active cells of one B x B block ----
// Blocks are aligned to the origin of the full frame; device cell (0, 0) sits at (oy, ox) inside its block, so frame row
// g = oy + j and frame column h = ox + i.  A wave owns frame columns [64 seg, 64 seg + 64) (lane <-> column, 8-byte loads:
// one 512-byte segment per row) and the kBlockRows = max(B, 16) frame rows of one row group, i.e. 64 / B blocks across and
// kBlockRows / B blocks down.  Each lane adds its column over the B rows of a block row top to bottom, starting from +0.0,
// with the 16 loads of a round issued before the first add; an xor butterfly over the aligned group of B lanes then leaves
// the block sum in every lane of the group, and the group's first lane stores it.  A cell enters through a select; a lane
// outside the device grid loads the nearest cell of the plane instead (so that no load sits behind a branch) and counts +0.0.  Which lane adds which cell depends on (ny, nx, oy, ox, B)
// alone - not on the plane - and every output has exactly one writer: no LDS, no workspace, no atomics.
template <int B>
__global__ void __launch_bounds__(256) block_sums_kernel(const double* __restrict__ s, const uint8_t* __restrict__ flags,
                                                         int ny, int nx, long members, int oy, int ox, int nseg,
                                                         int ngroup, int cny, int cnx, int nfield,
                                                         double* __restrict__ out) {
  constexpr int kBlockRows = B < 16 ? 16 : B;       // frame rows of a wave
  constexpr int kDown = kBlockRows / B;             // block rows of a wave
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wave >= (long)nseg * ngroup) return;          // wave-uniform: whole waves leave
  const int seg = (int)(wave % nseg), group = (int)(wave / nseg);
  const long m = blockIdx.y, f = blockIdx.z;
  const int i = seg * 64 + lane - ox;               // device column of this lane
  const bool col_in = i >= 0 && i < nx;
  const int ic = min(max(i, 0), nx - 1);
  const int j0 = group * kBlockRows - oy;           // device row of the wave's first frame row
  const double* p = s + (f * members + m) * ((long)ny * nx);
  double acc[kDown];
#pragma unroll
  for (int d = 0; d < kDown; ++d) acc[d] = 0.0;
#pragma unroll 1
  for (int r0 = 0; r0 < kBlockRows; r0 += 16) {   // one round for B <= 16; B / 16 rounds into the one block row else
    double v[16];
    unsigned on[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int j = j0 + r0 + u;
      const bool in = col_in && j >= 0 && j < ny;
      const long c = (long)min(max(j, 0), ny - 1) * nx + ic;      // always a cell of the plane: the load needs no branch
      v[u] = p[c];
      on[u] = (unsigned)flags[c] & (in ? QP_FLAG_ACTIVE : 0u);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[kDown == 1 ? 0 : (r0 + u) / B] += on[u] ? v[u] : 0.0;
  }
#pragma unroll
  for (int d = 0; d < kDown; ++d) {
#pragma unroll
    for (int off = 1; off < B; off <<= 1) acc[d] += __shfl_xor(acc[d], off, 64);
  }
  const int cx = seg * (64 / B) + lane / B;
  if (lane % B == 0 && cx < cnx) {
    double* o = out + ((m * nfield + f) * cny) * (long)cnx + cx;
#pragma unroll
    for (int d = 0; d < kDown; ++d) {
      const int cy = group * kDown + d;
      if (cy < cny) o[(long)cy * cnx] = acc[d];
    }
  }
}

template <int B>
static void block_sums_launch(hipStream_t stream, const double* s, const uint8_t* flags, int ny, int nx, long members,
                              int nfield, int oy, int ox, double* out) {
  constexpr int kBlockRows = B < 16 ? 16 : B;
  const int cny = (oy + ny + B - 1) / B, cnx = (ox + nx + B - 1) / B;
  const int nseg = (ox + nx + 63) / 64, ngroup = (oy + ny + kBlockRows - 1) / kBlockRows;
  const long nwave = (long)nseg * ngroup;
  const dim3 grid((unsigned)((nwave + 3) / 4), (unsigned)members, (unsigned)nfield);
  hipLaunchKernelGGL((block_sums_kernel<B>), grid, dim3(256), 0, stream, s, flags, ny, nx, members, oy, ox, nseg, ngroup,
                     cny, cnx, nfield, out);
}

__global__ void __launch_bounds__(256) absmax_partial_kernel(const double* __restrict__ a, long n, double* part) {
  double m = 0.0;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
    const double v = fabs(a[t]);
    // NaN must not be lost: propagate it as +inf so a diverged iteration is visible
    m = (v != v) ? __builtin_huge_val() : fmax(m, v);
  }
  __shared__ double sm[256];
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

__global__ void __launch_bounds__(256) absmax_final_kernel(const double* part, int nparts, double* out) {
  double m = 0.0;
  for (int k = threadIdx.x; k < nparts; k += blockDim.x) m = fmax(m, part[k]);
  __shared__ double sm[256];
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sm[0];
}

void absmax_finish(const double* parts, int nparts, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, stream, parts, nparts, out);
}

// per-field finish: block f reduces the `per` maxima its field's blocks left (parts [nfield][per]) to out[f]
__global__ void __launch_bounds__(256) absmax_fields_kernel(const double* part, int per, double* out) {
  const double* p = part + (long)blockIdx.x * per;
  double m = 0.0;
  for (int k = threadIdx.x; k < per; k += blockDim.x) m = fmax(m, p[k]);
  __shared__ double sm[256];
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}

void absmax_finish_fields(const double* parts, int nfield, int per, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(absmax_fields_kernel, dim3((unsigned)nfield), dim3(256), 0, stream, parts, per, out);
}

// direction and iterate update of the Chebyshev iteration in one pass: d = c1 z + c2 d (d not read when c2 == 0), v += d
__global__ void __launch_bounds__(256) cheb_update_kernel(long n, double c1, const double* __restrict__ z, double c2,
                                                          double* __restrict__ d, double* __restrict__ v) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
    const double dn = c2 == 0.0 ? c1 * z[t] : fma(c1, z[t], c2 * d[t]);
    d[t] = dn;
    v[t] += dn;
  }
}

__global__ void __launch_bounds__(256) axpy_kernel(long n, double alpha, const double* __restrict__ x,
                                                   double* __restrict__ y) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x)
    y[t] += alpha * x[t];
}

// Windows of an extended block <-> one packed buffer (halo refresh of the overlapped-halo decomposition).  blockIdx.y is
// the window; a thread moves two neighbouring doubles of one window row when the window width and both addresses allow
// 16-byte accesses (the 64-wide strips of the decomposition always do), single doubles otherwise.
struct HaloRects {
  int n;
  int row0[8], col0[8], rows[8], cols[8];
  long offset[8];      // start of the window in the packed buffer, in doubles
};

template <bool PACK>
__global__ void __launch_bounds__(256) halo_pack_kernel(double* __restrict__ u, int nfield, int ey, int ex, HaloRects r,
                                                        double* __restrict__ buf) {
  const int w = blockIdx.y;
  const int rows = r.rows[w], cols = r.cols[w];
  const long plane = (long)ey * ex;
  double* b = buf + r.offset[w];
  double* base = u + (long)r.row0[w] * ex + r.col0[w];
  const bool pair = (cols & 1) == 0 && (ex & 1) == 0 && (r.col0[w] & 1) == 0 && (r.offset[w] & 1) == 0 &&
                    (((unsigned long long)u | (unsigned long long)buf) & 15) == 0;
  if (pair) {
    const int hc = cols >> 1;
    const long total = (long)nfield * rows * hc;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
      const int c = (int)(t % hc);
      const long fr = t / hc;
      const int j = (int)(fr % rows), f = (int)(fr / rows);
      double2* pu = reinterpret_cast<double2*>(base + (long)f * plane + (long)j * ex) + c;
      double2* pb = reinterpret_cast<double2*>(b + ((long)f * rows + j) * cols) + c;
      if (PACK) *pb = *pu; else *pu = *pb;
    }
  } else {
    const long total = (long)nfield * rows * cols;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
      const int c = (int)(t % cols);
      const long fr = t / cols;
      const int j = (int)(fr % rows), f = (int)(fr / rows);
      double* pu = base + (long)f * plane + (long)j * ex + c;
      double* pb = b + ((long)f * rows + j) * cols + c;
      if (PACK) *pb = *pu; else *pu = *pb;
    }
  }
}

static inline unsigned grid_for(long n) {
  long b = (n + 255) / 256;
  return (unsigned)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

}  // namespace qp

extern "C" {

int qp_add_constant(const uint8_t* flags, int64_t ncell, int32_t nfield, double* state, double amount, void* stream) {
  QP_REQUIRE(flags && state && ncell > 0 && nfield > 0, "bad arguments");
  hipLaunchKernelGGL(qp::add_constant_kernel, dim3(qp::grid_for(ncell * nfield)), dim3(256), 0, (hipStream_t)stream,
                     flags, (long)ncell, (int)nfield, state, amount);
  return qp::check_launch("qp_add_constant");
}

int qp_nan_pad(const uint8_t* flags, int64_t ncell, int32_t nfield, const double* in, double scale, double* out,
               void* stream) {
  QP_REQUIRE(flags && in && out && ncell > 0 && nfield > 0, "bad arguments");
  hipLaunchKernelGGL(qp::nan_pad_kernel, dim3(qp::grid_for(ncell)), dim3(256), 0, (hipStream_t)stream, flags, (long)ncell,
                     (int)nfield, in, scale, out);
  return qp::check_launch("qp_nan_pad");
}

int qp_add_scaled(int64_t n, double* state, const double* g, double scale, void* stream) {
  QP_REQUIRE(state && g && n > 0, "bad arguments");
  hipLaunchKernelGGL(qp::add_scaled_kernel, dim3(qp::grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long)n, state,
                     g, scale);
  return qp::check_launch("qp_add_scaled");
}

int64_t qp_pauli_workspace_bytes(void) { return (int64_t)qp::kRedBlocks * (int64_t)sizeof(qp::PauliPartial); }

int qp_pauli_stats(const double* state, const double* rho, const int32_t* cls, const uint8_t* flags, int32_t ne,
                   int32_t nclass, int64_t ncell, double density_floor, void* workspace, double* out_vals,
                   int64_t* out_idx, void* stream) {
  QP_REQUIRE(state && rho && flags && workspace && out_vals && out_idx, "NULL argument");
  QP_REQUIRE(ne > 0 && nclass > 0 && ncell > 0, "ne, nclass, ncell must be positive");
  QP_REQUIRE(nclass == 1 || cls, "cls is required when nclass > 1");
  const long by = ne < qp::kRedBlocks ? ne : qp::kRedBlocks;
  long bx = (ncell + 255) / 256;
  if (bx > qp::kRedBlocks / by) bx = qp::kRedBlocks / by;
  if (bx < 1) bx = 1;
  const long blocks = bx * by;
  auto* part = (qp::PauliPartial*)workspace;
  hipLaunchKernelGGL(qp::pauli_partial_kernel, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, (hipStream_t)stream, state,
                     rho, cls, flags, (int)ne, (long)ncell, density_floor, part);
  hipLaunchKernelGGL(qp::pauli_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, (int)blocks, out_vals,
                     (long*)out_idx);
  return qp::check_launch("qp_pauli_stats");
}

int64_t qp_pauli_members_workspace_bytes(int64_t ncell_member, int64_t members) {
  (void)ncell_member;
  if (members < 1) members = 1;
  return (int64_t)members * qp::pauli_member_budget((long)members) * (int64_t)sizeof(qp::PauliPartial);
}

int qp_pauli_stats_members(const double* state, const double* rho, const int32_t* cls, const uint8_t* flags, int32_t ne,
                           int32_t nclass, int64_t ncell_member, int64_t members, double density_floor, void* workspace,
                           double* out_vals, int64_t* out_idx, void* stream) {
  QP_REQUIRE(state && rho && flags && workspace && out_vals && out_idx, "NULL argument");
  QP_REQUIRE(ne > 0 && nclass > 0 && ncell_member > 0 && members > 0, "ne, nclass, ncell_member, members must be positive");
  QP_REQUIRE(members <= 0x7fffffffL / 1024, "too many members for one launch");
  QP_REQUIRE(nclass == 1 || cls, "cls is required when nclass > 1");
  const long budget = qp::pauli_member_budget((long)members);
  const long by = ne < budget ? ne : budget;
  long bxm = (ncell_member + 255) / 256;
  if (bxm > budget / by) bxm = budget / by;
  if (bxm < 1) bxm = 1;
  auto* part = (qp::PauliPartial*)workspace;
  hipLaunchKernelGGL(qp::pauli_members_partial_kernel, dim3((unsigned)(bxm * members), (unsigned)by), dim3(256), 0,
                     (hipStream_t)stream, state, rho, cls, flags, (int)ne, (long)ncell_member, (long)members, (int)bxm,
                     density_floor, part);
  hipLaunchKernelGGL(qp::pauli_members_final_kernel, dim3((unsigned)members), dim3(256), 0, (hipStream_t)stream,
                     (const qp::PauliPartial*)part, bxm * by, (long)ncell_member, 0L, out_vals, (long*)out_idx);
  return qp::check_launch("qp_pauli_stats_members");
}

int qp_add_constant_members(const uint8_t* flags, int64_t ncell_member, int64_t members, int32_t nfield, double* state,
                            const double* amounts, void* stream) {
  QP_REQUIRE(flags && state && amounts && ncell_member > 0 && members > 0 && nfield > 0, "bad arguments");
  hipLaunchKernelGGL(qp::add_constant_members_kernel, dim3(qp::grid_for(ncell_member * members * nfield)), dim3(256), 0,
                     (hipStream_t)stream, flags, (long)ncell_member, (long)members, (int)nfield, state, amounts);
  return qp::check_launch("qp_add_constant_members");
}

int qp_energy_integrate(const double* state, int32_t ne, int64_t ncell, double dE, double* out, void* stream) {
  QP_REQUIRE(state && out && ne > 0 && ncell > 0, "bad arguments");
  hipLaunchKernelGGL(qp::energy_integrate_kernel, dim3(qp::grid_for(ncell)), dim3(256), 0, (hipStream_t)stream, state,
                     (int)ne, (long)ncell, dE, out);
  return qp::check_launch("qp_energy_integrate");
}

size_t qp_region_sums_workspace_bytes(int32_t nfield, int64_t ncell_member, int64_t members, int32_t nregion) {
  if (nfield < 1 || ncell_member < 1 || members < 1 || nregion < 1) return 0;
  return (size_t)nfield * (size_t)members * (size_t)qp::region_chunks((long)ncell_member) * (size_t)nregion * sizeof(double);
}

int qp_region_sums(const double* state, const uint8_t* region_bits, int32_t nfield, int64_t ncell_member, int64_t members,
                   int32_t nregion, void* workspace, double* out, void* stream) {
  QP_REQUIRE(state && region_bits && workspace && out, "NULL argument");
  QP_REQUIRE(nfield > 0 && ncell_member > 0 && members > 0, "nfield, ncell_member, members must be positive");
  QP_REQUIRE(nregion >= 1 && nregion <= 8, "1 to 8 regions per call");
  QP_REQUIRE(nfield <= 65535 && members <= 65535, "at most 65535 fields and 65535 members per call");
  const long nchunk = qp::region_chunks((long)ncell_member);
  QP_REQUIRE(nchunk <= 0x7fffffffL, "ncell_member too large for one launch");
  const bool vec = ((unsigned long long)state & 15) == 0;
  const dim3 grid((unsigned)nchunk, (unsigned)members, (unsigned)nfield);
  auto* part = (double*)workspace;
  const hipStream_t st = (hipStream_t)stream;
  if (nregion == 1)
    qp::region_partial_launch<1>(vec, grid, st, state, region_bits, (long)ncell_member, (long)members, 1, nchunk, part);
  else if (nregion == 2)
    qp::region_partial_launch<2>(vec, grid, st, state, region_bits, (long)ncell_member, (long)members, 2, nchunk, part);
  else if (nregion <= 4)
    qp::region_partial_launch<4>(vec, grid, st, state, region_bits, (long)ncell_member, (long)members, (int)nregion, nchunk,
                                 part);
  else
    qp::region_partial_launch<8>(vec, grid, st, state, region_bits, (long)ncell_member, (long)members, (int)nregion, nchunk,
                                 part);
  hipLaunchKernelGGL(qp::region_final_kernel, dim3((unsigned)members, (unsigned)nfield), dim3(64), 0, st,
                     (const double*)part, nchunk, (int)nregion, (long)members, (int)nfield, out);
  return qp::check_launch("qp_region_sums");
}

int qp_block_sums(const double* state, const uint8_t* flags, int32_t nfield, int32_t ny, int32_t nx, int64_t members,
                  int32_t bin, int32_t oy, int32_t ox, double* out, void* stream) {
  QP_REQUIRE(state && flags && out, "NULL argument");
  QP_REQUIRE(nfield > 0 && ny > 0 && nx > 0 && members > 0, "nfield, ny, nx, members must be positive");
  QP_REQUIRE(bin == 2 || bin == 4 || bin == 8 || bin == 16 || bin == 32 || bin == 64, "bin must be 2, 4, 8, 16, 32 or 64");
  QP_REQUIRE(oy >= 0 && oy < bin && ox >= 0 && ox < bin, "oy and ox must lie in [0, bin)");
  QP_REQUIRE(nfield <= 65535 && members <= 65535, "at most 65535 fields and 65535 members per call");
  QP_REQUIRE(ny <= (1 << 30) && nx <= (1 << 30), "ny and nx must not exceed 2^30");
  // waves of one plane: 64-column segments x groups of at least 16 rows
  QP_REQUIRE(((long)nx / 64 + 2) * ((long)ny / 16 + 2) <= 0x7fffffffL, "ny x nx too large for one launch");
  const hipStream_t st = (hipStream_t)stream;
  switch (bin) {
    case 2: qp::block_sums_launch<2>(st, state, flags, ny, nx, (long)members, nfield, oy, ox, out); break;
    case 4: qp::block_sums_launch<4>(st, state, flags, ny, nx, (long)members, nfield, oy, ox, out); break;
    case 8: qp::block_sums_launch<8>(st, state, flags, ny, nx, (long)members, nfield, oy, ox, out); break;
    case 16: qp::block_sums_launch<16>(st, state, flags, ny, nx, (long)members, nfield, oy, ox, out); break;
    case 32: qp::block_sums_launch<32>(st, state, flags, ny, nx, (long)members, nfield, oy, ox, out); break;
    default: qp::block_sums_launch<64>(st, state, flags, ny, nx, (long)members, nfield, oy, ox, out); break;
  }
  return qp::check_launch("qp_block_sums");
}

int qp_weighted_sum(const double* state, const double* weights, int32_t n, int64_t ncell, double* out, void* stream) {
  QP_REQUIRE(state && weights && out && n > 0 && ncell > 0, "bad arguments");
  hipLaunchKernelGGL(qp::weighted_sum_kernel, dim3(qp::grid_for(ncell)), dim3(256), 0, (hipStream_t)stream, state,
                     weights, (int)n, (long)ncell, out);
  return qp::check_launch("qp_weighted_sum");
}

int qp_absmax(const double* a, int64_t n, void* workspace, double* out_val, void* stream) {
  QP_REQUIRE(a && workspace && out_val && n > 0, "bad arguments");
  long blocks = (n + 255) / 256;
  if (blocks > qp::kRedBlocks) blocks = qp::kRedBlocks;
  hipLaunchKernelGGL(qp::absmax_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, (long)n,
                     (double*)workspace);
  hipLaunchKernelGGL(qp::absmax_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace,
                     (int)blocks, out_val);
  return qp::check_launch("qp_absmax");
}

int qp_halo_pack(double* u, int32_t nfield, int32_t ey, int32_t ex, const int32_t* rects, int32_t nrect, int32_t op,
                 double* buf, void* stream) {
  QP_REQUIRE(u && buf && rects, "u, buf, rects must be non-NULL");
  QP_REQUIRE(nfield > 0 && ey > 0 && ex > 0, "nfield, ey, ex must be positive");
  QP_REQUIRE(nrect >= 1 && nrect <= 8, "1 to 8 windows per call");
  QP_REQUIRE(op == 0 || op == 1, "op must be 0 (pack) or 1 (unpack)");
  qp::HaloRects r;
  r.n = nrect;
  long off = 0, largest = 0;
  for (int w = 0; w < nrect; ++w) {
    r.row0[w] = rects[4 * w]; r.col0[w] = rects[4 * w + 1]; r.rows[w] = rects[4 * w + 2]; r.cols[w] = rects[4 * w + 3];
    QP_REQUIRE(r.rows[w] > 0 && r.cols[w] > 0 && r.row0[w] >= 0 && r.col0[w] >= 0 && r.row0[w] + r.rows[w] <= ey &&
                   r.col0[w] + r.cols[w] <= ex, "window outside the block");
    r.offset[w] = off;
    const long cells = (long)nfield * r.rows[w] * r.cols[w];
    off += cells;
    if (cells > largest) largest = cells;
  }
  long bx = (largest / 2 + 255) / 256;
  if (bx > 2048) bx = 2048;
  if (bx < 1) bx = 1;
  if (op == 0)
    hipLaunchKernelGGL(qp::halo_pack_kernel<true>, dim3((unsigned)bx, (unsigned)nrect), dim3(256), 0, (hipStream_t)stream, u,
                       (int)nfield, (int)ey, (int)ex, r, buf);
  else
    hipLaunchKernelGGL(qp::halo_pack_kernel<false>, dim3((unsigned)bx, (unsigned)nrect), dim3(256), 0, (hipStream_t)stream, u,
                       (int)nfield, (int)ey, (int)ex, r, buf);
  return qp::check_launch("qp_halo_pack");
}

int qp_axpy(int64_t n, double alpha, const double* x, double* y, void* stream) {
  QP_REQUIRE(x && y && n > 0, "bad arguments");
  hipLaunchKernelGGL(qp::axpy_kernel, dim3(qp::grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long)n, alpha, x, y);
  return qp::check_launch("qp_axpy");
}

int qp_cheb_update(int64_t n, double c1, const double* z, double c2, double* d, double* v, void* stream) {
  QP_REQUIRE(z && d && v && n > 0, "bad arguments");
  hipLaunchKernelGGL(qp::cheb_update_kernel, dim3(qp::grid_for(n)), dim3(256), 0, (hipStream_t)stream, (long)n, c1, z, c2, d, v);
  return qp::check_launch("qp_cheb_update");
}

}  // extern "C"
