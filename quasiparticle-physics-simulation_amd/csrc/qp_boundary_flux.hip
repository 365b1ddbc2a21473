// Boundary outflow per surface (flux traces): out[m][s][i] = sum over the faces k of surface s of
// D * (diag_k * u_c - src_k), c = face_cell[k], on planes u = state[i][m][cell].  include/qpsim_hip.h has the contract.
//
// Fixed partition (determinism): block = (chunk of at most QP_FLUX_CHUNK faces of one surface, field f = i * members + m).
// Thread t owns the faces t + 256 j, j = 0 ... 3, of the chunk: the loads of face_cell / face_diag / face_src are
// coalesced, the gathers of u (and of D with a field of coefficients) go out together before the first use.  A term is
// formed by three rounded operations (contraction is off in the kernel: no fma), a face beyond the chunk counts +0.0
// through a select, the four terms are added in j order, the lanes of a wave by __shfl_down from offset 32 down to 1, the waves as ((w0 + w1) + w2) + w3.
// The second launch (one wave per field) lets lane s add the partials of the chunks of surface s in chunk order.
// Who adds what depends on the face list alone; there are no atomics and every output has one writer.
#include "qp_common.h"

namespace qp {

constexpr int kFluxPerThread = QP_FLUX_CHUNK / 256;
static_assert(QP_FLUX_CHUNK % 256 == 0, "a chunk is a whole number of faces per thread");

// chunks of surface s: [first[s], first[s + 1]) (by value: 65 ints)
struct FluxSurfaces {
  int first[65];
};

template <bool FIELD>
__global__ void __launch_bounds__(256) flux_partial_kernel(const double* __restrict__ state, const double* __restrict__ dco,
                                                           const int32_t* __restrict__ face_cell,
                                                           const double* __restrict__ face_diag,
                                                           const double* __restrict__ face_src,
                                                           const int32_t* __restrict__ chunks, long ncm, long nchunk,
                                                           double* __restrict__ part) {
#pragma clang fp contract(off)      // a term is three rounded operations: the product must not fuse into the difference
  __shared__ double sm[4];
  const long chunk = blockIdx.x, f = blockIdx.y;
  const long begin = chunks[3 * chunk];
  const int count = chunks[3 * chunk + 1];                  // 1 ... QP_FLUX_CHUNK (validated on the host)
  const double* u = state + f * ncm;
  const double* d = dco + (FIELD ? f * ncm : f);
  int cell[kFluxPerThread];
  double dg[kFluxPerThread], sr[kFluxPerThread], uu[kFluxPerThread], dd[kFluxPerThread];
  bool on[kFluxPerThread];
#pragma unroll
  for (int j = 0; j < kFluxPerThread; ++j) {
    const int k = (int)threadIdx.x + 256 * j;
    on[j] = k < count;
    const long idx = begin + (on[j] ? k : 0);              // a face of this chunk in any case: no load behind a branch
    cell[j] = face_cell[idx];
    dg[j] = face_diag[idx];
    sr[j] = face_src[idx];
  }
#pragma unroll
  for (int j = 0; j < kFluxPerThread; ++j) {
    uu[j] = u[cell[j]];
    dd[j] = FIELD ? d[cell[j]] : 0.0;
  }
  const double dc = FIELD ? 0.0 : d[0];
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kFluxPerThread; ++j) {
    double t = dg[j] * uu[j];
    t = t - sr[j];
    t = (FIELD ? dd[j] : dc) * t;
    t = on[j] ? t : 0.0;
    acc = j == 0 ? t : acc + t;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[f * nchunk + chunk] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

__global__ void __launch_bounds__(64) flux_final_kernel(const double* __restrict__ part, FluxSurfaces surf, long nchunk,
                                                        int nsurface, long members, int nplane,
                                                        double* __restrict__ out) {
  const long f = blockIdx.x;
  const long i = f / members, m = f % members;
  const int s = threadIdx.x;
  if (s >= nsurface) return;
  const double* src = part + f * nchunk;
  double acc = 0.0;
  for (int k = surf.first[s]; k < surf.first[s + 1]; ++k) acc += src[k];
  out[(m * nsurface + s) * nplane + i] = acc;
}

}  // namespace qp

extern "C" {

size_t qp_boundary_flux_workspace_bytes(int32_t nplane, int64_t members, int64_t nchunk) {
  if (nplane < 1 || members < 1 || nchunk < 0 || (int64_t)nplane * members > 65535 || nchunk > 0x7fffffffL) return 0;
  const size_t n = (size_t)nplane * (size_t)members * (size_t)nchunk;
  return (n ? n : 1) * sizeof(double);
}

int qp_boundary_flux(const double* state, const double* dcoef, const double* dfield, int32_t nplane, int64_t ncell_member,
                     int64_t members, const int32_t* face_cell, const double* face_diag, const double* face_src,
                     int64_t nface, const int32_t* surface_begin, int32_t nsurface, const int32_t* chunks_host,
                     const int32_t* chunks_dev, int64_t nchunk, void* workspace, double* out, void* stream) {
  QP_REQUIRE(state && workspace && out && surface_begin, "NULL argument");
  QP_REQUIRE((dcoef != nullptr) != (dfield != nullptr), "give exactly one of dcoef / dfield");
  QP_REQUIRE(nsurface >= 1 && nsurface <= 64, "1 to 64 surfaces per call");
  QP_REQUIRE(nplane > 0 && ncell_member > 0 && members > 0, "nplane, ncell_member, members must be positive");
  QP_REQUIRE(ncell_member <= 0x7fffffffL, "ncell_member must not exceed 2^31 - 1 (face_cell is int32)");
  QP_REQUIRE((int64_t)nplane * members <= 65535, "at most 65535 fields (nplane * members) per call");
  QP_REQUIRE(nface >= 0 && nface <= 0x7fffffffL && nchunk >= 0 && nchunk <= 0x7fffffffL, "nface / nchunk out of range");
  QP_REQUIRE((nface == 0) == (nchunk == 0), "nface and nchunk must be zero together");
  QP_REQUIRE(nchunk == 0 || (face_cell && face_diag && face_src && chunks_host && chunks_dev), "NULL face array or chunk table");
  QP_REQUIRE(surface_begin[0] == 0 && surface_begin[nsurface] == nface, "surface_begin must run from 0 to nface");
  for (int s = 0; s < nsurface; ++s)
    QP_REQUIRE(surface_begin[s] <= surface_begin[s + 1], "surface_begin must ascend");
  qp::FluxSurfaces surf;
  int s_prev = 0;
  long end_prev = 0;
  surf.first[0] = 0;
  for (long k = 0; k < nchunk; ++k) {
    const long begin = chunks_host[3 * k], count = chunks_host[3 * k + 1];
    const int s = chunks_host[3 * k + 2];
    QP_REQUIRE(count >= 1 && count <= QP_FLUX_CHUNK, "a chunk holds 1 to QP_FLUX_CHUNK faces");
    QP_REQUIRE(s >= s_prev && s < nsurface && begin >= end_prev, "chunk table out of order");
    QP_REQUIRE(begin >= surface_begin[s] && begin + count <= surface_begin[s + 1], "a chunk crosses its surface");
    for (int q = s_prev + 1; q <= s; ++q) surf.first[q] = (int)k;
    s_prev = s;
    end_prev = begin + count;
  }
  for (int q = s_prev + 1; q <= 64; ++q) surf.first[q] = (int)nchunk;
  const hipStream_t st = (hipStream_t)stream;
  auto* part = (double*)workspace;
  const unsigned nfield = (unsigned)(nplane * members);
  if (nchunk > 0) {
    const dim3 grid((unsigned)nchunk, nfield);
    if (dfield)
      hipLaunchKernelGGL((qp::flux_partial_kernel<true>), grid, dim3(256), 0, st, state, dfield, face_cell, face_diag,
                         face_src, chunks_dev, (long)ncell_member, (long)nchunk, part);
    else
      hipLaunchKernelGGL((qp::flux_partial_kernel<false>), grid, dim3(256), 0, st, state, dcoef, face_cell, face_diag,
                         face_src, chunks_dev, (long)ncell_member, (long)nchunk, part);
  }
  hipLaunchKernelGGL(qp::flux_final_kernel, dim3(nfield), dim3(64), 0, st, (const double*)part, surf, (long)nchunk,
                     (int)nsurface, (long)members, (int)nplane, out);
  return qp::check_launch("qp_boundary_flux");
}

}  // extern "C"
