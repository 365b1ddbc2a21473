// What the two rate-trace units share (private to qp_collision_rates.hip and qp_phonon_rates.hip): the partition, the
// kernel frame around a pixel body, the finish, and the host side of an entry (checks, NR ladder, launch, workspace).
//
// Fixed partition (determinism): block = (chunk of QP_RATES_CHUNK cells, member), wave w of the block owns the cells
// [RUN w, RUN w + RUN) of the chunk, walked in index order in groups of Body::PB.  Cell indices are member-local, so the
// partition of a member does not depend on where its planes start.  The waves combine through LDS in wave order, the
// block stores nregion * 4 * count partials, rates_final_kernel (qp_collision_rates.hip) adds them in chunk order.  No
// atomics, no completion counters.
#pragma once
#include <type_traits>

#include "qp_common.h"

namespace qp {

constexpr int RMAXBINS = 3;                          // phonon bins per lane: NW <= 3 * 64 - 1
constexpr int RWAVES = 4;                            // waves per block
constexpr int RCHUNK = QP_RATES_CHUNK;               // cells per block
constexpr int RRUN = RCHUNK / RWAVES;                // cells per wave
static_assert(RRUN == 4 * 64, "the region bits of a run are held 4 cells per lane");

__device__ __forceinline__ double bcast(double x, int srclane) {
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

// What a body sees of its wave and of the pixel at hand.  The wave's Body::lds_per_wave(nw) doubles start at index `o` of
// the block's dynamic LDS array.  There is no `lane < ne` here: a body forms it from `lane`.  Read from this struct the
// predicate gave both bodies other j-loops (2 registers more in the collision body, a wait for memory more per j in
// phonon <*, 2> and <*, 3>: 10 - 17 % at NE = 50; profiles/phonon_rates_resource_usage.txt).
struct RatesLane {
  const RatesView& t;
  int o;
  int lane;
  double dE;
  int use_r, use_s;
};
struct RatesPixel {
  double ni, qi;
  const double* ks;                                  // the tables of the pixel's class, NULL for a process that is off
  const double* kr;
};

// The frame of a rate kernel.  A Body states
//   NR, PB      accumulated regions (nregion rounded up to 1, 2, 4, 8), pixels per group (a divisor of 8)
//   PLANES      phonon planes a lane loads per pixel (bins lane + 64 s, s < PLANES, under s-th bin < nw)
//   SLOTS       values a lane accumulates per region and channel (lane + 64 s, s < SLOTS, stored under < count(view))
//   lds_per_wave(nw), count(view)
//   sums(L, px, N)           the pixel's j-loop between its wave barriers; N[PLANES] the lane's phonon occupations
//   values(L, px, N, s, v)   the four rounded channel values of slot s
// A lane adds the cells of its wave's run in index order whatever PB is, so PB is not part of the result.  The region bits
// are wave-uniform: the 256 bytes of a wave's run are read once, 4 per lane, a pixel's byte is broadcast with v_readlane,
// and the add of a pixel's values is under a scalar branch per region.
// LDS: [RWAVES][lds_per_wave] for the bodies; after the pixel loops the same bytes serve the wave-order combine,
// [NR * 4 * SLOTS][64].
template <class Body>
__global__ void __launch_bounds__(64 * RWAVES) rates_kernel(RatesView t, const uint8_t* __restrict__ bits, long ncm,
                                                           long members, int nregion, long nchunk,
                                                           const double* __restrict__ state,
                                                           const double* __restrict__ ph, double dE, int use_r, int use_s,
                                                           double* __restrict__ part) {
  constexpr int NR = Body::NR, PB = Body::PB, PLANES = Body::PLANES, SLOTS = Body::SLOTS;
  static_assert(RRUN % PB == 0 && PB <= 8, "a wave's run is a whole number of groups");
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NE = t.ne, NW = t.nw, NN = NE * NE;
  const int count = Body::count(t);
  const long chunk = blockIdx.x, m = blockIdx.y;
  const long ncell = ncm * members;                  // plane stride
  const long mbase = m * ncm;                        // first cell of the member in a plane
  const bool on = lane < NE;
  const unsigned rmask = (1u << nregion) - 1u;
  const RatesLane L{t, wave * Body::lds_per_wave(NW), lane, dE, use_r, use_s};

  double acc[NR][4][SLOTS];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) acc[r][ch][s] = 0.0;

  // the region bits of the wave's whole run in one round trip: lane l holds the bytes of cells run0 + 4 l ... + 3 (0 past the
  // member's end)
  const long run0 = chunk * RCHUNK + (long)wave * RRUN;
  unsigned word = 0u;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const long c = run0 + 4 * lane + b;
    if (c < ncm) word |= (unsigned)(bits[c] & rmask) << (8 * b);
  }
  for (int g = 0; g < RRUN / PB; ++g) {
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
    double n[PB], pb[PLANES][PB];
#pragma unroll
    for (int k = 0; k < PB; ++k) n[k] = (on && k < npx) ? state[(long)lane * ncell + p0 + k] : 0.0;
#pragma unroll
    for (int s = 0; s < PLANES; ++s) {
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
      const double ni = n[k];
      const RatesPixel px{ni, rho_i * fmax(1.0 - ni / fmax(rho_i, 1e-30), 0.0), use_s ? t.ks0 + (long)c * NN : nullptr,
                          use_r ? t.kr0 + (long)c * NN : nullptr};
      double N[PLANES];
#pragma unroll
      for (int s = 0; s < PLANES; ++s) N[s] = pb[s][k];
      Body body;
      body.sums(L, px, N);
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        double v[4];
        body.values(L, px, N, s, v);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          if (b & (1u << r)) {               // scalar branch: the bits of a pixel are wave-uniform
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) acc[r][ch][s] += v[ch];
          }
        }
      }
    }
  }

  // waves combine in wave order: wave 0 holds ((w0 + w1) + w2) + w3.  The combine area overlays the bodies' LDS, which
  // every wave has left after this barrier.
  __syncthreads();
  for (int w = 1; w < RWAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
          for (int s = 0; s < SLOTS; ++s) lds[((r * 4 + ch) * SLOTS + s) * 64 + lane] = acc[r][ch][s];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
          for (int s = 0; s < SLOTS; ++s) acc[r][ch][s] += lds[((r * 4 + ch) * SLOTS + s) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0) {
    double* dst = part + (m * nchunk + chunk) * ((long)nregion * 4 * count);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < nregion) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
          for (int s = 0; s < SLOTS; ++s) {
            const int w = lane + 64 * s;
            if (w < count) dst[((long)r * 4 + ch) * count + w] = acc[r][ch][s];
          }
      }
    }
  }
}

// ---- host side of an entry ---------------------------------------------------------------------------------------------
// the arguments of qp_collision_rates / qp_phonon_rates, in their order
struct RatesCall {
  const qp_collision_tables* t;
  const uint8_t* bits;
  int64_t ncm, members;
  int32_t nregion;
  const double* state;
  const double* ph;
  double dE;
  int en_r, en_s;
  void* workspace;
  double* out;
  void* stream;
};

inline long rates_chunks(long ncm) { return (ncm + RCHUNK - 1) / RCHUNK; }

// bytes of the chunk partials, `count` values per region and channel; the entry checks its ranges first
inline size_t rates_workspace_bytes(int32_t count, int64_t ncm, int64_t members, int32_t nregion) {
  return (size_t)members * (size_t)rates_chunks((long)ncm) * (size_t)nregion * 4 * (size_t)count * sizeof(double);
}

// QP_REQUIRE under the name of the public entry `func`
#define QP_RATES_REQUIRE(cond, msg)                \
  do {                                             \
    if (!(cond)) {                                 \
      set_error("%s: %s", func, msg);              \
      return QP_ERR_INVALID_ARGUMENT;              \
    }                                              \
  } while (0)

// The checks of an entry up to the table pointers; an entry's own requirement on the tables follows them, then
// rates_check_shape.
inline int rates_check_tables(const char* func, const RatesCall& c, int (*available)(int32_t, int32_t)) {
  const qp_collision_tables* t = c.t;
  QP_RATES_REQUIRE(t != nullptr, "tables are NULL");
  if (t->struct_size != sizeof(qp_collision_tables)) {
    set_error("%s: qp_collision_tables.struct_size is %u, this library expects %zu (binding built against another "
              "header revision)", func, t->struct_size, sizeof(qp_collision_tables));
    return QP_ERR_INVALID_ARGUMENT;
  }
  QP_RATES_REQUIRE(c.bits && c.state && c.ph && c.workspace && c.out, "NULL argument");
  QP_RATES_REQUIRE(c.ncm > 0 && c.members > 0, "ncell_member, members must be positive");
  QP_RATES_REQUIRE(t->ne > 0 && t->nw > 0 && t->nclass > 0, "ne, nw, nclass must be positive");
  if (!available(t->ne, t->nw)) {
    set_error("%s: no kernel for ne = %d, nw = %d (2 <= ne <= 64, 1 <= nw <= 191)", func, t->ne, t->nw);
    return QP_ERR_UNSUPPORTED;
  }
  if (c.nregion < 1 || c.nregion > 8) {
    set_error("%s: 1 to 8 regions per call, got %d", func, c.nregion);
    return QP_ERR_UNSUPPORTED;
  }
  QP_RATES_REQUIRE(t->rho && t->idx_diff && t->idx_sum && t->sign, "rho, idx maps and sign must be non-NULL");
  return QP_OK;
}

inline int rates_check_shape(const char* func, const RatesCall& c) {
  const qp_collision_tables* t = c.t;
  QP_RATES_REQUIRE(t->nclass == 1 || t->cls, "cls is required when nclass > 1");
  if (t->flags & QP_COLL_MEMBER_CLASSES)
    QP_RATES_REQUIRE(c.members % t->nclass == 0, "QP_COLL_MEMBER_CLASSES needs members to be a multiple of nclass");
  QP_RATES_REQUIRE(c.members <= 65535, "at most 65535 members per call");
  QP_RATES_REQUIRE(rates_chunks((long)c.ncm) <= 0x7fffffffL, "ncell_member too large for one launch");
  return QP_OK;
}
#undef QP_RATES_REQUIRE

// f(std::integral_constant<int, NR>) for NR = nregion rounded up to 1, 2, 4, 8
template <class F>
void rates_ladder(int nregion, F&& f) {
  if (nregion == 1) f(std::integral_constant<int, 1>{});
  else if (nregion == 2) f(std::integral_constant<int, 2>{});
  else if (nregion <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

template <class Body>
void rates_launch(const RatesCall& c) {
  const qp_collision_tables& t = *c.t;
  const size_t bodies = (size_t)RWAVES * Body::lds_per_wave(t.nw), combine = (size_t)Body::NR * 4 * Body::SLOTS * 64;
  const size_t shmem = (bodies > combine ? bodies : combine) * sizeof(double);
  const RatesView v{t.ne, t.nw, t.kr0, t.ks0, t.rho, t.idx_diff, t.idx_sum, t.sign, t.cls};
  const long nchunk = rates_chunks((long)c.ncm);
  const int use_r = c.en_r && t.kr0, use_s = c.en_s && t.ks0;
  hipLaunchKernelGGL((rates_kernel<Body>), dim3((unsigned)nchunk, (unsigned)c.members), dim3(64 * RWAVES), shmem,
                     (hipStream_t)c.stream, v, c.bits, (long)c.ncm, (long)c.members, (int)c.nregion, nchunk, c.state, c.ph,
                     c.dE, use_r, use_s, (double*)c.workspace);
}

// The finish (qp_collision_rates.hip): out[m][e] = sum over the chunks of `c`, in chunk order, of the partials in its
// workspace, e < nregion * 4 * count.
void rates_finish(const RatesCall& c, int count);

}  // namespace qp
