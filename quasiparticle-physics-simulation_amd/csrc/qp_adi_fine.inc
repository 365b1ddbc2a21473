// Fine tiles of the rectangle path: lines cut into chunks of FS = 32 cells, one wave per 32 x 64 (y-kernel) or 64 x 32
// (x-kernel) tile.  Included by qp_adi_rect.hip inside namespace qp.
//
// Why: a 64 x 64 tile is 64 doubles per lane, i.e. two waves per SIMD and a ~3 us serial stretch of arithmetic per tile.
// Grids of 1024^2 ... 3000^2 have 256 ... 2000 such tiles for 1024 SIMDs, so that stretch is exposed; halving the tile
// doubles the waves, halves the stretch and the registers (four waves per SIMD).  Price: twice the interface rows
// (+4.7 % bytes) and a decoupling limit reached at a ~ 0.32 instead of a ~ 5 (far coupling rho^31 against rho^63) -
// plans beyond it keep the 64 x 64 tiles.
//
// Same algorithm, tables (compact form only), interface arithmetic and pass structure as the 64 x 64 kernels
// (qp_adi_rect.hip).  A wave always holds ONE chunk of the direction it solves (32 registers per lane) and TWO chunks of
// the other direction, one per half-wave, for which it forms the reduced right-hand sides:
//   y-kernel: tile = y-chunk ty x columns [64 tx, 64 tx + 64): lane = column, register = row.  After the y-work the two
//             32 x 32 halves are transposed inside their half-waves -> lane = (x-chunk 2 tx + h, row), register = column:
//             the x-elimination of x-chunk 2 tx + h runs in registers.
//   x-kernel: tile = x-chunk tx x rows [64 ty, 64 ty + 64): global accesses as lane = (h, column), register r = row
//             64 ty + 32 h + r (two 256-byte row segments per instruction); transposed inside the half-waves ->
//             lane = row, register = column for the x-solve; transposed back for the stores, where lane (h, column) holds
//             exactly y-chunk 2 ty + h of its column: the y-elimination runs in registers.
// The two chunks of the other direction differ in their table only at the ends of a line (first / last chunk against an
// interior one); those tiles run the elimination with both tables and select per half-wave.

struct FineView {
  int ny, nx, nfield;
  int py, px;                   // 32-cell chunks per column / per row
  int stream;
  const double* alpha;          // [nfield]
  const double* ctab;           // [2 dirs][nfield][4 variants][2 parts][CT_PART]
  double* iface[2];             // per dir [nfield][2P+2][nlines] (rows 0 and 2P+1 unused: no decomposition here)
  const double* icoef[2];       // per dir [nfield][P+1][3]
  double other_src[2][2];
  // Peaceman-Rachford iteration passes (<..., SRC = true>): bscale * bsrc is added to every right-hand side formed
  const double* bsrc;           // [nfield][ny*nx]
  double bscale;
};

struct CoefFine {
  ctab_t part;
  __device__ __forceinline__ double at(int slot, int k) const {
    if (QP_ABL & 2) return 0.1 + 0.001 * slot;
    return part[cidx_len(FS, slot, k)];
  }
};

__device__ __forceinline__ CoefFine fine_coefs(const FineView& v, int dir, int b, int variant, int part) {
  return CoefFine{as_const(v.ctab + ((((long)dir * v.nfield + b) * 4 + variant) * 2 + part) * CT_PART)};
}

template <class Coef>
__device__ __forceinline__ void thomas32(double (&e)[FS], const Coef& t) {
  if (QP_ABL & 16) return;
  double dp = 0.0;
#pragma unroll
  for (int k = 0; k < FS; ++k) {
    dp = fma(t.at(T_AWF, k), dp, e[k] * t.at(T_W, k));
    e[k] = dp;
  }
  double x = 0.0;
#pragma unroll
  for (int k = FS - 1; k >= 0; --k) {
    x = fma(t.at(T_AWB, k), x, e[k]);
    e[k] = x;
  }
}

// e <- (I + a L) e + a s along the chunk, neighbour values gl / gr beyond its ends (zero at a wall), plus `extra`.
// Full chunks only: the off-diagonal weight is `a` wherever a neighbour exists and the neighbour value is zero where none
// does, so a (prev + next) serves every cell; the boundary source sits in the first / last cell of a line only.
template <class Coef>
__device__ __forceinline__ void explicit32(double (&e)[FS], double gl, double gr, const Coef& t, double a, double extra) {
  if (QP_ABL & 32) return;
  double prev = gl;
#pragma unroll
  for (int k = 0; k < FS; ++k) {
    const double cur = e[k];
    const double nxt = (k + 1 < FS) ? e[k + 1] : gr;
    const double add = (k == 0 || k == FS - 1) ? t.at(T_SRC, k) + extra : extra;
    e[k] = fma(a, prev + nxt, fma(t.at(T_C0, k), cur, add));
    prev = cur;
  }
}

// First / last entry of A_p^-1 e (the reduced right-hand sides of the chunk).  The fine tables carry the two eliminations
// in scaled form (fine_plan_prepare): d~_k = dp_k / ew_k obeys d~_k = eawf'_k d~_{k-1} + e_k, one FMA per cell, and
// yl = ew_last d~_last; likewise backwards with yf = ev_0 b~_0.
template <class Coef>
__device__ __forceinline__ void ends32(const double (&e)[FS], const Coef& t, double& yf, double& yl) {
  double dp = 0.0, bp = 0.0;
#pragma unroll
  for (int k = 0; k < FS; ++k) {
    const int j = FS - 1 - k;
    dp = fma(t.at(T_EAWF, k), dp, e[k]);
    bp = fma(t.at(T_EAV, j), bp, e[j]);
  }
  yf = bp * t.at(T_EV, 0);
  yl = dp * t.at(T_EW, FS - 1);
}

// reduced right-hand sides of the two chunks (one per half-wave) a wave holds of the direction it does not solve
__device__ __forceinline__ void ends32_pair(const double (&e)[FS], const FineView& v, int dir, int b, int p_even, int P,
                                            int h, double& yf, double& yl) {
  const int va = chunk_variant(p_even, P), vb = chunk_variant(p_even + 1, P);
  ends32(e, fine_coefs(v, dir, b, va, 1), yf, yl);
  if (va != vb) {     // wave-uniform: only the tiles at the two ends of a line
    double yf2, yl2;
    ends32(e, fine_coefs(v, dir, b, vb, 1), yf2, yl2);
    if (h) { yf = yf2; yl = yl2; }
  }
}

// 32 x 32 transpose inside each half-wave: v[k] on lane (h, l)  ->  v[l] on lane (h, k); its own inverse.  As 2 x 2 blocks
// of 16 x 16: v_permlane16_swap exchanges the off-diagonal blocks (registers 0..15 of lanes 16..31 <-> registers 16..31
// of lanes 0..15, in both half-waves at once), then every 16-lane row transposes its 16 x 16 block through its own
// 16 x 17 LDS patch, registers 0..15 first, 16..31 second: 8.5 KiB per wave (16 waves per CU fit), every lane busy in every
// LDS instruction, pitch 17 conflict-free both ways.
constexpr int QB = 16;
constexpr int QP = QB + 1;
constexpr int FINE_LDS_DOUBLES = 4 * QB * QP;
constexpr int FINE_LDS_PAIRS = 2 * 64;      // one (first, last) pair per lane of the one-pass kernel (fine_p_map)

__device__ __forceinline__ void swap_lane_rows(double& lo_reg, double& hi_reg) {
  // odd 16-lane rows of lo_reg <-> even 16-lane rows of hi_reg
  const unsigned long long a = __double_as_longlong(lo_reg), b = __double_as_longlong(hi_reg);
  const auto r0 = __builtin_amdgcn_permlane16_swap((unsigned)a, (unsigned)b, false, false);
  const auto r1 = __builtin_amdgcn_permlane16_swap((unsigned)(a >> 32), (unsigned)(b >> 32), false, false);
  lo_reg = __longlong_as_double(((unsigned long long)r1[0] << 32) | r0[0]);
  hi_reg = __longlong_as_double(((unsigned long long)r1[1] << 32) | r0[1]);
}

__device__ __forceinline__ void transpose32h(double (&v)[FS], double* lds, int lane) {
  if (QP_ABL & 4) return;
  const int l = lane & 15;
  double* blk = lds + (lane >> 4) * (QB * QP);
#pragma unroll
  for (int k = 0; k < QB; ++k) swap_lane_rows(v[k], v[QB + k]);
#pragma unroll
  for (int g = 0; g < 2; ++g) {
#pragma unroll
    for (int k = 0; k < QB; ++k) blk[k * QP + l] = v[g * QB + k];
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < QB; ++k) v[g * QB + k] = blk[l * QP + k];
    wave_lds_fence();
  }
}

// reduced right-hand sides next to chunk p of `line` (always in bounds: rows 0 and 2P+1 exist and hold zeros)
__device__ __forceinline__ GhostRaw fine_ghost_prefetch(const FineView& v, int dir, int b, int p, long line) {
  const int P = dir == 0 ? v.px : v.py;
  const long nlines = dir == 0 ? v.ny : v.nx;
  const double* ir = v.iface[dir] + (long)b * (2 * P + 2) * nlines + line;
  GhostRaw g;
  if (QP_ABL & 1) { g.q0 = g.q1 = g.q2 = g.q3 = 0.0; return g; }
  g.q0 = ir[(long)(2 * p) * nlines];
  g.q1 = ir[(long)(2 * p + 1) * nlines];
  g.q2 = ir[(long)(2 * p + 2) * nlines];
  g.q3 = ir[(long)(2 * p + 3) * nlines];
  return g;
}

// the two 2 x 2 interface systems of chunk p (see ghost_finish): gl = E_{p-1}, gr = F_{p+1}
__device__ __forceinline__ void fine_ghost_finish(const FineView& v, int dir, int b, int p, const GhostRaw& g, double& gl,
                                                  double& gr) {
  const int P = dir == 0 ? v.px : v.py;
  const ctab_t ic = as_const(v.icoef[dir] + (long)b * (P + 1) * 3);
  gl = 0.0;
  gr = 0.0;
  if (p > 0) gl = fma(ic[p * 3], g.q1, g.q0) * ic[p * 3 + 2];
  if (p < P - 1) gr = fma(ic[(p + 1) * 3 + 1], g.q2, g.q3) * ic[(p + 1) * 3 + 2];
}

template <int STREAM>
__device__ __forceinline__ void fine_load_rows(const double* __restrict__ p, long pitch, double (&v)[FS]) {
  if (STREAM & 1) {
#pragma unroll
    for (int r = 0; r < FS; ++r) v[r] = __builtin_nontemporal_load(p + (long)r * pitch);
  } else {
#pragma unroll
    for (int r = 0; r < FS; ++r) v[r] = p[(long)r * pitch];
  }
}

template <int STREAM>
__device__ __forceinline__ void fine_store_rows(double* __restrict__ p, long pitch, const double (&v)[FS]) {
  if (STREAM & 2) {
#pragma unroll
    for (int r = 0; r < FS; ++r) __builtin_nontemporal_store(v[r], p + (long)r * pitch);
  } else {
#pragma unroll
    for (int r = 0; r < FS; ++r) p[(long)r * pitch] = v[r];
  }
}

// Block -> (64 x 64 super-tile, half).  The two y-tiles and the two x-tiles of a super-tile are given to blocks with the
// same blockIdx % 8, i.e. (blocks are dealt round-robin over the 8 XCDs) to the same XCD in every launch: what one pass
// wrote is then still in that XCD's L2 when the next pass reads it.  Measured on the bare access pattern
// (tools/tile_xcd.hip): 4.1 against 6.8 us at 1024^2, 9.5 against 13.9 us at 2048^2; no effect once the plane exceeds the
// 32 MiB of L2.  (The 64 x 64 kernels have this property for free: both directions use the same tile.)  Speed only - any
// bijection is correct, and the last, partial group of super-tiles simply loses the alignment.
struct FineBlock {
  int b, sty, stx, sub;
};
__device__ __forceinline__ FineBlock fine_block(const FineView& v) {
  const int nsx = v.nx / 64, nsy = v.ny / 64;
  const int ns = v.nfield * nsy * nsx;           // super-tiles; the grid has 2 ns blocks
  const int bid = blockIdx.x;
  const int group = bid >> 4, r = bid & 15;
  const int m = min(8, ns - group * 8);          // super-tiles of this group (8 except in the last one)
  int S = group * 8 + r % m;
  FineBlock f;
  f.sub = r / m;
  f.stx = S % nsx;
  S /= nsx;
  f.sty = S % nsy;
  f.b = S / nsy;
  return f;
}

// x-kernel tile: x-chunk tx x rows [64 ty, 64 ty + 64) of field b (fine_block).  Wave-uniform tile origin + a 32-bit lane
// offset (half-wave h starts 32 rows further down).
struct FineXTile {
  int b, tx, ty;
  long origin;       // element offset of the tile's first cell in a [nfield][ny*nx] plane
  unsigned off;
};
__device__ __forceinline__ FineXTile fine_x_tile(const FineView& v) {
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  const FineBlock fb = fine_block(v);
  FineXTile t;
  t.tx = 2 * fb.stx + fb.sub;          // x-chunk (32 columns)
  t.ty = fb.sty;                       // pair of y-chunks (64 rows)
  t.b = fb.b;
  t.origin = (long)t.b * ((long)v.ny * v.nx) + (long)(t.ty * 64) * v.nx + t.tx * FS;
  t.off = (unsigned)(h * FS) * (unsigned)v.nx + (unsigned)c;
  return t;
}

// sources of the y-faces (up/down) belong to rows 0 and ny-1
__device__ __forceinline__ double fine_row_source(const FineView& v, double a, int row) {
  double srow = 0.0;
  if (row == 0) srow += a * v.other_src[1][0];
  if (row == v.ny - 1) srow += a * v.other_src[1][1];
  return srow;
}

struct FineNoHook {
  __device__ __forceinline__ void operator()() const {}
};

// Front half of every x-kernel tile: x-solve from rhs1 at `tile`, explicit x-operator (EXPLICIT), source plane (SRC), and
// the transpose back - on return lane (h, c) holds y-chunk 2 ty + h of column 32 tx + c, register r = row 64 ty + 32 h + r.
// parts[0] is the x-solve table; every part is warmed in the scalar cache while the rows are in flight.  `hook` runs right
// after the row loads are issued (work on values loaded before them, without waiting for the rows).
template <bool EXPLICIT, int STREAM, bool SRC, int NPART, class Hook = FineNoHook>
__device__ __forceinline__ void fine_x_front(const FineView& v, const FineXTile& t, const double* tile,
                                             const CoefFine (&parts)[NPART], double* lds, double (&e)[FS],
                                             const Hook& hook = Hook()) {
  const int lane = threadIdx.x;
  const int tx = t.tx, ty = t.ty, b = t.b;
  const unsigned off = t.off;
  const long ncell = (long)v.ny * v.nx;
  const double a = as_const(v.alpha)[b];
  const int row = ty * 64 + lane;      // lane = row between the transposes
  const GhostRaw graw = fine_ghost_prefetch(v, 0, b, tx, row);
  const CoefFine cx = parts[0];
  fine_load_rows<STREAM>(tile + off, v.nx, e);
  warm_scalar_cache(parts);
  hook();
  transpose32h(e, lds, lane);
  double gl, gr;
  fine_ghost_finish(v, 0, b, tx, graw, gl, gr);
  e[0] = fma(a, gl, e[0]);
  e[FS - 1] = fma(a, gr, e[FS - 1]);
  thomas32(e, cx);
  const double srow = fine_row_source(v, a, row);
  if (EXPLICIT) explicit32(e, gl, gr, cx, a, srow);
  double bv[SRC ? FS : 1];
  if (SRC) {                           // the source tile, in the storage layout: issued here, consumed after the transpose
    const double* bt = v.bsrc + (long)b * ncell + (long)(ty * 64) * v.nx + tx * FS + off;
#pragma unroll
    for (int r = 0; r < FS; ++r) bv[SRC ? r : 0] = bt[(long)r * v.nx];
  }
  transpose32h(e, lds, lane);
  if (SRC) {
#pragma unroll
    for (int r = 0; r < FS; ++r) e[r] = fma(v.bscale, bv[SRC ? r : 0], e[r]);
  }
}

// y-elimination of the two y-chunks the x-kernel tile holds after fine_x_front -> iface1 (in the layout of v.iface[1])
__device__ __forceinline__ void fine_x_ends(const FineView& v, const FineXTile& t, const double (&e)[FS], double* iface1) {
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  double yf, yl;
  ends32_pair(e, v, 1, t.b, 2 * t.ty, v.py, h, yf, yl);
  double* ir = iface1 + (long)t.b * (2 * v.py + 2) * v.nx + t.tx * FS + c;
  const int yc = 2 * t.ty + h;
  ir[(long)(2 * yc + 1) * v.nx] = yf;
  ir[(long)(2 * yc + 2) * v.nx] = yl;
}

__device__ __forceinline__ void fine_x_warm_parts(const FineView& v, const FineXTile& t, CoefFine (&parts)[3]) {
  parts[0] = fine_coefs(v, 0, t.b, chunk_variant(t.tx, v.px), 0);
  parts[1] = fine_coefs(v, 1, t.b, chunk_variant(2 * t.ty, v.py), 1);
  parts[2] = fine_coefs(v, 1, t.b, chunk_variant(2 * t.ty + 1, v.py), 1);
}

// x-kernel: finish the x-solve, apply the explicit x-operator, eliminate along y.   buf: rhs1 -> rhs2 in place
template <bool EXPLICIT, int STREAM, bool SRC = false>
__global__ void __launch_bounds__(64) QP_WAVES_ATTR fine_x_kernel(FineView v, double* __restrict__ buf) {
  __shared__ double lds[FINE_LDS_DOUBLES];
  FineXTile t = fine_x_tile(v);
  double* tile = buf + t.origin;
  CoefFine parts[3];
  fine_x_warm_parts(v, t, parts);
  double e[FS];
  fine_x_front<EXPLICIT, STREAM, SRC>(v, t, tile, parts, lds, e);
  asm volatile("" : "+v"(t.off));      // the 32 row addresses are formed again here instead of living through the solve
  fine_store_rows<STREAM>(tile + t.off, v.nx, e);
  if (QP_ABL & 8) return;
  fine_x_ends(v, t, e, v.iface[1]);
}

// Reduce pass R of a fused ADI step (qp_adi_rect_steps): the x-kernel without its plane store - rhs1 is only read, and
// what leaves the tile is the y-elimination of the rhs2 it holds (iface[1]).  fine_fused_kernel then forms the same rhs2
// again (same code, same bits) and finishes the step with it.
template <int STREAM>
__global__ void __launch_bounds__(64) QP_WAVES_ATTR fine_reduce_kernel(FineView v, const double* __restrict__ buf) {
  __shared__ double lds[FINE_LDS_DOUBLES];
  const FineXTile t = fine_x_tile(v);
  CoefFine parts[3];
  fine_x_warm_parts(v, t, parts);
  double e[FS];
  fine_x_front<true, STREAM, false>(v, t, buf + t.origin, parts, lds, e);
  if (QP_ABL & 8) return;
  fine_x_ends(v, t, e, v.iface[1]);
}

// sources of the x-faces (left/right) belong to columns 0 and nx-1
__device__ __forceinline__ double fine_col_source(const FineView& vn, double an, int col) {
  double scol = 0.0;
  if (col == 0) scol += an * vn.other_src[0][0];
  if (col == vn.nx - 1) scol += an * vn.other_src[0][1];
  return scol;
}

// Middle of a y-pass on one y-chunk per lane (lane = column, register = row), shared by fine_y_body and
// fine_fused_kernel; the ghosts gu / gd are finished.  `before_store` runs between the last arithmetic and the stores.  MODE 1 / 2: the y-solve; MODE 2 stores the solution and stops.
// MODE 0 / 1: the explicit y-operator (table cyn, weight an, column source scol), the source plane (SRC: bscale * bt),
// and the store.  MODE 3 does nothing here.
template <int MODE, int STREAM, bool SRC, class CoefY, class CoefYN, class Hook = FineNoHook>
__device__ __forceinline__ void fine_y_mid(double (&e)[FS], double gu, double gd, double a, const CoefY& cy, double an,
                                           const CoefYN& cyn, double scol, double bscale, const double* bt, double* dp,
                                           long pitch, const Hook& before_store = Hook()) {
  if (MODE == 1 || MODE == 2) {
    e[0] = fma(a, gu, e[0]);
    e[FS - 1] = fma(a, gd, e[FS - 1]);
    thomas32(e, cy);
  }
  if (MODE == 2) {
    fine_store_rows<STREAM>(dp, pitch, e);
    return;
  }
  if (MODE != 3) {
    explicit32(e, gu, gd, cyn, an, scol);
    if (SRC) {
#pragma unroll
      for (int r = 0; r < FS; ++r) e[r] = fma(bscale, bt[(long)r * pitch], e[r]);
    }
    before_store();      // loads whose values are wanted after the stores: a load issued behind them waits for all of them
    fine_store_rows<STREAM>(dp, pitch, e);
  }
}

// y-kernel, MODE as in rect_y_kernel (0 entry, 1 carry, 2 exit, 3 reduce).  `vn` is the view whose x-solve comes next: the
// same view, except in the carried Peaceman-Rachford cycle (NEXT), where the y-solve belongs to parameter p_j and the
// right-hand side it leaves (explicit operator, source scale, x-elimination, interface rows) to p_{j+1}.
template <int MODE, int STREAM, bool SRC, bool NEXT>
__device__ __forceinline__ void fine_y_body(const FineView& v, const FineView& vn, const double* src, double* dst,
                                            double* lds) {
  const int lane = threadIdx.x, h = lane >> 5;
  const FineBlock fb = fine_block(v);
  const int tx = fb.stx;               // pair of x-chunks (64 columns)
  const int ty = 2 * fb.sty + fb.sub;  // y-chunk (32 rows)
  const int b = fb.b;
  const long ncell = (long)v.ny * v.nx;
  const double a = as_const(v.alpha)[b];
  const int col = tx * 64 + lane;
  const int j0 = ty * FS;
  GhostRaw graw;
  if (MODE == 1 || MODE == 2) graw = fine_ghost_prefetch(v, 1, b, ty, col);
  const CoefFine cy = fine_coefs(v, 1, b, chunk_variant(ty, v.py), 0);
  const CoefFine cyn = NEXT ? fine_coefs(vn, 1, b, chunk_variant(ty, v.py), 0) : cy;
  const double an = NEXT ? as_const(vn.alpha)[b] : a;
  const double* sp = src + (long)b * ncell + (long)j0 * v.nx + col;
  double* dp = dst + (long)b * ncell + (long)j0 * v.nx + col;
  double gu = 0.0, gd = 0.0;           // values of the field just above / below the tile
  if (MODE == 0) {
    if (ty > 0) gu = sp[-(long)v.nx];
    if (ty < v.py - 1) gd = sp[(long)FS * v.nx];
  }
  double e[FS];
  fine_load_rows<STREAM>(sp, v.nx, e);
  if (MODE == 2) {
    const CoefFine parts[1] = {cy};
    warm_scalar_cache(parts);
  } else if (NEXT) {
    const CoefFine parts[4] = {cy, cyn, fine_coefs(vn, 0, b, chunk_variant(2 * tx, v.px), 1),
                               fine_coefs(vn, 0, b, chunk_variant(2 * tx + 1, v.px), 1)};
    warm_scalar_cache(parts);
  } else {
    const CoefFine parts[3] = {cy, fine_coefs(v, 0, b, chunk_variant(2 * tx, v.px), 1),
                               fine_coefs(v, 0, b, chunk_variant(2 * tx + 1, v.px), 1)};
    warm_scalar_cache(parts);
  }
  if (MODE == 1 || MODE == 2) fine_ghost_finish(v, 1, b, ty, graw, gu, gd);
  const double* bt = SRC ? vn.bsrc + (long)b * ncell + (long)j0 * v.nx + col : nullptr;
  fine_y_mid<MODE, STREAM, SRC>(e, gu, gd, a, cy, an, cyn, fine_col_source(vn, an, col), vn.bscale, bt, dp, v.nx);
  if (MODE == 2) return;
  if (QP_ABL & 8) return;
  transpose32h(e, lds, lane);          // lane = (x-chunk 2 tx + h, row j0 + (lane & 31)), register = column of the chunk
  double yf, yl;
  ends32_pair(e, vn, 0, b, 2 * tx, v.px, h, yf, yl);
  double* ir = vn.iface[0] + (long)b * (2 * v.px + 2) * v.ny + j0 + (lane & 31);
  const int xc = 2 * tx + h;
  ir[(long)(2 * xc + 1) * v.ny] = yf;
  ir[(long)(2 * xc + 2) * v.ny] = yl;
}

template <int MODE, int STREAM, bool SRC = false>
__global__ void __launch_bounds__(64) QP_WAVES_ATTR fine_y_kernel(FineView v, const double* src, double* dst) {   // src may alias dst
  __shared__ double lds[FINE_LDS_DOUBLES];
  fine_y_body<MODE, STREAM, SRC, false>(v, v, src, dst, lds);
}

// carried Peaceman-Rachford cycle: y-solve of parameter p_j (view v), right-hand side of the x-solve of p_{j+1} (view vn)
template <int STREAM>
__global__ void __launch_bounds__(64) QP_WAVES_ATTR fine_y_next_kernel(FineView v, FineView vn, double* w) {
  __shared__ double lds[FINE_LDS_DOUBLES];
  fine_y_body<1, STREAM, true, true>(v, vn, w, w, lds);
}

// Fused pass F of an ADI step (qp_adi_rect_steps on a fused plan), MODE 1 carry / 2 exit, on the x-kernel tile:
//   fine_x_front again from rhs1 (the x-solve of fine_reduce_kernel, same bits), then the y-work of fine_y_kernel<MODE> on
//   the y-chunk every lane holds (chunk 2 ty + h of column 32 tx + c), its ghosts from the iface[1] that R left;
//   MODE 1: explicit y-operator, rhs1' stored in place, transposed once more and the x-elimination of x-chunk tx into
//           iface0_next (the other buffer of the x-interface pair: the neighbouring tiles still read v.iface[0]);
//   MODE 2: the solution stored to dst.
// One read and one write of the plane per step where the two sweeps move two of each.
struct CoefFinePair {       // chunk p_even on lanes 0..31, chunk p_even + 1 on lanes 32..63 (tiles at the ends of a line)
  ctab_t lo, hi;
  bool h;
  __device__ __forceinline__ double at(int slot, int k) const {
    if (QP_ABL & 2) return 0.1 + 0.001 * slot;
    const double x = lo[cidx_len(FS, slot, k)], y = hi[cidx_len(FS, slot, k)];
    return h ? y : x;
  }
};

// fine_ghost_finish for chunk p_even + h on half-wave h (same coefficients, same operations, per-lane selects)
__device__ __forceinline__ void fine_ghost_finish_pair(const FineView& v, int dir, int b, int p_even, int h,
                                                       const GhostRaw& g, double& gl, double& gr) {
  const int P = dir == 0 ? v.px : v.py;
  const ctab_t ic = as_const(v.icoef[dir] + (long)b * (P + 1) * 3);
  const int p = p_even + h;
  const double l0 = h ? ic[(p_even + 1) * 3] : ic[p_even * 3];
  const double l2 = h ? ic[(p_even + 1) * 3 + 2] : ic[p_even * 3 + 2];
  const double r1 = h ? ic[(p_even + 2) * 3 + 1] : ic[(p_even + 1) * 3 + 1];
  const double r2 = h ? ic[(p_even + 2) * 3 + 2] : ic[(p_even + 1) * 3 + 2];
  gl = 0.0;
  gr = 0.0;
  if (p > 0) gl = fma(l0, g.q1, g.q0) * l2;
  if (p < P - 1) gr = fma(r1, g.q2, g.q3) * r2;
}

// One-pass steps (fine_steps_onepass, DESIGN.md 2.2).  The x-front is linear in the two x-ghosts, so the y-interface rows
// of the next step are P + phi_L[c] S_gl + phi_R[c] S_gr: P is the x-front and y-elimination of rhs1' with zero x-ghosts,
// formed by the one-pass kernel from the rhs1' it holds; S are the y-eliminations of the ghosts themselves, four scalars
// per (field, x-chunk, y-chunk).  The ghosts are linear in the x-interface values yf / yl, so every tile leaves the
// y-eliminations T of the yf / yl it has just formed (fine_tile_sums, while they are in registers) and
// fine_ghostsum_kernel combines the T of an x-chunk and its two neighbours into S once all tiles are done.
struct FineOnePass {
  const double* phi;     // [nfield][3 x-chunk variants][2][FS]: x-front response of column c to gl = 1 (phi_L), gr = 1 (phi_R)
  const double* sums;    // [nfield][px][py][4] S = (ends_f gl, ends_l gl, ends_f gr, ends_l gr) of this step (zeros: none)
  double* p_next;        // P of the next step, in the layout of iface[1]
  const double* wy;      // [nfield][3 y-chunk variants][2][FS] first / last rows of A_y^-1 (fine_plan_prepare)
  double* tsums;         // [nfield][px][py][4] T = (ends_f yf, ends_l yf, ends_f yl, ends_l yl) of the next step's x-rows
  const double* xmap;    // [nfield][3 x-chunk variants][FS c'][FS c] zero-ghost x-front of the unit vector e_c', no sources
  const double* pbias;   // [nfield][3 x-chunk variants][3 y-chunk variants][2][FS] P of an all-zero tile (the sources)
};

// what q0..q3 of y-chunk yc at column c of x-chunk tx add to P: phi_L / phi_R of the column and S of the chunks yc - 1
// (last entry), yc (both) and yc + 1 (first entry)
struct FineGhostSums {
  double fl, fr, s[8];
};

__device__ __forceinline__ FineGhostSums fine_ghost_sums_prefetch(const FineView& v, const FineOnePass& op, int b, int tx,
                                                                  int yc, int c) {
  FineGhostSums r;
  const double* ph = op.phi + ((long)b * 3 + chunk_variant(tx, v.px)) * 2 * FS + c;
  r.fl = ph[0];
  r.fr = ph[FS];
  const double* s = op.sums + (((long)b * v.px + tx) * v.py + yc) * 4;
  const double* sa = s + (yc > 0 ? -4 : 0);              // clamped at the ends of a column: rows 0 and 2 py + 1 take none
  const double* sb = s + (yc < v.py - 1 ? 4 : 0);
  r.s[0] = sa[1];
  r.s[1] = sa[3];
#pragma unroll
  for (int i = 0; i < 4; ++i) r.s[2 + i] = s[i];
  r.s[6] = sb[0];
  r.s[7] = sb[2];
  return r;
}

// q0..q3 in P form -> the y-reduced right-hand sides (rows 0 and 2 py + 1 hold zeros and keep them)
__device__ __forceinline__ void fine_ghost_correct(const FineView& v, int yc, const FineGhostSums& r, GhostRaw& g) {
  if (yc > 0) g.q0 = fma(r.fl, r.s[0], fma(r.fr, r.s[1], g.q0));
  g.q1 = fma(r.fl, r.s[2], fma(r.fr, r.s[4], g.q1));
  g.q2 = fma(r.fl, r.s[3], fma(r.fr, r.s[5], g.q2));
  if (yc < v.py - 1) g.q3 = fma(r.fl, r.s[6], fma(r.fr, r.s[7], g.q3));
}

// T of (field b, x-chunk tx, y-chunk yc = 2 ty + h): lane = row 64 ty + lane holds yf / yl of its row and the weights
// wf / wl of row k = lane & 31 of its y-chunk.  The four products are summed over each half-wave by the 5-level xor
// butterfly in its halving form: at distance 16 a lane keeps the two sums its bit 4 selects and hands the other two over,
// at distance 8 likewise one of two by bit 3 - the same pairwise additions in the same tree, 6 shuffles instead of 20 -
// and every lane of the group k / 8 = i ends with entry i.  All eight store it (one address per group, the same value): a
// store under a lane mask costs the one-pass kernel its third wave per SIMD (see fine_onepass_kernel).
__device__ __forceinline__ void fine_tile_sums(const FineView& v, int b, int tx, int yc, int k, double wf, double wl,
                                               double yf, double yl, double* tsums) {
  const bool hi16 = (k & 16) != 0, hi8 = (k & 8) != 0;
  const double s0 = wf * yf, s1 = wl * yf, s2 = wf * yl, s3 = wl * yl;
  double a0 = hi16 ? s2 : s0, a1 = hi16 ? s3 : s1;
  a0 += __shfl_xor(hi16 ? s0 : s2, 16);
  a1 += __shfl_xor(hi16 ? s1 : s3, 16);
  double a = hi8 ? a1 : a0;
  a += __shfl_xor(hi8 ? a0 : a1, 8);
#pragma unroll
  for (int m = 4; m >= 1; m >>= 1) a += __shfl_xor(a, m);
  tsums[(((long)b * v.px + tx) * v.py + yc) * 4 + (k >> 3)] = a;
}

// P of the next step from the y-eliminations (rf, rl) of rhs1': lane (h, c) formed those of column 32 tx + c over the rows
// of y-chunk yc = 2 ty + h.  The zero-ghost x-front acts along the columns and is the same affine map for every row up to
// its row source, the y-elimination is one linear form over the rows for every column, so the two commute:
//   P_f(yc, c) = pbias_f[c] + sum_c' M[c][c'] rf(c')     (likewise _l),
// M = op.xmap (x-front of the unit vectors), pbias = x-front and y-elimination of an all-zero tile (the sources).
// Where the loads sit decides what the tail costs: the wave's vector-memory counter retires in order, so a load issued
// behind the 32 row stores of the plane waits until all of them are acknowledged.  The end-row weights of fine_tile_sums
// and the bias are therefore loaded BEFORE the stores (fine_p_prefetch, from fine_y_mid); the map, which nothing can hold
// through the y-work and the last transpose, right after that transpose (fine_p_prefetch_map), so that its wait overlaps
// ends32 and the tile sums.  To fit the registers free there a lane keeps half a column of the map - lane (h, c) rows
// c' = 16 h .. 16 h + 15 of column c, both half-waves hold the same columns - and forms the partial sums of BOTH y-chunks
// over its 16 rows; the halves then trade the partial sum the other one needs.  The 64 pairs wait in LDS behind the
// transpose patches from the moment they exist.
// The summation order is part of the result: per half c' ascending from zero, then (bias + rows 0..15) + rows 16..31.
struct FinePTail {
  double wf, wl;          // fine_tile_sums: row c of the end rows of y-chunk yc
  double bf, bl;          // pbias of (x-variant, y-variant of yc) at column c
  double m[FS / 2];       // xmap[16 h + k][c]
};

__device__ __forceinline__ void fine_p_prefetch(const FineView& v, const FineXTile& t, const FineOnePass& op, int va, int vb,
                                                unsigned ln, FinePTail& p) {
  const unsigned h = ln >> 5, c = ln & 31;
  const int yvar = h ? vb : va;
  const double* wr = op.wy + ((long)t.b * 3 + yvar) * 2 * FS + c;
  p.wf = wr[0];
  p.wl = wr[FS];
  const long xv = (long)t.b * 3 + chunk_variant(t.tx, v.px);
  const double* bias = op.pbias + ((xv * 3 + yvar) * 2) * FS + c;
  p.bf = bias[0];
  p.bl = bias[FS];
}
__device__ __forceinline__ void fine_p_prefetch_map(const FineView& v, const FineXTile& t, const FineOnePass& op, unsigned ln,
                                                    FinePTail& p) {
  const unsigned h = ln >> 5, c = ln & 31;
  const long xv = (long)t.b * 3 + chunk_variant(t.tx, v.px);
  const double* mt = op.xmap + xv * (FS * FS) + (h * (FS / 2)) * FS + c;
#pragma unroll
  for (int k = 0; k < FS / 2; ++k) p.m[k] = mt[k * FS];
}

__device__ __forceinline__ void fine_p_map(const FineView& v, const FineXTile& t, const FineOnePass& op, unsigned ln,
                                           const FinePTail& p, const double* lds_pairs) {
  const unsigned h = ln >> 5, c = ln & 31;
  const double2* pairs = reinterpret_cast<const double2*>(lds_pairs) + h * (FS / 2);
  double f0 = 0.0, l0 = 0.0, f1 = 0.0, l1 = 0.0;      // partial sums over this half's 16 rows, y-chunks 2 ty and 2 ty + 1
#pragma unroll
  for (int k = 0; k < FS / 2; ++k) {
    const double2 r0 = pairs[k], r1 = pairs[FS + k];
    f0 = fma(p.m[k], r0.x, f0);
    l0 = fma(p.m[k], r0.y, l0);
    f1 = fma(p.m[k], r1.x, f1);
    l1 = fma(p.m[k], r1.y, l1);
  }
  // lane (h, c) keeps the partial sums of its own y-chunk and hands those of the other one to lane (1 - h, c)
  const double gf = __shfl_xor(h ? f0 : f1, 32), gl = __shfl_xor(h ? l0 : l1, 32);
  const double kf = h ? f1 : f0, kl = h ? l1 : l0;
  const double pf = (p.bf + (h ? gf : kf)) + (h ? kf : gf);
  const double pl = (p.bl + (h ? gl : kl)) + (h ? kl : gl);
  double* ir = op.p_next + (long)t.b * (2 * v.py + 2) * v.nx + t.tx * FS + c;
  const int yc = 2 * t.ty + h;
  ir[(long)(2 * yc + 1) * v.nx] = pf;
  ir[(long)(2 * yc + 2) * v.nx] = pl;
}

// The fused pass, and with ONEPASS its one-pass form F': the y-ghosts come from v.iface[1] in P form and op.sums (all
// zeros on the first step, whose rows R left in full), and MODE 1 also forms P of the next step from the rhs1' it holds:
// its y-elimination right after the plane store, where the rows are in the layout of fine_x_ends, and the x-front of
// those two values per lane at the end (fine_p_map) -> op.p_next, and T of the x-interface rows it writes
// (fine_tile_sums) -> op.tsums.
template <int MODE, int STREAM, bool ONEPASS>
__device__ __forceinline__ void fine_fused_body(const FineView& v, double* iface0_next, double* w, double* dst,
                                                const FineOnePass& op, double* lds) {
  static_assert(MODE == 1 || MODE == 2, "fused pass: carry or exit");
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  FineXTile t = fine_x_tile(v);
  const int b = t.b, tx = t.tx, ty = t.ty;
  const int col = tx * FS + c;
  const int yc = 2 * ty + h;           // the y-chunk of this lane after fine_x_front
  const int va = chunk_variant(2 * ty, v.py), vb = chunk_variant(2 * ty + 1, v.py);
  GhostRaw gyraw = fine_ghost_prefetch(v, 1, b, yc, col);
  FineGhostSums gs{};
  if (ONEPASS) gs = fine_ghost_sums_prefetch(v, op, b, tx, yc, c);
  CoefFine parts[4];
  parts[0] = fine_coefs(v, 0, b, chunk_variant(tx, v.px), 0);
  parts[1] = fine_coefs(v, 1, b, va, 0);
  parts[2] = fine_coefs(v, 1, b, vb, 0);
  parts[3] = fine_coefs(v, 0, b, chunk_variant(tx, v.px), 1);
  double e[FS];
  if (ONEPASS) {     // the correction waits for the sums only, not for the rows
    fine_x_front<true, STREAM, false>(v, t, w + t.origin, parts, lds, e, [&]() { fine_ghost_correct(v, yc, gs, gyraw); });
  } else {
    fine_x_front<true, STREAM, false>(v, t, w + t.origin, parts, lds, e);
  }
  const double a = as_const(v.alpha)[b];
  double gu, gd;
  fine_ghost_finish_pair(v, 1, b, 2 * ty, h, gyraw, gu, gd);
  const double scol = fine_col_source(v, a, col);
  asm volatile("" : "+v"(t.off));
  double* dp = dst + t.origin + t.off;
  // One-pass form: what the tail needs from memory is loaded between the y-work and the plane stores (fine_p_prefetch), and
  // everything the lane needs from there on (LDS patch, interface rows) is formed again from the lane index instead of
  // living through the y-work - at the edge of three waves per SIMD that decides between no scratch and a spilled column.
  FinePTail pt{};
  int ln = lane;
  auto prefetch = [&]() {
    if (ONEPASS && MODE == 1) {
      asm volatile("" : "+v"(ln) : "v"(e[FS - 1]));      // not before the y-work is done
      if (!(QP_ABL & 128)) fine_p_prefetch(v, t, op, va, vb, (unsigned)ln, pt);
      else {
        const double* wr = op.wy + ((long)b * 3 + ((ln >> 5) ? vb : va)) * 2 * FS + (ln & 31);
        pt.wf = wr[0];
        pt.wl = wr[FS];
      }
    }
  };
  if (va == vb) {                      // wave-uniform: interior tile rows
    fine_y_mid<MODE, STREAM, false>(e, gu, gd, a, parts[1], a, parts[1], scol, 0.0, nullptr, dp, v.nx, prefetch);
  } else {
    const CoefFinePair cy{parts[1].part, parts[2].part, h != 0};
    fine_y_mid<MODE, STREAM, false>(e, gu, gd, a, cy, a, cy, scol, 0.0, nullptr, dp, v.nx, prefetch);
  }
  if (MODE == 2) return;
  if (QP_ABL & 8) return;
  const int hn = ln >> 5, cn = ln & 31;
  if (ONEPASS && !(QP_ABL & 128)) {    // y-elimination of the rhs1' this lane holds, parked in LDS for fine_p_map
    double rf, rl;
    ends32_pair(e, v, 1, b, 2 * ty, v.py, hn, rf, rl);
    reinterpret_cast<double2*>(lds + FINE_LDS_DOUBLES)[ln] = make_double2(rf, rl);
  }
  transpose32h(e, lds, ln);            // lane = row 64 ty + lane, register = column of x-chunk tx
  if (ONEPASS && !(QP_ABL & 128)) {    // the half column of the map: issued here, where 32 registers are free to hold it
    unsigned l2 = ln;
    asm volatile("" : "+v"(l2) : "v"(e[0]));
    fine_p_prefetch_map(v, t, op, l2, pt);
  }
  double yf, yl;
  ends32(e, parts[3], yf, yl);
  double* ir = iface0_next + (long)b * (2 * v.px + 2) * v.ny + ty * 64 + ln;
  ir[(long)(2 * tx + 1) * v.ny] = yf;
  ir[(long)(2 * tx + 2) * v.ny] = yl;
  if (ONEPASS) {     // T of these rows, then P of the next step
    fine_tile_sums(v, b, tx, 2 * ty + hn, cn, pt.wf, pt.wl, yf, yl, op.tsums);
    if (QP_ABL & 128) return;
    fine_p_map(v, t, op, (unsigned)ln, pt, lds + FINE_LDS_DOUBLES);
  }
}

template <int MODE, int STREAM>
__global__ void __launch_bounds__(64) QP_WAVES_ATTR fine_fused_kernel(FineView v, double* iface0_next, double* w,
                                                                      double* dst) {   // dst == w in MODE 1
  __shared__ double lds[FINE_LDS_DOUBLES];
  fine_fused_body<MODE, STREAM, false>(v, iface0_next, w, dst, FineOnePass{}, lds);
}

// One-pass step F' (MODE 1) and the exit pass of one-pass steps (MODE 2).  F' with the tile sums sits at the edge of three
// waves per SIMD (168 VGPRs): left to itself the scheduler gives the third wave up (174 VGPRs); held to three it
// allocates 167 without scratch.  The exit pass (132 VGPRs) is not affected.
#ifdef QP_FORCE_WAVES
#define QP_ONEPASS_WAVES_ATTR QP_WAVES_ATTR
#else
#define QP_ONEPASS_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(3)))
#endif
template <int MODE, int STREAM>
__global__ void __launch_bounds__(64) QP_ONEPASS_WAVES_ATTR fine_onepass_kernel(FineView v, double* iface0_next, double* w,
                                                                        double* dst, FineOnePass op) {
  // MODE 1: 64 pairs behind the transpose patches (FINE_LDS_PAIRS), written before the last transpose, read after it
  __shared__ __attribute__((aligned(16))) double lds[FINE_LDS_DOUBLES + (MODE == 1 ? FINE_LDS_PAIRS : 0)];
  fine_fused_body<MODE, STREAM, true>(v, iface0_next, w, dst, op, lds);
}

// Ghost-sum pass X of the one-pass steps: one thread per (field, x-chunk tx, y-chunk q) combines T of tx - 1, tx and
// tx + 1 (fine_tile_sums of the pass before) into S = (ends_f gl, ends_l gl, ends_f gr, ends_l gr) with the interface
// coefficients of fine_ghost_finish: gl = (ic0 yf(tx) + yl(tx - 1)) ic2 and gr = (ic1' yl(tx) + yf(tx + 1)) ic2' row by
// row, hence the same combination of their y-eliminations; no ghost beyond the first / last x-chunk.
__global__ void __launch_bounds__(256) fine_ghostsum_kernel(FineView v, const double* __restrict__ tsums,
                                                            double* __restrict__ sums) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // ((b px) + tx) py + q
  if (i >= v.nfield * v.px * v.py) return;
  const int r = i / v.py, tx = r % v.px, b = r / v.px;
  const double* ic = v.icoef[0] + ((long)b * (v.px + 1) + tx) * 3;
  const double2* t = reinterpret_cast<const double2*>(tsums) + 2 * (long)i;
  const double2 tf = t[0], tl = t[1];                // (ends_f, ends_l) of yf and of yl
  double2 sl = make_double2(0.0, 0.0), sr = sl;
  if (tx > 0) {
    const double2 pl = t[1 - 2 * (long)v.py];        // yl of x-chunk tx - 1
    sl.x = fma(ic[0], tf.x, pl.x) * ic[2];
    sl.y = fma(ic[0], tf.y, pl.y) * ic[2];
  }
  if (tx < v.px - 1) {
    const double2 nf = t[2 * (long)v.py];            // yf of x-chunk tx + 1
    sr.x = fma(ic[4], tl.x, nf.x) * ic[5];
    sr.y = fma(ic[4], tl.y, nf.y) * ic[5];
  }
  double2* s = reinterpret_cast<double2*>(sums) + 2 * (long)i;
  s[0] = sl;
  s[1] = sr;
}
