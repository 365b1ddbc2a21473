// Custom generation expressions g(E, x, y, t, params) evaluated on the device (qpsim_hip.h).
//
// Limits (qpsim_hip.h): QP_EXPR_MAX_WORDS = 64 instruction words, QP_EXPR_MAX_REGS = 8 live temporaries,
// QP_EXPR_MAX_SLOTS = 16 host-evaluated values per energy bin.  The host compiler (qpsim_amd/device_expr.py) refuses an
// expression beyond them, and the entry points below check every word again before anything is launched.
//
// The program is wave-uniform: the instruction words are a kernel argument passed by value (scalar loads from the
// kernarg segment), the slots of the block's energy bin are read through a uniform index (scalar loads), and every branch
// of the interpreter depends on those alone.  The temporaries are eight named doubles picked by a switch on the uniform
// register number - no runtime-indexed private array, so nothing goes to scratch (private segment size 0).
#include <math.h>

#include "qp_common.h"

namespace qp {

struct ExprWords {
  uint32_t w[QP_EXPR_MAX_WORDS];
};

struct ExprRegs {
  double r0, r1, r2, r3, r4, r5, r6, r7;
};

__host__ __device__ inline double expr_operand(unsigned k, const ExprRegs& r, double x, double y, const double* slots) {
  if (k >= (unsigned)QP_EXPR_SLOT0) return slots[k - QP_EXPR_SLOT0];
  switch (k) {
    case 0: return r.r0;
    case 1: return r.r1;
    case 2: return r.r2;
    case 3: return r.r3;
    case 4: return r.r4;
    case 5: return r.r5;
    case 6: return r.r6;
    case 7: return r.r7;
    case QP_EXPR_X: return x;
    default: return y;
  }
}

// One instruction on its operand values.  No contraction in here: a product feeding a sum stays two roundings, as in NumPy.
__host__ __device__ inline double expr_apply(unsigned op, double a, double b, double c) {
#pragma clang fp contract(off)
  switch (op) {
    case QP_OP_COPY: return a;
    case QP_OP_NEG: return -a;
    case QP_OP_ADD: return a + b;
    case QP_OP_SUB: return a - b;
    case QP_OP_MUL: return a * b;
    case QP_OP_DIV: return a / b;
    case QP_OP_POW: return pow(a, b);
    case QP_OP_SQUARE: return a * a;
    case QP_OP_SQRT: return sqrt(a);
    case QP_OP_RECIP: return 1.0 / a;
    case QP_OP_ABS: return fabs(a);
    case QP_OP_MAX: return (a >= b || a != a) ? a : b;      // np.maximum: a NaN on either side comes out
    case QP_OP_MIN: return (a <= b || a != a) ? a : b;
    case QP_OP_WHERE: return c != 0.0 ? a : b;
    case QP_OP_HEAVISIDE: return a != a ? a : (a == 0.0 ? b : (a < 0.0 ? 0.0 : 1.0));
    case QP_OP_LT: return a < b ? 1.0 : 0.0;
    case QP_OP_LE: return a <= b ? 1.0 : 0.0;
    case QP_OP_GT: return a > b ? 1.0 : 0.0;
    case QP_OP_GE: return a >= b ? 1.0 : 0.0;
    case QP_OP_EQ: return a == b ? 1.0 : 0.0;
    case QP_OP_NE: return a != b ? 1.0 : 0.0;
    case QP_OP_EXP: return exp(a);
    case QP_OP_LOG: return log(a);
    case QP_OP_LOG10: return log10(a);
    case QP_OP_SIN: return sin(a);
    case QP_OP_COS: return cos(a);
    case QP_OP_TAN: return tan(a);
    case QP_OP_ASIN: return asin(a);
    case QP_OP_ACOS: return acos(a);
    case QP_OP_ATAN: return atan(a);
    case QP_OP_SINH: return sinh(a);
    case QP_OP_COSH: return cosh(a);
    case QP_OP_TANH: return tanh(a);
    default: return __builtin_nan("");
  }
}

// g at (x, y) for the bin whose slots are `slots`: the value the last word writes.
__host__ __device__ inline double expr_eval(const uint32_t* words, int nword, const double* slots, double x, double y) {
  ExprRegs r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double v = 0.0;
  for (int i = 0; i < nword; ++i) {
    const uint32_t w = words[i];
    const unsigned op = w & 0xffu, dst = (w >> 8) & 0xfu;
    const double a = expr_operand((w >> 12) & 0x3fu, r, x, y, slots);
    double b = 0.0, c = 0.0;
    if (op == QP_OP_WHERE) c = expr_operand((w >> 24) & 0x3fu, r, x, y, slots);
    if ((op >= QP_OP_ADD && op <= QP_OP_POW) || (op >= QP_OP_MAX && op <= QP_OP_NE))
      b = expr_operand((w >> 18) & 0x3fu, r, x, y, slots);
    v = expr_apply(op, a, b, c);
    switch (dst) {
      case 0: r.r0 = v; break;
      case 1: r.r1 = v; break;
      case 2: r.r2 = v; break;
      case 3: r.r3 = v; break;
      case 4: r.r4 = v; break;
      case 5: r.r5 = v; break;
      case 6: r.r6 = v; break;
      default: r.r7 = v; break;
    }
  }
  return v;
}

__host__ __device__ inline double pixel_centre(int index, int extent_full) {
#pragma clang fp contract(off)
  return ((double)index + 0.5) / (double)extent_full;
}

// block = 256 cells of one (bin, listed member) plane: blockIdx.y = bin, blockIdx.z = position in the member list
__global__ void __launch_bounds__(256) add_generation_expr_kernel(
    ExprWords words, int nword, const double* __restrict__ slots, int nslot, int ny, int nx, int ny_full, int nx_full,
    int row0, int col0, const uint8_t* __restrict__ flags, long members, const int32_t* __restrict__ member_ids,
    double* __restrict__ state, double dt, uint32_t* __restrict__ status) {
  const long ncm = (long)ny * nx;
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long bin = blockIdx.y;
  const long m = member_ids ? (long)member_ids[blockIdx.z] : (long)blockIdx.z;
  if (m < 0 || m >= members || c >= ncm) return;
  if (!(flags[m * ncm + c] & QP_FLAG_ACTIVE)) return;      // holes are neither evaluated nor written
  const int row = (int)(c / nx), col = (int)(c - (long)row * nx);
  const double x = pixel_centre(col0 + col, nx_full);
  const double y = pixel_centre(row0 + row, ny_full);
  const double g = expr_eval(words.w, nword, slots + bin * nslot, x, y);
  const long at = (bin * members + m) * ncm + c;
  state[at] += dt * g;                                      // same form as add_scaled_kernel (qp_misc.hip)
  const bool nonfinite = !__builtin_isfinite(g), negative = g < 0.0;
  if (nonfinite) atomicOr(&status[0], 1u);
  if (negative) atomicOr(&status[1], 1u);
}

// Every word of a program against the limits: ops known, destinations in range, operands either x, y, a slot below
// `nslot` or a register an earlier word wrote.
static int validate_program(const qp_generation_program* p, const char* who) {
  if (!p) { set_error("%s: NULL program", who); return QP_ERR_INVALID_ARGUMENT; }
  if (p->struct_size != sizeof(qp_generation_program)) {
    set_error("%s: qp_generation_program.struct_size is %u but this library was built with %zu: the binding and the "
              "library come from different header revisions", who, p->struct_size, sizeof(qp_generation_program));
    return QP_ERR_INVALID_ARGUMENT;
  }
  if (p->ny <= 0 || p->nx <= 0 || p->ne <= 0) { set_error("%s: ny, nx, ne must be positive", who); return QP_ERR_INVALID_ARGUMENT; }
  if (p->row0 < 0 || p->col0 < 0 || (long)p->row0 + p->ny > p->ny_full || (long)p->col0 + p->nx > p->nx_full) {
    set_error("%s: the device grid does not lie inside the full mask", who);
    return QP_ERR_INVALID_ARGUMENT;
  }
  if (p->nslot < 0 || p->nslot > QP_EXPR_MAX_SLOTS || (p->nslot > 0 && !p->slots)) {
    set_error("%s: nslot must be 0 .. %d with a slot table", who, (int)QP_EXPR_MAX_SLOTS);
    return QP_ERR_INVALID_ARGUMENT;
  }
  if (p->nword < 1 || p->nword > QP_EXPR_MAX_WORDS || !p->words) {
    set_error("%s: nword must be 1 .. %d", who, (int)QP_EXPR_MAX_WORDS);
    return QP_ERR_INVALID_ARGUMENT;
  }
  unsigned written = 0;
  for (int i = 0; i < p->nword; ++i) {
    const uint32_t w = p->words[i];
    const unsigned op = w & 0xffu, dst = (w >> 8) & 0xfu;
    const unsigned opnd[3] = {(w >> 12) & 0x3fu, (w >> 18) & 0x3fu, (w >> 24) & 0x3fu};
    if (op >= QP_OP_COUNT || dst >= QP_EXPR_MAX_REGS || (w >> 30)) {
      set_error("%s: word %d: unknown op or register", who, i);
      return QP_ERR_INVALID_ARGUMENT;
    }
    const bool binary = (op >= QP_OP_ADD && op <= QP_OP_POW) || (op >= QP_OP_MAX && op <= QP_OP_NE);
    const int used = op == QP_OP_WHERE ? 3 : (binary ? 2 : 1);
    for (int k = 0; k < used; ++k) {
      const unsigned o = opnd[k];
      const bool ok = o < QP_EXPR_MAX_REGS ? ((written >> o) & 1u) != 0
                    : (o == QP_EXPR_X || o == QP_EXPR_Y) ? true
                    : (o >= QP_EXPR_SLOT0 && o < (unsigned)(QP_EXPR_SLOT0 + p->nslot));
      if (!ok) {
        set_error("%s: word %d: operand %d reads an unwritten register or a slot that does not exist", who, i, k);
        return QP_ERR_INVALID_ARGUMENT;
      }
    }
    written |= 1u << dst;
  }
  return QP_OK;
}

}  // namespace qp

extern "C" {

int qp_add_generation_expr(const qp_generation_program* prog, const uint8_t* flags, int64_t members,
                           const int32_t* member_ids, int64_t nlisted, double* state, double dt, uint32_t* status,
                           void* stream) {
  const int rc = qp::validate_program(prog, "qp_add_generation_expr");
  if (rc != QP_OK) return rc;
  QP_REQUIRE(flags && state && status, "NULL argument");
  QP_REQUIRE(members > 0 && nlisted > 0 && nlisted <= members, "members and nlisted must be positive, nlisted <= members");
  QP_REQUIRE(member_ids || nlisted == members, "member_ids is required unless every member is listed");
  QP_REQUIRE(prog->ne <= 65535 && nlisted <= 65535, "at most 65535 bins and 65535 listed members per call");
  const long ncm = (long)prog->ny * prog->nx;
  QP_REQUIRE(ncm < (1L << 31), "a member must hold fewer than 2^31 cells");
  qp::ExprWords words = {};
  for (int i = 0; i < prog->nword; ++i) words.w[i] = prog->words[i];
  if (hipMemsetAsync(status, 0, 2 * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess)
    return qp::check_launch("qp_add_generation_expr (status)");
  const dim3 grid((unsigned)((ncm + 255) / 256), (unsigned)prog->ne, (unsigned)nlisted);
  hipLaunchKernelGGL(qp::add_generation_expr_kernel, grid, dim3(256), 0, (hipStream_t)stream, words, (int)prog->nword,
                     prog->slots, (int)prog->nslot, (int)prog->ny, (int)prog->nx, (int)prog->ny_full, (int)prog->nx_full,
                     (int)prog->row0, (int)prog->col0, flags, (long)members, member_ids, state, dt, status);
  return qp::check_launch("qp_add_generation_expr");
}

int qp_expr_eval_host(const qp_generation_program* prog, double* out) {
  const int rc = qp::validate_program(prog, "qp_expr_eval_host");
  if (rc != QP_OK) return rc;
  QP_REQUIRE(out, "NULL argument");
  const long ncm = (long)prog->ny * prog->nx;
  for (int bin = 0; bin < prog->ne; ++bin)
    for (int row = 0; row < prog->ny; ++row)
      for (int col = 0; col < prog->nx; ++col)
        out[(long)bin * ncm + (long)row * prog->nx + col] =
            qp::expr_eval(prog->words, prog->nword, prog->slots + (long)bin * prog->nslot,
                          qp::pixel_centre(prog->col0 + col, prog->nx_full), qp::pixel_centre(prog->row0 + row, prog->ny_full));
  return QP_OK;
}

}  // extern "C"
