// What the collision units share (private): the per-call arguments, the route of a call, the sizes each kernel family is
// instantiated for, and the launcher naming scheme.  The kernels themselves live in qp_collision*.inc / *.hip; the rule
// for which of them runs is qp::collision_route in qp_collision.hip and nowhere else.
#pragma once
#include "qp_common.h"

namespace qp {

// The arguments of one collision call, as every dispatcher and launcher receives them.  s / r / u are the EFFECTIVE
// switches (process enabled and its table present; phonons updated by an effective process).  The single-step kernels
// ignore dt_b and gen.
struct CollCall {
  const uint8_t* flags;
  long ncell;
  const double* sin;
  double* sout;
  double* ph;
  double* stash;          // the caller's ph_scratch (merged bins), or NULL
  double dE, dt, dt_b, gen;
  bool s, r, u;
  PauliPartial* guard;    // per-wave partials of the fused Pauli guard, or NULL
  double guard_floor;
  hipStream_t stream;
};

// Argument of collision_wave_kernel (qp_collision_wave.hip); qp_collision.hip fills it.
struct WaveCollView {
  int ne, nw, nclass;
  const double* kr0;
  const double* ks0;
  const double* rho;
  const int32_t* idx_diff;
  const int32_t* idx_sum;
  const int8_t* sign;
  const int32_t* cls;
  const int32_t* diag_bin;   // non-NULL: the host vouches for the |i-j| / i+j structure of the maps
  const int32_t* anti_bin;
};

// n(t+dt) for dn/dt = gain - loss n with frozen coefficients (solver.py:640-665); wave and generic kernels
__device__ __forceinline__ double relax_update(double n, double gain, double loss, double dt) {
  const double mu = fmax(loss, 0.0);
  const double P = fmax(gain + fmax(-loss, 0.0) * n, 0.0);      // mu - loss, safe from contraction (relax_update_f)
  const double decay = exp(-mu * dt);
  const double coeff = (mu < 1e-14) ? dt : (1.0 - decay) / mu;
  return fmax(decay * n + coeff * P, 0.0);
}

// y(t+dt) for y' = a + b y with frozen coefficients (solver.py:686-700)
__device__ __forceinline__ double affine_update(double y, double a, double b, double dt) {
  const double xx = fmin(fmax(b * dt, -80.0), 80.0);
  const double ex = exp(xx);
  const double coeff = (fabs(b) < 1e-14) ? dt : (ex - 1.0) / b;
  return fmax(ex * y + coeff * a, 0.0);
}

// ---- the sizes each family is instantiated for: X(NE, A), A passed through -------------------------------------------
// register kernel, one gap class (NE >= 32: the three-launch split)
#define QP_DIAG_NE_LIST(X, A) X(2, A) X(3, A) X(4, A) X(5, A) X(6, A) X(7, A) X(8, A) X(9, A) X(10, A) X(11, A) X(12, A) \
  X(13, A) X(14, A) X(15, A) X(16, A) X(18, A) X(20, A) X(24, A) X(30, A) X(32, A) X(40, A) X(50, A)
// register kernel, gap classes (PARAM): the sizes defined in qp_collision_fast.hip ...
#define QP_DIAGP_NE_LIST(X, A) X(2, A) X(3, A) X(4, A) X(5, A) X(6, A) X(7, A) X(8, A) X(9, A) X(10, A) X(11, A) X(12, A) \
  X(13, A) X(14, A) X(15, A) X(16, A)
// ... and in qp_collision_fast_u*.hip
#define QP_DIAGP_NE_LIST_EXT(X, A) X(18, A) X(20, A) X(24, A) X(30, A) X(32, A) X(40, A) X(50, A)
// member tables (QP_COLL_MEMBER_CLASSES): single-pass register kernel and double half-step kernel alike
#define QP_MEMBER_NE_LIST(X, A) X(4, A) X(5, A) X(6, A) X(7, A) X(8, A) X(9, A) X(10, A) X(11, A) X(12, A) X(13, A) \
  X(14, A) X(15, A) X(16, A)
// double half-step kernel
#define QP_PAIR_NE_LIST(X, A) X(4, A) X(5, A) X(6, A) X(7, A) X(8, A) X(9, A) X(10, A) X(11, A) X(12, A) X(13, A) \
  X(14, A) X(15, A) X(16, A)
// one-pass kernel, one gap class / gap classes
#define QP_ONEPASS_NE_LIST(X, A) X(50, A) X(40, A) X(32, A) X(30, A)
#define QP_ONEPASS_CLASSES_NE_LIST(X, A) X(50, A)
#define QP_NE_CASE(N, A) case N:

constexpr int kOnePassMaxClasses = 16;      // rows of the per-class rho table the LDS image of a PARAM one-pass kernel holds

int collision_fast_supported(int ne);
int collision_fast_classes_supported(int ne);
int collision_member_tables_supported(int ne);
int collision_pair_supported(int ne);
int collision_onepass_supported(int ne);
int collision_onepass_classes_supported(int ne);

// ---- launchers -----------------------------------------------------------------------------------------------------
// A launcher is the non-template function qp::coll_<family>_<NE>_<S><R>(view, call): defined in exactly one instantiation
// unit, declared and looked up in the family's dispatcher unit, so a missing instantiation fails to link.  Family F is
// backed by the host template launch_F<NE, S, R, ...> of its .inc; the register and pair families take a CollFastViewM
// (the kernels without member tables are launched with its CollFastView part), the one-pass families an OnePassView.
struct CollFastViewM;
struct OnePassView;
typedef void (*coll_launcher_t)(const CollFastViewM&, const CollCall&);
typedef void (*onepass_launcher_t)(const OnePassView&, const CollCall&);
typedef CollFastViewM view_diag, view_diagp, view_diagm, view_pair, view_pairm;
typedef OnePassView view_onepass, view_onepassc_u0, view_onepassc_u1;

#define QP_LAUNCHER(N, F, S, R) coll_##F##_##N##_##S##R
// one (S, R) launcher; the variadic part goes to launch_F as further template arguments (tile sizes of the one-pass kernels)
#define QP_DEFINE_LAUNCHER(N, F, S, R, ...) \
  void QP_LAUNCHER(N, F, S, R)(const view_##F& v, const CollCall& c) { launch_##F<N, S != 0, R != 0, ##__VA_ARGS__>(v, c); }
#define QP_DEFINE_LAUNCHERS(N, F, ...)                                                        \
  QP_DEFINE_LAUNCHER(N, F, 1, 1, ##__VA_ARGS__) QP_DEFINE_LAUNCHER(N, F, 0, 1, ##__VA_ARGS__) \
  QP_DEFINE_LAUNCHER(N, F, 1, 0, ##__VA_ARGS__)
#define QP_DECLARE_LAUNCHERS(N, F)                                \
  void QP_LAUNCHER(N, F, 1, 1)(const view_##F&, const CollCall&); \
  void QP_LAUNCHER(N, F, 0, 1)(const view_##F&, const CollCall&); \
  void QP_LAUNCHER(N, F, 1, 0)(const view_##F&, const CollCall&);
// find_F(ne, s, r): the launcher of family F for this size and process combination (s || r), NULL for a size not in LISTS
#define QP_LOOKUP_CASE(N, F) \
  case N: return (s && r) ? QP_LAUNCHER(N, F, 1, 1) : r ? QP_LAUNCHER(N, F, 0, 1) : QP_LAUNCHER(N, F, 1, 0);
#define QP_DEFINE_LOOKUP(F, LISTS)                                                                  \
  static auto find_##F(int ne, bool s, bool r) -> void (*)(const view_##F&, const CollCall&) {      \
    switch (ne) {                                                                                   \
      LISTS                                                                                         \
      default: return nullptr;                                                                      \
    }                                                                                               \
  }

// ---- routes --------------------------------------------------------------------------------------------------------
typedef qp_collision_route_kind Route;
// Which kernel family a single collision step runs.  Pure: launches nothing, dereferences no table pointer; `t` has passed
// the entry point's validation.  en_r / en_s / upd are the caller's switches, have_scratch whether ph_scratch was given.
Route collision_route(const qp_collision_tables& t, long ncell, bool en_r, bool en_s, bool upd, bool have_scratch);
// true when the route's kernels write the per-wave guard partials they are handed (CollCall::guard)
inline bool route_writes_guard(Route route, int ne) {
  return route == QP_ROUTE_REGISTER_MEMBERS || ((route == QP_ROUTE_REGISTER || route == QP_ROUTE_REGISTER_CLASSES) && ne < 32);
}
// The double half-step call: no fused kernel for these tables (QP_ERR_UNSUPPORTED), shared tables, member tables.
enum class PairRoute { None, Shared, Members };
PairRoute collision_pair_route(const qp_collision_tables& t, long ncell, bool s, bool r);

// ---- dispatchers: build the view of the route's family, look the launcher up, launch --------------------------------
void collision_fast_dispatch(Route route, const qp_collision_tables& t, const CollCall& c);      // register routes + copy
void collision_onepass_dispatch(Route route, const qp_collision_tables& t, const CollCall& c);   // the two one-pass routes
void collision_pair_dispatch(PairRoute route, const qp_collision_tables& t, const CollCall& c);
void collision_wave_dispatch(const WaveCollView& v, bool structured, const CollCall& c);
void collision_wave_wide_dispatch(const WaveCollView& v, bool structured, const CollCall& c);   // qp_collision_wave_wide.hip

}  // namespace qp
