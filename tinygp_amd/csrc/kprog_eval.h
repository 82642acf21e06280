// kprog_eval.h -- the general evaluator of a kernel program at one pair of points: the pair's distances (pair_dist), one
// leaf (leaf_value) and the postfix program (eval_kprog).  Shared by kmat.hip (matrices, products, gradients) and
// small.hip (whole small problems in one workgroup).  Both are built with -ffp-contract=off: the scalar formulas keep
// the reference's operation order (kmat.hip).  Internal linkage: every translation unit compiles its own copy.
#pragma once

#include "tgp_common.h"

namespace tgp {

namespace {

template <typename T> struct MathC;
template <> struct MathC<double> {
  static constexpr double SQRT3 = 1.7320508075688772;   // np.sqrt(3)
  static constexpr double SQRT5 = 2.23606797749979;     // np.sqrt(5)
  static constexpr double PI = 3.141592653589793;
  static constexpr double TWO_PI = 6.283185307179586;   // 2 * np.pi
};
template <> struct MathC<float> {
  static constexpr float SQRT3 = 1.7320508075688772f;
  static constexpr float SQRT5 = 2.23606797749979f;
  static constexpr float PI = 3.141592653589793f;
  static constexpr float TWO_PI = 6.283185307179586f;
};

// One leaf of the program (a stationary kernel or a constant) at the pair's r1 = sum|d| and
// r2 = sum d^2.  The distance a leaf does not use is not computed: the metric and the op are
// wave-uniform, so e.g. ExpSquared never pays for the fp64 square root of the L2 distance.
// distance.py:51-56: zero-safe sqrt; distance.py:30-38: L1 "squared" = distance^2
// FAM = 1: the program holds only Constant / Exp / ExpSquared / Matern leaves (checked on the
// host): the cosine, sine and power paths -- and their registers -- are compiled out.
// FAM = 2: the program holds a DOT leaf or a POW (kfamily()): every leaf, plus r3 = sum x_ik x_jk,
// which only this family's loops accumulate (FAM 0 / 1 callers pass 0 and compile as before).
// DOT divides the RAW sum once by p0^2 instead of dividing every coordinate first as the
// reference does ((X1 / scale) @ (X2 / scale), base.py:254-256): one accumulator serves leaves of
// different scales, at a parity cost of a few ulp of sum |x_ik x_jk| / p0^2 (the rounding of p0^2
// and of the quotient; the reference's own matmul has no fixed summation order either).
template <typename T, int FAM = 0>
__device__ __forceinline__ T leaf_value(const KProg& kp, int i, T r1, T r2, T r3 = T(0)) {
  const int op = kp.op[i];
  const bool l2 = kp.metric[i] == TGP_METRIC_L2;
  auto dist = [&]() -> T { return l2 ? ((r2 == T(0)) ? r1 : sqrt(r2)) : r1; };
  auto sq = [&]() -> T { return l2 ? r2 : r1 * r1; };
  const T p0 = T(kp.p0[i]);
  const T p1 = T(kp.p1[i]);
  switch (op) {
    case TGP_K_CONST: return p0;
    case TGP_K_EXP: return exp(-dist() / p0);
    case TGP_K_EXPSQ: return exp(T(-0.5) * (sq() / (p0 * p0)));
    case TGP_K_M32: { const T a = MathC<T>::SQRT3 * (dist() / p0); return (T(1) + a) * exp(-a); }
    case TGP_K_M52: { const T a = MathC<T>::SQRT5 * (dist() / p0);
                      return (T(1) + a + (a * a) / T(3)) * exp(-a); }
    default: break;
  }
  if constexpr (FAM != 1) {
    switch (op) {
      case TGP_K_COS: return cos(MathC<T>::TWO_PI * (dist() / p0));
      case TGP_K_ESS: { const T s = sin(MathC<T>::PI * (dist() / p0)); return exp(-p1 * (s * s)); }
      case TGP_K_RQ: return pow(T(1) + T(0.5) * (sq() / (p0 * p0)) / p1, -p1);
      default: break;
    }
  }
  if constexpr (FAM == 2) {
    if (op == TGP_K_DOT) return r3 / (p0 * p0) + p1 * p1;
  }
  (void)p1;
  (void)r3;
  return T(0);
}

// Evaluate the postfix program for one pair given r1 = sum|d|, r2 = sum d^2 (and, FAM = 2,
// r3 = sum x_ik x_jk).  Programs of one leaf, or of two leaves and one operator (e.g.
// `amp**2 * ExpSquared(l)`), take a direct path; anything else runs the general stack machine,
// whose evaluation stack lives in 8 named registers (no runtime-indexed array -> no scratch).
// All branches are wave-uniform (the program sits in kernarg / SGPRs).  Only FAM = 2 programs
// hold the unary POW (ops >= TGP_K_ADD are binary everywhere else).
template <typename T, int FAM = 0>
__device__ __forceinline__ T eval_kprog(const KProg& kp, T r1, T r2, T r3 = T(0)) {
  if (kp.n == 1) return leaf_value<T, FAM>(kp, 0, r1, r2, r3);
  if (kp.n == 3 && kp.op[0] < TGP_K_ADD && kp.op[1] < TGP_K_ADD &&
      (FAM != 2 || kp.op[2] == TGP_K_ADD || kp.op[2] == TGP_K_MUL)) {
    const T a = leaf_value<T, FAM>(kp, 0, r1, r2, r3);
    const T b = leaf_value<T, FAM>(kp, 1, r1, r2, r3);
    return (kp.op[2] == TGP_K_ADD) ? (a + b) : (a * b);
  }
  T s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
  for (int i = 0; i < kp.n; ++i) {
    const int op = kp.op[i];
    if constexpr (FAM == 2) {
      if (op == TGP_K_POW) {  // base.py:254-256: (dot + sigma^2) ** order
        s0 = pow(s0, T(kp.p0[i]));
        continue;
      }
    }
    if (op >= TGP_K_ADD) {
      const T r = (op == TGP_K_ADD) ? (s1 + s0) : (s1 * s0);
      s0 = r; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
      continue;
    }
    const T v = leaf_value<T, FAM>(kp, i, r1, r2, r3);
    s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
  }
  return s0;
}

struct NoCapture {
  template <typename T> __device__ __forceinline__ void operator()(int, T, T, T) const {}
};

// The distances of one pair of points a, b: r1 = sum |a_t - b_t|, r2 = sum (a_t - b_t)^2 and, FAM = 2 only,
// r3 = sum a_t b_t, dimension by dimension in this order.  D > 0: an unrolled loop over D coordinates with the row
// point `a` in registers (PARTIAL: only the first d <= D of them exist); D = 0: the dynamic loop over d.
// `capture(t, dx, a_t, b_t)` sees every dimension (the gradient keeps one of them).
template <typename T, int FAM, int D, bool PARTIAL = false, typename Capture = NoCapture>
__device__ __forceinline__ void pair_dist(const T* a, const T* b, int d, T& r1, T& r2, T& r3,
                                          Capture capture = Capture()) {
  r1 = r2 = r3 = T(0);
  auto step = [&](int t) {
    const T dx = a[t] - b[t];
    r1 += fabs(dx);
    r2 += dx * dx;
    if constexpr (FAM == 2) r3 += a[t] * b[t];
    capture(t, dx, a[t], b[t]);
  };
  if constexpr (D > 0) {
#pragma unroll
    for (int t = 0; t < D; ++t)
      if (!PARTIAL || t < d) step(t);
  } else {
    for (int t = 0; t < d; ++t) step(t);
  }
}

}  // namespace

}  // namespace tgp
