// kprog_eval.h -- the general evaluator of a kernel program at one pair of points: the pair's distances (pair_dist), one
// leaf (leaf_value), the postfix program (eval_kprog) and its forward-mode derivatives with respect to one leaf
// parameter (eval_kprog_deriv) or to the log-scale of one input dimension (eval_kprog_deriv_dim).  Shared by kmat.hip
// (matrices, products, gradients) and small.hip (whole small problems in one workgroup, values and gradients).  Both
// are built with -ffp-contract=off: the scalar formulas keep the reference's operation order (kmat.hip).  Internal
// linkage: every translation unit compiles its own copy.
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

// d(leaf)/d(param) at the pair's distances: param 0 = p0 (scale or constant), 1 = p1
// (gamma / alpha / sigma).  Derived from the forms of kernels/stationary.py:76-235 and (FAM = 2)
// of DOT, u = s + p1^2 with s = r3 / p0^2:  du/dp0 = -2 s / p0,  du/dp1 = 2 p1.
template <typename T, int FAM = 0>
__device__ __forceinline__ T leaf_deriv(const KProg& kp, int i, int param, T r1, T r2, T r3 = T(0)) {
  const int op = kp.op[i];
  const bool l2 = kp.metric[i] == TGP_METRIC_L2;
  // (the derivative passes are not the hot ones: both distances up front)
  const T dist = l2 ? ((r2 == T(0)) ? r1 : sqrt(r2)) : r1;
  const T sq = l2 ? r2 : r1 * r1;
  const T p0 = T(kp.p0[i]);
  const T p1 = T(kp.p1[i]);
  switch (op) {
    case TGP_K_CONST: return param == 0 ? T(1) : T(0);
    case TGP_K_EXP: return param == 0 ? exp(-dist / p0) * dist / (p0 * p0) : T(0);
    case TGP_K_EXPSQ: return param == 0 ? exp(T(-0.5) * (sq / (p0 * p0))) * sq / (p0 * p0 * p0) : T(0);
    case TGP_K_M32: { const T a = MathC<T>::SQRT3 * (dist / p0);
                      return param == 0 ? a * a * exp(-a) / p0 : T(0); }
    case TGP_K_M52: { const T a = MathC<T>::SQRT5 * (dist / p0);
                      return param == 0 ? (a * a / T(3)) * (T(1) + a) * exp(-a) / p0 : T(0); }
    case TGP_K_COS: { const T u = MathC<T>::TWO_PI * (dist / p0);
                      return param == 0 ? sin(u) * u / p0 : T(0); }
    case TGP_K_ESS: { const T u = MathC<T>::PI * (dist / p0);
                      const T sn = sin(u), v = exp(-p1 * (sn * sn));
                      return param == 0 ? v * p1 * T(2) * sn * cos(u) * u / p0 : -(sn * sn) * v; }
    case TGP_K_RQ: { const T q = T(0.5) * (sq / (p0 * p0)) / p1;  // r^2 / (2 alpha l^2)
                     const T u = T(1) + q, v = pow(u, -p1);
                     // log1p(q), not log(u): u rounds to 1 below q = eps, and q / u - log(u) = q there where the
                     // derivative is -q^2 / 2 -- an error of the size of the scale derivative, 2 alpha q / l
                     return param == 0 ? v / u * sq / (p0 * p0 * p0) : v * (q / u - log1p(q)); }
    default: break;
  }
  if constexpr (FAM == 2) {
    if (op == TGP_K_DOT) return param == 0 ? T(-2) * (r3 / (p0 * p0)) / p0 : T(2) * p1;
  }
  (void)r3;
  return T(0);
}

// POW on the stack: (v, dv) -> (v^p, p v^(p-1) dv [+ v^p log v when p itself is differentiated]).
// The log is taken of v with v == 0 replaced by 1 -- JAX's rule for x ** y (a zero base gives 0,
// not NaN); a negative base gives NaN there, as in the reference.
template <typename T>
__device__ __forceinline__ void pow_deriv(T p, bool seed, T& v, T& dv) {
  const T w = pow(v, p);
  T d = p * pow(v, p - T(1)) * dv;
  if (seed) d += w * log(v == T(0) ? T(1) : v);
  v = w;
  dv = d;
}

// Forward-mode derivative of the whole program with respect to ONE leaf parameter: the stack
// carries (value, derivative) pairs; only op `which_op` (a leaf, or FAM = 2 a POW) seeds a
// non-zero derivative.
template <typename T, int FAM = 0>
__device__ __forceinline__ T eval_kprog_deriv(const KProg& kp, int which_op, int which_param, T r1,
                                              T r2, T r3 = T(0)) {
  T s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
  T d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0, d6 = 0, d7 = 0;
  for (int i = 0; i < kp.n; ++i) {
    const int op = kp.op[i];
    if constexpr (FAM == 2) {
      if (op == TGP_K_POW) {
        pow_deriv<T>(T(kp.p0[i]), i == which_op, s0, d0);
        continue;
      }
    }
    if (op >= TGP_K_ADD) {
      const T v = (op == TGP_K_ADD) ? (s1 + s0) : (s1 * s0);
      const T dv = (op == TGP_K_ADD) ? (d1 + d0) : (d1 * s0 + s1 * d0);
      s0 = v; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
      d0 = dv; d1 = d2; d2 = d3; d3 = d4; d4 = d5; d5 = d6; d6 = d7;
      continue;
    }
    const T v = leaf_value<T, FAM == 2 ? 2 : 0>(kp, i, r1, r2, r3);
    const T dv = (i == which_op) ? leaf_deriv<T, FAM>(kp, i, which_param, r1, r2, r3) : T(0);
    s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
    d7 = d6; d6 = d5; d5 = d4; d4 = d3; d3 = d2; d2 = d1; d1 = d0; d0 = dv;
  }
  return d0;
}

// This pair's weights of one input dimension (eval_kprog_deriv_dim's w1 / w2), dx its coordinate difference there:
// w1 = |dx| / r1 and w2 = dx^2 / r2, zero at coincident points.  Where r2 underflows to zero while r1 > 0 the L2
// distance of every leaf IS r1 (the zero-safe square root of leaf_value / leaf_deriv), so the weight is the L1 one
// there, not zero.
template <typename T>
__device__ __forceinline__ void dim_weights(T dx, T r1, T r2, T& w1, T& w2) {
  w1 = r1 > T(0) ? fabs(dx) / r1 : T(0);
  w2 = r2 > T(0) ? dx * dx / r2 : w1;
}

// Forward-mode derivative of the whole program with respect to the LOG-SCALE of one input dimension d (x_d -> s x_d
// for every point): what `transforms.Linear` / `Cholesky` with a per-dimension scale need (reference
// transforms.py:39-133; JAX differentiates through them for free).  Every stationary leaf depends on the
// coordinates through dist / p0 resp. sq / p0^2 only, so
//   d leaf / d log s_d = -p0 * (d leaf / d p0) * w_d,   w_d = dx_d^2 / r2 (L2 metric) or |dx_d| / r1 (L1),
// (the w_d sum to one: scaling every dimension is scaling 1 / p0).  w1 / w2 are this pair's weights (dim_weights).
// FAM = 2: a DOT leaf contributes 2 (z_id / p0)(z_jd / p0), zz = z_id z_jd, and POW chains.
template <typename T, int FAM = 0>
__device__ __forceinline__ T eval_kprog_deriv_dim(const KProg& kp, T r1, T r2, T w1, T w2, T r3 = T(0),
                                                  T zz = T(0)) {
  T s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
  T d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0, d6 = 0, d7 = 0;
  for (int i = 0; i < kp.n; ++i) {
    const int op = kp.op[i];
    if constexpr (FAM == 2) {
      if (op == TGP_K_POW) {
        pow_deriv<T>(T(kp.p0[i]), false, s0, d0);
        continue;
      }
    }
    if (op >= TGP_K_ADD) {
      const T v = (op == TGP_K_ADD) ? (s1 + s0) : (s1 * s0);
      const T dv = (op == TGP_K_ADD) ? (d1 + d0) : (d1 * s0 + s1 * d0);
      s0 = v; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
      d0 = dv; d1 = d2; d2 = d3; d3 = d4; d4 = d5; d5 = d6; d6 = d7;
      continue;
    }
    const T v = leaf_value<T, FAM == 2 ? 2 : 0>(kp, i, r1, r2, r3);
    const T w = kp.metric[i] == TGP_METRIC_L2 ? w2 : w1;
    T dv = (op == TGP_K_CONST) ? T(0) : -T(kp.p0[i]) * leaf_deriv<T, FAM>(kp, i, 0, r1, r2, r3) * w;
    if constexpr (FAM == 2) {
      if (op == TGP_K_DOT) { const T p0 = T(kp.p0[i]); dv = T(2) * (zz / (p0 * p0)); }
    }
    (void)zz;
    s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
    d7 = d6; d6 = d5; d5 = d4; d4 = d3; d3 = d2; d2 = d1; d1 = d0; d0 = dv;
  }
  return d0;
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
