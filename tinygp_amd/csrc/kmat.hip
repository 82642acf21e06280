// kmat.hip -- pairwise-distance + stationary-kernel evaluator (K1/K2/K3/K9 of SURVEY 2a), with the
// dot-product leaves of reference kernels/base.py:212-256 (DotProduct, Polynomial) in the same loop.
//
// Replaces reference kernels/base.py:84-103 (nested vmap of Kernel.evaluate) fused with
// noise.py:77-78 (diagonal scatter-add).  HBM-write bound: every lane owns one ROW of a
// 128x128 tile and walks 64 columns, so each wave store is 512 contiguous bytes of the
// column-major output; the X tiles are staged once through LDS.
//
// Built with -ffp-contract=off: the scalar formulas below keep the reference's operation
// order (kernels/stationary.py:76-235, kernels/distance.py:41-59) so entries agree with a
// NumPy evaluation to the last ulp or two (libm-vs-ocml exp is the only difference).
#include <algorithm>

#include "tgp_common.h"
#include "kprog_eval.h"

namespace tgp {

namespace {

constexpr int KT = 128;  // tile edge

// Zero-padded load of two 128-point tiles -- rows r0.. of X1 into s1, rows c0.. of X2 into s2, [KT][d] each -- by the
// block's 256 threads, and the barrier after it.
template <typename T>
__device__ __forceinline__ void load_tile_pair(T* s1, T* s2, const T* __restrict__ X1, const T* __restrict__ X2,
                                               int64_t r0, int64_t c0, int64_t n1, int64_t n2, int d) {
  for (int t = threadIdx.x; t < KT * d; t += 256) {
    const int64_t gi = r0 + t / d, gj = c0 + t / d;
    s1[t] = (gi < n1) ? X1[gi * d + t % d] : T(0);
    s2[t] = (gj < n2) ? X2[gj * d + t % d] : T(0);
  }
  __syncthreads();
}

// acc[a] <- the sum of acc[a] over the block's NT threads, valid in thread 0: a fixed LDS tree (t pairs with t + NT/2,
// then with t + NT/4, ...), so the result does not depend on timing.
template <int NT, int NACC>
__device__ __forceinline__ void block_sum(double (&acc)[NACC]) {
  __shared__ double red[NACC][NT];
#pragma unroll
  for (int a = 0; a < NACC; ++a) red[a][threadIdx.x] = acc[a];
  __syncthreads();
  for (int sft = NT / 2; sft > 0; sft >>= 1) {
    if ((int)threadIdx.x < sft) {
#pragma unroll
      for (int a = 0; a < NACC; ++a) red[a][threadIdx.x] += red[a][threadIdx.x + sft];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = red[a][0];
  }
}

// ---- fast path: the program is one exp-family leaf, optionally times a constant ("amp * leaf") --
// OP and the metric are template parameters, so the inner loops below are straight-line code the
// compiler can unroll and interleave across elements (the general evaluator runs a chain of
// wave-uniform branches per element).  Same expressions, same order: bit-identical values.
struct FastProg {
  int op = -1, l2 = 0;   // op < 0: not a fast program
  double p0 = 1, amp = 1;
  int leaf = -1, konst = -1;  // positions of the leaf and of the constant (-1: none) in the program
};
static FastProg fast_prog(const KProg& kp) {
  FastProg f;
  auto leaf_ok = [](int op) { return op == TGP_K_EXP || op == TGP_K_EXPSQ || op == TGP_K_M32 || op == TGP_K_M52; };
  int li = -1, ci = -1;
  if (kp.n == 1 && leaf_ok(kp.op[0])) li = 0;
  else if (kp.n == 3 && kp.op[2] == TGP_K_MUL) {
    if (kp.op[0] == TGP_K_CONST && leaf_ok(kp.op[1])) { ci = 0; li = 1; }
    else if (kp.op[1] == TGP_K_CONST && leaf_ok(kp.op[0])) { ci = 1; li = 0; }
  }
  if (li < 0) return f;
  f.op = kp.op[li];
  f.l2 = kp.metric[li] == TGP_METRIC_L2;
  f.p0 = kp.p0[li];
  f.amp = ci >= 0 ? kp.p0[ci] : 1.0;  // x * 1 == x exactly
  f.leaf = li;
  f.konst = ci;
  return f;
}

// a / b for a wave-uniform divisor whose reciprocal y = RN(1 / b) was taken once per thread: the IEEE quotient, bit for
// bit, in one multiply and four FMAs instead of the ~11-instruction division sequence (v_div_scale x2, quarter-rate
// v_rcp, 5 FMAs, v_div_fmas, v_div_fixup) -- Markstein's theorem: with y the correctly rounded reciprocal and q1 a
// faithful quotient, RN(q1 + (a - b q1) y) is the correctly rounded a / b, EXCEPT for divisors whose significand is all
// ones (the one case where RN(1 / b) is not close enough): UDiv::exact is false there and for divisors outside
// [2^-200, 2^200], and the caller divides.  q0 = RN(a y) is within 2.5 ulp, q1 = RN(q0 + (a - b q0) y) is faithful
// (both residuals are exact: FMA).  Dividends above 2^600 (infinities) must take the division -- the caller tracks the
// largest distance it saw (`seen` in kmat_fast_kernel) and redoes its entries with FAST = false beyond 2^300; below 2^-600 nothing of
// the fast path can be trusted to the last bit any more (the residuals leave the normal range), but there the
// quotient is below 2^-400 by either route and every leaf that consumes it returns exactly 1 (exp(-q / 2),
// (1 + a) exp(-a), ...: 1 + O(q) rounds to 1) -- the kernel VALUE is the division's.  The entries stay the reference's quotients
// (kernels/stationary.py:104-106: r / scale, r2 / scale^2), which a multiply by the reciprocal alone does not give:
// up to 36 ulp in exp() on config 2.  Checked against the division on 4 x 10^8 structured and random
// pairs on the host (tests/markstein_check.c) and entry for entry on the device (tests/test_gpu_kernels.py).
template <typename T>
struct UDiv {
  T b, y;
  bool exact;
  __device__ __forceinline__ explicit UDiv(T b_) : b(b_), y(T(1) / b_), exact(false) {
    if constexpr (sizeof(T) == 8) {
      unsigned long long u;
      __builtin_memcpy(&u, &b_, 8);
      const unsigned long long frac = u & 0xFFFFFFFFFFFFFull;
      exact = b_ >= 0x1p-200 && b_ <= 0x1p200 && frac != 0xFFFFFFFFFFFFFull;
    }
  }
  template <bool FAST>
  __device__ __forceinline__ T div(T a) const {
    if constexpr (!FAST || sizeof(T) != 8) {
      return a / b;
    } else {
      const T q0 = a * y;
      const T r0 = __builtin_fma(-b, q0, a);
      const T q1 = __builtin_fma(r0, y, q0);
      const T r1 = __builtin_fma(-b, q1, a);
      return __builtin_fma(r1, y, q1);
    }
  }
};

template <typename T, int OP, int L2, bool FAST>
__device__ __forceinline__ T leaf_fast(T r1, T r2, const UDiv<T>& by_p0, const UDiv<T>& by_p0sq, const UDiv<T>& by3) {
  if constexpr (OP == TGP_K_EXPSQ) {
    const T sq = L2 ? r2 : r1 * r1;
    return exp(T(-0.5) * by_p0sq.template div<FAST>(sq));
  } else {
    const T dist = L2 ? ((r2 == T(0)) ? r1 : sqrt(r2)) : r1;
    if constexpr (OP == TGP_K_EXP) {
      return exp(-by_p0.template div<FAST>(dist));
    } else if constexpr (OP == TGP_K_M32) {
      const T a = MathC<T>::SQRT3 * by_p0.template div<FAST>(dist);
      return (T(1) + a) * exp(-a);
    } else {
      const T a = MathC<T>::SQRT5 * by_p0.template div<FAST>(dist);
      return (T(1) + a + by3.template div<FAST>(a * a)) * exp(-a);
    }
  }
}

// (the gradient and matrix-vector kernels: the division itself)
template <typename T, int OP, int L2>
__device__ __forceinline__ T leaf_fast(T r1, T r2, T p0, T p0sq) {
  const UDiv<T> by_p0(p0), by_p0sq(p0sq), by3(T(3));
  return leaf_fast<T, OP, L2, false>(r1, r2, by_p0, by_p0sq, by3);
}

// Full interior tiles only (every row and column inside n1 x n2): no bounds checks in the loop.
// One 128 x 128 tile per workgroup: wave w its columns 32w .. 32w + 31, lane l its rows 2l and 2l + 1 -- one 16-byte
// store per lane and column, a wave store is the tile's whole 1-KiB column.  (Rounds 1-2: lane = one row, 64 columns,
// 8-byte stores: 4.48 / 4.20 / 4.49 TB/s at N = 16 384 / 32 768 / 65 536; this shape 4.54 / 4.48 / 4.78.  A 512 x 32
// shape -- 4 KiB of one matrix column per workgroup and column -- measured 3.18 / 3.97 / 4.49: profiles/r03_j.)
template <typename T, int D, int OP, int L2>
__global__ __launch_bounds__(256) void kmat_fast_kernel(T p0, T amp, int64_t n1, int64_t n2,
                                                        const T* __restrict__ X1,
                                                        const T* __restrict__ X2,
                                                        const T* __restrict__ diag, T* __restrict__ out,
                                                        int64_t ld, int flags, int tc0, int tri_h) {
  typedef T T2 __attribute__((ext_vector_type(2)));
  constexpr int NCOL = 32;
  const int cq = threadIdx.x >> 6, l = threadIdx.x & 63;
  int tr, tc;
  if (flags & KMAT_LOWER) {
    // 1-D grid over the tiles on and below the diagonal, column by column (local column j = 0.. holds tri_h - j tiles):
    // a 2-D grid whose upper half returns at once spent 0.07 of 0.27 ms at N = 16 384 dispatching empty workgroups
    // (scripts/probe_kmat.hip, profiles/r04_d)
    const int b = blockIdx.x;
    const double h2 = 2.0 * tri_h + 1.0;
    int j = int((h2 - sqrt(h2 * h2 - 8.0 * double(b))) * 0.5);
    while (j > 0 && j * tri_h - j * (j - 1) / 2 > b) --j;
    while ((j + 1) * tri_h - (j + 1) * j / 2 <= b) ++j;
    tc = tc0 + j;
    tr = tc + (b - (j * tri_h - j * (j - 1) / 2));
  } else {
    tr = blockIdx.x;
    tc = blockIdx.y + tc0;
  }
  __shared__ T s2all[KT * D];
  for (int t = threadIdx.x; t < KT * D; t += 256) s2all[t] = X2[int64_t(tc) * KT * D + t];
  __syncthreads();
  const T* s2 = s2all + cq * NCOL * D;
  const int64_t c0 = int64_t(tc) * KT + cq * NCOL;
  const int64_t gi = int64_t(tr) * KT + 2 * l;
  T xr[2][D];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int t = 0; t < D; ++t) xr[h][t] = X1[(gi + h) * D + t];
  const bool on_diag = diag != nullptr && tr == tc;
  const T dg0 = on_diag ? diag[gi] : T(0), dg1 = on_diag ? diag[gi + 1] : T(0);
  const UDiv<T> by_p0(p0), by_p0sq(p0 * p0), by3(T(3));
  const int ldiag = 2 * l - cq * NCOL;  // column index (within the wave's 32) of this lane's first diagonal entry
  T* o = out + c0 * ld + gi;
  auto columns = [&](auto fast) -> T {
    constexpr bool FAST = decltype(fast)::value;
    T seen = 0;  // the largest distance of this lane's entries (a NaN passes through both routes alike)
#pragma unroll 4
    for (int c = 0; c < NCOL; ++c) {
      T v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        T r1 = 0, r2 = 0;
#pragma unroll
        for (int t = 0; t < D; ++t) {
          const T dx = xr[h][t] - s2[c * D + t];
          r1 += fabs(dx);
          r2 += dx * dx;
        }
        v[h] = amp * leaf_fast<T, OP, L2, FAST>(r1, r2, by_p0, by_p0sq, by3);
        if constexpr (FAST) seen = fmax(seen, L2 ? r2 : r1);
      }
      if (on_diag) {  // noise.py:77-78 fused
        if (c == ldiag) v[0] += dg0;
        if (c == ldiag + 1) v[1] += dg1;
      }
      T2 pair;
      pair.x = v[0];
      pair.y = v[1];
      // (non-temporal stores: 6 % in the stand-alone probe at N = 16 384, nothing at 32 768 and nothing in the library)
      *reinterpret_cast<T2*>(o + int64_t(c) * ld) = pair;
    }
    return seen;
  };
  // (wave-uniform: the divisors are kernel arguments; KMAT_PLAIN_DIV is the tests' switch to the division itself)
  bool plain = true;
  if (sizeof(T) == 8 && !(flags & KMAT_PLAIN_DIV) && by_p0.exact && by_p0sq.exact) {
    // every dividend -- r, r^2, (sqrt(5) r / l)^2 -- stays below 2^1010 while r <= 2^300
    plain = !(columns(std::true_type{}) <= T(0x1p300));
  }
  if (plain) columns(std::false_type{});
}

// D = 0: dynamic dimension (coordinates re-read from LDS); D > 0: row point in registers.
template <typename T, int D, int FAM>
__global__ __launch_bounds__(256) void kmat_kernel(KProg kp, int64_t n1, int64_t n2, int d,
                                                   const T* __restrict__ X1,
                                                   const T* __restrict__ X2,
                                                   const T* __restrict__ diag, T* __restrict__ out,
                                                   int64_t ld, int64_t rows_out, int64_t cols_out,
                                                   int flags, int tc0, int ftr, int ftc) {
  const int tr = blockIdx.x, tc = blockIdx.y + tc0;
  if ((flags & KMAT_LOWER) && tr < tc) return;
  if (tr < ftr && tc < ftc) return;  // full tiles already written by kmat_fast_kernel
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* s1 = reinterpret_cast<T*>(smem);  // [KT][d]
  T* s2 = s1 + KT * d;                 // [KT][d]
  const int64_t r0 = int64_t(tr) * KT, c0 = int64_t(tc) * KT;
  load_tile_pair(s1, s2, X1, X2, r0, c0, n1, n2, d);

  const int il = threadIdx.x & (KT - 1);
  const int g = threadIdx.x >> 7;  // column half
  const int64_t gi = r0 + il;
  T xr[D > 0 ? D : 1];
  if constexpr (D > 0) {
#pragma unroll
    for (int t = 0; t < D; ++t) xr[t] = s1[il * D + t];
  }
  const T dg = (diag != nullptr && gi < n1) ? diag[gi] : T(0);
  if (gi >= rows_out) return;
  for (int c = 0; c < KT / 2; ++c) {
    const int jl = g * (KT / 2) + c;
    const int64_t gj = c0 + jl;
    if (gj >= cols_out) break;
    T v;
    if (gi < n1 && gj < n2) {
      T r1, r2, r3;
      if constexpr (D > 0) pair_dist<T, FAM, D>(xr, s2 + jl * D, d, r1, r2, r3);
      else pair_dist<T, FAM, 0>(s1 + il * d, s2 + jl * d, d, r1, r2, r3);
      v = eval_kprog<T, FAM>(kp, r1, r2, r3);
      if (diag != nullptr && gi == gj) v += dg;  // noise.py:77-78 fused
    } else {
      v = ((flags & KMAT_PAD_IDENTITY) && gi == gj) ? T(1) : T(0);
    }
    out[gj * ld + gi] = v;
  }
}

// d(leaf)/d(scale), the expressions of leaf_deriv with op and metric fixed at compile time
template <typename T, int OP, int L2>
__device__ __forceinline__ T leaf_deriv_fast(T r1, T r2, T p0) {
  if constexpr (OP == TGP_K_EXPSQ) {
    const T sq = L2 ? r2 : r1 * r1;
    return exp(T(-0.5) * (sq / (p0 * p0))) * sq / (p0 * p0 * p0);
  } else {
    const T dist = L2 ? ((r2 == T(0)) ? r1 : sqrt(r2)) : r1;
    if constexpr (OP == TGP_K_EXP) {
      return exp(-dist / p0) * dist / (p0 * p0);
    } else if constexpr (OP == TGP_K_M32) {
      const T a = MathC<T>::SQRT3 * (dist / p0);
      return a * a * exp(-a) / p0;
    } else {
      const T a = MathC<T>::SQRT5 * (dist / p0);
      return (a * a / T(3)) * (T(1) + a) * exp(-a) / p0;
    }
  }
}

// ---- what is evaluated per pair: the two evaluators of the gradient and the matrix-vector kernels -------------------
// value(): the kernel at the pair's distances.  capture() / add_sums(): the gradient's side -- NSUM derivatives of the
// kernel, each weighted with gij = alpha_i alpha_j - Kinv_ij and `half` (1/2 on the diagonal, 1 below it) into acc[].
// Each evaluator keeps the order of its own products (gij * dk * half here, (gij * half) * dk in FastEval).

// Any program: one derivative per pass, with respect to parameter `which_param` of op `which_op` (>= 0), or to the
// log-scale of input dimension -1 - which_op (< 0), whose dx and (FAM = 2) x_i x_j capture() keeps.
template <typename T, int FAM>
struct GeneralEval {
  static constexpr int FAMILY = FAM, NSUM = 1, UNROLL = 1;
  KProg kp;
  int which_op, which_param;
  struct Pair { T dxd = 0, zz = 0; };
  __device__ __forceinline__ T value(T r1, T r2, T r3) const { return eval_kprog<T, FAM>(kp, r1, r2, r3); }
  __device__ __forceinline__ void capture(Pair& p, int t, T dx, T a, T b) const {
    if (t == -1 - which_op) p.dxd = dx;
    if constexpr (FAM == 2) {
      if (t == -1 - which_op) p.zz = a * b;
    }
  }
  __device__ __forceinline__ void add_sums(const Pair& p, T r1, T r2, T r3, T gij, double half,
                                           double (&acc)[NSUM]) const {
    T w1 = 0, w2 = 0;
    if (which_op < 0) dim_weights<T>(p.dxd, r1, r2, w1, w2);
    const T dk = which_op >= 0 ? eval_kprog_deriv<T, FAM>(kp, which_op, which_param, r1, r2, r3)
                               : eval_kprog_deriv_dim<T, FAM>(kp, r1, r2, w1, w2, r3, p.zz);
    acc[0] += double(gij) * double(dk) * half;
  }
};

// "leaf" / "amp * leaf" programs (fast_prog()): straight-line code (see kmat_fast_kernel), and BOTH derivatives in
// one pass over K^-1: acc[0] for d/d amp = leaf, acc[1] for d/d scale = amp * d leaf.
template <typename T, int OP, int L2>
struct FastEval {
  static constexpr int FAMILY = 0, NSUM = 2, UNROLL = 2;
  T p0, amp;
  struct Pair {};
  __device__ __forceinline__ T value(T r1, T r2, T) const { return amp * leaf_fast<T, OP, L2>(r1, r2, p0, p0 * p0); }
  __device__ __forceinline__ void capture(Pair&, int, T, T, T) const {}
  __device__ __forceinline__ void add_sums(const Pair&, T r1, T r2, T, T gij, double half, double (&acc)[NSUM]) const {
    const T leaf = leaf_fast<T, OP, L2>(r1, r2, p0, p0 * p0);
    const T dk = amp * leaf_deriv_fast<T, OP, L2>(r1, r2, p0);
    const double w = double(gij) * half;
    acc[0] += w * double(leaf);
    acc[1] += w * double(dk);
  }
};

// ---- where Kinv_ij lives and which tiles contribute ------------------------------------------------------------
// The square matrix, column-major: the tiles on and below the diagonal; the result overwrites.
template <typename T>
struct SquareKinv {
  static constexpr bool ACCUMULATE = false;
  const T* Kinv;
  int64_t ld;
  __device__ __forceinline__ int64_t first_col() const { return 0; }
  __device__ __forceinline__ bool skip(int64_t r0, int64_t c0, int64_t) const { return r0 < c0; }
  __device__ __forceinline__ T at(int64_t gi, int64_t gj) const { return Kinv[gj * ld + gi]; }
};

// A CHUNK OF COLUMNS of K^-1 held as rows (the gradient on the block-column path): `Kc` is (n_pad, R) ROW-major --
// K^-1[i, c0 + r] at i * R + r, the layout of the distributed solves' right-hand sides --, and only row tiles inside
// block rows THIS RANK owns contribute (block row b = row / nb belongs to rank b mod G): the ranks' partial sums add up
// to the lower triangle of the chunk, and the chunks add up in the result.
template <typename T>
struct ChunkKinv {
  static constexpr bool ACCUMULATE = true;
  const T* Kc;
  int64_t R, c0, nb;
  int G, rank;
  __device__ __forceinline__ int64_t first_col() const { return c0; }
  __device__ __forceinline__ bool skip(int64_t r0, int64_t cc0, int64_t n) const {
    const bool mine = int((r0 / nb) % G) == rank;
    return !mine || r0 + KT <= cc0 || cc0 >= n || r0 >= n;  // not this rank's rows, or strictly above the diagonal
  }
  __device__ __forceinline__ T at(int64_t gi, int64_t gj) const { return Kc[gi * R + (gj - c0)]; }
};

// One 128x128 tile (rows tr * 128 .., columns src.first_col() + tc * 128 ..) of
//   sum w_ij (alpha_i alpha_j - Kinv_ij) dK_ij/dtheta,  w = 1/2 on the diagonal, 1 strictly below it, 0 above
// (the 1/2 of 1/2 tr(G dK) folded with symmetry), for each of the evaluator's NSUM derivatives:
// partial[s * ntiles + tile] gets the tile's sum (zero for a tile that does not contribute); fixed LDS tree ->
// deterministic.
template <typename T, typename Eval, typename Src>
__global__ __launch_bounds__(256) void kgrad_tile_kernel(Eval ev, Src src, int64_t n, int d,
                                                         const T* __restrict__ X, const T* __restrict__ alpha,
                                                         double* __restrict__ partial) {
  constexpr int NSUM = Eval::NSUM;
  const int tr = blockIdx.x, tc = blockIdx.y;
  const int tile_id = tr * gridDim.y + tc, ntiles = gridDim.x * gridDim.y;
  const int64_t r0 = int64_t(tr) * KT, c0 = src.first_col() + int64_t(tc) * KT;
  if (src.skip(r0, c0, n)) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int s = 0; s < NSUM; ++s) partial[s * ntiles + tile_id] = 0.0;
    }
    return;
  }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* s1 = reinterpret_cast<T*>(smem);  // [KT][d]
  T* s2 = s1 + KT * d;                 // [KT][d]
  load_tile_pair(s1, s2, X, X, r0, c0, n, n, d);
  const int il = threadIdx.x & (KT - 1), g = threadIdx.x >> 7;
  const int64_t gi = r0 + il;
  const T ai = (gi < n) ? alpha[gi] : T(0);
  double acc[NSUM] = {};
  if (gi < n) {
    for (int c = 0; c < KT / 2; ++c) {
      const int jl = g * (KT / 2) + c;
      const int64_t gj = c0 + jl;
      if (gj >= n || gj > gi) continue;
      typename Eval::Pair p;
      T r1, r2, r3;
      pair_dist<T, Eval::FAMILY, 0>(s1 + il * d, s2 + jl * d, d, r1, r2, r3,
                                    [&](int t, T dx, T a, T b) { ev.capture(p, t, dx, a, b); });
      ev.add_sums(p, r1, r2, r3, ai * alpha[gj] - src.at(gi, gj), gi == gj ? 0.5 : 1.0, acc);
    }
  }
  block_sum<256, NSUM>(acc);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NSUM; ++s) partial[s * ntiles + tile_id] = acc[s];
  }
}

// *out = sum(partial), or *out += sum(partial) (one workgroup, fixed tree: deterministic)
template <bool ACCUMULATE>
__global__ __launch_bounds__(1024) void sum_partials_kernel(int64_t count, const double* __restrict__ partial,
                                                            double* __restrict__ out) {
  double acc[1] = {0};
  for (int64_t i = threadIdx.x; i < count; i += 1024) acc[0] += partial[i];
  block_sum<1024, 1>(acc);
  if (threadIdx.x == 0) {
    if constexpr (ACCUMULATE) *out += acc[0];
    else *out = acc[0];
  }
}

// diag[c0 + r] = Kc[c0 + r, r] for the chunk's columns (K^-1_jj: the noise gradient's second term)
template <typename T>
__global__ __launch_bounds__(256) void kcols_diag_kernel(int64_t n, const T* __restrict__ Kc, int64_t R, int64_t c0,
                                                         T* __restrict__ diag) {
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (r < R && c0 + r < n) diag[c0 + r] = Kc[(c0 + r) * R + r];
}

// d loglik / d noise_i = 1/2 (alpha_i^2 - Kinv_ii)
template <typename T>
__global__ __launch_bounds__(256) void noise_grad_kernel(int64_t n, const T* __restrict__ alpha,
                                                         const T* __restrict__ Kinv, int64_t ld,
                                                         T* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) out[i] = T(0.5) * (alpha[i] * alpha[i] - Kinv[i * ld + i]);
}

// FAM: 0, or 2 (kfamily()): the dot-product leaves read the point itself, r3 = sum x_ik^2
template <typename T, int FAM>
__global__ __launch_bounds__(256) void kdiag_kernel(KProg kp, int64_t n, int d, const T* __restrict__ X,
                                                    const T* __restrict__ add, T* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  // evaluate_diag = evaluate(x, x) (base.py:59-66): every distance is exactly zero
  T r3 = 0;
  if constexpr (FAM == 2) {
    for (int t = 0; t < d; ++t) r3 += X[i * d + t] * X[i * d + t];
  }
  (void)d;
  (void)X;
  T v = eval_kprog<T, FAM>(kp, T(0), T(0), r3);
  if (add != nullptr) v += add[i];
  out[i] = v;
}

// Fused K9: partial[chunk][r][i] = sum_{j in chunk} k(X1[i], X2[j]) v[r][j] for up to GV_NV
// right-hand sides at once (every kernel value is evaluated ONCE per pass, whatever the number
// of columns of `y` in Kernel.matmul).  One lane per row i, X2 / v chunks staged through LDS and
// broadcast-read.  Eval: GeneralEval, or FastEval with its inner loop unrolled twice.
constexpr int GV_ROWS = 256, GV_JB = 256, GV_NV = 8;
template <typename T, typename Eval>
__global__ __launch_bounds__(256) void kmat_gemv_kernel(Eval ev, int64_t n1, int64_t n2, int d,
                                                        const T* __restrict__ X1,
                                                        const T* __restrict__ X2,
                                                        const T* __restrict__ v, int nv,
                                                        T* __restrict__ partial, int64_t jchunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sx = reinterpret_cast<T*>(smem);  // [GV_JB][d]
  T* sv = sx + GV_JB * d;              // [GV_JB][GV_NV]
  const int64_t i = int64_t(blockIdx.x) * GV_ROWS + threadIdx.x;
  const int64_t j0 = int64_t(blockIdx.y) * jchunk;
  const int64_t j1 = (j0 + jchunk < n2) ? j0 + jchunk : n2;
  T xi[TGP_MAX_DIM];
#pragma unroll
  for (int t = 0; t < TGP_MAX_DIM; ++t) xi[t] = (t < d && i < n1) ? X1[i * d + t] : T(0);
  T acc[GV_NV];
#pragma unroll
  for (int r = 0; r < GV_NV; ++r) acc[r] = 0;
  for (int64_t jb = j0; jb < j1; jb += GV_JB) {
    const int cnt = int((j1 - jb < GV_JB) ? (j1 - jb) : GV_JB);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt * d; t += 256) sx[t] = X2[jb * d + t];
    for (int t = threadIdx.x; t < cnt * GV_NV; t += 256) {
      const int jj = t / GV_NV, r = t % GV_NV;
      sv[t] = (r < nv) ? v[int64_t(r) * n2 + jb + jj] : T(0);
    }
    __syncthreads();
#pragma unroll Eval::UNROLL
    for (int jj = 0; jj < cnt; ++jj) {
      T r1, r2, r3;
      pair_dist<T, Eval::FAMILY, TGP_MAX_DIM, true>(xi, sx + jj * d, d, r1, r2, r3);
      const T kv = ev.value(r1, r2, r3);
#pragma unroll
      for (int r = 0; r < GV_NV; ++r) acc[r] += kv * sv[jj * GV_NV + r];
    }
  }
  if (i < n1)
    for (int r = 0; r < nv; ++r) partial[(int64_t(blockIdx.y) * nv + r) * n1 + i] = acc[r];
}

// out[r][i] = sum over chunks, fixed order
template <typename T>
__global__ __launch_bounds__(256) void reduce_partials_kernel(int64_t n1, int nchunks, int nv,
                                                              const T* __restrict__ partial,
                                                              T* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (i >= n1) return;
  T acc = 0;
  for (int c = 0; c < nchunks; ++c) acc += partial[(int64_t(c) * nv + r) * n1 + i];
  out[int64_t(r) * n1 + i] = acc;
}

}  // namespace

int make_kprog(const tgp_kop* prog, int nops, KProg* out) {
  TGP_ARG_CHECK(prog != nullptr && nops >= 1 && nops <= TGP_KPROG_MAX,
                "kernel program must have 1..%d ops (got %d)", TGP_KPROG_MAX, nops);
  int depth = 0;
  out->n = nops;
  for (int i = 0; i < nops; ++i) {
    const int op = prog[i].op;
    if (op == TGP_K_ADD || op == TGP_K_MUL) {
      TGP_ARG_CHECK(depth >= 2, "kernel program: stack underflow at op %d", i);
      depth -= 1;
    } else if (op == TGP_K_POW) {  // unary: replaces the top of the stack
      TGP_ARG_CHECK(depth >= 1, "kernel program: stack underflow at op %d", i);
    } else {
      TGP_ARG_CHECK(op >= TGP_K_CONST && op <= TGP_K_DOT, "kernel program: bad opcode %d at %d", op, i);
      TGP_ARG_CHECK(prog[i].metric == TGP_METRIC_L1 || prog[i].metric == TGP_METRIC_L2,
                    "kernel program: bad metric at op %d", i);
      TGP_ARG_CHECK(op != TGP_K_DOT || prog[i].metric == TGP_METRIC_L1,
                    "kernel program: DOT takes no metric (TGP_METRIC_L1) at op %d", i);
      depth += 1;
      TGP_ARG_CHECK(depth <= TGP_KSTACK_MAX, "kernel program: stack deeper than %d", TGP_KSTACK_MAX);
    }
    out->op[i] = op;
    out->metric[i] = prog[i].metric;
    out->p0[i] = prog[i].p0;
    out->p1[i] = prog[i].p1;
  }
  TGP_ARG_CHECK(depth == 1, "kernel program leaves %d values on the stack", depth);
  return TGP_OK;
}

// only Constant / Exp / ExpSquared / Matern leaves (+ sums and products): the FAM = 1 kernels
static bool exp_family(const KProg& kp) {
  for (int i = 0; i < kp.n; ++i) {
    const int op = kp.op[i];
    if (!(op == TGP_K_CONST || op == TGP_K_EXP || op == TGP_K_EXPSQ || op == TGP_K_M32 ||
          op == TGP_K_M52 || op == TGP_K_ADD || op == TGP_K_MUL))
      return false;
  }
  return true;
}

// the program family of the general kernels: 2 with a DOT leaf or a POW (the only family whose
// loops accumulate sum x_ik x_jk and know a unary op), else 1 for exp_family, else 0
static int kfamily(const KProg& kp) {
  for (int i = 0; i < kp.n; ++i)
    if (kp.op[i] == TGP_K_DOT || kp.op[i] == TGP_K_POW) return 2;
  return exp_family(kp) ? 1 : 0;
}

// ---- run-time values to template arguments: f is a generic lambda taking std::integral_constants ----------------
template <int V> using IC = std::integral_constant<int, V>;

// f(OP, L2) for the leaf and metric of a fast program (fp.op >= 0)
template <typename F>
static void with_fast_leaf(const FastProg& fp, F&& f) {
  auto with_metric = [&](auto op) {
    if (fp.l2) f(op, IC<1>{});
    else f(op, IC<0>{});
  };
  switch (fp.op) {
    case TGP_K_EXP: with_metric(IC<TGP_K_EXP>{}); break;
    case TGP_K_EXPSQ: with_metric(IC<TGP_K_EXPSQ>{}); break;
    case TGP_K_M32: with_metric(IC<TGP_K_M32>{}); break;
    default: with_metric(IC<TGP_K_M52>{}); break;
  }
}

// f(FAM) for the program's family; entry points without an exp-family instantiation (EXP_FAMILY = false: the
// gradient and the diagonal) take the general one, FAM = 0, for those programs
template <bool EXP_FAMILY, typename F>
static void with_family(const KProg& kp, F&& f) {
  const int fam = kfamily(kp);
  if (fam == 2) return f(IC<2>{});
  if constexpr (EXP_FAMILY) {
    if (fam == 1) return f(IC<1>{});
  }
  f(IC<0>{});
}

// f(D) with D = d up to MAXD (3 or 4); beyond it D = 0, the dynamic loop, where MAXD = 4, and nothing where MAXD = 3
// (kmat_fast_kernel has no such form)
template <int MAXD, typename F>
static void with_dim(int d, F&& f) {
  if (d == 1) f(IC<1>{});
  else if (d == 2) f(IC<2>{});
  else if (d == 3) f(IC<3>{});
  else if constexpr (MAXD == 4) {
    if (d == 4) f(IC<4>{});
    else f(IC<0>{});
  }
}

template <typename T>
int launch_kmat_cols(tgp_ctx* ctx, hipStream_t st, const KProg& kp, int64_t n1, int64_t n2, int d,
                     const T* X1, const T* X2, const T* diag, T* out, int64_t ld, int64_t rows_out,
                     int64_t cols_out, int flags, int64_t tc0, int64_t ntc) {
  TGP_ARG_CHECK(d >= 1 && d <= TGP_MAX_DIM, "input dimension must be 1..%d (got %d)", TGP_MAX_DIM, d);
  TGP_ARG_CHECK(rows_out >= n1 && cols_out >= n2 && ld >= rows_out, "kmat: bad output extents");
  if (rows_out == 0 || cols_out == 0 || ntc <= 0) return TGP_OK;
  const int64_t tr = (rows_out + KT - 1) / KT, tc = (cols_out + KT - 1) / KT;
  TGP_ARG_CHECK(tc0 >= 0 && tc0 + ntc <= tc, "kmat: column tile range outside the matrix");
  if (ctx->trace) {  // v: first column tile, number of column tiles, ld, flags
    trace_push(ctx, 7, st, tc0, ntc, ld, flags);
    return TGP_OK;
  }
  TGP_ARG_CHECK(ntc <= 65535, "kmat: too many column tiles");
  // full tiles of "leaf" / "amp * leaf" programs: the straight-line kernel
  int ftr = 0, ftc = 0;
  const FastProg fp = fast_prog(kp);
  // (its 16-byte stores need an even leading dimension and a 16-byte aligned matrix)
  if (fp.op >= 0 && d <= 3 && ld % 2 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) {
    ftr = int(n1 / KT);
    ftc = int(n2 / KT);
    const int64_t fc = std::min<int64_t>(tc0 + ntc, ftc) - tc0;  // column tiles of this call that are full
    // lower-only: column tile c holds the row tiles c .. ftr-1 (the matrix is square there)
    const int64_t tri_h = (flags & KMAT_LOWER) ? ftr - tc0 : 0;
    const int64_t tri_c = std::min<int64_t>(fc, tri_h);  // columns of this call with a tile on or below the diagonal
    const bool any = (flags & KMAT_LOWER) ? (tri_c > 0) : (ftr > 0 && fc > 0);
    if (any) {
      dim3 fgrid((unsigned)ftr, (unsigned)fc);
      if (flags & KMAT_LOWER) fgrid = dim3((unsigned)(tri_c * tri_h - tri_c * (tri_c - 1) / 2));
      const int fflags = flags | (ctx->kmat_plain_div != 0 ? KMAT_PLAIN_DIV : 0);
      with_dim<3>(d, [&](auto dd) {
        with_fast_leaf(fp, [&](auto op, auto l2) {
          constexpr int D = decltype(dd)::value, OP = decltype(op)::value, L2 = decltype(l2)::value;
          hipLaunchKernelGGL((kmat_fast_kernel<T, D, OP, L2>), fgrid, dim3(256), 0, st, T(fp.p0), T(fp.amp), n1, n2, X1,
                             X2, diag, out, ld, fflags, (int)tc0, (int)tri_h);
        });
      });
    } else {
      ftr = ftc = 0;
    }
    if (ftr == tr && ftc >= tc0 + ntc) {  // nothing ragged left
      TGP_HIP_TRY(hipGetLastError());
      return TGP_OK;
    }
  }
  dim3 grid((unsigned)tr, (unsigned)ntc);
  const size_t shmem = 2 * size_t(KT) * d * sizeof(T);
  with_dim<4>(d, [&](auto dd) {
    with_family<true>(kp, [&](auto fam) {
      constexpr int D = decltype(dd)::value, FAM = decltype(fam)::value;
      hipLaunchKernelGGL((kmat_kernel<T, D, FAM>), grid, dim3(256), shmem, st, kp, n1, n2, d, X1, X2, diag, out, ld,
                         rows_out, cols_out, flags, (int)tc0, ftr, ftc);
    });
  });
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

template <typename T>
int launch_kmat(tgp_ctx* ctx, const KProg& kp, int64_t n1, int64_t n2, int d, const T* X1,
                const T* X2, const T* diag, T* out, int64_t ld, int64_t rows_out, int64_t cols_out,
                int flags) {
  return launch_kmat_cols<T>(ctx, ctx->stream, kp, n1, n2, d, X1, X2, diag, out, ld, rows_out,
                             cols_out, flags, 0, (cols_out + KT - 1) / KT);
}

template <typename T>
int launch_kdiag(tgp_ctx* ctx, const KProg& kp, int64_t n, int d, const T* X, const T* add, T* out) {
  if (n == 0) return TGP_OK;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (kfamily(kp) == 2)
    TGP_ARG_CHECK(X != nullptr && d >= 1 && d <= TGP_MAX_DIM, "kdiag: a DOT program needs the points");
  with_family<false>(kp, [&](auto fam) {
    constexpr int FAM = decltype(fam)::value;
    hipLaunchKernelGGL((kdiag_kernel<T, FAM>), grid, dim3(256), 0, ctx->stream, kp, n, d, X, add, out);
  });
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// out (nv x n1, row-major) = [K(X1, X2) v_r]_r for the nv vectors v (nv x n2, row-major)
template <typename T>
int launch_kmat_gemv_multi(tgp_ctx* ctx, const KProg& kp, int64_t n1, int64_t n2, int d, const T* X1,
                           const T* X2, const T* v, int64_t nv_total, T* out) {
  TGP_ARG_CHECK(d >= 1 && d <= TGP_MAX_DIM, "input dimension must be 1..%d (got %d)", TGP_MAX_DIM, d);
  if (n1 == 0 || nv_total == 0) return TGP_OK;
  const int64_t rb = (n1 + GV_ROWS - 1) / GV_ROWS;
  // enough column chunks to fill the chip when there are few rows of test points
  int64_t nch = (2048 + rb - 1) / rb;
  const int64_t max_ch = (n2 + GV_JB - 1) / GV_JB;
  if (nch > max_ch) nch = max_ch;
  if (nch < 1) nch = 1;
  if (nch > 65535) nch = 65535;
  int64_t jchunk = round_up((n2 + nch - 1) / nch, GV_JB);
  if (jchunk < GV_JB) jchunk = GV_JB;
  nch = (n2 + jchunk - 1) / jchunk;
  if (nch < 1) nch = 1;
  TGP_TRY(ensure_work(ctx, size_t(nch) * GV_NV * n1 * sizeof(T)));
  T* partial = static_cast<T*>(ctx->d_work);
  const size_t shmem = size_t(GV_JB) * (d + GV_NV) * sizeof(T);
  for (int64_t r0 = 0; r0 < nv_total; r0 += GV_NV) {
    const int nv = int(std::min<int64_t>(GV_NV, nv_total - r0));
    auto launch = [&](auto ev) {
      hipLaunchKernelGGL((kmat_gemv_kernel<T, decltype(ev)>), dim3((unsigned)rb, (unsigned)nch), dim3(256), shmem,
                         ctx->stream, ev, n1, n2, d, X1, X2, v + r0 * n2, nv, partial, jchunk);
    };
    const FastProg fp = fast_prog(kp);
    if (fp.op >= 0)
      with_fast_leaf(fp, [&](auto op, auto l2) {
        launch(FastEval<T, decltype(op)::value, decltype(l2)::value>{T(fp.p0), T(fp.amp)});
      });
    else
      with_family<true>(kp, [&](auto fam) { launch(GeneralEval<T, decltype(fam)::value>{kp, 0, 0}); });
    hipLaunchKernelGGL((reduce_partials_kernel<T>), dim3((unsigned)((n1 + 255) / 256), (unsigned)nv), dim3(256), 0,
                       ctx->stream, n1, (int)nch, nv, partial, out + r0 * n1);
  }
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

template <typename T>
int launch_kmat_gemv(tgp_ctx* ctx, const KProg& kp, int64_t n1, int64_t n2, int d, const T* X1,
                     const T* X2, const T* v, T* out) {
  return launch_kmat_gemv_multi<T>(ctx, kp, n1, n2, d, X1, X2, v, 1, out);
}

// The gradient launchers' common body: kgrad_tile_kernel over tr x tc tiles, then each of the evaluator's sums over
// the tiles into out[s] (added to it where the source accumulates).
template <typename T, typename Eval, typename Src>
static int run_kgrad(tgp_ctx* ctx, const Eval& ev, const Src& src, int64_t tr, int64_t tc, int64_t n, int d,
                     const T* X, const T* alpha, double* out) {
  const int64_t tiles = tr * tc;
  TGP_TRY(ensure_work(ctx, Eval::NSUM * size_t(tiles) * sizeof(double)));
  double* partial = static_cast<double*>(ctx->d_work);
  const size_t shmem = 2 * size_t(KT) * d * sizeof(T);
  hipLaunchKernelGGL((kgrad_tile_kernel<T, Eval, Src>), dim3((unsigned)tr, (unsigned)tc), dim3(256), shmem,
                     ctx->stream, ev, src, n, d, X, alpha, partial);
  for (int s = 0; s < Eval::NSUM; ++s)
    hipLaunchKernelGGL((sum_partials_kernel<Src::ACCUMULATE>), dim3(1), dim3(1024), 0, ctx->stream, tiles,
                       partial + s * tiles, out + s);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

template <typename T>
int launch_kgrad(tgp_ctx* ctx, const KProg& kp, int which_op, int which_param, int64_t n, int d,
                 const T* X, const T* alpha, const T* Kinv, int64_t ld, double* out_dev) {
  const int64_t tiles = (n + KT - 1) / KT;
  TGP_ARG_CHECK(tiles <= 65535, "kgrad: too many tiles");
  int rc = TGP_OK;
  with_family<false>(kp, [&](auto fam) {
    const GeneralEval<T, decltype(fam)::value> ev{kp, which_op, which_param};
    rc = run_kgrad<T>(ctx, ev, SquareKinv<T>{Kinv, ld}, tiles, tiles, n, d, X, alpha, out_dev);
  });
  return rc;
}

// out_accum[0] += this rank's share of  sum_{i >= j, j in chunk} w_ij (alpha_i alpha_j - Kinv_ij) dK_ij / dtheta  over the
// chunk of R columns from c0 (Kc: (n_pad, R) row-major)
template <typename T>
int launch_kgrad_cols(tgp_ctx* ctx, const KProg& kp, int which_op, int which_param, int64_t n, int d, const T* X,
                      const T* alpha, const T* Kc, int64_t R, int64_t c0, int64_t nb, int G, int rank,
                      double* out_accum) {
  const int64_t tr = (n + KT - 1) / KT, tc = (std::min<int64_t>(R, n - c0) + KT - 1) / KT;
  TGP_ARG_CHECK(tr <= 65535 && tc >= 1 && tc <= 65535 && c0 % KT == 0, "kgrad_cols: bad chunk");
  int rc = TGP_OK;
  with_family<false>(kp, [&](auto fam) {
    const GeneralEval<T, decltype(fam)::value> ev{kp, which_op, which_param};
    rc = run_kgrad<T>(ctx, ev, ChunkKinv<T>{Kc, R, c0, nb, G, rank}, tr, tc, n, d, X, alpha, out_accum);
  });
  return rc;
}

template <typename T>
int launch_kcols_diag(tgp_ctx* ctx, int64_t n, const T* Kc, int64_t R, int64_t c0, T* diag) {
  hipLaunchKernelGGL((kcols_diag_kernel<T>), dim3((unsigned)((R + 255) / 256)), dim3(256), 0, ctx->stream, n, Kc, R, c0,
                     diag);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// Gradient sums of a "leaf" / "amp * leaf" program in one pass: out_dev[0] = d/d(constant) (only
// meaningful when the program has one), out_dev[1] = d/d(scale).  Returns 1 when the program is
// of that shape (*leaf / *konst = their positions, -1: none), 0 when the caller must use launch_kgrad.
template <typename T>
int launch_kgrad_fast(tgp_ctx* ctx, const KProg& kp, int64_t n, int d, const T* X, const T* alpha,
                      const T* Kinv, int64_t ld, double* out_dev, int* leaf, int* konst) {
  const FastProg fp = fast_prog(kp);
  if (fp.op < 0) return 0;
  const int64_t tiles = (n + KT - 1) / KT;
  TGP_ARG_CHECK(tiles <= 65535, "kgrad: too many tiles");
  int rc = TGP_OK;
  with_fast_leaf(fp, [&](auto op, auto l2) {
    const FastEval<T, decltype(op)::value, decltype(l2)::value> ev{T(fp.p0), T(fp.amp)};
    rc = run_kgrad<T>(ctx, ev, SquareKinv<T>{Kinv, ld}, tiles, tiles, n, d, X, alpha, out_dev);
  });
  if (rc != TGP_OK) return rc;
  *leaf = fp.leaf;
  *konst = fp.konst;
  return 1;
}

template <typename T>
int launch_noise_grad(tgp_ctx* ctx, int64_t n, const T* alpha, const T* Kinv, int64_t ld, T* out) {
  hipLaunchKernelGGL((noise_grad_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     ctx->stream, n, alpha, Kinv, ld, out);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

#define TGP_INST(T)                                                                               \
  template int launch_kgrad_cols<T>(tgp_ctx*, const KProg&, int, int, int64_t, int, const T*, const T*, const T*,   \
                                    int64_t, int64_t, int64_t, int, int, double*);                                  \
  template int launch_kcols_diag<T>(tgp_ctx*, int64_t, const T*, int64_t, int64_t, T*);                            \
  template int launch_kgrad<T>(tgp_ctx*, const KProg&, int, int, int64_t, int, const T*, const T*, \
                               const T*, int64_t, double*);                                       \
  template int launch_noise_grad<T>(tgp_ctx*, int64_t, const T*, const T*, int64_t, T*);          \
  template int launch_kgrad_fast<T>(tgp_ctx*, const KProg&, int64_t, int, const T*, const T*,     \
                                    const T*, int64_t, double*, int*, int*);                      \
  template int launch_kmat<T>(tgp_ctx*, const KProg&, int64_t, int64_t, int, const T*, const T*,  \
                              const T*, T*, int64_t, int64_t, int64_t, int);                      \
  template int launch_kmat_cols<T>(tgp_ctx*, hipStream_t, const KProg&, int64_t, int64_t, int,    \
                                   const T*, const T*, const T*, T*, int64_t, int64_t, int64_t,   \
                                   int, int64_t, int64_t);                                        \
  template int launch_kdiag<T>(tgp_ctx*, const KProg&, int64_t, int, const T*, const T*, T*);     \
  template int launch_kmat_gemv<T>(tgp_ctx*, const KProg&, int64_t, int64_t, int, const T*,       \
                                   const T*, const T*, T*);                                       \
  template int launch_kmat_gemv_multi<T>(tgp_ctx*, const KProg&, int64_t, int64_t, int, const T*, \
                                         const T*, const T*, int64_t, T*);
TGP_INST(float)
TGP_INST(double)
#undef TGP_INST

}  // namespace tgp
