// small.hip -- batches of SMALL dense problems, one workgroup each (tgp_small_logprob, tgp_small_logprob_grad,
// tgp_small_predict, tgp_small_condition).
//
// The dense path of chol.hip pads every matrix to 128-row tiles and pays a handle, uploads, a launch chain and a host
// join per evaluation: at N <= 192 that is all overhead.  Here a workgroup of 256 threads owns a whole member: it
// assembles K + diag(noise) in LDS with the general evaluator of kprog_eval.h, factors it there, carries the residual
// through the same eliminations and writes back ONE number.  Nothing crosses workgroups: a member's value depends on
// that member's data alone, whatever the batch around it.
//
// Layout (dynamic LDS, doubles).  The residual is row n of the matrix: the lower trapezoid of the (n + 1) x n array
// [K + diag(noise); r^T] is packed by columns, column j holding rows j .. n at
//   off(j) = j (n + 1) - j (j - 1) / 2,        n (n + 1) / 2 + n doubles in all,
// and the right-looking factorisation of the square part leaves z^T = (L^-1 r)^T in that last row: the step that
// scales column p below the pivot also forms z_p = (r_p - sum_{k < p} L_pk z_k) / L_pp, the rank-1 update of the
// columns right of p also takes z_p L_jp from r_j.  This IS the column-oriented forward substitution of L z = r, in
// its order, carried along by the factorisation's two barriers per column instead of 2 n more of its own.
//
// Every sum runs in an order fixed by the indices alone: entry (i, j) receives its updates p = 0, 1, .. j - 1 one
// after another from ONE thread per step (explicit FMAs; the file is built with -ffp-contract=off like kmat.hip, so
// that the kernel's entries are kmat.hip's to the bit), the two reductions are a fixed LDS tree.
//
// The gradient (small_grad_kernel) goes on in the same workgroup and the same LDS: alpha = K^-1 r by the backward
// substitution in row n, K^-1 in place in the packed triangle (L -> L^-1 -> L^-T L^-1, both as rank-1 updates in the
// access pattern of the factorisation), then one pass over the entries i >= j per derivative with the evaluators of
// kprog_eval.h.  The assembly, the factorisation and the two value reductions are ONE text for both kernels: the
// gradient kernel's value has the bits of small_logprob_kernel's.
//
// The prediction (small_predict_kernel) shares the value's text and the gradient's alpha (small_alpha); L and alpha
// then stay in LDS, read-only, and every wave walks test points of its own without another barrier: the cross
// covariances of a point in registers, the mean as their product with alpha, the variance by a forward substitution
// against L inside the wave.
//
// The conditional covariance and joint draws (small_condition_kernel) carry the m test points as further COLUMNS of
// the same trapezoid, P = n + m columns and the residual in row P: the first n steps of the one elimination leave the
// Schur complement Sigma* = k** + diag(tau) - A^T A in the trailing triangle and -mu* in row P behind it, a second
// phase of the same steps on that triangle is its Cholesky factor, and a draw is a triangular product per wave.
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "tgp_common.h"
#include "kprog_eval.h"

namespace tgp {

namespace {

constexpr int SMALL_THREADS = 256;
constexpr int SMALL_WAVES = SMALL_THREADS / 64;
constexpr int64_t SMALL_STAGE_BYTES = int64_t(1) << 30;  // staging per launch, the cap of the quasisep batches (qsep.hip)

// one member of a launch; offsets in elements from the launch's X (rows of d doubles), noise and residual arrays
// (the gradient's outputs: noise gradient and alpha at noise_off like the inputs, the parameter gradients at gp_off,
// the per-dimension scale gradients at member * d; want_dims: this member asks for the latter)
struct SmallRow {
  int64_t x_off, noise_off, resid_off, gp_off;
  int32_t n, d, prog, want_dims;
};
static_assert(sizeof(SmallRow) == 48 && sizeof(KProg) % 8 == 0, "the staging buffer is carved in 8-byte units");

// one table row of a prediction launch: a member, or one chunk of a member's test points (every chunk factors the
// member again).  The member's fields as in SmallRow; xt_off in rows of the launch's Xt and out_off in the launch's
// mean / variance arrays, both at this chunk's first point; m: this chunk's points (0 .. TGP_SMALL_PRED_CHUNK);
// pred_prog: the program of k* and k**, or -1 for the member's own; slot: where the value and info go, -1 for every
// chunk but a member's first
struct SmallPredRow {
  int64_t x_off, noise_off, resid_off, xt_off, out_off;
  int32_t n, d, prog, pred_prog, m, slot;
};
static_assert(sizeof(SmallPredRow) == 64, "the staging buffer is carved in 8-byte units");

// one table row of a conditioning launch: a member with its m test points as columns n .. n + m - 1.  The member's
// fields as in SmallRow; xt_off in rows of the launch's Xt; tvec_off into the launch's test diagonal and means (m
// entries); cov_off into its covariances (m^2 entries); xi_off into its normals and samples (S m entries, draw-major);
// pred_prog: the program of the rows >= n, or -1 for the member's own; S: the draws asked for
struct SmallCondRow {
  int64_t x_off, noise_off, resid_off, xt_off, tvec_off, cov_off, xi_off;
  int32_t n, d, prog, pred_prog, m, S;
};
static_assert(sizeof(SmallCondRow) == 80, "the staging buffer is carved in 8-byte units");

// test points a wave carries through the forward substitution at once (one LDS read of l_ip feeds this many FMAs)
#ifndef TGP_SMALL_PRED_T
#define TGP_SMALL_PRED_T 4
#endif
constexpr int SMALL_PRED_T = TGP_SMALL_PRED_T;
static_assert(SMALL_PRED_T == 1 || SMALL_PRED_T == 2 || SMALL_PRED_T == 4, "T is chosen from {1, 2, 4}");
constexpr int SMALL_PRED_ROWS = (TGP_SMALL_MAX_N + 63) / 64;  // rows of a member one lane holds in registers

__host__ __device__ constexpr int64_t small_lds_doubles(int64_t n) { return n * (n + 1) / 2 + n; }
static_assert(small_lds_doubles(TGP_SMALL_MAX_N) * 8 + 2 * SMALL_THREADS * 8 <= 163840,
              "a member at the cap, with the reduction scratch, fits the 160 KiB of one workgroup");

__device__ __forceinline__ int col_off(int j, int n) { return j * (n + 1) - j * (j - 1) / 2; }

// Steps 1 - 4 of a member: assemble the trapezoid [K + diag(noise); r^T] in A, factor it there.  Returns 0, or the
// 1-based index of the first pivot that is not > 0 -- the same number in every thread of the workgroup.
// COND (small_condition_kernel): the trapezoid has P = n + m columns and its residual in row P,
//   [ k(X, X) + diag(noise)            .            ]   rows 0 .. n - 1
//   [ pk(X*, X)          pk(X*, X*) + diag(tau)     ]   rows n .. P - 1
//   [ r^T                           0^T             ]   row P
// and the SAME n elimination steps run over all P columns and P + 1 rows: entry (i, j) with i, j < n and row P in the
// first n columns receive the operations of the plain form in its order (the value's bits do not change), the
// trailing triangle becomes the Schur complement and row P behind column n becomes -mu*.
template <bool COND = false>
__device__ __forceinline__ int small_assemble_factor(double* A, const KProg& kp, const double* x, const double* nz,
                                                     const double* rs, int n, int d, const KProg* pk = nullptr,
                                                     const double* xt = nullptr, const double* tau = nullptr,
                                                     int m = 0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int P = COND ? n + m : n;

  // 1 + 2: wave w assembles columns w, w + 4, ..; lane l their rows j + l, j + l + 64, ..; row P is the residual
  for (int j = wave; j < P; j += SMALL_WAVES) {
    double* col = A + col_off(j, P);
    const bool tj = COND && j >= n;
    const double* b = tj ? xt + int64_t(j - n) * d : x + int64_t(j) * d;
    for (int i = j + lane; i <= P; i += 64) {
      double v;
      if (i == P) {
        v = tj ? 0.0 : rs[j];
      } else {
        const bool ti = COND && i >= n;
        const double* a = ti ? xt + int64_t(i - n) * d : x + int64_t(i) * d;
        double r1, r2, r3;
        pair_dist<double, 2, 0>(a, b, d, r1, r2, r3);
        v = eval_kprog<double, 2>(ti ? *pk : kp, r1, r2, r3);
        if (i == j) v += tj ? tau[j - n] : nz[j];  // noise.py:77-78 fused, as in kmat_kernel
      }
      col[i - j] = v;
    }
  }
  __syncthreads();

  // 3 + 4: right-looking, column by column.  The pivot is read by every thread from the same LDS word: the decision to
  // leave is the workgroup's, no barrier sits under divergent control flow.
  int fail = 0;
  for (int p = 0; p < n; ++p) {
    double* cp = A + col_off(p, P);
    const double pivot = cp[0];
    if (!(pivot > 0.0)) {
      fail = p + 1;
      break;
    }
    // (the diagonal word keeps the pivot L_pp^2: a thread may still be reading it while the column is scaled)
    const double lpp = sqrt(pivot);
    for (int i = p + 1 + int(threadIdx.x); i <= P; i += SMALL_THREADS) cp[i - p] = cp[i - p] / lpp;
    __syncthreads();
    for (int j = p + 1 + wave; j < P; j += SMALL_WAVES) {
      double* col = A + col_off(j, P);
      const double ljp = cp[j - p];
      for (int i = j + lane; i <= P; i += 64) col[i - j] = __builtin_fma(-cp[i - p], ljp, col[i - j]);
    }
    __syncthreads();
  }
  return fail;
}

// Steps 5 + 6: the value from the factored trapezoid (the pivots on the diagonal, z in row n), written by thread 0 to
// entry `slot` of out and info (a negative slot: computed, not written -- a later chunk of a prediction).  P: the
// columns of the trapezoid (n, or n + m for small_condition_kernel: the value comes from the first n columns alone).
__device__ __forceinline__ void small_write_value(const double* A, double (&red)[2][SMALL_THREADS], int n, int fail,
                                                  double* __restrict__ out, int32_t* __restrict__ info, int64_t slot,
                                                  int P) {
  // 5: sum log L_pp and sum z_p^2 (one term per thread: n < 256), a fixed tree
  double sl = 0.0, sz = 0.0;
  if (fail == 0 && int(threadIdx.x) < n) {
    const double* cp = A + col_off(int(threadIdx.x), P);
    const double z = cp[P - int(threadIdx.x)];
    sl = log(sqrt(cp[0]));
    sz = z * z;
  }
  red[0][threadIdx.x] = sl;
  red[1][threadIdx.x] = sz;
  __syncthreads();
  for (int sft = SMALL_THREADS / 2; sft > 0; sft >>= 1) {
    if (int(threadIdx.x) < sft) {
      red[0][threadIdx.x] += red[0][threadIdx.x + sft];
      red[1][threadIdx.x] += red[1][threadIdx.x + sft];
    }
    __syncthreads();
  }
  // 6
  if (threadIdx.x == 0 && slot >= 0) {
    const double v = -0.5 * red[1][0] - red[0][0] - 0.5 * double(n) * 1.8378770664093453;  // log(2 pi)
    out[slot] = fail ? __builtin_nan("") : v;
    info[slot] = fail;
  }
}

// Steps 7 + 8 of the gradient and of the prediction: the diagonal words become L_pp (they held the pivots L_pp^2),
// once; then alpha = K^-1 r by the backward substitution L^T alpha = z in place in row n: thread k carries z_k in a
// register and takes L_pk alpha_p from it for p = n - 1 .. k + 1, one barrier per step.  alpha_p lands where z_p was;
// the last barrier of the loop follows the last write.
__device__ __forceinline__ void small_alpha(double* A, int n) {
  const int tid = threadIdx.x;
  // 7
  if (tid < n) A[col_off(tid, n)] = sqrt(A[col_off(tid, n)]);
  __syncthreads();
  // 8
  double zk = tid < n ? A[col_off(tid, n) + n - tid] : 0.0;
  for (int p = n - 1; p >= 0; --p) {
    const double* cp = A + col_off(p, n);
    if (tid == p) A[col_off(p, n) + n - p] = zk / cp[0];
    __syncthreads();
    if (tid < p) zk = __builtin_fma(-A[col_off(tid, n) + p - tid], cp[n - p], zk);
  }
}

__global__ __launch_bounds__(SMALL_THREADS) void small_logprob_kernel(const SmallRow* __restrict__ rows,
                                                                        const KProg* __restrict__ progs,
                                                                        const double* __restrict__ X,
                                                                        const double* __restrict__ noise,
                                                                        const double* __restrict__ resid,
                                                                        double* __restrict__ out,
                                                                        int32_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double A[];  // the packed trapezoid
  __shared__ double red[2][SMALL_THREADS];
  const SmallRow row = rows[blockIdx.x];
  const KProg& kp = progs[row.prog];
  const int n = row.n, d = row.d;
  const int fail = small_assemble_factor(A, kp, X + row.x_off * d, noise + row.noise_off, resid + row.resid_off, n, d);
  small_write_value(A, red, n, fail, out, info, blockIdx.x, n);
}

// Value AND gradient of one member.  After the value (the text above):
//   7  the diagonal words become L_pp (they held the pivots L_pp^2), once;
//   8  alpha = K^-1 r: the backward substitution L^T alpha = z in place in row n.  Thread k carries z_k in a register
//      and takes L_pk alpha_p from it for p = n - 1 .. k + 1, one barrier per step;
//   9  W = L^-1 in place, column by column: column j below the diagonal becomes -L_ij / L_jj, then the block left of
//      it takes the rank-1 update B_ic += B_ij B_jc (i > j > c) -- the elimination of L W = I carried on all right-hand
//      sides at once, B_jc = L_jj W_jc; a last pass divides row j by L_jj and sets W_jj = 1 / L_jj;
//  10  K^-1 = W^T W in place: entry (i, k), k <= i, is sum_{m >= i} W_mi W_mk, and row m of W is last needed at step
//      m, so step m copies row m aside (the reduction scratch holds two rows: the copy of row m + 1 runs under step
//      m's update) and adds its outer product to the rows above it, entry (m, k) itself STARTING from W_mm W_mk;
//  11  per derivative one pass over the entries i >= j: g_ij = alpha_i alpha_j - K^-1_ij, weight 1/2 on the diagonal,
//      the pair's distances recomputed from the points, one fp64 accumulator per thread, the fixed tree, thread 0
//      writes; the noise gradient 1/2 (alpha_i^2 - K^-1_ii) and the mean gradient alpha, one entry per thread.
// Every entry receives its updates one after another from ONE thread per step, in the order of the step index; the
// loops' trip counts and every branch around a barrier depend on n, the program and `fail` alone.
__global__ __launch_bounds__(SMALL_THREADS) void small_grad_kernel(const SmallRow* __restrict__ rows,
                                                                     const KProg* __restrict__ progs,
                                                                     const double* __restrict__ X,
                                                                     const double* __restrict__ noise,
                                                                     const double* __restrict__ resid,
                                                                     double* __restrict__ out,
                                                                     int32_t* __restrict__ info,
                                                                     double* __restrict__ grad_params,
                                                                     double* __restrict__ grad_noise,
                                                                     double* __restrict__ alpha_out,
                                                                     double* __restrict__ grad_dims) {
  extern __shared__ __attribute__((aligned(16))) double A[];  // the packed trapezoid
  __shared__ double red[2][SMALL_THREADS];
  const SmallRow row = rows[blockIdx.x];
  const KProg& kp = progs[row.prog];
  const int n = row.n, d = row.d;
  const double* x = X + row.x_off * d;
  const int tid = threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* gp = grad_params + row.gp_off;
  double* gn = grad_noise + row.noise_off;
  double* ga = alpha_out + row.noise_off;
  double* gd = grad_dims + int64_t(blockIdx.x) * d;

  const int fail = small_assemble_factor(A, kp, x, noise + row.noise_off, resid + row.resid_off, n, d);
  small_write_value(A, red, n, fail, out, info, blockIdx.x, n);
  if (fail) {  // the workgroup's decision: NaN in every gradient of this member
    const double nan = __builtin_nan("");
    for (int t = tid; t < 2 * kp.n; t += SMALL_THREADS) gp[t] = nan;
    for (int t = tid; t < n; t += SMALL_THREADS) gn[t] = ga[t] = nan;
    for (int t = tid; t < d; t += SMALL_THREADS) gd[t] = nan;
    return;
  }
  __syncthreads();  // thread 0 has read the scratch

  // 7 + 8
  small_alpha(A, n);

  // 9 (rows j + 1 .. n - 1 only: row n is alpha's)
  for (int j = 0; j < n; ++j) {
    double* cj = A + col_off(j, n);
    const double ljj = cj[0];
    for (int i = j + 1 + tid; i < n; i += SMALL_THREADS) cj[i - j] = -(cj[i - j] / ljj);
    __syncthreads();
    for (int c = wave; c < j; c += SMALL_WAVES) {
      double* col = A + col_off(c, n);
      const double bjc = col[j - c];
      for (int i = j + 1 + lane; i < n; i += 64) col[i - c] = __builtin_fma(cj[i - j], bjc, col[i - c]);
    }
    __syncthreads();
  }
  for (int c = wave; c < n; c += SMALL_WAVES) {
    double* col = A + col_off(c, n);
    for (int i = c + 1 + lane; i < n; i += 64) col[i - c] = col[i - c] / A[col_off(i, n)];
  }
  __syncthreads();
  double* rowbuf = &red[0][0];  // two rows of up to SMALL_THREADS entries
  if (tid < n) {
    const double wjj = 1.0 / A[col_off(tid, n)];
    A[col_off(tid, n)] = wjj;
    if (tid == 0) rowbuf[0] = wjj;  // row 0 of W, for step 10
  }
  __syncthreads();

  // 10
  for (int m = 0; m < n; ++m) {
    const double* tm = rowbuf + (m & 1) * SMALL_THREADS;
    for (int k = wave; k <= m; k += SMALL_WAVES) {
      double* col = A + col_off(k, n);
      const double tk = tm[k];
      for (int i = k + lane; i <= m; i += 64) col[i - k] = (i == m) ? tm[i] * tk : __builtin_fma(tm[i], tk, col[i - k]);
    }
    if (m + 1 < n) {
      double* tn = rowbuf + ((m + 1) & 1) * SMALL_THREADS;
      for (int c = tid; c <= m + 1; c += SMALL_THREADS) tn[c] = A[col_off(c, n) + m + 1 - c];
    }
    __syncthreads();
  }

  // 11: the noise and mean gradients, then one pass per derivative: parameter q of op i is task 2 i + q (zero for
  // ADD / MUL and a p1 the leaf does not have, as in tgp_solver_grad), input dimension t is task 2 kp.n + t
  if (tid < n) {
    const double a = A[col_off(tid, n) + n - tid];
    gn[tid] = 0.5 * (a * a - A[col_off(tid, n)]);
    ga[tid] = a;
  }
  const int ntask = 2 * kp.n + d;
  for (int task = 0; task < ntask; ++task) {
    int which_op, which_param = 0;
    double* dst;
    if (task < 2 * kp.n) {
      which_op = task >> 1, which_param = task & 1;
      dst = gp + task;
      const int op = kp.op[which_op];
      const bool two = op == TGP_K_ESS || op == TGP_K_RQ || op == TGP_K_DOT;
      if (op == TGP_K_ADD || op == TGP_K_MUL || (which_param == 1 && !two)) {
        if (tid == 0) *dst = 0.0;
        continue;
      }
    } else {
      which_op = -1 - (task - 2 * kp.n);
      dst = gd + (task - 2 * kp.n);
      if (!row.want_dims) {
        if (tid == 0) *dst = 0.0;
        continue;
      }
    }
    double acc = 0.0;
    for (int j = wave; j < n; j += SMALL_WAVES) {
      const double* col = A + col_off(j, n);
      const double aj = col[n - j];
      for (int i = j + lane; i < n; i += 64) {
        const double gij = A[col_off(i, n) + n - i] * aj - col[i - j];
        double r1, r2, r3, dxd = 0.0, zz = 0.0;
        pair_dist<double, 2, 0>(x + int64_t(i) * d, x + int64_t(j) * d, d, r1, r2, r3,
                                [&](int t, double dx, double a, double b) {
                                  if (t == -1 - which_op) dxd = dx, zz = a * b;
                                });
        double w1 = 0.0, w2 = 0.0;
        if (which_op < 0) dim_weights<double>(dxd, r1, r2, w1, w2);
        const double dk = which_op >= 0 ? eval_kprog_deriv<double, 2>(kp, which_op, which_param, r1, r2, r3)
                                        : eval_kprog_deriv_dim<double, 2>(kp, r1, r2, w1, w2, r3, zz);
        acc += gij * dk * (i == j ? 0.5 : 1.0);
      }
    }
    red[0][tid] = acc;
    __syncthreads();
    for (int sft = SMALL_THREADS / 2; sft > 0; sft >>= 1) {
      if (tid < sft) red[0][tid] += red[0][tid + sft];
      __syncthreads();
    }
    if (tid == 0) *dst = red[0][0];
    __syncthreads();  // the next pass writes the scratch again
  }
}
static_assert(TGP_SMALL_MAX_N < SMALL_THREADS, "one reduction term per thread");

// Value and prediction of one table row.  After the value (steps 1 - 6, the text above) and alpha (small_alpha), L and
// alpha are read-only and no barrier follows: wave w takes the groups g = w, w + 4, .. of T test points
// t = g T .. g T + T - 1.  Lane l holds rows i = l, l + 64, l + 128 of every point of the group in registers:
//   k*   k*_i = k(x_i, x*) and k** = k(x*, x*) from ONE loop over the (row, point) pairs -- one inlined copy of the
//        evaluator, the registers picked by selects -- with the row's prediction program, or the member's own;
//   mean sum_i k*_i alpha_i: each lane adds its rows in increasing i, then the fixed 64-lane butterfly;
//   var  k** - sum_p v_p^2 with v = L^-1 k*, the column-oriented forward substitution inside the wave: for
//        p = 0 .. n - 1 the lanes divide their row of p's 64-row block by l_pp, the owner's quotient v_p = k_p / l_pp
//        is read from lane p mod 64 (p is wave-uniform), every lane takes l_ip v_p from its rows i > p by fma -- column p of L from LDS,
//        consecutive rows, ONE read for the T points -- and adds v_p^2 to a sum that every lane carries alike, in
//        increasing p.  Skipped when no variance is asked for.
// A point's arithmetic never looks at the other points of its group: the last, partial group computes its missing
// points on the chunk's last point and does not store them.  A failed pivot puts NaN into every prediction of the row.
template <int T>
__global__ __launch_bounds__(SMALL_THREADS) void small_predict_kernel(const SmallPredRow* __restrict__ rows,
                                                                        const KProg* __restrict__ progs,
                                                                        const double* __restrict__ X,
                                                                        const double* __restrict__ noise,
                                                                        const double* __restrict__ resid,
                                                                        const double* __restrict__ Xt,
                                                                        double* __restrict__ out,
                                                                        int32_t* __restrict__ info,
                                                                        double* __restrict__ mean_out,
                                                                        double* __restrict__ var_out) {
  extern __shared__ __attribute__((aligned(16))) double A[];  // the packed trapezoid
  __shared__ double red[2][SMALL_THREADS];
  const SmallPredRow row = rows[blockIdx.x];
  const KProg& kp = progs[row.prog];
  const KProg& pk = progs[row.pred_prog >= 0 ? row.pred_prog : row.prog];
  const int n = row.n, d = row.d, m = row.m;
  const double* x = X + row.x_off * d;
  const double* xt = Xt + row.xt_off * d;
  const int tid = threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* pm = mean_out + row.out_off;
  double* pv = var_out ? var_out + row.out_off : nullptr;

  const int fail = small_assemble_factor(A, kp, x, noise + row.noise_off, resid + row.resid_off, n, d);
  small_write_value(A, red, n, fail, out, info, row.slot, n);
  if (fail) {  // the workgroup's decision: NaN in every prediction of this row
    const double nan = __builtin_nan("");
    for (int t = tid; t < m; t += SMALL_THREADS) {
      pm[t] = nan;
      if (pv) pv[t] = nan;
    }
    return;
  }
  __syncthreads();  // thread 0 has read the scratch

  // 7 + 8
  small_alpha(A, n);

  constexpr int R = SMALL_PRED_ROWS;
  // this lane's alpha_i and the offsets of its rows (rows past n: weight zero, never read)
  double al[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane + 64 * r;
    al[r] = i < n ? A[col_off(i, n) + n - i] : 0.0;
  }

  const int groups = (m + T - 1) / T;
  for (int g = wave; g < groups; g += SMALL_WAVES) {
    double k[R][T] = {}, kss[T] = {};
    // k* and k**: pair q = r T + t is (row lane + 64 r, point t), pairs R T .. R T + T - 1 are (point t, point t)
#pragma unroll 1
    for (int q = 0; q < (R + 1) * T; ++q) {
      const int r = q / T, t = q - r * T;
      const int pt = min(g * T + t, m - 1);
      const int i = lane + 64 * r;
      if (r < R && 64 * r >= n) continue;  // (wave-uniform: no lane has a row here)
      const double* b = xt + int64_t(pt) * d;
      const double* a = r < R ? x + int64_t(min(i, n - 1)) * d : b;
      double r1, r2, r3;
      pair_dist<double, 2, 0>(a, b, d, r1, r2, r3);
      double v = eval_kprog<double, 2>(pk, r1, r2, r3);
      if (r < R && i >= n) v = 0.0;
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
#pragma unroll
        for (int tt = 0; tt < T; ++tt)
          if (q == rr * T + tt) k[rr][tt] = v;
#pragma unroll
      for (int tt = 0; tt < T; ++tt)
        if (q == R * T + tt) kss[tt] = v;
    }

    // the mean
#pragma unroll
    for (int t = 0; t < T; ++t) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) s += k[r][t] * al[r];
#pragma unroll
      for (int sft = 32; sft > 0; sft >>= 1) s += __shfl_xor(s, sft);
      if (lane == 0 && g * T + t < m) pm[g * T + t] = s;
    }
    if (!pv) continue;

    // the variance
    double ss[T];
#pragma unroll
    for (int t = 0; t < T; ++t) ss[t] = 0.0;
#pragma unroll
    for (int r0 = 0; r0 < R; ++r0) {
      const int pend = min(n, 64 * r0 + 64);
      for (int p = 64 * r0; p < pend; ++p) {
        const double* cp = A + col_off(p, n);
        const double lpp = cp[0];
        double vp[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const double q = k[r0][t] / lpp;  // (the owner's is v_p)
          const int lo = __builtin_amdgcn_readlane(__double2loint(q), p & 63);
          const int hi = __builtin_amdgcn_readlane(__double2hiint(q), p & 63);
          vp[t] = __hiloint2double(hi, lo);
          ss[t] += vp[t] * vp[t];
        }
#pragma unroll
        for (int r = r0; r < R; ++r) {
          const int i = lane + 64 * r;
          if (i > p && i < n) {
            const double lip = cp[i - p];
#pragma unroll
            for (int t = 0; t < T; ++t) k[r][t] = __builtin_fma(-lip, vp[t], k[r][t]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (lane == 0 && g * T + t < m) pv[g * T + t] = kss[t] - ss[t];
  }
}

// Value, conditional mean, conditional covariance and joint draws of one member at its m test points.
//   1 - 6  small_assemble_factor<true> and the value: phase 1 of the elimination, p = 0 .. n - 1 over P = n + m columns
//          and rows <= P.  The trailing triangle then holds Sigma* = pk(X*, X*) + diag(tau) - A^T A, A = L11^-1 K*, and
//          row P behind column n holds -mu* (it started from 0 and took -z_p l_{n+i,p} for p = 0 .. n - 1).
//   C1     mu*_i is the negation of that word; Sigma* goes out as a full row-major m x m matrix, both halves from the
//          one LDS word (when the launch asks for covariances).
//   C2     only with S > 0 -- phase 2, the same steps for p = n .. P - 1 on rows < P (row P keeps -mu*): the Cholesky
//          of Sigma*.  The first pivot that is not > 0 gives cond_info = p - n + 1 and NaN draws; value, mean and
//          covariance are out already.
//   C3     the diagonal words of the trailing block become L_pp, once, behind one barrier.
//   C4     L22 and mu* are read-only, no barrier follows: wave w takes the draws s = w, w + 4, ..; lane l holds rows
//          i = l, l + 64, l + 128 of f in registers, starting from mu*_i, and for k = 0 .. m - 1 in that order takes
//          f_i <- fma(L22[i, k], xi[s, k], f_i) for its rows i >= k (column k from LDS, consecutive rows; xi[s, k]
//          wave-uniform from global memory).  A draw's bits depend on its member and its own normals alone.
// Every barrier sits under control flow that depends on n, m, S, the program and the two `fail` values alone.
__global__ __launch_bounds__(SMALL_THREADS) void small_condition_kernel(const SmallCondRow* __restrict__ rows,
                                                                          const KProg* __restrict__ progs,
                                                                          const double* __restrict__ X,
                                                                          const double* __restrict__ noise,
                                                                          const double* __restrict__ resid,
                                                                          const double* __restrict__ Xt,
                                                                          const double* __restrict__ tdiag,
                                                                          const double* __restrict__ xi,
                                                                          double* __restrict__ out,
                                                                          int32_t* __restrict__ info,
                                                                          int32_t* __restrict__ cond_info,
                                                                          double* __restrict__ mean_out,
                                                                          double* __restrict__ cov_out,
                                                                          double* __restrict__ samples) {
  extern __shared__ __attribute__((aligned(16))) double A[];  // the packed trapezoid of P columns
  __shared__ double red[2][SMALL_THREADS];
  const SmallCondRow row = rows[blockIdx.x];
  const KProg& kp = progs[row.prog];
  const KProg& pk = progs[row.pred_prog >= 0 ? row.pred_prog : row.prog];
  const int n = row.n, d = row.d, m = row.m, S = row.S, P = n + m;
  const int tid = threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* pm = mean_out + row.tvec_off;
  double* pc = cov_out ? cov_out + row.cov_off : nullptr;
  double* ps = samples + row.xi_off;  // (never dereferenced with S = 0)
  const double nan = __builtin_nan("");

  const int fail = small_assemble_factor<true>(A, kp, X + row.x_off * d, noise + row.noise_off, resid + row.resid_off,
                                               n, d, &pk, Xt + row.xt_off * d, tdiag + row.tvec_off, m);
  small_write_value(A, red, n, fail, out, info, blockIdx.x, P);
  if (fail) {  // the workgroup's decision: NaN in every output of this member
    for (int t = tid; t < m; t += SMALL_THREADS) pm[t] = nan;
    if (pc)
      for (int t = tid; t < m * m; t += SMALL_THREADS) pc[t] = nan;
    for (int64_t t = tid; t < int64_t(S) * m; t += SMALL_THREADS) ps[t] = nan;
    if (tid == 0) cond_info[blockIdx.x] = 0;
    return;
  }

  // C1 (the last barrier of phase 1 lies behind; nothing is written to A before the barrier below)
  for (int t = tid; t < m; t += SMALL_THREADS) pm[t] = -A[col_off(n + t, P) + m - t];
  if (pc) {
    for (int j = wave; j < m; j += SMALL_WAVES) {
      const double* col = A + col_off(n + j, P);
      for (int i = j + lane; i < m; i += 64) {
        const double v = col[i - j];
        pc[int64_t(i) * m + j] = v;
        pc[int64_t(j) * m + i] = v;
      }
    }
  }
  if (S == 0) {
    if (tid == 0) cond_info[blockIdx.x] = 0;
    return;
  }
  __syncthreads();

  // C2
  int fail2 = 0;
  for (int p = n; p < P; ++p) {
    double* cp = A + col_off(p, P);
    const double pivot = cp[0];
    if (!(pivot > 0.0)) {
      fail2 = p - n + 1;
      break;
    }
    const double lpp = sqrt(pivot);
    for (int i = p + 1 + tid; i < P; i += SMALL_THREADS) cp[i - p] = cp[i - p] / lpp;
    __syncthreads();
    for (int j = p + 1 + wave; j < P; j += SMALL_WAVES) {
      double* col = A + col_off(j, P);
      const double ljp = cp[j - p];
      for (int i = j + lane; i < P; i += 64) col[i - j] = __builtin_fma(-cp[i - p], ljp, col[i - j]);
    }
    __syncthreads();
  }
  if (tid == 0) cond_info[blockIdx.x] = fail2;
  if (fail2) {  // the workgroup's decision: NaN in every draw of this member
    for (int64_t t = tid; t < int64_t(S) * m; t += SMALL_THREADS) ps[t] = nan;
    return;
  }

  // C3
  if (tid < m) A[col_off(n + tid, P)] = sqrt(A[col_off(n + tid, P)]);
  __syncthreads();

  // C4
  constexpr int R = SMALL_PRED_ROWS;
  const double* px = xi + row.xi_off;
  double mu[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane + 64 * r;
    mu[r] = i < m ? -A[col_off(n + i, P) + m - i] : 0.0;
  }
  for (int s = wave; s < S; s += SMALL_WAVES) {
    const double* z = px + int64_t(s) * m;
    double f[R];
#pragma unroll
    for (int r = 0; r < R; ++r) f[r] = mu[r];
    for (int k = 0; k < m; ++k) {
      const double* ck = A + col_off(n + k, P);
      const double zk = z[k];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i >= k && i < m) f[r] = __builtin_fma(ck[i - k], zk, f[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = lane + 64 * r;
      if (i < m) ps[int64_t(s) * m + i] = f[r];
    }
  }
}

// the gradient's host outputs (tgp_small_logprob_grad); `on` is false for the value alone
struct SmallGradOut {
  bool on = false;
  const int32_t* want_dims = nullptr;
  double* params = nullptr;
  double* noise = nullptr;
  double* alpha = nullptr;
  double* logscale = nullptr;
};

// the prediction's host arguments (tgp_small_predict); null for the other two entry points
struct SmallPredIn {
  const double* Xt = nullptr;
  int64_t xt_rows = 0;
  const int64_t* xt_off = nullptr;
  const int32_t* m = nullptr;
  const tgp_kop* progs = nullptr;
  const int32_t* prog_off = nullptr;
  const int64_t* out_off = nullptr;
  double* mean = nullptr;
  double* var = nullptr;
};

// the conditioning's host arguments beside the prediction's (tgp_small_condition: SmallPredIn carries the test
// points, the second programs, and the means with mean_off as out_off; var stays null); null for the other three
struct SmallCondIn {
  const double* tdiag = nullptr;
  const int64_t* tvec_off = nullptr;
  const int64_t* cov_off = nullptr;
  double* cov = nullptr;
  const int32_t* ndraw = nullptr;
  const double* xi = nullptr;
  const int64_t* xi_off = nullptr;
  double* samples = nullptr;
  int32_t* cond_info = nullptr;
};

// what members [b0, b1) need in the staging buffer, and where
struct SmallLaunch {
  int64_t cov_doubles = 0, xi_doubles = 0;  // a conditioning's covariances and normals (= samples); its max_n is the
                                            // largest n + m, its out_doubles the test diagonal (= means)
  int64_t b0 = 0, b1 = 0, max_n = 0;
  int64_t x_doubles = 0, vec_doubles = 0, ops = 0;
  int64_t pred_rows = 0, pred_progs = 0, xt_doubles = 0, out_doubles = 0;  // a prediction's table rows, second
                                                                           // programs, test points and outputs
  std::vector<char> host;  // rows | programs | X | noise | residual (| test points), as on the device
  std::vector<double> back;  // the gradient's noise gradient | alpha, or the prediction's mean | variance, as on the
                             // device, scattered after the join
};

// inputs | values | info, and for the gradient | parameter gradients | noise gradient | alpha | scale gradients
int64_t launch_bytes(int64_t nb, int64_t x_doubles, int64_t vec_doubles, int64_t grad_doubles) {
  return nb * int64_t(sizeof(SmallRow) + sizeof(KProg)) + (x_doubles + 2 * vec_doubles) * 8 + nb * 8 +
         round_up(nb * 4, 8) + grad_doubles * 8;
}

int64_t grad_doubles(bool grad, int64_t nb, int64_t ops, int64_t vec_doubles, int64_t d) {
  return grad ? 2 * ops + 2 * vec_doubles + nb * d : 0;
}

// a prediction launch: table rows (one per chunk of test points) | programs, the second ones behind the members' |
// X | noise | residual | test points | values | info | means (| variances)
int64_t pred_launch_bytes(int64_t nb, int64_t rows, int64_t pred_progs, int64_t x_doubles, int64_t vec_doubles,
                          int64_t xt_doubles, int64_t out_doubles, bool var) {
  return rows * int64_t(sizeof(SmallPredRow)) + (nb + pred_progs) * int64_t(sizeof(KProg)) +
         (x_doubles + 2 * vec_doubles + xt_doubles) * 8 + nb * 8 + round_up(nb * 4, 8) + out_doubles * (var ? 16 : 8);
}

// a conditioning launch: table rows (one per member) | programs, the second ones behind the members' | X | noise |
// residual | test points | test diagonal | normals | values | info | cond_info | means (| covariances) | samples
int64_t cond_launch_bytes(int64_t nb, int64_t pred_progs, int64_t x_doubles, int64_t vec_doubles, int64_t xt_doubles,
                          int64_t out_doubles, int64_t cov_doubles, int64_t xi_doubles, bool cov) {
  return nb * int64_t(sizeof(SmallCondRow)) + (nb + pred_progs) * int64_t(sizeof(KProg)) +
         (x_doubles + 2 * vec_doubles + xt_doubles + 2 * out_doubles + (cov ? cov_doubles : 0) + 2 * xi_doubles) * 8 +
         nb * 8 + 2 * round_up(nb * 4, 8);
}

int64_t pred_chunks(int64_t m) { return m <= 0 ? 1 : (m + TGP_SMALL_PRED_CHUNK - 1) / TGP_SMALL_PRED_CHUNK; }

// enqueues every launch; the host buffers in `launches` must outlive the join
int small_enqueue(tgp_ctx* ctx, std::vector<SmallLaunch>& launches, int32_t d, const int32_t* prog_off,
                  int32_t* info_host, double* out_host, const SmallGradOut& g, const SmallPredIn* p,
                  const SmallCondIn* c) {
  hipStream_t st = ctx->stream;
  if (c && !ctx->small_cond_lds_raised) {
    TGP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(small_condition_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    int(small_lds_doubles(TGP_SMALL_MAX_N) * 8)));
    ctx->small_cond_lds_raised = true;
  }
  if (p && !c && !ctx->small_pred_lds_raised) {
    TGP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(small_predict_kernel<SMALL_PRED_T>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    int(small_lds_doubles(TGP_SMALL_MAX_N) * 8)));
    ctx->small_pred_lds_raised = true;
  }
  if (!p && !g.on && !ctx->small_lds_raised) {
    TGP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(small_logprob_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    int(small_lds_doubles(TGP_SMALL_MAX_N) * 8)));
    ctx->small_lds_raised = true;
  }
  if (g.on && !ctx->small_grad_lds_raised) {
    TGP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(small_grad_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    int(small_lds_doubles(TGP_SMALL_MAX_N) * 8)));
    ctx->small_grad_lds_raised = true;
  }
  int64_t need = 0;
  for (const SmallLaunch& l : launches)
    need = std::max(need, c ? cond_launch_bytes(l.b1 - l.b0, l.pred_progs, l.x_doubles, l.vec_doubles, l.xt_doubles,
                                                l.out_doubles, l.cov_doubles, l.xi_doubles, c->cov != nullptr)
                          : p ? pred_launch_bytes(l.b1 - l.b0, l.pred_rows, l.pred_progs, l.x_doubles, l.vec_doubles,
                                                l.xt_doubles, l.out_doubles, p->var != nullptr)
                            : launch_bytes(l.b1 - l.b0, l.x_doubles, l.vec_doubles,
                                           grad_doubles(g.on, l.b1 - l.b0, l.ops, l.vec_doubles, d)));
  TGP_TRY(ensure_work(ctx, size_t(need)));
  for (SmallLaunch& l : launches) {
    const int64_t nb = l.b1 - l.b0;
    char* base = static_cast<char*>(ctx->d_work);
    if (c) {
      const SmallCondRow* crows = reinterpret_cast<const SmallCondRow*>(base);
      const KProg* progs = reinterpret_cast<const KProg*>(base + nb * sizeof(SmallCondRow));
      const double* X = reinterpret_cast<const double*>(progs + nb + l.pred_progs);
      const double* noise = X + l.x_doubles;
      const double* resid = noise + l.vec_doubles;
      const double* Xt = resid + l.vec_doubles;
      const double* tdiag = Xt + l.xt_doubles;
      const double* xi = tdiag + l.out_doubles;
      double* out = const_cast<double*>(xi) + l.xi_doubles;
      int32_t* info = reinterpret_cast<int32_t*>(out + nb);
      int32_t* cinfo = info + round_up(nb * 4, 8) / 4;
      double* mean = out + nb + 2 * (round_up(nb * 4, 8) / 8);
      double* cov = c->cov ? mean + l.out_doubles : nullptr;
      double* samples = mean + l.out_doubles + (c->cov ? l.cov_doubles : 0);
      TGP_HIP_TRY(hipMemcpyAsync(base, l.host.data(), l.host.size(), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(small_condition_kernel, dim3(unsigned(nb)), dim3(SMALL_THREADS),
                         size_t(small_lds_doubles(l.max_n) * 8), st, crows, progs, X, noise, resid, Xt, tdiag, xi, out,
                         info, cinfo, mean, cov, samples);
      TGP_HIP_TRY(hipGetLastError());
      l.back.resize(size_t(l.out_doubles + (c->cov ? l.cov_doubles : 0) + l.xi_doubles));
      if (!l.back.empty())
        TGP_HIP_TRY(hipMemcpyAsync(l.back.data(), mean, l.back.size() * 8, hipMemcpyDeviceToHost, st));
      TGP_HIP_TRY(hipMemcpyAsync(out_host + l.b0, out, size_t(nb) * 8, hipMemcpyDeviceToHost, st));
      TGP_HIP_TRY(hipMemcpyAsync(info_host + l.b0, info, size_t(nb) * 4, hipMemcpyDeviceToHost, st));
      TGP_HIP_TRY(hipMemcpyAsync(c->cond_info + l.b0, cinfo, size_t(nb) * 4, hipMemcpyDeviceToHost, st));
      continue;
    }
    if (p) {
      const SmallPredRow* prows = reinterpret_cast<const SmallPredRow*>(base);
      const KProg* progs = reinterpret_cast<const KProg*>(base + l.pred_rows * sizeof(SmallPredRow));
      const double* X = reinterpret_cast<const double*>(progs + nb + l.pred_progs);
      const double* noise = X + l.x_doubles;
      const double* resid = noise + l.vec_doubles;
      const double* Xt = resid + l.vec_doubles;
      double* out = const_cast<double*>(Xt) + l.xt_doubles;
      int32_t* info = reinterpret_cast<int32_t*>(out + nb);
      double* mean = out + nb + round_up(nb * 4, 8) / 8;
      double* var = p->var ? mean + l.out_doubles : nullptr;
      TGP_HIP_TRY(hipMemcpyAsync(base, l.host.data(), l.host.size(), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(small_predict_kernel<SMALL_PRED_T>, dim3(unsigned(l.pred_rows)), dim3(SMALL_THREADS),
                         size_t(small_lds_doubles(l.max_n) * 8), st, prows, progs, X, noise, resid, Xt, out, info, mean,
                         var);
      TGP_HIP_TRY(hipGetLastError());
      l.back.resize(size_t(l.out_doubles * (p->var ? 2 : 1)));
      if (!l.back.empty())
        TGP_HIP_TRY(hipMemcpyAsync(l.back.data(), mean, l.back.size() * 8, hipMemcpyDeviceToHost, st));
      TGP_HIP_TRY(hipMemcpyAsync(out_host + l.b0, out, size_t(nb) * 8, hipMemcpyDeviceToHost, st));
      TGP_HIP_TRY(hipMemcpyAsync(info_host + l.b0, info, size_t(nb) * 4, hipMemcpyDeviceToHost, st));
      continue;
    }
    const SmallRow* rows = reinterpret_cast<const SmallRow*>(base);
    const KProg* progs = reinterpret_cast<const KProg*>(base + nb * sizeof(SmallRow));
    const double* X = reinterpret_cast<const double*>(base + nb * (sizeof(SmallRow) + sizeof(KProg)));
    const double* noise = X + l.x_doubles;
    const double* resid = noise + l.vec_doubles;
    double* out = const_cast<double*>(resid) + l.vec_doubles;
    int32_t* info = reinterpret_cast<int32_t*>(out + nb);
    TGP_HIP_TRY(hipMemcpyAsync(base, l.host.data(), l.host.size(), hipMemcpyHostToDevice, st));
    if (!g.on) {
      hipLaunchKernelGGL(small_logprob_kernel, dim3(unsigned(nb)), dim3(SMALL_THREADS),
                         size_t(small_lds_doubles(l.max_n) * 8), st, rows, progs, X, noise, resid, out, info);
      TGP_HIP_TRY(hipGetLastError());
    } else {
      double* gparams = out + nb + round_up(nb * 4, 8) / 8;
      double* gnoise = gparams + 2 * l.ops;
      double* galpha = gnoise + l.vec_doubles;
      double* gdims = galpha + l.vec_doubles;
      hipLaunchKernelGGL(small_grad_kernel, dim3(unsigned(nb)), dim3(SMALL_THREADS),
                         size_t(small_lds_doubles(l.max_n) * 8), st, rows, progs, X, noise, resid, out, info, gparams,
                         gnoise, galpha, gdims);
      TGP_HIP_TRY(hipGetLastError());
      TGP_HIP_TRY(hipMemcpyAsync(g.params + 2 * int64_t(prog_off[l.b0]), gparams, size_t(2 * l.ops) * 8,
                                 hipMemcpyDeviceToHost, st));
      if (g.noise || g.alpha) {
        l.back.resize(size_t(2 * l.vec_doubles));
        TGP_HIP_TRY(hipMemcpyAsync(l.back.data(), gnoise, l.back.size() * 8, hipMemcpyDeviceToHost, st));
      }
      if (g.logscale)
        TGP_HIP_TRY(hipMemcpyAsync(g.logscale + l.b0 * d, gdims, size_t(nb * d) * 8, hipMemcpyDeviceToHost, st));
    }
    TGP_HIP_TRY(hipMemcpyAsync(out_host + l.b0, out, size_t(nb) * 8, hipMemcpyDeviceToHost, st));
    TGP_HIP_TRY(hipMemcpyAsync(info_host + l.b0, info, size_t(nb) * 4, hipMemcpyDeviceToHost, st));
  }
  return TGP_OK;
}

// the body of both entry points: validation, the split into launches, one host join
int small_call(tgp_ctx* ctx, int32_t nb, const tgp_kop* progs, const int32_t* prog_off, const int64_t* x_off,
               const int32_t* n, int32_t d, const double* X_host, int64_t x_rows, const int64_t* vec_off,
               const double* noise_host, const double* resid_host, int32_t* info_host, double* out_host,
               const SmallGradOut& g, const SmallPredIn* p = nullptr, const SmallCondIn* c = nullptr) {
  TGP_ARG_CHECK(ctx != nullptr, "null context");
  TGP_ARG_CHECK(nb >= 0, "negative number of members (%d)", nb);
  if (nb == 0) return TGP_OK;
  std::unique_lock<std::recursive_mutex> lock(ctx->mu);
  TGP_HIP_TRY(hipSetDevice(ctx->device));
  TGP_ARG_CHECK(progs && prog_off && x_off && n && X_host && vec_off && noise_host && resid_host && info_host && out_host &&
                    (!g.on || g.params) && (!p || (p->xt_off && p->m && p->out_off && p->mean && (p->Xt || p->xt_rows == 0) &&
                                                   (!p->progs == !p->prog_off))) &&
                    (!c || (c->tdiag && c->tvec_off && c->ndraw && c->xi_off && c->cond_info && (!c->cov || c->cov_off))),
                "null argument");
  TGP_ARG_CHECK(d >= 1 && d <= TGP_MAX_DIM, "the input dimension must be 1 .. %d (got %d)", TGP_MAX_DIM, d);
  TGP_ARG_CHECK(x_rows >= 0, "negative number of coordinate rows (%lld)", (long long)x_rows);
  TGP_ARG_CHECK(!p || p->xt_rows >= 0, "negative number of test rows (%lld)", (long long)(p ? p->xt_rows : 0));
  std::vector<KProg> kps(size_t(nb), KProg{});
  std::vector<KProg> pks(p && p->progs ? size_t(nb) : 0, KProg{});  // the second programs, where a member names one
  std::vector<char> has_pk(size_t(nb), 0);
  for (int64_t b = 0; b < nb; ++b) {
    TGP_ARG_CHECK(n[b] >= 1 && n[b] <= TGP_SMALL_MAX_N, "member %lld: n must be 1 .. %d (got %d)", (long long)b,
                  TGP_SMALL_MAX_N, n[b]);
    TGP_ARG_CHECK(x_off[b] >= 0 && x_off[b] <= x_rows - n[b], "member %lld: rows %lld .. %lld lie outside X (%lld rows)",
                  (long long)b, (long long)x_off[b], (long long)(x_off[b] + n[b]), (long long)x_rows);
    TGP_ARG_CHECK(vec_off[b] >= 0, "member %lld: negative offset into noise and residual (%lld)", (long long)b,
                  (long long)vec_off[b]);
    TGP_ARG_CHECK(prog_off[b] >= 0 && prog_off[b + 1] > prog_off[b], "member %lld: empty or negative program extent",
                  (long long)b);
    if (make_kprog(progs + prog_off[b], prog_off[b + 1] - prog_off[b], &kps[size_t(b)]) != TGP_OK) {
      const std::string why = tgp_last_error();
      set_error("member %lld: %s", (long long)b, why.c_str());
      return TGP_E_ARG;
    }
    if (!p) continue;
    TGP_ARG_CHECK(p->m[b] >= 0, "member %lld: negative number of test points (%d)", (long long)b, p->m[b]);
    TGP_ARG_CHECK(p->xt_off[b] >= 0 && p->xt_off[b] <= p->xt_rows - p->m[b],
                  "member %lld: test rows %lld .. %lld lie outside Xt (%lld rows)", (long long)b, (long long)p->xt_off[b],
                  (long long)(p->xt_off[b] + p->m[b]), (long long)p->xt_rows);
    TGP_ARG_CHECK(p->out_off[b] >= 0, "member %lld: negative offset into the predictions (%lld)", (long long)b,
                  (long long)p->out_off[b]);
    if (c) {
      TGP_ARG_CHECK(int64_t(n[b]) + p->m[b] <= TGP_SMALL_MAX_N,
                    "member %lld: data and test points together must be at most %d (got %d + %d)", (long long)b,
                    TGP_SMALL_MAX_N, n[b], p->m[b]);
      TGP_ARG_CHECK(c->ndraw[b] >= 0, "member %lld: negative number of draws (%d)", (long long)b, c->ndraw[b]);
      TGP_ARG_CHECK(c->tvec_off[b] >= 0 && c->xi_off[b] >= 0 && (!c->cov || c->cov_off[b] >= 0),
                    "member %lld: negative offset into the test diagonal, the covariances or the normals", (long long)b);
      TGP_ARG_CHECK(c->ndraw[b] == 0 || (c->xi && c->samples),
                    "member %lld: %d draws are asked for, but xi_host or samples_host is null", (long long)b, c->ndraw[b]);
    }
    if (p->progs) {
      TGP_ARG_CHECK(p->prog_off[b] >= 0 && p->prog_off[b + 1] >= p->prog_off[b],
                    "member %lld: negative prediction program extent", (long long)b);
      if (p->prog_off[b + 1] > p->prog_off[b]) {
        if (make_kprog(p->progs + p->prog_off[b], p->prog_off[b + 1] - p->prog_off[b], &pks[size_t(b)]) != TGP_OK) {
          const std::string why = tgp_last_error();
          set_error("member %lld: prediction program: %s", (long long)b, why.c_str());
          return TGP_E_ARG;
        }
        has_pk[size_t(b)] = 1;
      }
    }
  }
  // the split: launches are filled in the order given and end before the member that would take the staging buffer
  // past its cap; coordinates that several members of a launch share (same offset, same length) are staged once
  std::vector<SmallLaunch> launches;
  for (int64_t b0 = 0; b0 < nb;) {
    SmallLaunch l;
    l.b0 = b0;
    std::map<std::pair<int64_t, int32_t>, int64_t> seen;  // (x_off, n) -> first row in the launch's X
    std::map<std::pair<int64_t, int32_t>, int64_t> seen_t;  // (xt_off, m) -> first row in the launch's Xt
    std::vector<SmallRow> rows;
    std::vector<SmallPredRow> prows;
    std::vector<SmallCondRow> crows;
    std::vector<KProg> lpks;
    int64_t b = b0;
    for (; b < nb; ++b) {
      const auto key = std::make_pair(x_off[b], n[b]);
      const bool fresh = seen.find(key) == seen.end();
      const int64_t xd = l.x_doubles + (fresh ? int64_t(n[b]) * d : 0), vd = l.vec_doubles + n[b];
      const int64_t ops = int64_t(prog_off[b + 1]) - prog_off[b0];
      if (c) {  // one row per member: its second program, test points, test diagonal, normals and outputs
        const int64_t mb = p->m[b], sb = c->ndraw[b];
        const auto key_t = std::make_pair(p->xt_off[b], p->m[b]);
        const bool fresh_t = mb > 0 && seen_t.find(key_t) == seen_t.end();
        const int64_t np = l.pred_progs + has_pk[size_t(b)];
        const int64_t td = l.xt_doubles + (fresh_t ? mb * d : 0), od = l.out_doubles + mb;
        const int64_t cd = l.cov_doubles + mb * mb, zd = l.xi_doubles + sb * mb;
        if (b > b0 && cond_launch_bytes(b - b0 + 1, np, xd, vd, td, od, cd, zd, c->cov != nullptr) > SMALL_STAGE_BYTES) break;
        if (fresh) seen[key] = l.x_doubles / d;
        if (fresh_t) seen_t[key_t] = l.xt_doubles / d;
        crows.push_back(SmallCondRow{seen[key], l.vec_doubles, l.vec_doubles, mb > 0 ? seen_t[key_t] : 0, l.out_doubles,
                                     l.cov_doubles, l.xi_doubles, n[b], d, int32_t(b - b0),
                                     has_pk[size_t(b)] ? int32_t(l.pred_progs) : -1, int32_t(mb), int32_t(sb)});
        if (has_pk[size_t(b)]) lpks.push_back(pks[size_t(b)]);
        l.pred_progs = np, l.xt_doubles = td, l.out_doubles = od, l.cov_doubles = cd, l.xi_doubles = zd;
        l.max_n = std::max<int64_t>(l.max_n, n[b] + mb);
      } else if (p) {  // the member's chunks, second program, test points (staged once per (offset, count)) and outputs
        const auto key_t = std::make_pair(p->xt_off[b], p->m[b]);
        const bool fresh_t = p->m[b] > 0 && seen_t.find(key_t) == seen_t.end();
        const int64_t nr = l.pred_rows + pred_chunks(p->m[b]), np = l.pred_progs + has_pk[size_t(b)];
        const int64_t td = l.xt_doubles + (fresh_t ? int64_t(p->m[b]) * d : 0), od = l.out_doubles + p->m[b];
        if (b > b0 && pred_launch_bytes(b - b0 + 1, nr, np, xd, vd, td, od, p->var != nullptr) > SMALL_STAGE_BYTES) break;
        if (fresh) seen[key] = l.x_doubles / d;
        if (fresh_t) seen_t[key_t] = l.xt_doubles / d;
        for (int64_t c = 0; c < pred_chunks(p->m[b]); ++c) {
          const int64_t at = c * TGP_SMALL_PRED_CHUNK;
          prows.push_back(SmallPredRow{seen[key], l.vec_doubles, l.vec_doubles,
                                       (p->m[b] > 0 ? seen_t[key_t] : 0) + at, l.out_doubles + at, n[b], d,
                                       int32_t(b - b0), has_pk[size_t(b)] ? int32_t(l.pred_progs) : -1,
                                       int32_t(std::min<int64_t>(p->m[b] - at, TGP_SMALL_PRED_CHUNK)),
                                       c == 0 ? int32_t(b - b0) : -1});
        }
        if (has_pk[size_t(b)]) lpks.push_back(pks[size_t(b)]);
        l.pred_rows = nr, l.pred_progs = np, l.xt_doubles = td, l.out_doubles = od;
      } else {
        if (b > b0 && launch_bytes(b - b0 + 1, xd, vd, grad_doubles(g.on, b - b0 + 1, ops, vd, d)) > SMALL_STAGE_BYTES) break;
        if (fresh) seen[key] = l.x_doubles / d;
      }
      rows.push_back(SmallRow{seen[key], l.vec_doubles, l.vec_doubles, 2 * (int64_t(prog_off[b]) - prog_off[b0]), n[b], d,
                              int32_t(b - b0), int32_t(g.want_dims && g.want_dims[b] ? 1 : 0)});
      l.x_doubles = xd, l.vec_doubles = vd, l.ops = ops;
      if (!c) l.max_n = std::max<int64_t>(l.max_n, n[b]);
    }
    l.b1 = b;
    const int64_t cnt = b - b0;
    for (SmallPredRow& r : prows)  // the second programs follow the launch's cnt member programs
      if (r.pred_prog >= 0) r.pred_prog += int32_t(cnt);
    for (SmallCondRow& r : crows)
      if (r.pred_prog >= 0) r.pred_prog += int32_t(cnt);
    const int64_t table = c   ? cnt * int64_t(sizeof(SmallCondRow))
                          : p ? l.pred_rows * int64_t(sizeof(SmallPredRow))
                              : cnt * int64_t(sizeof(SmallRow));
    l.host.resize(size_t(table + (cnt + l.pred_progs) * int64_t(sizeof(KProg)) +
                         (l.x_doubles + 2 * l.vec_doubles + l.xt_doubles + (c ? l.out_doubles + l.xi_doubles : 0)) * 8));
    char* w = l.host.data();
    if (c) {
      std::memcpy(w, crows.data(), size_t(table));
    } else if (p) {
      std::memcpy(w, prows.data(), size_t(table));
    } else {
      std::memcpy(w, rows.data(), size_t(table));
    }
    w += table;
    std::memcpy(w, &kps[size_t(b0)], size_t(cnt) * sizeof(KProg));
    w += cnt * sizeof(KProg);
    if (l.pred_progs) std::memcpy(w, lpks.data(), size_t(l.pred_progs) * sizeof(KProg));
    w += l.pred_progs * sizeof(KProg);
    double* xs = reinterpret_cast<double*>(w);
    double* nzs = xs + l.x_doubles;
    double* rss = nzs + l.vec_doubles;
    double* xts = rss + l.vec_doubles;
    for (const auto& kv : seen_t)
      std::memcpy(xts + kv.second * d, p->Xt + kv.first.first * d, size_t(kv.first.second) * d * 8);
    for (const auto& kv : seen)
      std::memcpy(xs + kv.second * d, X_host + kv.first.first * d, size_t(kv.first.second) * d * 8);
    for (int64_t m = 0; m < cnt; ++m) {
      const SmallRow& r = rows[size_t(m)];
      std::memcpy(nzs + r.noise_off, noise_host + vec_off[b0 + m], size_t(r.n) * 8);
      std::memcpy(rss + r.resid_off, resid_host + vec_off[b0 + m], size_t(r.n) * 8);
      if (c) {  // the test diagonal and the normals follow the test points
        const SmallCondRow& cr = crows[size_t(m)];
        double* tds = xts + l.xt_doubles;
        std::memcpy(tds + cr.tvec_off, c->tdiag + c->tvec_off[b0 + m], size_t(cr.m) * 8);
        if (int64_t(cr.S) * cr.m > 0)
          std::memcpy(tds + l.out_doubles + cr.xi_off, c->xi + c->xi_off[b0 + m], size_t(int64_t(cr.S) * cr.m) * 8);
      }
    }
    launches.push_back(std::move(l));
    b0 = b;
  }
  // one host join, on every path: the host buffers above are read by the copies that were enqueued
  const int status = small_enqueue(ctx, launches, d, prog_off, info_host, out_host, g, p, c);
  const hipError_t joined = hipStreamSynchronize(ctx->stream);
  TGP_TRY(status);
  TGP_HIP_TRY(joined);
  // the two vectors go back to the caller's offsets (the launch holds them member after member)
  for (const SmallLaunch& l : launches) {
    if (l.back.empty()) continue;
    int64_t at = 0;
    if (c) {  // means | covariances | samples go to the caller's offsets
      const double* covs = l.back.data() + l.out_doubles;
      const double* smp = covs + (c->cov ? l.cov_doubles : 0);
      int64_t cat = 0, sat = 0;
      for (int64_t b = l.b0; b < l.b1; ++b) {
        const int64_t mb = p->m[b], sm = int64_t(c->ndraw[b]) * mb;
        std::memcpy(p->mean + p->out_off[b], l.back.data() + at, size_t(mb) * 8);
        if (c->cov) std::memcpy(c->cov + c->cov_off[b], covs + cat, size_t(mb * mb) * 8);
        if (sm > 0) std::memcpy(c->samples + c->xi_off[b], smp + sat, size_t(sm) * 8);
        at += mb, cat += mb * mb, sat += sm;
      }
      continue;
    }
    if (p) {  // the predictions go to the caller's offsets
      for (int64_t b = l.b0; b < l.b1; at += p->m[b], ++b) {
        std::memcpy(p->mean + p->out_off[b], l.back.data() + at, size_t(p->m[b]) * 8);
        if (p->var) std::memcpy(p->var + p->out_off[b], l.back.data() + l.out_doubles + at, size_t(p->m[b]) * 8);
      }
      continue;
    }
    for (int64_t b = l.b0; b < l.b1; at += n[b], ++b) {
      if (g.noise) std::memcpy(g.noise + vec_off[b], l.back.data() + at, size_t(n[b]) * 8);
      if (g.alpha) std::memcpy(g.alpha + vec_off[b], l.back.data() + l.vec_doubles + at, size_t(n[b]) * 8);
    }
  }
  return TGP_OK;
}

}  // namespace

}  // namespace tgp

using namespace tgp;

extern "C" int tgp_small_logprob(tgp_ctx* ctx, int32_t nb, const tgp_kop* progs, const int32_t* prog_off,
                                 const int64_t* x_off, const int32_t* n, int32_t d, const double* X_host,
                                 int64_t x_rows, const int64_t* vec_off, const double* noise_host,
                                 const double* resid_host, int32_t* info_host, double* out_host) {
  return small_call(ctx, nb, progs, prog_off, x_off, n, d, X_host, x_rows, vec_off, noise_host, resid_host, info_host,
                    out_host, SmallGradOut{});
}

extern "C" int tgp_small_logprob_grad(tgp_ctx* ctx, int32_t nb, const tgp_kop* progs, const int32_t* prog_off,
                                      const int64_t* x_off, const int32_t* n, int32_t d, const double* X_host,
                                      int64_t x_rows, const int64_t* vec_off, const double* noise_host,
                                      const double* resid_host, const int32_t* want_dims, int32_t* info_host,
                                      double* out_host, double* grad_params_host, double* grad_noise_host,
                                      double* alpha_host, double* grad_logscale_host) {
  SmallGradOut g;
  g.on = true;
  g.want_dims = want_dims;
  g.params = grad_params_host;
  g.noise = grad_noise_host;
  g.alpha = alpha_host;
  g.logscale = grad_logscale_host;
  return small_call(ctx, nb, progs, prog_off, x_off, n, d, X_host, x_rows, vec_off, noise_host, resid_host, info_host,
                    out_host, g);
}

extern "C" int tgp_small_predict(tgp_ctx* ctx, int32_t nb, const tgp_kop* progs, const int32_t* prog_off,
                                 const int64_t* x_off, const int32_t* n, int32_t d, const double* X_host,
                                 int64_t x_rows, const int64_t* vec_off, const double* noise_host,
                                 const double* resid_host, const double* Xt_host, int64_t xt_rows,
                                 const int64_t* xt_off, const int32_t* m, const tgp_kop* pred_progs,
                                 const int32_t* pred_prog_off, const int64_t* out_off, int32_t* info_host,
                                 double* out_host, double* mean_host, double* var_host) {
  SmallPredIn p;
  p.Xt = Xt_host;
  p.xt_rows = xt_rows;
  p.xt_off = xt_off;
  p.m = m;
  p.progs = pred_progs;
  p.prog_off = pred_prog_off;
  p.out_off = out_off;
  p.mean = mean_host;
  p.var = var_host;
  return small_call(ctx, nb, progs, prog_off, x_off, n, d, X_host, x_rows, vec_off, noise_host, resid_host, info_host,
                    out_host, SmallGradOut{}, &p);
}

extern "C" int tgp_small_condition(tgp_ctx* ctx, int32_t nb, const tgp_kop* progs, const int32_t* prog_off,
                                   const int64_t* x_off, const int32_t* n, int32_t d, const double* X_host,
                                   int64_t x_rows, const int64_t* vec_off, const double* noise_host,
                                   const double* resid_host, const double* Xt_host, int64_t xt_rows,
                                   const int64_t* xt_off, const int32_t* m, const tgp_kop* pred_progs,
                                   const int32_t* pred_prog_off, const double* test_diag_host, const int64_t* tvec_off,
                                   const int64_t* mean_off, double* mean_host, const int64_t* cov_off, double* cov_host,
                                   const int32_t* ndraw, const double* xi_host, const int64_t* xi_off,
                                   double* samples_host, int32_t* info_host, int32_t* cond_info_host, double* out_host) {
  SmallPredIn p;
  p.Xt = Xt_host;
  p.xt_rows = xt_rows;
  p.xt_off = xt_off;
  p.m = m;
  p.progs = pred_progs;
  p.prog_off = pred_prog_off;
  p.out_off = mean_off;
  p.mean = mean_host;
  SmallCondIn c;
  c.tdiag = test_diag_host;
  c.tvec_off = tvec_off;
  c.cov_off = cov_off;
  c.cov = cov_host;
  c.ndraw = ndraw;
  c.xi = xi_host;
  c.xi_off = xi_off;
  c.samples = samples_host;
  c.cond_info = cond_info_host;
  return small_call(ctx, nb, progs, prog_off, x_off, n, d, X_host, x_rows, vec_off, noise_host, resid_host, info_host,
                    out_host, SmallGradOut{}, &p, &c);
}
