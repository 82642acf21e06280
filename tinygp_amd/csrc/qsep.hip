// qsep.hip -- quasiseparable (state-space) GP solver for sorted 1-D inputs, state dimension J <= 8.
//
// K + diag(noise) for a kernel k(t_i, t_j) = h^T A(|t_i - t_j|) P h has the lower Cholesky factor
//   L[n,n] = sqrt(c_n),  L[i,j] = h^T A_i ... A_{j+1} w_j  (i > j)
// with c_n, w_n from the Riccati (Kalman covariance) recursion over the filtered covariance P_n:
//   P^-_n = A_n (P_{n-1} - P) A_n^T + P,  g = P^-_n h,  c_n = h^T g + noise_n,  w_n = g / sqrt(c_n),
//   P_n = P^-_n - g g^T / c_n.
// The factor is computed by a reduce-then-scan over chunks of steps:
//   1. qs_fold     one wavefront per chunk folds its steps into one associative filtering element (A, C, J) of
//                  the parallel Kalman filter (Sarkka & Garcia-Fernandez 2021, covariance part).  One scalar
//                  observation per step: the step's J is rank one and the fold needs no inverse (Sherman-Morrison).
//   2. qs_scan_reduce / qs_scan_down   hierarchical exclusive scan of the chunk elements, 64 per group; the full
//                  combine (a J x J solve by Gauss-Jordan with partial pivoting) runs only here.  Going down, only
//                  the filtered covariance is carried: P <- A (I + P J)^-1 P A^T + C.
//   3. qs_emit     each chunk re-runs the sequential recursion from its incoming P, writing c_n, w_n and a
//                  per-chunk sum of log c_n and its first non-positive pivot.
// L^-1 y, L^-T y and L z are affine recurrences g <- M_n g + v_n over a J-vector per right-hand side (the M_n
// shared by all columns); they run the same three phases with element (M, V) and combine M = M2 M1, V = M2 V1 + V2.
// A_n is regenerated from dt_n = t_n - t_{n-1} (dt_0 = 0, A = I) in every kernel instead of being stored.
// Prediction at test points (qs_pred_*) runs two more scans of the same shape, one per direction, whose elements pair
// a congruence recurrence X <- M X M^T + V (J x J) with an affine one f <- Mf f + Vf (J-vector); see below.
// Posterior samples (qs_prior, qs_cm_*, qs_smp_*) are affine scans too: a prior draw of the state over the merged grid of
// data and test points, and the conditional mean for J x 8 blocks of columns; see "posterior samples" below.
// Phase 2 is one kernel pair for every recurrence, instantiated over the four element types of "scan policies" below.
//
// Layout: one wavefront holds a J x J matrix (or a J x 8 block of right-hand sides) as one entry per lane,
// lane = 8 r + c; entries outside J x J are zero.  Products read operands through __shfl.  Every reduction runs in
// a fixed order, so results are bit-identical from run to run.  Arithmetic is fp64 throughout.
//
// Batches of models: the kernels of the fused log-probability (qs_fold, qs_emit, qs_aff_fold, qs_aff_emit, qs_finish)
// and both scan kernels serve one model per blockIdx.y (qs_finish: per block) over the shared t: model mp[blockIdx.y],
// every array of that member `stride` doubles after its neighbour's.  A single evaluation is the batch of one (grid
// y = 1, where no stride matters): launch_factor and launch_affine enqueue the chain for both, so a member's result
// has the bits of its single call.  The gradient's kernels take the same member axis (see "gradient" below).
// Sets of series: the same kernels, instantiated over an extent policy ("extents" below), serve members that each have
// a series of their own -- their own slice of t, length, chunk length, chunk count and scan depth -- from a device table.
// The gradient's kernels take the same two kinds of extent, so a set of series has value and gradient in one launch chain;
// so does the prediction's emit pass (qs_pred_emit over UniformPExtent / TablePExtent, the members' test points in a
// small table of their own, QTest), so a set predicts at every member's own test points in one chain as well.  The
// samples' kernels (qs_prior, qs_cm_fold, qs_cm_emit, qs_smp_locate, qs_smp_place over UniformSExtent / TableSExtent) take
// a second extent table beside the data's, that of every member's merged grid, and both solves run for a block of columns
// per member (TableColsExtent): a set draws from every member's posterior in one chain ("sets of series: value and
// posterior draws" below).
#include "tgp_common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace {

constexpr int QJ = TGP_QSEP_MAX_J;          // 8
constexpr int QL = TGP_QSEP_MAX_LEAVES;     // 8
constexpr int WAVE = 64;
constexpr int WPB = 4;                      // wavefronts per block
constexpr int GROUP = 64;                   // scan fan-in per level
constexpr double kLog2Pi = 1.8378770664093454836;

struct QModel {
  int32_t J, nleaves;
  int32_t kind[QL];
  int32_t map[QJ][QL];
  double par[QL][4];
  double h[QJ];
  double P[QJ * QJ];  // padded 8 x 8
};

__device__ __forceinline__ double sh(double v, int lane) { return __shfl(v, lane, WAVE); }
__device__ __forceinline__ double at(double v, int r, int c) { return sh(v, r * 8 + c); }

// X Y, X^T Y, X Y^T for lane-layout matrices (uniform loops: every lane runs every __shfl)
__device__ __forceinline__ double mm(double x, double y, int J, int r, int c) {
  double s = 0.0;
  for (int k = 0; k < J; ++k) s += at(x, r, k) * at(y, k, c);
  return s;
}
__device__ __forceinline__ double mm_tn(double x, double y, int J, int r, int c) {
  double s = 0.0;
  for (int k = 0; k < J; ++k) s += at(x, k, r) * at(y, k, c);
  return s;
}
__device__ __forceinline__ double mm_nt(double x, double y, int J, int r, int c) {
  double s = 0.0;
  for (int k = 0; k < J; ++k) s += at(x, r, k) * at(y, c, k);
  return s;
}
__device__ __forceinline__ double symm(double x, int r, int c) { return 0.5 * (x + at(x, c, r)); }

// entry (i, j) of one leaf's forward transition A(dt); selects, not arrays, so that nothing lives in scratch
__device__ __forceinline__ double pick2(int i, int j, double a00, double a01, double a10, double a11) {
  return i == 0 ? (j == 0 ? a00 : a01) : (j == 0 ? a10 : a11);
}

__device__ __forceinline__ double leaf_phi(int kind, const double* p, double dt, int i, int j) {
  switch (kind) {
    case TGP_QS_EXP:
      return exp(-p[0] * dt);
    case TGP_QS_M32: {
      const double f = p[0], fd = f * dt;
      return exp(-fd) * pick2(i, j, 1 + fd, dt, -f * fd, 1 - fd);
    }
    case TGP_QS_M52: {
      const double f = p[0], f2 = f * f, fd = f * dt, d2 = dt * dt;
      double v;
      switch (i * 3 + j) {
        case 0: v = 0.5 * f2 * d2 + fd + 1; break;
        case 1: v = dt * (fd + 1); break;
        case 2: v = 0.5 * d2; break;
        case 3: v = -0.5 * f * f2 * d2; break;
        case 4: v = -f2 * d2 + fd + 1; break;
        case 5: v = 0.5 * dt * (2 - fd); break;
        case 6: v = 0.5 * f2 * f * dt * (fd - 2); break;
        case 7: v = f2 * dt * (fd - 3); break;
        default: v = 0.5 * f2 * d2 - 2 * fd + 1; break;
      }
      return exp(-fd) * v;
    }
    case TGP_QS_COS:
    case TGP_QS_CELERITE: {
      const double decay = kind == TGP_QS_COS ? 1.0 : exp(-p[0] * dt);
      const double a = (kind == TGP_QS_COS ? p[0] : p[1]) * dt;
      const double co = cos(a), si = sin(a);
      return decay * pick2(i, j, co, -si, si, co);
    }
    case TGP_QS_SHO_CRIT: {
      const double w = p[0], wd = w * dt;
      return exp(-wd) * pick2(i, j, 1 + wd, dt, -w * wd, 1 - wd);
    }
    default: {  // SHO under- / over-damped: p = (omega, quality, f)
      const double w = p[0], q = p[1], f = p[2];
      const double arg = 0.5 * f * w * dt / q;
      if (kind == TGP_QS_SHO_UNDER) {
        const double s = sin(arg), co = cos(arg);
        return exp(-0.5 * w * dt / q) * pick2(i, j, co + s / f, 2 * q * s / (w * f), -2 * q * w * s / f, co - s / f);
      }
      // Over-damped: with a = w dt / 2q, s = e^-a sinh(arg) and co = e^-a cosh(arg) are formed from e^-(a - arg) and
      // e^-2arg, both <= 1 (f < 1), never as e^-a cosh(arg) = 0 * inf beyond arg ~ 710.  a - arg = 2 w q dt / (1 + f)
      // because 1 - f^2 = 4 q^2: no cancellation for small q; expm1 keeps s accurate for small arg.
      const double ep = exp(-2 * w * q * dt / (1 + f)), em = expm1(-2 * arg);
      const double s = -0.5 * ep * em, co = 0.5 * ep * (2 + em);
      return pick2(i, j, co + s / f, 2 * q * s / (w * f), -2 * q * w * s / f, co - s / f);
    }
  }
}

// this lane's entry of the global transition: the product over the leaves of the term that r and c belong to
__device__ __forceinline__ double phi_entry(const QModel& m, double dt, int r, int c) {
  if (r >= m.J || c >= m.J) return 0.0;
  double v = 1.0;
  for (int l = 0; l < m.nleaves; ++l) {
    const int a = m.map[r][l], b = m.map[c][l];
    if ((a < 0) != (b < 0)) return 0.0;
    if (a >= 0) v *= leaf_phi(m.kind[l], m.par[l], dt, a, b);
  }
  return v;
}

// Tangent of the model along one parameter direction: a tangent for every stored leaf parameter (SHO's dependent f
// included), for h and for P (padded 8 x 8).  The host forms these (kernels/quasisep.py, _ssm_tangents).
struct QDir {
  double dpar[QL][4];
  double dh[QJ];
  double dP[QJ * QJ];
};

// directional derivative of leaf_phi along dp; every term carries a factor dt, so it is 0 at dt = 0
__device__ __forceinline__ double leaf_dphi(int kind, const double* p, const double* dp, double dt, int i, int j) {
  switch (kind) {
    case TGP_QS_EXP:
      return -dt * exp(-p[0] * dt) * dp[0];
    case TGP_QS_M32:
    case TGP_QS_SHO_CRIT: {
      const double f = p[0], fd = f * dt;
      return dp[0] * dt * exp(-fd) * pick2(i, j, -fd, -dt, f * (fd - 2), fd - 2);
    }
    case TGP_QS_M52: {
      const double f = p[0], f2 = f * f, fd = f * dt, d2 = dt * dt;
      double v, vf;  // the polynomial factor of leaf_phi and its derivative with respect to f
      switch (i * 3 + j) {
        case 0: v = 0.5 * f2 * d2 + fd + 1, vf = f * d2 + dt; break;
        case 1: v = dt * (fd + 1), vf = d2; break;
        case 2: v = 0.5 * d2, vf = 0.0; break;
        case 3: v = -0.5 * f * f2 * d2, vf = -1.5 * f2 * d2; break;
        case 4: v = -f2 * d2 + fd + 1, vf = -2 * f * d2 + dt; break;
        case 5: v = 0.5 * dt * (2 - fd), vf = -0.5 * d2; break;
        case 6: v = 0.5 * f2 * f * dt * (fd - 2), vf = 2 * f2 * f * d2 - 3 * f2 * dt; break;
        case 7: v = f2 * dt * (fd - 3), vf = 3 * f2 * d2 - 6 * fd; break;
        default: v = 0.5 * f2 * d2 - 2 * fd + 1, vf = f * d2 - 2 * dt; break;
      }
      return dp[0] * exp(-fd) * (vf - dt * v);
    }
    case TGP_QS_COS:
    case TGP_QS_CELERITE: {
      const bool cosk = kind == TGP_QS_COS;
      const double decay = cosk ? 1.0 : exp(-p[0] * dt);
      const double a = (cosk ? p[0] : p[1]) * dt;
      const double dom = cosk ? dp[0] : dp[1], ddec = cosk ? 0.0 : dp[0];
      const double co = cos(a), si = sin(a);
      return decay * dt * (dom * pick2(i, j, -si, -co, co, -si) - ddec * pick2(i, j, co, -si, si, co));
    }
    default: {  // SHO under- / over-damped, entries built from S = e^-a sin(h)(arg), Cc = e^-a cos(h)(arg)
      const double w = p[0], q = p[1], f = p[2], dw = dp[0], dq = dp[1], df = dp[2];
      const double a = 0.5 * w * dt / q, arg = f * a;
      const double da = a * (dw / w - dq / q), darg = df * a + f * da;
      double S, dS, dC;
      if (kind == TGP_QS_SHO_UNDER) {
        const double e = exp(-a), Cc = e * cos(arg);
        S = e * sin(arg);
        dS = -da * S + Cc * darg, dC = -da * Cc - S * darg;
      } else {
        // as in leaf_phi: S and Cc from e^-(a - arg) and e^-2arg, both <= 1.  dS = -da S + Cc darg is regrouped
        // around Cc - S = e^-(a + arg) so that the two nearly equal large terms never meet: nothing overflows
        const double ep = exp(-2 * w * q * dt / (1 + f)), em = expm1(-2 * arg);
        const double Cc = 0.5 * ep * (2 + em), diff = ep * (1 + em), dd = da - darg;
        S = -0.5 * ep * em;
        dS = -dd * S + diff * darg, dC = -dd * Cc - diff * darg;
      }
      const double rel = df / f;
      switch (i * 2 + j) {
        case 0: return dC + (dS - S * rel) / f;
        case 1: return 2 * q / (w * f) * (dS + S * (dq / q - dw / w - rel));
        case 2: return -2 * q * w / f * (dS + S * (dq / q + dw / w - rel));
        default: return dC - (dS - S * rel) / f;
      }
    }
  }
}

// phi_entry and its tangent along d: the product rule over the leaves
__device__ __forceinline__ void phi_entry_d(const QModel& m, const QDir& d, double dt, int r, int c, double* phi,
                                            double* dphi) {
  *phi = 0.0, *dphi = 0.0;
  if (r >= m.J || c >= m.J) return;
  double v = 1.0, dv = 0.0;
  for (int l = 0; l < m.nleaves; ++l) {
    const int a = m.map[r][l], b = m.map[c][l];
    if ((a < 0) != (b < 0)) return;
    if (a >= 0) {
      const double f = leaf_phi(m.kind[l], m.par[l], dt, a, b);
      dv = dv * f + v * leaf_dphi(m.kind[l], m.par[l], d.dpar[l], dt, a, b);
      v *= f;
    }
  }
  *phi = v, *dphi = dv;
}

__device__ __forceinline__ double dt_at(const double* t, int64_t n) { return n == 0 ? 0.0 : t[n] - t[n - 1]; }

// row-vector h^T X (one value per column c) and X h (one value per row r)
__device__ __forceinline__ double hT(const QModel& m, double x, int c) {
  double s = 0.0;
  for (int k = 0; k < m.J; ++k) s += m.h[k] * at(x, k, c);
  return s;
}
__device__ __forceinline__ double Xh(const QModel& m, double x, int r) {
  double s = 0.0;
  for (int k = 0; k < m.J; ++k) s += at(x, r, k) * m.h[k];
  return s;
}

// Solve (G) [X1 | X2] = [X1 | X2] in place, Gauss-Jordan with partial pivoting over the leading J x J block.
__device__ __forceinline__ void gj_solve(double& G, double& X1, double& X2, int J, int r, int c) {
  for (int p = 0; p < J; ++p) {
    int piv = p;
    double best = fabs(at(G, p, p));
    for (int i = p + 1; i < J; ++i) {
      const double v = fabs(at(G, i, p));
      if (v > best) { best = v; piv = i; }
    }
    const int src = (r == p ? piv : r == piv ? p : r) * 8 + c;
    G = sh(G, src), X1 = sh(X1, src), X2 = sh(X2, src);
    const double d = at(G, p, p);
    const double g = at(G, p, c) / d, x1 = at(X1, p, c) / d, x2 = at(X2, p, c) / d;
    const double f = at(G, r, p);
    if (r == p) {
      G = g, X1 = x1, X2 = x2;
    } else {
      G -= f * g, X1 -= f * x1, X2 -= f * x2;
    }
  }
}

struct Lane {
  int lane, r, c;
  int64_t wave;
  __device__ Lane() {
    lane = threadIdx.x & (WAVE - 1);
    r = lane >> 3;
    c = lane & 7;
    wave = int64_t(blockIdx.x) * WPB + (threadIdx.x >> 6);
  }
};

// ---- extents: what a kernel of the fused log-probability knows of the member it serves ------------------------------
// The kernels are instantiated over a policy that resolves member blockIdx.y to a Member: the steps it covers and where
// its arrays start, as offsets from the pointers the kernel was given.
//   UniformExtent   every member covers the same n steps in chunks of lc; its arrays lie a stride after its neighbour's
//                   (batches of models over one series, and the single call: the batch of one)
//   TableExtent     every member has an extent of its own, one QExtent of a device table (sets of series): its slice of
//                   the concatenated t, noise, residual, c, w and z, its own n, lc, chunk count and scan levels.  Inside a
//                   member every index is local, so step 0 is the one that absorbs the stationary prior.  The grid is
//                   sized for the largest member; the waves beyond a member's own count exit at once.
// The scans (UniformLevel / TableLevel) and qs_finish (UniformSums / TableSums) resolve their members the same way.
constexpr int MAXLEV = 4;  // scan levels a series of the table may have (64^4 chunks)

struct QExtent {
  int64_t off;              // of its slice in the concatenated arrays (w: J times that)
  int64_t n, lc, nchunks;
  int64_t lev[MAXLEV + 1];  // its scan's level sizes, continued with 1 beyond its own depth
  int64_t work, chunks;     // offsets of its scan work space and of its per-chunk sums and bad-pivot slots
  int64_t keep, twork;      // gradient: offsets of its kept chunk prefixes and, per direction of a pass, of the tangent
                            // scans' work space (a pass of d directions puts the member d twork doubles in)
};

struct Member {
  int64_t n, lc, nchunks;
  int64_t t, noise, y, fac;     // its coordinates, noise, right-hand side, c (w: J times fac)
  int64_t work, pre, sums, bad; // its scan work space, chunk prefixes, per-chunk sums, bad-pivot slots
};

struct UniformExtent {
  int64_t n, lc, nchunks, noise_stride, y_stride, work_stride, red_stride;
  // eblocks: unused, the prefix pointer a kernel gets is member 0's already
  __device__ __forceinline__ Member operator()(int64_t mem, int64_t eblocks = 0) const {
    return {n, lc, nchunks, 0, mem * noise_stride, mem * y_stride, mem * n, mem * work_stride, mem * work_stride,
            mem * red_stride, mem * nchunks};
  }
};

struct TableExtent {
  const QExtent* tab;
  // eblocks: lane-blocks of level-0 elements per chunk, which precede the chunk prefixes in the member's work space
  // (one right-hand side per member: y lies where the noise does)
  __device__ __forceinline__ Member operator()(int64_t mem, int64_t eblocks = 0) const {
    const QExtent& x = tab[mem];
    return {x.n, x.lc, x.nchunks, x.off, x.off, x.off, x.off, x.work, x.work + x.nchunks * eblocks * WAVE, x.chunks,
            x.chunks};
  }
};

// The members of a table with nrhs right-hand sides each (the solves of the samples): y and the output lie nrhs times the
// slice offset in, and the scans of the ncg column groups run ncg x twork into the work space, as those of a direction pass.
struct TableColsExtent {
  const QExtent* tab;
  int64_t nrhs, ncg;
  __device__ __forceinline__ Member operator()(int64_t mem, int64_t eblocks = 0) const {
    const QExtent& x = tab[mem];
    const int64_t w = x.twork * ncg;
    return {x.n, x.lc, x.nchunks, x.off, x.off, x.off * nrhs, x.off, w, w + x.nchunks * eblocks * WAVE, x.chunks,
            x.chunks};
  }
};

// The gradient's kernels resolve their member through a policy of the same two kinds (UniformGExtent / TableGExtent),
// called with the directions of the pass (nd; 0: a kernel without directions, which works in the primal work space) and
// the lane-blocks of level-0 elements per chunk and direction that precede the chunk prefixes.
// Layout of dc, dw and the per-chunk tangent sums, for kernels and host alike: with nd directions in the pass, a
// member's part starts at nd x (its slice offset) -- GMember::tan for dc (dw: J times that), nd x (its chunk offset),
// GMember::sums, for the sums -- and its directions lie n (dw: n J; sums: nchunks) apart.  Uniform members have the
// slice offset member x n, so direction d of member b is row b nd + d of an (members nd) x n array.
struct GMember {
  int64_t n, lc, nchunks;
  int64_t t, noise, y, fac;  // as Member
  int64_t keep;              // the primal scans' kept chunk prefixes: filtered covariances, then (nchunks x WAVE on) solve states
  int64_t work, pre;         // the scan work space of this pass and its chunk prefixes
  int64_t tan, sums;
};

struct UniformGExtent {  // keep, work space, noise and residual one stride per member apart; the prefix pointer is member 0's
  int64_t n, lc, nchunks, noise_stride, y_stride, keep_stride, work_stride;
  __device__ __forceinline__ GMember operator()(int64_t mem, int64_t nd, int64_t eblocks) const {
    return {n, lc, nchunks, 0, mem * noise_stride, mem * y_stride, mem * n, mem * keep_stride, mem * work_stride,
            mem * work_stride, nd * mem * n, nd * mem * nchunks};
  }
};

struct TableGExtent {  // the pointers are the bases of the chain's arrays
  const QExtent* tab;
  __device__ __forceinline__ GMember operator()(int64_t mem, int64_t nd, int64_t eblocks) const {
    const QExtent& x = tab[mem];
    const int64_t work = nd ? x.twork * nd : x.work, width = nd ? nd : 1;
    return {x.n, x.lc, x.nchunks, x.off, x.off, x.off, x.off, x.keep, work, work + x.nchunks * width * eblocks * WAVE,
            nd * x.off, nd * x.chunks};
  }
};

// ---- factor, phase 1: fold each chunk into one filtering element (A, C, J) ----------------------------------
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_fold(const QModel* __restrict__ mp, const double* __restrict__ t,
                                                      const double* __restrict__ noise, E ext,
                                                      double* __restrict__ elem) {
  const Lane L;
  const int64_t mem = blockIdx.y;
  const Member M = ext(mem);
  if (L.wave >= M.nchunks) return;
  const QModel& m = mp[mem];
  t += M.t, noise += M.noise, elem += M.work;
  const int64_t n = M.n, lc = M.lc;
  const int J = m.J, r = L.r, c = L.c;
  const double P = m.P[L.lane];
  double A = (r == c && r < J) ? 1.0 : 0.0, C = 0.0, Jm = 0.0;
  const int64_t n0 = L.wave * lc, n1 = min(n, n0 + lc);
  for (int64_t i = n0; i < n1; ++i) {
    if (i == 0) {  // the first point absorbs the stationary prior: A = 0, C = filtered covariance, J = 0
      const double Ph = Xh(m, P, r);
      const double Ph_c = sh(Ph, c * 8);
      double s = noise[0];
      for (int k = 0; k < J; ++k) s += m.h[k] * sh(Ph, k * 8);
      A = 0.0, Jm = 0.0;
      C = (r < J && c < J) ? P - Ph * Ph_c / s : 0.0;
      continue;
    }
    const double Phi = phi_entry(m, dt_at(t, i), r, c);
    const double Q = P - mm_nt(mm(Phi, P, J, r, c), Phi, J, r, c);  // P - A P A^T
    const double Qh = Xh(m, Q, r), Qh_c = sh(Qh, c * 8);
    double s = noise[i];
    for (int k = 0; k < J; ++k) s += m.h[k] * sh(Qh, k * 8);
    const double v_c = hT(m, Phi, c), v_r = sh(v_c, r);  // v = A^T h
    const double Aj = Phi - Qh * v_c / s;                // (I - K h^T) A,  K = Q h / s
    const double Cj = Q - Qh * Qh_c / s;                 // (I - K h^T) Q
    // fold (A, C, J) o (Aj, Cj, v v^T / s):  M = (I + C v v^T / s)^-1 = I - u v^T / beta
    double u = 0.0;
    for (int k = 0; k < J; ++k) u += at(C, r, k) * sh(v_r, k * 8);
    double beta = s;
    for (int k = 0; k < J; ++k) beta += sh(v_r, k * 8) * sh(u, k * 8);
    const double u_c = sh(u, c * 8);
    double a_c = 0.0;  // a = A^T v
    for (int k = 0; k < J; ++k) a_c += at(A, k, c) * sh(v_r, k * 8);
    const double a_r = sh(a_c, r);
    const double T = A - u * a_c / beta;
    const double U = C - u * u_c / beta;
    A = mm(Aj, T, J, r, c);
    C = symm(mm_nt(mm(Aj, U, J, r, c), Aj, J, r, c) + Cj, r, c);
    Jm = symm(Jm + a_r * a_c / beta, r, c);
  }
  double* e = elem + L.wave * 3 * WAVE;
  e[L.lane] = A, e[WAVE + L.lane] = C, e[2 * WAVE + L.lane] = Jm;
}

// ---- factor, phase 2: the combine of two filtering elements (the scan itself: qs_scan_reduce / qs_scan_down) ------
__device__ void ric_combine(double& A, double& C, double& Jm, double A2, double C2, double J2, int J, int r,
                            int c) {
  double G = mm(C, J2, J, r, c) + ((r == c && r < J) ? 1.0 : 0.0);
  double XA = A, XC = C;
  gj_solve(G, XA, XC, J, r, c);  // (I + C J2)^-1 [A | C]
  const double An = mm(A2, XA, J, r, c);
  const double Cn = symm(mm_nt(mm(A2, XC, J, r, c), A2, J, r, c) + C2, r, c);
  const double Jn = symm(mm_tn(A, mm(J2, XA, J, r, c), J, r, c) + Jm, r, c);
  A = An, C = Cn, Jm = Jn;
}

// ---- scan policies: the element types of phase 2 ------------------------------------------------------------------
// An element is ESZ lane-blocks (one double per lane each), the state carried down PSZ of them.  combine(a, x) makes
// the accumulated element a that of "a, then x"; advance(p, x) takes the state p across x.  All but the Riccati scan
// are built from two steps over (M2, V2) blocks:
//   lin_step   X <- M2 X + V2              cong_step   X <- sym(M2 X M2^T + V2)
//   ScanRiccati  (A, C, J)       | P       ric_combine; down: X = (I + P J2)^-1 P by gj_solve, then cong_step(A2, X, C2)
//   ScanAffine   (M, V)          | X       M <- M2 M, V by lin_step
//   ScanCong     (M, V)          | X       M <- M2 M, V by cong_step
//   ScanPred     (M, V, Mf, Vf)  | (X, f)  a ScanCong on blocks 0-1 beside a ScanAffine on blocks 2-3
__device__ __forceinline__ double lin_step(double M2, double X, double V2, int J, int r, int c) {
  return mm(M2, X, J, r, c) + V2;
}
__device__ __forceinline__ double cong_step(double M2, double X, double V2, int J, int r, int c) {
  return symm(mm_nt(mm(M2, X, J, r, c), M2, J, r, c) + V2, r, c);
}

struct ScanRiccati {
  static constexpr int ESZ = 3, PSZ = 1;
  static __device__ __forceinline__ void combine(double* a, const double* x, int J, int r, int c) {
    ric_combine(a[0], a[1], a[2], x[0], x[1], x[2], J, r, c);
  }
  static __device__ __forceinline__ void advance(double* p, const double* x, int J, int r, int c) {
    double G = mm(p[0], x[2], J, r, c) + ((r == c && r < J) ? 1.0 : 0.0);
    double X = p[0], dummy = 0.0;
    gj_solve(G, X, dummy, J, r, c);  // (I + P J2)^-1 P
    p[0] = cong_step(x[0], X, x[1], J, r, c);
  }
};

struct ScanAffine {
  static constexpr int ESZ = 2, PSZ = 1;
  static __device__ __forceinline__ void combine(double* a, const double* x, int J, int r, int c) {
    const double Mn = mm(x[0], a[0], J, r, c);
    a[1] = lin_step(x[0], a[1], x[1], J, r, c);
    a[0] = Mn;
  }
  static __device__ __forceinline__ void advance(double* p, const double* x, int J, int r, int c) {
    p[0] = lin_step(x[0], p[0], x[1], J, r, c);
  }
};

struct ScanCong {
  static constexpr int ESZ = 2, PSZ = 1;
  static __device__ __forceinline__ void combine(double* a, const double* x, int J, int r, int c) {
    a[1] = cong_step(x[0], a[1], x[1], J, r, c);
    a[0] = mm(x[0], a[0], J, r, c);
  }
  static __device__ __forceinline__ void advance(double* p, const double* x, int J, int r, int c) {
    p[0] = cong_step(x[0], p[0], x[1], J, r, c);
  }
};

struct ScanPred {
  static constexpr int ESZ = 4, PSZ = 2;
  static __device__ __forceinline__ void combine(double* a, const double* x, int J, int r, int c) {
    ScanCong::combine(a, x, J, r, c);
    ScanAffine::combine(a + 2, x + 2, J, r, c);
  }
  static __device__ __forceinline__ void advance(double* p, const double* x, int J, int r, int c) {
    ScanCong::advance(p, x, J, r, c);
    ScanAffine::advance(p + 1, x + 2, J, r, c);
  }
};

// this lane's entries of NB consecutive lane-blocks
template <int NB>
__device__ __forceinline__ void load_blocks(double* v, const double* p, int lane) {
#pragma unroll
  for (int k = 0; k < NB; ++k) v[k] = p[k * WAVE + lane];
}
template <int NB>
__device__ __forceinline__ void store_blocks(double* p, const double* v, int lane) {
#pragma unroll
  for (int k = 0; k < NB; ++k) p[k * WAVE + lane] = v[k];
}

// Work layout of a scan over level sizes sz[]: level 0's elements (where the fold put them), then per level the
// prefixes and the next level's elements.  *el, *pre: where level l's elements and prefixes start.
template <class S>
__host__ __device__ inline void level_offsets(const int64_t* sz, int l, int64_t width, int64_t* el, int64_t* pre) {
  constexpr int64_t esz = S::ESZ * WAVE, psz = S::PSZ * WAVE;
  int64_t e = 0, cur = sz[0] * width * esz;
  for (int k = 0; k < l; ++k) {
    cur += sz[k] * width * psz;
    e = cur;
    cur += sz[k + 1] * width * esz;
  }
  *el = e, *pre = cur;
}

// One level of one member's scan: its elements and groups, and where they lie from the pointers the kernel was given
// (reduce: in, out; down: in, pre_in, pre_out)
struct Level {
  int64_t count, ngroups, in, out, pre_in, pre_out;
};

struct UniformLevel {  // the pointers are member 0's, member b's work_stride doubles after member b - 1's
  int64_t count, ngroups, work_stride;
  template <class S>
  __device__ __forceinline__ Level at(int64_t mem, int64_t width) const {
    const int64_t o = mem * work_stride;
    return {count, ngroups, o, o, o, o};
  }
};

struct TableLevel {  // level `level` of every member's own scan; the pointers are the base of the work space
  const QExtent* tab;
  int32_t level;
  int32_t tangent;  // the scans of a direction pass: the member's work space lies width x twork in, not at work
  template <class S>
  __device__ __forceinline__ Level at(int64_t mem, int64_t width) const {
    const QExtent& x = tab[mem];
    const int64_t w = tangent ? x.twork * width : x.work;
    int64_t el, pre, el_up, pre_up;
    level_offsets<S>(x.lev, level, width, &el, &pre);
    level_offsets<S>(x.lev, level + 1, width, &el_up, &pre_up);
    return {x.lev[level], x.lev[level + 1], w + el, w + el_up, w + pre_up, w + pre};
  }
};

// One level of a scan: `width` independent scans over `count` elements each, interleaved as element * width + scan;
// one wavefront per group of GROUP elements of one scan.  Member blockIdx.y: model mp[blockIdx.y], its level from the
// policy E.  qs_scan_reduce folds each group into one element of the next level; qs_scan_down writes the state before
// every element of a group from the state before the group (prefix_in: one per group; nullptr: the top level, which
// starts from 0).  A member of a table whose own scan is shallower than the launch has one element per upper level:
// the reduce copies it, the top-level down pass stores the zero state, and its level-0 prefixes start from the same
// +0.0 as when its own top level is the launch's.
template <class S, class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_scan_reduce(const QModel* __restrict__ mp,
                                                             const double* __restrict__ in, int64_t width,
                                                             double* __restrict__ out, E lev) {
  const Lane L;
  const int64_t mem = blockIdx.y;
  const Level V = lev.template at<S>(mem, width);
  if (L.wave >= V.ngroups * width) return;
  const int J = mp[mem].J;
  in += V.in, out += V.out;
  const int64_t g = L.wave / width, d = L.wave % width;
  const int64_t b = g * GROUP, e = min(V.count, b + GROUP);
  double a[S::ESZ], x[S::ESZ];
  load_blocks<S::ESZ>(a, in + (b * width + d) * S::ESZ * WAVE, L.lane);
  for (int64_t i = b + 1; i < e; ++i) {
    load_blocks<S::ESZ>(x, in + (i * width + d) * S::ESZ * WAVE, L.lane);
    S::combine(a, x, J, L.r, L.c);
  }
  store_blocks<S::ESZ>(out + L.wave * S::ESZ * WAVE, a, L.lane);
}

template <class S, class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_scan_down(const QModel* __restrict__ mp,
                                                           const double* __restrict__ elem, int64_t width,
                                                           const double* __restrict__ prefix_in,
                                                           double* __restrict__ prefix_out, E lev) {
  const Lane L;
  const int64_t mem = blockIdx.y;
  const Level V = lev.template at<S>(mem, width);
  if (L.wave >= V.ngroups * width) return;
  const int J = mp[mem].J;
  elem += V.in, prefix_out += V.pre_out;
  const int64_t g = L.wave / width, d = L.wave % width;
  const int64_t b = g * GROUP, e = min(V.count, b + GROUP);
  double p[S::PSZ], x[S::ESZ];
#pragma unroll
  for (int k = 0; k < S::PSZ; ++k) p[k] = 0.0;
  if (prefix_in) load_blocks<S::PSZ>(p, prefix_in + V.pre_in + L.wave * S::PSZ * WAVE, L.lane);
  for (int64_t i = b; i < e; ++i) {
    store_blocks<S::PSZ>(prefix_out + (i * width + d) * S::PSZ * WAVE, p, L.lane);
    load_blocks<S::ESZ>(x, elem + (i * width + d) * S::ESZ * WAVE, L.lane);
    S::advance(p, x, J, L.r, L.c);
  }
}

// ---- factor, phase 3: the sequential recursion from each chunk's incoming filtered covariance ------------------
// member blockIdx.y (uniform: c at cbuf + y n, w at wbuf + y n J, its bad-pivot slots at bad + y nchunks)
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_emit(const QModel* __restrict__ mp, const double* __restrict__ t,
                                                      const double* __restrict__ noise, E ext,
                                                      const double* __restrict__ prefix, double* __restrict__ cbuf,
                                                      double* __restrict__ wbuf, double* __restrict__ logsum,
                                                      int64_t* __restrict__ bad) {
  const Lane L;
  const int64_t mem = blockIdx.y;
  const Member M = ext(mem, ScanRiccati::ESZ);
  if (L.wave >= M.nchunks) return;
  const QModel& m = mp[mem];
  const int J = m.J, r = L.r, c = L.c;
  t += M.t, noise += M.noise, prefix += M.pre, cbuf += M.fac, wbuf += M.fac * J;
  logsum += M.sums, bad += M.bad;
  const int64_t n = M.n, lc = M.lc;
  const double Pinf = m.P[L.lane];
  double P = prefix[L.wave * WAVE + L.lane];
  double acc = 0.0;
  int64_t first_bad = INT64_MAX;
  const int64_t n0 = L.wave * lc, n1 = min(n, n0 + lc);
  for (int64_t i = n0; i < n1; ++i) {
    double Pm = Pinf;
    if (i > 0) {
      const double Phi = phi_entry(m, dt_at(t, i), r, c);
      Pm = symm(mm_nt(mm(Phi, P - Pinf, J, r, c), Phi, J, r, c) + Pinf, r, c);
    }
    const double g = Xh(m, Pm, r), g_c = sh(g, c * 8);
    double cv = noise[i];
    for (int k = 0; k < J; ++k) cv += m.h[k] * sh(g, k * 8);
    if (!(cv > 0.0) && first_bad == INT64_MAX) first_bad = i;
    const double sq = sqrt(cv);
    if (L.lane == 0) cbuf[i] = cv;
    if (c == 0 && r < J) wbuf[i * J + r] = g / sq;
    acc += log(cv);
    P = symm(Pm - g * g_c / cv, r, c);
  }
  if (L.lane == 0) logsum[L.wave] = acc, bad[L.wave] = first_bad;
}

// ---- affine recurrences: L^-1 y (FWD), L^-T y (BWD), L z (DOT) -------------------------------------------------
// One step on a lane-layout block X (J rows; columns = right-hand sides, or the columns of M when y = 0).
//   FWD: f = A X; e = y - h^T f; X' = f + (w / sqrt c) e          out z = e / sqrt c
//   DOT: f = A X; X' = f + w y                                    out sqrt(c) y + h^T f
//   BWD: x = (y - w^T X) / sqrt c; X' = A^T (X + h x)             out x
struct StepData {
  double Phi, w_r, sq, h_r;
};

__device__ __forceinline__ StepData step_data(const QModel& m, const double* t, const double* cbuf, const double* wbuf,
                                     int64_t i, int r, int c) {
  StepData d;
  d.Phi = phi_entry(m, dt_at(t, i), r, c);
  d.w_r = r < m.J ? wbuf[i * m.J + r] : 0.0;
  d.sq = sqrt(cbuf[i]);
  d.h_r = r < m.J ? m.h[r] : 0.0;
  return d;
}

// returns X', writes the step's output value (meaningful in lanes of row 0) to *o
__device__ __forceinline__ double step_apply(int op, const QModel& m, const StepData& d, double X, double y, double* o, int r,
                                    int c) {
  const int J = m.J;
  if (op == TGP_QS_BWD) {
    double wx = 0.0;
    for (int k = 0; k < J; ++k) wx += sh(d.w_r, k * 8) * at(X, k, c);
    const double x = (y - wx) / d.sq;
    *o = x;
    const double B = X + d.h_r * x;
    return mm_tn(d.Phi, B, J, r, c);
  }
  const double f = mm(d.Phi, X, J, r, c);
  const double hf = hT(m, f, c);
  if (op == TGP_QS_FWD) {
    const double z = (y - hf) / d.sq;
    *o = z;
    return f + d.w_r * z;
  }
  *o = d.sq * y + hf;
  return f + d.w_r * y;
}

// The chunk at scan position k: its steps [n0, n1) and its j-th step.  A backward walk (L^-T y, the backward pass of
// the prediction) takes the chunks and their steps from the end.
struct Chunk {
  int64_t n0, n1;
  bool back;
  __device__ Chunk(bool back_, int64_t k, int64_t nchunks, int64_t lc, int64_t n) : back(back_) {
    n0 = (back ? nchunks - 1 - k : k) * lc;
    n1 = min(n, n0 + lc);
  }
  __device__ int64_t len() const { return n1 - n0; }
  __device__ int64_t step(int64_t j) const { return back ? n1 - 1 - j : n0 + j; }
};

template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_aff_fold(int op, const QModel* __restrict__ mp,
                                                          const double* __restrict__ t, const double* __restrict__ cbuf,
                                                          const double* __restrict__ wbuf, E ext, int64_t nrhs,
                                                          int64_t ncg, const double* __restrict__ y,
                                                          double* __restrict__ elem) {
  const Lane L;
  const int64_t mem = blockIdx.y;
  const Member mx = ext(mem);
  if (L.wave >= mx.nchunks * ncg) return;
  const QModel& m = mp[mem];
  t += mx.t, cbuf += mx.fac, wbuf += mx.fac * m.J, y += mx.y, elem += mx.work;
  const int64_t n = mx.n, lc = mx.lc, nchunks = mx.nchunks;
  const int r = L.r, c = L.c;
  const int64_t k = L.wave / ncg, cg = L.wave % ncg, col = cg * 8 + c;
  double M = (r == c && r < m.J) ? 1.0 : 0.0, V = 0.0, o;
  const Chunk ch(op == TGP_QS_BWD, k, nchunks, lc, n);
  for (int64_t j = 0, len = ch.len(); j < len; ++j) {
    const int64_t i = ch.step(j);
    const StepData d = step_data(m, t, cbuf, wbuf, i, r, c);
    const double yv = col < nrhs ? y[i * nrhs + col] : 0.0;
    M = step_apply(op, m, d, M, 0.0, &o, r, c);
    V = step_apply(op, m, d, V, yv, &o, r, c);
  }
  double* e = elem + L.wave * 2 * WAVE;
  e[L.lane] = M, e[WAVE + L.lane] = V;
}

template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_aff_emit(int op, const QModel* __restrict__ mp,
                                                          const double* __restrict__ t, const double* __restrict__ cbuf,
                                                          const double* __restrict__ wbuf, E ext, int64_t nrhs,
                                                          int64_t ncg, const double* __restrict__ prefix,
                                                          const double* __restrict__ y, double* __restrict__ out,
                                                          double* __restrict__ sumsq) {
  const Lane L;
  const int64_t mem = blockIdx.y;
  const Member mx = ext(mem, ScanAffine::ESZ * ncg);
  if (L.wave >= mx.nchunks * ncg) return;
  const QModel& m = mp[mem];
  t += mx.t, cbuf += mx.fac, wbuf += mx.fac * m.J, prefix += mx.pre, y += mx.y, out += mx.fac * nrhs;
  const int64_t n = mx.n, lc = mx.lc, nchunks = mx.nchunks;
  const int r = L.r, c = L.c;
  const int64_t k = L.wave / ncg, cg = L.wave % ncg, col = cg * 8 + c;
  double X = prefix[L.wave * WAVE + L.lane], o = 0.0, acc = 0.0;
  const Chunk ch(op == TGP_QS_BWD, k, nchunks, lc, n);
  for (int64_t j = 0, len = ch.len(); j < len; ++j) {
    const int64_t i = ch.step(j);
    const StepData d = step_data(m, t, cbuf, wbuf, i, r, c);
    const double yv = col < nrhs ? y[i * nrhs + col] : 0.0;
    X = step_apply(op, m, d, X, yv, &o, r, c);
    if (r == 0 && col < nrhs) {
      out[i * nrhs + col] = o;
      acc += o * o;
    }
  }
  if (sumsq) {  // fixed-order sum over the 8 columns of row 0
    double s = 0.0;
    for (int q = 0; q < 8; ++q) s += sh(acc, q);
    if (L.lane == 0) sumsq[mx.sums + L.wave] = s;
  }
}

// ---- prediction: conditional mean and variance at test points ---------------------------------------------------
// With alpha = K^-1 r, i the last data index with t_i <= x, A_l = A(x - t_i), A_r = A(t_{i+1} - x):
//   forward   D_n = A_n D_{n-1} A_n^T + w_n w_n^T,             F_n = A_n F_{n-1} + P h alpha_n
//   backward  O_n = T_n^T O_{n+1} T_n + h h^T / c_n,           B_n = A_{n+1}^T B_{n+1} + h alpha_n
//             T_n = A_{n+1} (I - w_n h^T / sqrt c_n)   (the closed-loop map of the forward solve)
//   q = A_l^T h,  e = P h - A_l D_i q,  e^- = A_r e
//   mean = q^T F_i + (A_r P h)^T B_{i+1},   var = h^T P h - q^T D_i q - e^-T O_{i+1} e^-
// Both directions are scans over elements (M, V, Mf, Vf): X <- M X M^T + V and f <- Mf f + Vf, combined as
// (M2 M1, M2 V1 M2^T + V2, Mf2 Mf1, Mf2 Vf1 + Vf2).  f lives in column 0 of a lane-layout block.  D_n and O_n are
// never stored: the emit pass of each direction walks its chunk once and serves the test points whose interval ends
// (forward) or starts (backward) there.  Test points are visited in the order of their interval index; the forward
// pass leaves (q^T F, q^T D q, e) per test point and term in `pt` (PT doubles each), the backward pass finishes both outputs.
constexpr int PT = 2 + QJ;

// (number of t_n <= x) - 1: the interval of x, -1 before the first point (NaN lands there too)
__device__ __forceinline__ int64_t interval_of(const double* __restrict__ t, int64_t n, double xv) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (t[mid] <= xv) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// idx[m]: the interval of x_m
__global__ void qs_pred_locate(const double* __restrict__ t, int64_t n, const double* __restrict__ x, int64_t m,
                               int64_t* __restrict__ idx) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= m) return;
  idx[j] = interval_of(t, n, x[j]);
}

// Sets of series: the test points of one prediction call, one QTest per member of the chain (a small table that goes up
// with every chain: test points change from call to call, so they are not part of the resident QExtent).  A member's
// xt, sidx, order, pt, mean and var lie `off` entries (pt: PT times that) into the chain's concatenated arrays; inside
// its slice every index is local.  own: the test points are the member's own data (m == its n), nothing was uploaded.
struct QTest {
  int64_t off, m, own;
};

// The locate kernel for the members of an extent table (blockIdx.y): sorted position j of member b holds its test point
// order[j] (sorted by value on the host, NaN first), so sidx comes out non-decreasing.  A member at its own data is
// qs_pred_identity's route: the data are sorted already, the order is the identity and is written here.
__global__ void qs_pred_locate_table(const QExtent* __restrict__ tab, const QTest* __restrict__ tests,
                                     const double* __restrict__ t, const double* __restrict__ x,
                                     int64_t* __restrict__ order, int64_t* __restrict__ sidx) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const QTest& T = tests[blockIdx.y];
  if (j >= T.m) return;
  const QExtent& e = tab[blockIdx.y];
  t += e.off, order += T.off, sidx += T.off;
  if (T.own) order[j] = j;
  sidx[j] = interval_of(t, e.n, T.own ? t[j] : x[T.off + order[j]]);
}

// the test points are the sorted data themselves: their intervals are already non-decreasing, the order is the identity
__global__ void qs_pred_identity(const int64_t* __restrict__ idx, int64_t m, int64_t* __restrict__ sidx,
                                 int64_t* __restrict__ order) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= m) return;
  sidx[j] = idx[j];
  order[j] = j;
}

// first position p in the sorted sidx[0..m) with sidx[p] >= v
__device__ __forceinline__ int64_t lower_bound_idx(const int64_t* sidx, int64_t m, int64_t v) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (sidx[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one forward / backward step of the pair (X, f); dir 0: step i consumes A_i, dir 1: step i consumes A_{i+1}
struct PredStep {
  double Phi, T, V, Vf;  // T: the congruence map (dir 0: A_i, used as T X T^T; dir 1: T_i, used as T^T X T)
};

__device__ __forceinline__ PredStep pred_step(int dir, const QModel& m, const double* t, const double* cbuf,
                                              const double* wbuf, const double* alpha, int64_t n, int64_t i, int r,
                                              int c, double Ph_r) {
  PredStep s;
  const int J = m.J;
  const double w_r = r < J ? wbuf[i * J + r] : 0.0;
  const double a = alpha ? alpha[i] : 0.0;
  if (dir == 0) {
    s.Phi = phi_entry(m, dt_at(t, i), r, c);
    s.T = s.Phi;
    s.V = w_r * sh(w_r, c * 8);
    s.Vf = c == 0 ? Ph_r * a : 0.0;
  } else {
    s.Phi = phi_entry(m, i + 1 < n ? t[i + 1] - t[i] : 0.0, r, c);
    const double cv = cbuf[i];
    const double h_r = r < J ? m.h[r] : 0.0, h_c = c < J ? m.h[c] : 0.0;
    double Aw = 0.0;
    for (int k = 0; k < J; ++k) Aw += at(s.Phi, r, k) * sh(w_r, k * 8);
    s.T = s.Phi - Aw * h_c / sqrt(cv);
    s.V = h_r * h_c / cv;
    s.Vf = c == 0 ? h_r * a : 0.0;
  }
  return s;
}

__device__ __forceinline__ double cong(int dir, double T, double X, int J, int r, int c) {
  return dir == 0 ? mm_nt(mm(T, X, J, r, c), T, J, r, c) : mm_tn(T, mm(X, T, J, r, c), J, r, c);
}
__device__ __forceinline__ double lin(int dir, double A, double X, int J, int r, int c) {
  return dir == 0 ? mm(A, X, J, r, c) : mm_tn(A, X, J, r, c);
}

template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_pred_fold(int dir, int want_mean, int want_var,
                                                           const QModel* __restrict__ mp, const double* __restrict__ t,
                                                           const double* __restrict__ cbuf,
                                                           const double* __restrict__ wbuf,
                                                           const double* __restrict__ alpha, E ext,
                                                           double* __restrict__ elem) {
  const Lane L;
  const int64_t mem = blockIdx.y;  // member: c, w and alpha as in qs_aff_emit, elements in its (primal) work space
  const GMember G = ext(mem, 0, 0);
  if (L.wave >= G.nchunks) return;
  const int64_t n = G.n, lc = G.lc, nchunks = G.nchunks;
  const QModel& m = mp[mem];
  const int J = m.J, r = L.r, c = L.c;
  t += G.t, cbuf += G.fac, wbuf += G.fac * J, elem += G.work;
  if (alpha) alpha += G.fac;
  const double Ph_r = Xh(m, m.P[L.lane], r);
  const double I = (r == c && r < J) ? 1.0 : 0.0;
  double M = I, V = 0.0, Mf = I, Vf = 0.0;
  const Chunk ch(dir != 0, L.wave, nchunks, lc, n);
  for (int64_t j = 0, len = ch.len(); j < len; ++j) {
    const int64_t i = ch.step(j);
    const PredStep s = pred_step(dir, m, t, cbuf, wbuf, want_mean ? alpha : nullptr, n, i, r, c, Ph_r);
    if (want_var) {
      M = lin(dir, s.T, M, J, r, c);
      V = symm(cong(dir, s.T, V, J, r, c) + s.V, r, c);
    }
    if (want_mean) {
      Mf = lin(dir, s.Phi, Mf, J, r, c);
      Vf = lin(dir, s.Phi, Vf, J, r, c) + s.Vf;
    }
  }
  double* e = elem + L.wave * 4 * WAVE;
  e[L.lane] = M, e[WAVE + L.lane] = V, e[2 * WAVE + L.lane] = Mf, e[3 * WAVE + L.lane] = Vf;
}

// The test side of both serves is a J-vector g per term (gv: nterms x 8 doubles, rows zero-padded, wave-uniform
// loads): g = h is the model's own kernel, h masked to the states of some addends of a sum is those addends' kernel.
// Only the gathers below depend on g; D, F, O and B are driven by the data-side h whatever the term.
// forward: the left parts of sorted test point p, whose interval starts dt before it with state (D, F); Pl: this
// lane's entry of P; pt: nterms x PT
__device__ __forceinline__ void pred_serve_fwd(const QModel& m, const double* __restrict__ gv, int nterms, double D,
                                               double F, double dt, double Pl, int lane, int r, int c,
                                               double* __restrict__ pt) {
  const int J = m.J;
  const double Al = phi_entry(m, dt, r, c);
  for (int term = 0; term < nterms; ++term, gv += QJ, pt += PT) {
    double Pg_r = 0.0, q_c = 0.0;  // P g by row; q = A_l^T g, by column
    for (int k = 0; k < J; ++k) Pg_r += at(Pl, r, k) * gv[k];
    for (int k = 0; k < J; ++k) q_c += gv[k] * at(Al, k, c);
    double Dq = 0.0, qDq = 0.0, u = 0.0, qF = 0.0;
    for (int k = 0; k < J; ++k) Dq += at(D, r, k) * sh(q_c, k);
    for (int k = 0; k < J; ++k) qDq += sh(q_c, k) * sh(Dq, k * 8);
    for (int k = 0; k < J; ++k) u += at(Al, r, k) * sh(Dq, k * 8);
    for (int k = 0; k < J; ++k) qF += sh(q_c, k) * sh(F, k * 8);
    if (lane == 0) pt[0] = qF, pt[1] = qDq;
    if (c == 0) pt[2 + r] = Pg_r - u;
  }
}

// backward: finish sorted test point p, whose interval ends dt after it with state (O, B); term k's outputs land
// `stride` after term k - 1's
__device__ __forceinline__ void pred_serve_bwd(const QModel& m, const double* __restrict__ gv, int nterms, double O,
                                               double B, double dt, double Pl, int lane, int r, int c,
                                               const double* __restrict__ pt, double* __restrict__ mean,
                                               double* __restrict__ var, int64_t stride) {
  const int J = m.J;
  const double Ar = phi_entry(m, dt, r, c);
  for (int term = 0; term < nterms; ++term, gv += QJ, pt += PT) {
    double Pg_r = 0.0, gPg = 0.0;
    for (int k = 0; k < J; ++k) Pg_r += at(Pl, r, k) * gv[k];
    for (int k = 0; k < J; ++k) gPg += gv[k] * sh(Pg_r, k * 8);
    const double e_r = pt[2 + r];
    double em = 0.0, g = 0.0, Oe = 0.0, right = 0.0, gB = 0.0;
    for (int k = 0; k < J; ++k) em += at(Ar, r, k) * sh(e_r, k * 8);
    for (int k = 0; k < J; ++k) g += at(Ar, r, k) * sh(Pg_r, k * 8);
    for (int k = 0; k < J; ++k) Oe += at(O, r, k) * sh(em, k * 8);
    for (int k = 0; k < J; ++k) right += sh(em, k * 8) * sh(Oe, k * 8);
    for (int k = 0; k < J; ++k) gB += sh(g, k * 8) * sh(B, k * 8);
    if (lane == 0) {
      if (mean) mean[term * stride] = pt[0] + gB;
      if (var) var[term * stride] = gPg - pt[1] - right;
    }
  }
}

// What the emit pass knows of the member it serves: its series (a GMember whose `pre` is where its chunk prefixes lie from
// the prefix pointer) and its test points -- mt of them, `at` entries into xt, sidx, order, mean and var (pt: PT times
// that per term); its model and, a model's doubles apart like it, its test-side vectors are number `model` of theirs (the
// single call: 0 whatever the block, so that its model pointer stays the kernel's argument); own: the test points are
// the member's t.
struct PMember {
  GMember g;
  int64_t at, mt, model;
  bool own;
};
struct UniformPExtent {  // the single call: one series, mt test points, every pointer the member's own
  int64_t n, lc, nchunks, mt;
  __device__ __forceinline__ PMember operator()(int64_t) const {
    return {{n, lc, nchunks, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, mt, 0, false};
  }
};
struct TablePExtent {  // sets of series: the pointers are the bases of the chain's arrays, gv the first model's h (one term)
  const QExtent* tab;
  const QTest* tests;
  __device__ __forceinline__ PMember operator()(int64_t mem) const {
    const QTest& x = tests[mem];
    return {TableGExtent{tab}(mem, 0, ScanPred::ESZ), x.off, x.m, mem, x.own != 0};
  }
};

// Member blockIdx.y (the single call: member 0 of one).  sidx: the test points' interval indices, sorted; order: the test
// point at each sorted position; gv: the nterms test-side vectors; pt: mt x nterms x PT; mean, var: nterms x mt
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_pred_emit(int dir, int want_mean, int want_var,
                                                           const QModel* __restrict__ mp, const double* __restrict__ t,
                                                           const double* __restrict__ cbuf,
                                                           const double* __restrict__ wbuf,
                                                           const double* __restrict__ alpha, E ext,
                                                           const double* __restrict__ prefix,
                                                           const double* __restrict__ xt,
                                                           const int64_t* __restrict__ sidx,
                                                           const int64_t* __restrict__ order,
                                                           const double* __restrict__ gv, int nterms,
                                                           double* __restrict__ pt, double* __restrict__ mean,
                                                           double* __restrict__ var) {
  const Lane L;
  const PMember T = ext(blockIdx.y);
  if (L.wave >= T.g.nchunks) return;
  const int64_t n = T.g.n, lc = T.g.lc, nchunks = T.g.nchunks, mt = T.mt;
  const QModel& m = mp[T.model];
  const int J = m.J, r = L.r, c = L.c;
  t += T.g.t, cbuf += T.g.fac, wbuf += T.g.fac * J, prefix += T.g.pre;
  if (alpha) alpha += T.g.fac;
  xt = T.own ? t : xt + T.at;
  sidx += T.at, order += T.at, gv += T.model * int64_t(sizeof(QModel) / sizeof(double));
  pt += T.at * nterms * PT, mean += T.at * nterms, var += T.at * nterms;
  const double Pl = m.P[L.lane];
  const double Ph_r = Xh(m, Pl, r);
  const int64_t ptsz = int64_t(nterms) * PT;
  double X = prefix[L.wave * 2 * WAVE + L.lane], f = prefix[L.wave * 2 * WAVE + WAVE + L.lane];
  const Chunk ch(dir != 0, L.wave, nchunks, lc, n);
  const int64_t n0 = ch.n0, n1 = ch.n1;
  if (dir == 0) {
    // data point i serves the test points of interval i; chunk 0 also those before the first point (state 0)
    int64_t p = L.wave == 0 ? 0 : lower_bound_idx(sidx, mt, n0);
    for (; p < mt && sidx[p] < n0; ++p) pred_serve_fwd(m, gv, nterms, X, f, 0.0, Pl, L.lane, r, c, pt + p * ptsz);
    for (int64_t i = n0; i < n1; ++i) {
      const PredStep s = pred_step(0, m, t, cbuf, wbuf, want_mean ? alpha : nullptr, n, i, r, c, Ph_r);
      if (want_var) X = symm(cong(0, s.T, X, J, r, c) + s.V, r, c);
      if (want_mean) f = lin(0, s.Phi, f, J, r, c) + s.Vf;
      for (; p < mt && sidx[p] == i; ++p)
        pred_serve_fwd(m, gv, nterms, X, f, xt[order[p]] - t[i], Pl, L.lane, r, c, pt + p * ptsz);
    }
  } else {
    // data point i serves the test points of interval i - 1; the last chunk also those of interval n - 1 (state 0)
    int64_t p = lower_bound_idx(sidx, mt, n1 - 1);  // first position past this chunk's points
    if (L.wave == 0) {
      for (int64_t e = mt; e-- > p;) {
        const int64_t o = order[e];
        pred_serve_bwd(m, gv, nterms, X, f, 0.0, Pl, L.lane, r, c, pt + e * ptsz, want_mean ? mean + o : nullptr,
                       want_var ? var + o : nullptr, mt);
      }
    }
    for (int64_t i = n1 - 1; i >= n0; --i) {
      const PredStep s = pred_step(1, m, t, cbuf, wbuf, want_mean ? alpha : nullptr, n, i, r, c, Ph_r);
      if (want_var) X = symm(cong(1, s.T, X, J, r, c) + s.V, r, c);
      if (want_mean) f = lin(1, s.Phi, f, J, r, c) + s.Vf;
      for (; p > 0 && sidx[p - 1] == i - 1; --p) {
        const int64_t o = order[p - 1];
        pred_serve_bwd(m, gv, nterms, X, f, t[i] - xt[o], Pl, L.lane, r, c, pt + (p - 1) * ptsz,
                       want_mean ? mean + o : nullptr, want_var ? var + o : nullptr, mt);
      }
    }
  }
}

// ---- gradient of the log-likelihood: forward-mode tangents, one parameter direction per blockIdx.y ---------------
// With D_n = P - P_n (P the stationary, P_n the filtered covariance; D^-_n = A_n D_{n-1} A_n^T, D_{-1} = 0) and a dot
// for the derivative along one direction:
//   factor   dD_n = M_n dD_{n-1} M_n^T + G_n,   M_n = (I - w_n h^T / sqrt c_n) A_n   (the closed-loop map again)
//   solve    ds_n = M_n ds_{n-1} + u_n          (s_n the state of L^-1 r)
// G_n and u_n are what the plain tangent of one step gives from dD_{n-1} = 0 / ds_{n-1} = 0; they depend on the primal
// D_{n-1} / s_{n-1}, which are not stored, so fold and emit re-run the primal step from the chunk's incoming filtered
// covariance / state (kept from the primal scans).  The factor pass writes dc_n, dw_n (n (1 + J) doubles per
// direction) and a per-chunk sum of dc_n / c_n; the solve pass, which needs them, a per-chunk sum of z_n dz_n:
//   d log p = -1/2 sum dc_n / c_n - sum z_n dz_n.
// Scan elements are (M, V), `ndir` independent scans interleaved as element * ndir + direction.
// Batches of models and sets of series: member blockIdx.z (qs_pred_fold and qs_invdiag_emit, which have no direction:
// blockIdx.y) with model mp[member] and directions dirs[member * ndir + direction]; where the member's arrays lie is
// the gradient extent policy's answer ("extents" above, which also states the layout of dc, dw and the per-chunk sums).
// Uniform: noise, residual, kept prefixes and scan work space lie one stride per member apart (0: shared); c, w, alpha
// and the noise gradient n (n J) apart as in qs_emit.  The single call is member 0 of one.
struct GStep {
  double Phi, cv, dc, w, dw;  // w, dw: by row
};

// one step of the Riccati recursion (as qs_emit) and of its tangent: P, dD in and out
__device__ __forceinline__ GStep gfac_step(const QModel& m, const QDir& d, const double* t, const double* noise,
                                           int64_t i, double Pinf, double dPinf, double& P, double& dD, int r, int c) {
  const int J = m.J;
  GStep s;
  double dPhi;
  phi_entry_d(m, d, dt_at(t, i), r, c, &s.Phi, &dPhi);
  const double N = i > 0 ? P - Pinf : 0.0;  // -D_{n-1}
  const double Pm = symm(mm_nt(mm(s.Phi, N, J, r, c), s.Phi, J, r, c) + Pinf, r, c);
  const double X = mm_nt(mm(dPhi, N, J, r, c), s.Phi, J, r, c);  // -dA D A^T
  const double dPm = dPinf + X + at(X, c, r) - mm_nt(mm(s.Phi, dD, J, r, c), s.Phi, J, r, c);  // dP - dD^-
  const double g = Xh(m, Pm, r), g_c = sh(g, c * 8);
  double cv = noise[i], dg = 0.0, dc = 0.0;
  for (int k = 0; k < J; ++k) cv += m.h[k] * sh(g, k * 8);
  for (int k = 0; k < J; ++k) dg += at(dPm, r, k) * m.h[k] + at(Pm, r, k) * d.dh[k];
  for (int k = 0; k < J; ++k) dc += d.dh[k] * sh(g, k * 8) + m.h[k] * sh(dg, k * 8);
  const double sq = sqrt(cv);
  s.cv = cv, s.dc = dc, s.w = g / sq;
  s.dw = dg / sq - s.w * dc / (2 * cv);
  P = symm(Pm - g * g_c / cv, r, c);
  dD = symm(dPinf - dPm + s.dw * sh(s.w, c * 8) + s.w * sh(s.dw, c * 8), r, c);
  return s;
}

// keep: the base of the kept prefixes (GMember::keep)
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_gfac_fold(const QModel* __restrict__ mp,
                                                           const QDir* __restrict__ dirs, const double* __restrict__ t,
                                                           const double* __restrict__ noise, E ext,
                                                           const double* __restrict__ keep, double* __restrict__ elem) {
  const Lane L;
  const int64_t mem = blockIdx.z;
  const GMember G = ext(mem, gridDim.y, 0);
  if (L.wave >= G.nchunks) return;
  const int64_t n = G.n, lc = G.lc;
  const QModel& m = mp[mem];
  const QDir& d = dirs[mem * gridDim.y + blockIdx.y];
  const double* prefixP = keep + G.keep;
  t += G.t, noise += G.noise, elem += G.work;
  const int J = m.J, r = L.r, c = L.c;
  const double Pinf = m.P[L.lane], dPinf = d.dP[L.lane];
  double P = prefixP[L.wave * WAVE + L.lane], V = 0.0, M = (r == c && r < J) ? 1.0 : 0.0;
  const int64_t n0 = L.wave * lc, n1 = min(n, n0 + lc);
  for (int64_t i = n0; i < n1; ++i) {
    const GStep s = gfac_step(m, d, t, noise, i, Pinf, dPinf, P, V, r, c);
    const double Ms = s.Phi - s.w * hT(m, s.Phi, c) / sqrt(s.cv);
    M = mm(Ms, M, J, r, c);
  }
  double* e = elem + (L.wave * gridDim.y + blockIdx.y) * 2 * WAVE;
  e[L.lane] = M, e[WAVE + L.lane] = V;
}

// dcbuf, dwbuf, dsum: laid out as "extents" states (uniform: members x ndir x n, x n x J, x nchunks)
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_gfac_emit(const QModel* __restrict__ mp,
                                                           const QDir* __restrict__ dirs, const double* __restrict__ t,
                                                           const double* __restrict__ noise, E ext,
                                                           const double* __restrict__ keep,
                                                           const double* __restrict__ prefixD,
                                                           double* __restrict__ dcbuf, double* __restrict__ dwbuf,
                                                           double* __restrict__ dsum) {
  const Lane L;
  const int64_t mem = blockIdx.z;
  const GMember G = ext(mem, gridDim.y, ScanCong::ESZ);
  if (L.wave >= G.nchunks) return;
  const int64_t n = G.n, lc = G.lc;
  const QModel& m = mp[mem];
  const QDir& d = dirs[mem * gridDim.y + blockIdx.y];
  const double* prefixP = keep + G.keep;
  t += G.t, noise += G.noise, prefixD += G.pre;
  const int64_t row = G.tan + blockIdx.y * n;  // of this direction's dc (dw: J times that)
  const int J = m.J, r = L.r, c = L.c;
  const double Pinf = m.P[L.lane], dPinf = d.dP[L.lane];
  double P = prefixP[L.wave * WAVE + L.lane], acc = 0.0;
  double dD = prefixD[(L.wave * gridDim.y + blockIdx.y) * WAVE + L.lane];
  const int64_t n0 = L.wave * lc, n1 = min(n, n0 + lc);
  for (int64_t i = n0; i < n1; ++i) {
    const GStep s = gfac_step(m, d, t, noise, i, Pinf, dPinf, P, dD, r, c);
    if (L.lane == 0) dcbuf[row + i] = s.dc;
    if (c == 0 && r < J) dwbuf[(row + i) * J + r] = s.dw;
    acc += s.dc / s.cv;
  }
  if (L.lane == 0) dsum[G.sums + blockIdx.y * G.nchunks + L.wave] = acc;
}

// one step of L^-1 y (one column) and of its tangent; s, ds: the state by row, in and out; returns z dz
__device__ __forceinline__ double gsol_step(const QModel& m, const QDir& d, double Phi, double dPhi, double w,
                                            double dw, double cv, double dc, double y, double& s, double& ds, int r) {
  const int J = m.J;
  double f = 0.0, df = 0.0, hf = 0.0, dhf = 0.0;
  for (int k = 0; k < J; ++k) {
    const double s_k = sh(s, k * 8);
    f += at(Phi, r, k) * s_k;
    df += at(dPhi, r, k) * s_k + at(Phi, r, k) * sh(ds, k * 8);
  }
  for (int k = 0; k < J; ++k) {
    const double f_k = sh(f, k * 8);
    hf += m.h[k] * f_k;
    dhf += d.dh[k] * f_k + m.h[k] * sh(df, k * 8);
  }
  const double sq = sqrt(cv), z = (y - hf) / sq, dz = -dhf / sq - z * dc / (2 * cv);
  s = f + w * z;
  ds = df + dw * z + w * dz;
  return z * dz;
}

// fold (elem) or emit (prefixT) of the solve's tangent; the primal scan's chunk states (column 0) come from the kept
// prefixes.  elem and prefixT lie in the scan's work space.
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_gsol(const QModel* __restrict__ mp, const QDir* __restrict__ dirs,
                                                      const double* __restrict__ t, const double* __restrict__ cbuf,
                                                      const double* __restrict__ wbuf, const double* __restrict__ dcbuf,
                                                      const double* __restrict__ dwbuf, const double* __restrict__ y,
                                                      E ext, const double* __restrict__ keep,
                                                      const double* __restrict__ prefixT, double* __restrict__ elem,
                                                      double* __restrict__ dsum) {
  const Lane L;
  const int64_t mem = blockIdx.z;
  const GMember G = ext(mem, gridDim.y, ScanAffine::ESZ);
  if (L.wave >= G.nchunks) return;
  const int64_t n = G.n, lc = G.lc, slot = L.wave * gridDim.y + blockIdx.y;
  const QModel& m = mp[mem];
  const QDir& d = dirs[mem * gridDim.y + blockIdx.y];
  const int J = m.J, r = L.r, c = L.c;
  const double* prefixS = keep + G.keep + G.nchunks * WAVE;
  t += G.t, cbuf += G.fac, wbuf += G.fac * J, y += G.y;
  if (prefixT) prefixT += G.pre; else elem += G.work;
  const int64_t row = G.tan + blockIdx.y * n;  // of this direction's dc (dw: J times that)
  const double h_r = r < J ? m.h[r] : 0.0;
  double s = prefixS[L.wave * WAVE + r * 8], ds = prefixT ? prefixT[slot * WAVE + L.lane] : 0.0;
  double M = (r == c && r < J) ? 1.0 : 0.0, acc = 0.0, o;
  const int64_t n0 = L.wave * lc, n1 = min(n, n0 + lc);
  for (int64_t i = n0; i < n1; ++i) {
    double Phi, dPhi;
    phi_entry_d(m, d, dt_at(t, i), r, c, &Phi, &dPhi);
    const double w = r < J ? wbuf[i * J + r] : 0.0, dw = r < J ? dwbuf[(row + i) * J + r] : 0.0;
    const double cv = cbuf[i];
    acc += gsol_step(m, d, Phi, dPhi, w, dw, cv, dcbuf[row + i], y[i], s, ds, r);
    if (!prefixT) M = step_apply(TGP_QS_FWD, m, StepData{Phi, w, sqrt(cv), h_r}, M, 0.0, &o, r, c);
  }
  if (prefixT) {
    if (L.lane == 0) dsum[G.sums + blockIdx.y * G.nchunks + L.wave] = acc;
  } else {
    elem[slot * 2 * WAVE + L.lane] = M, elem[slot * 2 * WAVE + WAVE + L.lane] = ds;
  }
}

// ---- gradient with respect to the noise: 1/2 (alpha_n^2 - (K^-1)_nn) -------------------------------------------------
// (K^-1)_nn = (1 + u^T O_{n+1} u) / c_n, u = A_{n+1} w_n, with O the backward recurrence of the prediction (qs_pred_*,
// dir 1, variance part): this is its emit pass with N outputs instead of test points.
// (4 waves per SIMD asked for: the member's model pointer costs SGPRs that spill into VGPR lanes, 127 -> 135 without it)
template <class E>
__global__ __launch_bounds__(WAVE * WPB) __attribute__((amdgpu_waves_per_eu(4, 4))) void qs_invdiag_emit(
                                                              const QModel* __restrict__ mp,
                                                              const double* __restrict__ t,
                                                              const double* __restrict__ cbuf,
                                                              const double* __restrict__ wbuf,
                                                              const double* __restrict__ alpha, E ext,
                                                              const double* __restrict__ prefix,
                                                              double* __restrict__ out) {
  const Lane L;
  const int64_t mem = blockIdx.y;
  const GMember G = ext(mem, 0, ScanPred::ESZ);
  if (L.wave >= G.nchunks) return;
  const int64_t n = G.n, lc = G.lc, nchunks = G.nchunks;
  const QModel& m = mp[mem];
  const int J = m.J, r = L.r, c = L.c;
  t += G.t, cbuf += G.fac, wbuf += G.fac * J, alpha += G.fac, prefix += G.pre, out += G.fac;
  double X = prefix[L.wave * 2 * WAVE + L.lane];
  const Chunk ch(true, L.wave, nchunks, lc, n);
  for (int64_t j = 0, len = ch.len(); j < len; ++j) {
    const int64_t i = ch.step(j);
    const PredStep s = pred_step(1, m, t, cbuf, wbuf, nullptr, n, i, r, c, 0.0);
    const double w_r = r < J ? wbuf[i * J + r] : 0.0;
    double u = 0.0, Ou = 0.0, q = 0.0;
    for (int k = 0; k < J; ++k) u += at(s.Phi, r, k) * sh(w_r, k * 8);
    for (int k = 0; k < J; ++k) Ou += at(X, r, k) * sh(u, k * 8);
    for (int k = 0; k < J; ++k) q += sh(u, k * 8) * sh(Ou, k * 8);
    if (L.lane == 0) {
      const double a = alpha[i];
      out[i] = 0.5 * (a * a - (1.0 + q) / cbuf[i]);
    }
    X = symm(cong(1, s.T, X, J, r, c) + s.V, r, c);
  }
}

// ---- posterior samples: prior states on a merged grid, conditional mean for blocks of columns ------------------------
// Matheron's rule: with f a joint prior draw at data and test points and eps a draw of the noise,
//   s(.) = f(.) + k(., X) alpha,   alpha = (K + D)^-1 v,   v = r - f(X) - D^1/2 eps
// has the posterior's mean and covariance.  The prior draw is the state-space recurrence over the merged sorted grid
// of G = N + M points (grid point g is point gp[g] of [X; X_test], at coordinate gt[g]; gp == nullptr: the identity),
//   x_0 = chol(P) xi_0,   x_g = A(dt_g) x_{g-1} + chol(Q(dt_g)) xi_g,   Q(dt) = sym(P - A(dt) P A(dt)^T),   f_g = h^T x_g,
// an affine recurrence over a J x 8 block of columns (element (A, chol(Q) xi); ScanAffine).  xi is indexed by point,
// (G x J x nrhs), and f is written by point, so the caller's order needs no pass of its own.  States are not stored.
// chol is the unpivoted lower Cholesky with a guard: a pivot d <= kCholGuard P[j, j] gives a zero column and leaves the
// Schur complement as it is.  dt = 0 has A = I and Q = 0 exactly, so a tie gets one value.
constexpr double kCholGuard = 16 * 0x1p-52;

__device__ __forceinline__ double chol_psd(double S, double Pinf, int J, int r, int c) {
  double Lm = 0.0;
  for (int j = 0; j < J; ++j) {
    const double d = at(S, j, j);
    const bool ok = d > kCholGuard * at(Pinf, j, j);
    const double sq = sqrt(ok ? d : 1.0);
    const double l_r = ok ? (r == j ? sq : at(S, r, j) / sq) : 0.0;  // L[r, j], meaningful for r >= j
    const double l_c = sh(l_r, c * 8);
    if (c == j && r >= j) Lm = l_r;
    if (ok && r > j && c > j) S -= l_r * l_c;
  }
  return Lm;
}

// the element of grid point g: *Phi = A(dt) (0 at the first point, which draws from the stationary prior) and the
// return value chol(Q) xi, both by lane
__device__ __forceinline__ double prior_step(const QModel& m, double Pinf, const double* __restrict__ gt, int64_t g,
                                             double xi, int r, int c, double* Phi) {
  const int J = m.J;
  double S = Pinf;
  *Phi = 0.0;
  if (g > 0) {
    *Phi = phi_entry(m, gt[g] - gt[g - 1], r, c);
    S = symm(Pinf - mm_nt(mm(*Phi, Pinf, J, r, c), *Phi, J, r, c), r, c);
  }
  return mm(chol_psd(S, Pinf, J, r, c), xi, J, r, c);
}

// What a kernel of the samples knows of the member it serves (blockIdx.y): its data (n points in nchunks chunks of lc),
// its mt test points and its merged grid (G = n + mt points in ncG chunks of lcG), and where its rows lie from the
// pointers the kernel was given -- dat: t, alpha and the data side of f; tst: xt, sidx, order and the test side of f;
// grd: gt, gp and xi (J rows per point) -- every array `nrhs` columns wide.  work, pre: the elements and chunk prefixes of
// the scan over its data's chunks, gwork, gpre: of the scan over its grid's, with ncg column groups interleaved.
//   UniformSExtent   the single call: one series, every pointer the member's own
//   TableSExtent     sets of series: data extent `tab[mem]` of the resident table beside grid extent `grid[mem]` of a
//                    second table that goes up with the chain (test points change from call to call): the grid's n,
//                    lc, nchunks and levels are those of G, its off the member's first grid row, so that mt and tst
//                    are the differences of the two.  Either scan runs in the member's `twork` (the same in both
//                    tables), ncg times that into the work space, as the scans of a direction pass do.
struct SMember {
  int64_t n, lc, nchunks, mt, G, lcG, ncG;
  int64_t dat, tst, grd;
  int64_t work, pre, gwork, gpre;
  int64_t model;  // its model is number `model` of the kernel's (the single call: 0 whatever the block, as PMember's)
};
struct UniformSExtent {
  int64_t n, lc, nchunks, mt, G, lcG, ncG;
  __device__ __forceinline__ SMember operator()(int64_t, int64_t) const {
    return {n, lc, nchunks, mt, G, lcG, ncG, 0, 0, 0, 0, 0, 0, 0, 0};
  }
};
struct TableSExtent {
  const QExtent *tab, *grid;
  __device__ __forceinline__ SMember operator()(int64_t mem, int64_t ncg) const {
    const QExtent &x = tab[mem], &g = grid[mem];
    const int64_t w = x.twork * ncg, eb = ScanAffine::ESZ * ncg * WAVE;
    return {x.n, x.lc, x.nchunks, g.n - x.n, g.n, g.lc, g.nchunks, x.off, g.off - x.off, g.off, w, w + x.nchunks * eb,
            w, w + g.nchunks * eb, mem};
  }
};

// Member blockIdx.y.  emit == 0: fold chunk k of column group cg into elem; emit != 0: walk it from its incoming state
// (prefix) and write f = h^T x of point p to fdata[p x nrhs + column], of test point p - n to ftest (may be null: not
// wanted) likewise
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_prior(int emit, const QModel* __restrict__ mp,
                                                       const double* __restrict__ gt, const int64_t* __restrict__ gp,
                                                       E ext, const double* __restrict__ xi, int64_t nrhs, int64_t ncg,
                                                       const double* __restrict__ prefix, double* __restrict__ elem,
                                                       double* __restrict__ fdata, double* __restrict__ ftest) {
  const Lane L;
  const SMember S = ext(blockIdx.y, ncg);
  if (L.wave >= S.ncG * ncg) return;
  const QModel& m = mp[S.model];
  const int J = m.J, r = L.r, c = L.c;
  gt += S.grd, xi += S.grd * J * nrhs;
  if (gp) gp += S.grd;
  const int64_t k = L.wave / ncg, cg = L.wave % ncg, col = cg * 8 + c;
  const bool live = r < J && col < nrhs;
  const double Pinf = m.P[L.lane];
  double M = (r == c && r < J) ? 1.0 : 0.0, X = emit ? prefix[S.gpre + L.wave * WAVE + L.lane] : 0.0, Phi;
  const int64_t g0 = k * S.lcG, g1 = min(S.G, g0 + S.lcG);
  for (int64_t g = g0; g < g1; ++g) {
    const int64_t p = gp ? gp[g] : g;
    const double W = prior_step(m, Pinf, gt, g, live ? xi[(p * J + r) * nrhs + col] : 0.0, r, c, &Phi);
    X = mm(Phi, X, J, r, c) + W;
    if (emit) {
      const double f = hT(m, X, c);
      if (r == 0 && col < nrhs) {
        if (p < S.n) fdata[(S.dat + p) * nrhs + col] = f;
        else if (ftest) ftest[(S.tst + p - S.n) * nrhs + col] = f;
      }
    } else {
      M = mm(Phi, M, J, r, c);
    }
  }
  if (!emit) {
    double* e = elem + S.gwork + L.wave * 2 * WAVE;
    e[L.lane] = M, e[WAVE + L.lane] = X;
  }
}

// key of a test point in the sort by value: NaN goes first, where qs_pred_locate puts it (interval -1)
__host__ __device__ inline double sort_key(double x) { return x != x ? -INFINITY : x; }

// Member blockIdx.y: sorted position j holds its test point order[j] (sorted by value, ties in the caller's order): its
// interval as qs_pred_locate finds it and, with a grid to build, its place in the merged grid (after the data of the same
// value)
template <class E>
__global__ void qs_smp_locate(E ext, const double* __restrict__ t, const double* __restrict__ x,
                              const int64_t* __restrict__ order, int64_t* __restrict__ sidx, double* __restrict__ gt,
                              int64_t* __restrict__ gp) {
  const int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const SMember S = ext(blockIdx.y, 0);
  if (j >= S.mt) return;
  t += S.dat, x += S.tst, order += S.tst, sidx += S.tst;
  const double xv = x[order[j]];
  const int64_t lo = interval_of(t, S.n, xv) + 1;
  sidx[j] = lo - 1;
  if (gt) gt[S.grd + lo + j] = xv, gp[S.grd + lo + j] = S.n + order[j];
}

// its data point i goes after the test points below it
template <class E>
__global__ void qs_smp_place(E ext, const double* __restrict__ t, const double* __restrict__ x,
                             const int64_t* __restrict__ order, double* __restrict__ gt, int64_t* __restrict__ gp) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const SMember S = ext(blockIdx.y, 0);
  if (i >= S.n) return;
  t += S.dat, x += S.tst, order += S.tst, gt += S.grd, gp += S.grd;
  const double tv = t[i];
  int64_t lo = 0, hi = S.mt;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (x[order[mid]] < tv) lo = mid + 1; else hi = mid;
  }
  gt[i + lo] = tv, gp[i + lo] = i;
}

// The two element-wise kernels run over rows x nrhs entries whoever the rows belong to: a chain's members lie row after
// row in arrays of one pitch, so one launch over the chain's rows serves them all.
// e (n x nrhs): eps in, v = r - f(X) - sqrt(noise) eps out
__global__ void qs_smp_resid(const double* __restrict__ resid, const double* __restrict__ noise,
                             const double* __restrict__ f, double* __restrict__ e, int64_t n, int64_t nrhs) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n * nrhs) return;
  const int64_t row = i / nrhs;
  e[i] = resid[row] - f[i] - sqrt(noise[row]) * e[i];
}

// v (n x nrhs): v in, the latent sample at the data f(X) + v - noise alpha (= f + K alpha) out
__global__ void qs_smp_data(const double* __restrict__ noise, const double* __restrict__ f,
                            const double* __restrict__ alpha, double* __restrict__ v, int64_t n, int64_t nrhs) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n * nrhs) return;
  v[i] = f[i] + v[i] - noise[i / nrhs] * alpha[i];
}

// The conditional mean k(x, X) alpha for a block of alpha columns: the F (dir 0) and B (dir 1) recurrences of the
// prediction over J x 8 blocks, F_n = A_n F_{n-1} + P h alpha_n, B_n = A_{n+1}^T B_{n+1} + h alpha_n, with no
// congruence beside them.  alpha: n x nrhs.  This lane's entry of step i's transition and of its forcing term:
__device__ __forceinline__ double cm_step(int dir, const QModel& m, const double* __restrict__ t,
                                          const double* __restrict__ alpha, int64_t n, int64_t i, int64_t nrhs,
                                          int64_t col, double Ph_r, int r, int c, double* Phi) {
  *Phi = phi_entry(m, dir == 0 ? dt_at(t, i) : (i + 1 < n ? t[i + 1] - t[i] : 0.0), r, c);
  const double a = col < nrhs ? alpha[i * nrhs + col] : 0.0;
  return (dir == 0 ? Ph_r : (r < m.J ? m.h[r] : 0.0)) * a;
}

template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_cm_fold(int dir, const QModel* __restrict__ mp,
                                                         const double* __restrict__ t, const double* __restrict__ alpha,
                                                         E ext, int64_t nrhs, int64_t ncg, double* __restrict__ elem) {
  const Lane L;
  const SMember S = ext(blockIdx.y, ncg);
  if (L.wave >= S.nchunks * ncg) return;
  const QModel& m = mp[S.model];
  const int J = m.J, r = L.r, c = L.c;
  const int64_t n = S.n, lc = S.lc, nchunks = S.nchunks;
  t += S.dat, alpha += S.dat * nrhs, elem += S.work;
  const int64_t k = L.wave / ncg, cg = L.wave % ncg, col = cg * 8 + c;
  const double Ph_r = Xh(m, m.P[L.lane], r);
  double M = (r == c && r < J) ? 1.0 : 0.0, V = 0.0, Phi;
  const Chunk ch(dir != 0, k, nchunks, lc, n);
  for (int64_t j = 0, len = ch.len(); j < len; ++j) {
    const double Vf = cm_step(dir, m, t, alpha, n, ch.step(j), nrhs, col, Ph_r, r, c, &Phi);
    M = lin(dir, Phi, M, J, r, c);
    V = lin(dir, Phi, V, J, r, c) + Vf;
  }
  double* e = elem + L.wave * 2 * WAVE;
  e[L.lane] = M, e[WAVE + L.lane] = V;
}

// The gathers, for the test point o whose interval starts dt before it with state F / ends dt after it with state B:
// out[o, column] (+)= q^T F, q = A_l^T h  /  += (A_r P h)^T B
__device__ __forceinline__ void cm_serve(int dir, int accumulate, const QModel& m, double X, double dt, double Ph_r,
                                         int r, int c, bool writes, double* __restrict__ out) {
  const int J = m.J;
  const double A = phi_entry(m, dt, r, c);
  double s = 0.0;
  if (dir == 0) {
    const double q_c = hT(m, A, c);
    for (int k = 0; k < J; ++k) s += sh(q_c, k) * at(X, k, c);
  } else {
    double g = 0.0;
    for (int k = 0; k < J; ++k) g += at(A, r, k) * sh(Ph_r, k * 8);
    for (int k = 0; k < J; ++k) s += sh(g, k * 8) * at(X, k, c);
  }
  if (writes) *out = (accumulate ? *out : 0.0) + s;
}

// Member blockIdx.y; sidx, order, xt as in qs_pred_emit; out: mt x nrhs.  dir 0 writes (accumulate: adds to) its part,
// dir 1 adds its own.
template <class E>
__global__ __launch_bounds__(WAVE * WPB) void qs_cm_emit(int dir, int accumulate, const QModel* __restrict__ mp,
                                                         const double* __restrict__ t, const double* __restrict__ alpha,
                                                         E ext, int64_t nrhs, int64_t ncg,
                                                         const double* __restrict__ prefix,
                                                         const double* __restrict__ xt,
                                                         const int64_t* __restrict__ sidx,
                                                         const int64_t* __restrict__ order, double* __restrict__ out) {
  const Lane L;
  const SMember S = ext(blockIdx.y, ncg);
  if (L.wave >= S.nchunks * ncg) return;
  const QModel& m = mp[S.model];
  const int J = m.J, r = L.r, c = L.c;
  const int64_t n = S.n, lc = S.lc, nchunks = S.nchunks, mt = S.mt;
  t += S.dat, alpha += S.dat * nrhs, prefix += S.pre;
  xt += S.tst, sidx += S.tst, order += S.tst, out += S.tst * nrhs;
  const int64_t k = L.wave / ncg, cg = L.wave % ncg, col = cg * 8 + c;
  const bool writes = r == 0 && col < nrhs;
  const double Ph_r = Xh(m, m.P[L.lane], r);
  double X = prefix[L.wave * WAVE + L.lane], Phi;
  const Chunk ch(dir != 0, k, nchunks, lc, n);
  const int64_t n0 = ch.n0, n1 = ch.n1;
  out += writes ? col : 0;
  if (dir == 0) {
    int64_t p = k == 0 ? 0 : lower_bound_idx(sidx, mt, n0);
    for (; p < mt && sidx[p] < n0; ++p)
      cm_serve(0, accumulate, m, X, 0.0, Ph_r, r, c, writes, out + order[p] * nrhs);
    for (int64_t i = n0; i < n1; ++i) {
      const double Vf = cm_step(0, m, t, alpha, n, i, nrhs, col, Ph_r, r, c, &Phi);
      X = lin(0, Phi, X, J, r, c) + Vf;
      for (; p < mt && sidx[p] == i; ++p) {
        const int64_t o = order[p];
        cm_serve(0, accumulate, m, X, xt[o] - t[i], Ph_r, r, c, writes, out + o * nrhs);
      }
    }
  } else {
    int64_t p = lower_bound_idx(sidx, mt, n1 - 1);
    if (k == 0)
      for (int64_t e = mt; e-- > p;) cm_serve(1, 1, m, X, 0.0, Ph_r, r, c, writes, out + order[e] * nrhs);
    for (int64_t i = n1 - 1; i >= n0; --i) {
      const double Vf = cm_step(1, m, t, alpha, n, i, nrhs, col, Ph_r, r, c, &Phi);
      X = lin(1, Phi, X, J, r, c) + Vf;
      for (; p > 0 && sidx[p - 1] == i - 1; --p) {
        const int64_t o = order[p - 1];
        cm_serve(1, 1, m, X, t[i] - xt[o], Ph_r, r, c, writes, out + o * nrhs);
      }
    }
  }
}

// What qs_finish sums for member `mem`: a[0..na), b[0..nb) and the minimum of bad[0..na), as offsets from its pointers
struct Sums {
  int64_t na, nb, a, b, bad;
};
struct UniformSums {  // member x reads a and b x in_stride doubles, bad x bad_stride slots further on
  int64_t na, nb, in_stride, bad_stride;
  __device__ __forceinline__ Sums operator()(int64_t mem) const {
    return {na, nb, mem * in_stride, mem * in_stride, mem * bad_stride};
  }
};
// a, b and bad: the per-chunk arrays of all members, each member's part where its extent says.  With nd directions per
// member, block x serves direction x % nd of member x / nd (the layout "extents" states); the values have nd = 1.
struct TableSums {
  const QExtent* tab;
  int64_t nd;
  __device__ __forceinline__ Sums operator()(int64_t blk) const {
    const QExtent& x = tab[blk / nd];
    const int64_t o = nd * x.chunks + (blk % nd) * x.nchunks;
    return {x.nchunks, x.nchunks, o, o, o};
  }
};

// one wavefront per block: fixed-order sums and the first bad pivot of member blockIdx.x, which writes out and first_bad
// x out_stride slots further on
template <class E>
__global__ __launch_bounds__(WAVE) void qs_finish(const double* __restrict__ a, const double* __restrict__ b,
                                                  const int64_t* __restrict__ bad, double* __restrict__ out,
                                                  int64_t* __restrict__ first_bad, E sums, int64_t out_stride) {
  const int lane = threadIdx.x;
  const int64_t mem = blockIdx.x;
  const Sums U = sums(mem);
  const int64_t na = U.na, nb = U.nb;
  a += U.a, out += mem * out_stride;
  if (b) b += U.b;
  if (bad) bad += U.bad;
  if (first_bad) first_bad += mem * out_stride;
  double sa = 0.0, sb = 0.0;
  int64_t mb = INT64_MAX;
  for (int64_t i = lane; i < na; i += WAVE) sa += a[i];
  for (int64_t i = lane; b && i < nb; i += WAVE) sb += b[i];
  for (int64_t i = lane; bad && i < na; i += WAVE) mb = min(mb, bad[i]);
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    sa += __shfl_down(sa, off, WAVE);
    sb += __shfl_down(sb, off, WAVE);
    const int64_t o = __shfl_down(mb, off, WAVE);
    mb = min(mb, o);
  }
  if (lane == 0) {
    out[0] = sa, out[1] = sb;
    if (first_bad) *first_bad = mb;
  }
}

// member blockIdx.y: dst[i] = src[i], i < len, the members' rows src_stride and dst_stride doubles apart (the chunk
// prefixes a scan leaves in its work space, set aside before the next scan writes there)
__global__ void qs_keep_rows(const double* __restrict__ src, int64_t src_stride, double* __restrict__ dst,
                             int64_t dst_stride, int64_t len) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, mem = blockIdx.y;
  if (i < len) dst[mem * dst_stride + i] = src[mem * src_stride + i];
}

// the same for the members of an extent table: member blockIdx.y's chunk prefixes of a width-1 scan with `eblocks`
// lane-blocks per element, from its work space to slot `which` (0: filtered covariances, 1: solve states) of its keep
__global__ void qs_keep_table(const QExtent* __restrict__ tab, const double* __restrict__ work, int64_t eblocks,
                              double* __restrict__ keep, int64_t which) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const QExtent& x = tab[blockIdx.y];
  const int64_t len = x.nchunks * WAVE;
  if (i < len) keep[x.keep + which * len + i] = work[x.work + x.nchunks * eblocks * WAVE + i];
}

inline int64_t blocks_for(int64_t waves) { return (waves + WPB - 1) / WPB; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

struct tgp_qsep {
  tgp_ctx* ctx = nullptr;
  int64_t n = 0, lc = 0, nchunks = 0;
  int32_t J = 0;
  bool factored = false;
  int32_t info = 0;
  double logdet = 0.0;
  QModel host_model{};
  QModel* model = nullptr;
  double *t = nullptr, *noise = nullptr, *c = nullptr, *w = nullptr;
  double *io = nullptr, *io2 = nullptr;
  int64_t io_elems = 0, io2_elems = 0;
  double* work = nullptr;  // elements and prefixes of every scan level
  int64_t work_elems = 0;
  double* red = nullptr;   // per-chunk partial sums (2 x nchunks x ncg) + finish output
  int64_t red_elems = 0;
  int64_t* bad = nullptr;  // per-chunk first bad pivot + finish output
  double* pred = nullptr;  // prediction: test points, per-point partial results, mean, variance
  int64_t pred_elems = 0;
  int64_t* pidx = nullptr;  // prediction: interval index per test point, then sorted indices and their order
  int64_t pidx_elems = 0;
  double host_g[QJ * QJ] = {};  // prediction of terms: the test-side vectors (8 x 8, rows zero-padded) and their
  double* gvec = nullptr;       // device copy
  // gradient: chunk prefixes kept from the primal scans (filtered covariance | solve state), the directions of one
  // batch, their dc, dw (the capped scratch), per-chunk partial sums + results, the noise gradient
  double *gkeep = nullptr, *gdir = nullptr, *gtan = nullptr, *gred = nullptr, *gout = nullptr;
  int64_t gkeep_elems = 0, gdir_elems = 0, gtan_elems = 0, gred_elems = 0, gout_elems = 0;
  // batches of models: the models and every array of one launch chain (the capped scratch; batch_layout)
  double* bat = nullptr;
  int64_t bat_elems = 0;
  // posterior samples and the conditional mean of many columns: the arrays of one pass of columns (the capped scratch)
  double* smp = nullptr;
  int64_t smp_elems = 0;
};

// A set of series, each on coordinates of its own: the concatenated t and the extent table stay resident
struct tgp_qsep_series {
  tgp_ctx* ctx = nullptr;
  int64_t nseries = 0;
  std::vector<int64_t> offsets;  // nseries + 1: series b is [offsets[b], offsets[b + 1]) of the concatenated arrays
  std::vector<QExtent> ext;      // the table's host copy; series_fill sets the offsets inside a chain
  std::vector<int64_t> chain0;   // the split the table was cut for: every chain's first member, then nseries
  std::vector<int64_t> chain_d;  // gradient: every chain's directions per pass; posterior draws: its columns per pass
  // what the resident table's chains were cut for: the call (0: none yet, 1: value, 2: value and gradient, 3: value and
  // prediction, 4: value and posterior draws), the state dimension, the directions per member and whether the vectors were
  // wanted (gradient only; prediction: 1, its scan shares the primal work space), for a prediction what was wanted (1:
  // mean, 2: variance; draws: 1: at the data, 2: at the test points) and every member's number of test points, and for
  // draws their number of columns
  struct Cut {
    int32_t call = 0, J = 0, P = 0, vectors = 0, want = 0;
    std::vector<int64_t> tests;
    int64_t cols = 0;
    bool operator==(const Cut& o) const {
      return call == o.call && J == o.J && P == o.P && vectors == o.vectors && want == o.want && tests == o.tests &&
             cols == o.cols;
    }
  } cut;
  int64_t buf_need = 0;          // what the largest of those chains needs, in doubles
  double* t = nullptr;
  QExtent* tab = nullptr;
  double* buf = nullptr;         // the models and every array of one launch chain (the capped scratch)
  int64_t buf_elems = 0;
};

namespace {

using tgp::set_error;

template <class T>
int grow(T** p, int64_t* have, int64_t want) {
  if (*have >= want) return TGP_OK;
  if (*p) hipFree(*p);
  *p = nullptr;
  *have = 0;
  TGP_HIP_TRY(hipMalloc(p, size_t(want) * sizeof(T)));
  *have = want;
  return TGP_OK;
}

// levels of the hierarchical scan over `count` elements: sizes[0] = count, sizes[l+1] = ceil(sizes[l] / GROUP)
std::vector<int64_t> level_sizes(int64_t count) {
  std::vector<int64_t> s{count};
  while (s.back() > GROUP) s.push_back(ceil_div(s.back(), GROUP));
  return s;
}

// Exclusive scan with elements S (a scan policy) over the `count` elements already in `elem0`, `width` independent
// scans interleaved: the level-0 prefixes land in the returned pointer.  Work layout: per level, elements then
// prefixes.  `members` models run at once (grid y): member b uses models[b] and the same layout `work_stride` doubles
// after member b - 1's.
template <class S>
int run_scan(const QModel* models, hipStream_t st, int64_t count, int64_t width, double* elem0, double** prefix0,
             int64_t members = 1, int64_t work_stride = 0) {
  const std::vector<int64_t> sz = level_sizes(count);
  std::vector<double*> el(sz.size()), pre(sz.size());
  for (size_t l = 0; l < sz.size(); ++l) {
    int64_t e, p;
    level_offsets<S>(sz.data(), int(l), width, &e, &p);
    el[l] = elem0 + e, pre[l] = elem0 + p;
  }
  for (size_t l = 0; l + 1 < sz.size(); ++l) {
    const int64_t g = sz[l + 1];
    qs_scan_reduce<S, UniformLevel><<<dim3(unsigned(blocks_for(g * width)), unsigned(members)), WAVE * WPB, 0, st>>>(
        models, el[l], width, el[l + 1], UniformLevel{sz[l], g, work_stride});
  }
  for (size_t l = sz.size(); l-- > 0;) {
    const int64_t g = l + 1 < sz.size() ? sz[l + 1] : 1;
    const double* pin = l + 1 < sz.size() ? pre[l + 1] : nullptr;
    qs_scan_down<S, UniformLevel><<<dim3(unsigned(blocks_for(g * width)), unsigned(members)), WAVE * WPB, 0, st>>>(
        models, el[l], width, pin, pre[l], UniformLevel{sz[l], g, work_stride});
  }
  TGP_HIP_TRY(hipGetLastError());
  *prefix0 = pre[0];
  return TGP_OK;
}

// The same over the members of an extent table, each with a scan of its own: the levels of the deepest member are
// launched (top[l]: the largest level-l size, `depth` levels), every grid sized for the largest member.  The level-0
// prefixes land in each member's work space, where TableExtent / TableGExtent look for them.  width 0: one scan per
// member in its primal work space; width >= 1: the scans of a direction pass, `width` per member, in its tangent one.
template <class S>
int run_scan_table(const QModel* models, hipStream_t st, const QExtent* tab, int64_t members, const int64_t* top,
                   int depth, double* work, int64_t width = 0) {
  const int32_t tangent = width > 0;
  const int64_t w = tangent ? width : 1;
  for (int l = 0; l + 1 < depth; ++l)
    qs_scan_reduce<S, TableLevel><<<dim3(unsigned(blocks_for(top[l + 1] * w)), unsigned(members)), WAVE * WPB, 0, st>>>(
        models, work, w, work, TableLevel{tab, l, tangent});
  for (int l = depth; l-- > 0;)
    qs_scan_down<S, TableLevel><<<dim3(unsigned(blocks_for(top[l + 1] * w)), unsigned(members)), WAVE * WPB, 0, st>>>(
        models, work, w, l + 1 < depth ? work : nullptr, work, TableLevel{tab, l, tangent});
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// chunk length: about 4096 chunks, 16..256 steps each (a function of n only: results depend neither on the device nor
// on what else a launch serves)
int64_t chunk_length(int64_t n) {
  int64_t lc = 16;
  while (lc < 256 && lc * 4096 < n) lc *= 2;
  return lc;
}

// the extent of a series of n points by itself (the single call's rule: a member's chunks are those of its own solver);
// where it lies in a chain is the split's to say
QExtent extent_of(int64_t n) {
  QExtent x{};
  x.n = n;
  x.lc = chunk_length(n);
  x.nchunks = ceil_div(n, x.lc);
  x.lev[0] = x.nchunks;
  for (int l = 0; l < MAXLEV; ++l) x.lev[l + 1] = ceil_div(x.lev[l], GROUP);
  return x;
}

template <class S>
int64_t scan_work(int64_t count, int64_t width) {
  int64_t total = 0;
  for (int64_t s : level_sizes(count)) total += s * width * (S::ESZ + S::PSZ) * WAVE;
  return total;
}

// checks one model's host arrays and packs them
int pack_model(QModel* out, const double* leaves, int32_t nleaves, const int32_t* state_map, int32_t J,
               const double* hvec, const double* Pinf) {
  TGP_ARG_CHECK(J >= 1 && J <= QJ, "quasiseparable state dimension must be 1..%d (got %d)", QJ, J);
  TGP_ARG_CHECK(nleaves >= 1 && nleaves <= QL, "quasiseparable kernels hold 1..%d leaves (got %d)", QL, nleaves);
  TGP_ARG_CHECK(leaves && state_map && hvec && Pinf, "null model array");
  QModel m{};
  m.J = J;
  m.nleaves = nleaves;
  for (int l = 0; l < nleaves; ++l) {
    const int kind = int(leaves[l * 5]);
    TGP_ARG_CHECK(kind >= TGP_QS_EXP && kind <= TGP_QS_SHO_OVER, "unknown quasiseparable leaf kind %d", kind);
    m.kind[l] = kind;
    for (int p = 0; p < 4; ++p) m.par[l][p] = leaves[l * 5 + 1 + p];
  }
  for (int r = 0; r < QJ; ++r)
    for (int l = 0; l < QL; ++l) m.map[r][l] = (r < J && l < nleaves) ? state_map[r * nleaves + l] : -1;
  for (int r = 0; r < J; ++r) {
    m.h[r] = hvec[r];
    for (int c = 0; c < J; ++c) m.P[r * QJ + c] = Pinf[r * J + c];
  }
  *out = m;
  return TGP_OK;
}

int set_model(tgp_qsep* q, const double* leaves, int32_t nleaves, const int32_t* state_map, int32_t J,
              const double* hvec, const double* Pinf) {
  QModel m{};
  TGP_TRY(pack_model(&m, leaves, nleaves, state_map, J, hvec, Pinf));
  q->host_model = m;
  q->J = J;
  TGP_HIP_TRY(hipMemcpyAsync(q->model, &q->host_model, sizeof(QModel), hipMemcpyHostToDevice, q->ctx->stream));
  return TGP_OK;
}

// ---- who the members of a launch chain are -------------------------------------------------------------------------------
// The launch helpers and the chain below are written once over a host-side description of the chain's members, of the
// same two kinds as the device policies:
//   UniformMembers   `count` models over the one series of a handle, every array one stride per member apart; the single
//                    call is such a chain of one member
//   TableMembers     `count` series of a set, each where the resident extent table says
// Either kind supplies
//   t, count          the first member's coordinates (device) and the grid's member extent
//   chunks()          the grid's x extent: the chain's largest chunk count
//   ext(), gext(tangent), sums(nd)
//                     the device policies; `tangent`: the work space is that of a direction pass
//   scan<S>()         the hierarchical scan over the elements a fold kernel left in `work`, `width` scans per member
//                     interleaved; *prefix: what the emit kernel takes as its prefix argument, valid until `work` is
//                     written again (uniform: level 0's prefixes, member 0's; table: `work` itself, where the extent
//                     policies look for each member's)
//   set_aside<S>()    the chunk prefixes of that scan (width 1) into slot `which` of every member's keep (0: filtered
//                     covariances, 1: solve states)
//   own_rhs()         the same members for a right-hand side the chain made itself: one per member
//   own_noise(), own_resid(), room(), held(), n_of(b), off_of(b)
//                     for the chain's buffer: whether every member brings its noise / residual, the totals the buffer
//                     is carved for and those of the members held, member b's length and where it lies in the
//                     chain's arrays
struct Totals {
  int64_t members, points, chunks, work, twork;  // twork: the tangent scans' work space for a pass of D directions
};

struct UniformMembers {
  const double* t;
  int64_t n, lc, nchunks;
  int64_t count = 1, cap = 1;  // members held; members the buffer is carved for (the layout depends on the call alone)
  // member b's noise, right-hand side, primal and tangent scan work space lie one stride after member b - 1's; its
  // per-chunk sums nchunks and its keep 2 nchunks WAVE doubles, its c, out and z n doubles
  int64_t noise_stride = 0, y_stride = 0, work_stride = 0, twork_stride = 0;

  int64_t chunks() const { return nchunks; }
  UniformExtent ext() const { return {n, lc, nchunks, noise_stride, y_stride, work_stride, nchunks}; }
  UniformGExtent gext(bool tangent) const {
    return {n, lc, nchunks, noise_stride, y_stride, 2 * nchunks * WAVE, tangent ? twork_stride : work_stride};
  }
  // block x: row x of the per-chunk arrays, whatever nd (the layout "extents" states)
  UniformSums sums(int64_t) const { return {nchunks, nchunks, nchunks, nchunks}; }
  template <class S>
  int scan(hipStream_t st, const QModel* models, double* work, int64_t width, bool tangent, double** prefix) const {
    return run_scan<S>(models, st, nchunks, width, work, prefix, count, tangent ? twork_stride : work_stride);
  }
  template <class S>
  void set_aside(hipStream_t st, const double* prefix, double* keep, int64_t which) const {
    const int64_t len = nchunks * WAVE;
    qs_keep_rows<<<dim3(unsigned(ceil_div(len, 256)), unsigned(count)), 256, 0, st>>>(prefix, work_stride,
                                                                                     keep + which * len, 2 * len, len);
  }
  UniformMembers own_rhs() const {
    UniformMembers m = *this;
    m.y_stride = n;
    return m;
  }
  bool own_noise() const { return noise_stride != 0; }
  bool own_resid() const { return y_stride != 0; }
  Totals totals(int64_t k) const { return {k, k * n, k * nchunks, k * work_stride, k * twork_stride}; }
  Totals room() const { return totals(cap); }
  Totals held() const { return totals(count); }
  int64_t n_of(int64_t) const { return n; }
  int64_t off_of(int64_t b) const { return b * n; }
};

struct TableMembers {
  const double* t;
  const QExtent* tab;            // the first member's extent (device)
  const QExtent* mine;           // and its host copy
  int64_t count = 0;
  int64_t top[MAXLEV + 1] = {};  // the largest size of every scan level
  int depth = 1;                 // the deepest member's levels: the level sizes grow with the chunk count
  Totals tot{};                  // the buffer holds what the chain's own members need and no more

  int64_t chunks() const { return top[0]; }
  TableExtent ext() const { return {tab}; }
  TableGExtent gext(bool) const { return {tab}; }
  TableSums sums(int64_t nd) const { return {tab, nd}; }
  // the primal work space has room for one scan per member (width 1)
  template <class S>
  int scan(hipStream_t st, const QModel* models, double* work, int64_t width, bool tangent, double** prefix) const {
    *prefix = work;
    return run_scan_table<S>(models, st, tab, count, top, depth, work, tangent ? width : 0);
  }
  template <class S>
  void set_aside(hipStream_t st, const double* prefix, double* keep, int64_t which) const {
    qs_keep_table<<<dim3(unsigned(ceil_div(top[0] * WAVE, 256)), unsigned(count)), 256, 0, st>>>(tab, prefix, S::ESZ,
                                                                                                keep, which);
  }
  const TableMembers& own_rhs() const { return *this; }  // y lies where the extent says, whose it is
  bool own_noise() const { return true; }
  bool own_resid() const { return true; }
  Totals room() const { return tot; }
  Totals held() const { return tot; }
  int64_t n_of(int64_t b) const { return mine[b].n; }
  int64_t off_of(int64_t b) const { return mine[b].off; }
};

// the single call: a uniform chain of one member in the handle's own arrays
UniformMembers single(const tgp_qsep* q) { return {q->t, q->n, q->lc, q->nchunks}; }

// The factor of the members' models (grid y) over their t: qs_fold, the Riccati scan, qs_emit.  c, w, the per-chunk sums
// of log c and the bad-pivot slots as in qs_emit.  *prefix: the chunks' incoming filtered covariances (see scan).
template <class M>
int launch_factor(const M& m, hipStream_t st, const QModel* models, const double* noise, double* work, double* cbuf,
                  double* wbuf, double* logsum, int64_t* bad, double** prefix) {
  const dim3 grid(unsigned(blocks_for(m.chunks())), unsigned(m.count));
  const auto ext = m.ext();
  qs_fold<<<grid, WAVE * WPB, 0, st>>>(models, m.t, noise, ext, work);
  TGP_TRY(m.template scan<ScanRiccati>(st, models, work, 1, false, prefix));
  qs_emit<<<grid, WAVE * WPB, 0, st>>>(models, m.t, noise, ext, *prefix, cbuf, wbuf, logsum, bad);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// out = op(y) for nrhs columns (N x nrhs, row-major) against the members' factors c, w: qs_aff_fold, the affine scan,
// qs_aff_emit.  sumsq: the per-chunk sums of out^2 (optional).  *prefix: the chunks' incoming states (nchunks x ncg x
// WAVE per member; see scan).  Table members take one column.
template <class M>
int launch_affine(const M& m, hipStream_t st, int op, const QModel* models, const double* cbuf, const double* wbuf,
                  int64_t nrhs, const double* y, double* work, double* out, double* sumsq, double** prefix) {
  const int64_t ncg = ceil_div(nrhs, 8);
  const dim3 grid(unsigned(blocks_for(m.chunks() * ncg)), unsigned(m.count));
  const auto ext = m.ext();
  qs_aff_fold<<<grid, WAVE * WPB, 0, st>>>(op, models, m.t, cbuf, wbuf, ext, nrhs, ncg, y, work);
  TGP_TRY(m.template scan<ScanAffine>(st, models, work, ncg, false, prefix));
  qs_aff_emit<<<grid, WAVE * WPB, 0, st>>>(op, models, m.t, cbuf, wbuf, ext, nrhs, ncg, *prefix, y, out, sumsq);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// One direction pass for the members x nd directions (grid z x y), after their factors and forward solves: the factor's
// tangent (qs_gfac_fold, the congruence scan, qs_gfac_emit), the solve's (qs_gsol, the affine scan, qs_gsol) and one
// qs_finish block per (member, direction), which leaves (sum dc / c, sum z dz) at res[2 (member nd + direction)].
// dirs: members x nd; keep: per member the chunks' incoming filtered covariances, then solve states; work: the tangent
// scans' work space; tan: dc | dw (nd n (1 + J) per member) and red: the per-chunk sums (2 nd nchunks per member), laid
// out as "extents" states.
template <class M>
int launch_tangents(const M& m, hipStream_t st, const QModel* models, const QDir* dirs, int64_t nd, const double* noise,
                    const double* cbuf, const double* wbuf, const double* resid, const double* keep, double* work,
                    double* tan, double* red, double* res) {
  const Totals h = m.held();
  const dim3 grid(unsigned(blocks_for(m.chunks())), unsigned(nd), unsigned(m.count));
  const auto ext = m.gext(true);
  double *dcb = tan, *dwb = tan + nd * h.points, *dsum = red, *dsum2 = red + nd * h.chunks;
  double* prefix = nullptr;
  qs_gfac_fold<<<grid, WAVE * WPB, 0, st>>>(models, dirs, m.t, noise, ext, keep, work);
  TGP_TRY(m.template scan<ScanCong>(st, models, work, nd, true, &prefix));
  qs_gfac_emit<<<grid, WAVE * WPB, 0, st>>>(models, dirs, m.t, noise, ext, keep, prefix, dcb, dwb, dsum);
  qs_gsol<<<grid, WAVE * WPB, 0, st>>>(models, dirs, m.t, cbuf, wbuf, dcb, dwb, resid, ext, keep, nullptr, work,
                                       nullptr);
  TGP_TRY(m.template scan<ScanAffine>(st, models, work, nd, true, &prefix));
  qs_gsol<<<grid, WAVE * WPB, 0, st>>>(models, dirs, m.t, cbuf, wbuf, dcb, dwb, resid, ext, keep, prefix, nullptr,
                                       dsum2);
  // block b nd + d: (member b, direction d)'s two sums
  qs_finish<<<unsigned(m.count * nd), WAVE, 0, st>>>(dsum, dsum2, nullptr, res, nullptr, m.sums(nd), 2);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// The noise gradient 1/2 (alpha^2 - diag K^-1) of the members from their factors and alpha: the variance half of
// qs_pred_fold from the end, the prediction's scan, qs_invdiag_emit.  In the primal work space.
template <class M>
int launch_invdiag(const M& m, hipStream_t st, const QModel* models, const double* cbuf, const double* wbuf,
                   const double* alpha, double* work, double* out) {
  const dim3 grid(unsigned(blocks_for(m.chunks())), unsigned(m.count));
  const auto ext = m.gext(false);
  qs_pred_fold<<<grid, WAVE * WPB, 0, st>>>(1, 0, 1, models, m.t, cbuf, wbuf, nullptr, ext, work);
  double* prefix = nullptr;
  TGP_TRY(m.template scan<ScanPred>(st, models, work, 1, false, &prefix));
  qs_invdiag_emit<<<grid, WAVE * WPB, 0, st>>>(models, m.t, cbuf, wbuf, alpha, ext, prefix, out);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// keep: optional device buffer (nchunks x WAVE) that receives the chunks' incoming filtered covariances
int factor(tgp_qsep* q, const double* noise_host, double* keep = nullptr) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, nc = q->nchunks;
  TGP_ARG_CHECK(noise_host != nullptr, "null noise array");
  TGP_HIP_TRY(hipMemcpyAsync(q->noise, noise_host, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
  TGP_TRY(grow(&q->work, &q->work_elems, scan_work<ScanRiccati>(nc, 1)));
  double* prefix = nullptr;
  TGP_TRY(launch_factor(single(q), st, q->model, q->noise, q->work, q->c, q->w, q->red, q->bad, &prefix));
  if (keep)
    TGP_HIP_TRY(hipMemcpyAsync(keep, prefix, size_t(nc) * WAVE * sizeof(double), hipMemcpyDeviceToDevice, st));
  qs_finish<<<1, WAVE, 0, st>>>(q->red, nullptr, q->bad, q->red + 2 * nc, q->bad + nc, UniformSums{nc, 0, 0, 0}, 0);
  TGP_HIP_TRY(hipGetLastError());
  double sums[2];
  int64_t bad = 0;
  TGP_HIP_TRY(hipMemcpyAsync(sums, q->red + 2 * nc, sizeof(sums), hipMemcpyDeviceToHost, st));
  TGP_HIP_TRY(hipMemcpyAsync(&bad, q->bad + nc, sizeof(bad), hipMemcpyDeviceToHost, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  q->logdet = sums[0];
  q->info = bad == INT64_MAX ? 0 : int32_t(bad + 1);
  q->factored = true;
  return TGP_OK;
}

// out = op(y) for nrhs columns, y / out device buffers (N x nrhs, row-major); sumsq: optional sum of out^2;
// keep: optional device buffer (nchunks x ncg x WAVE) that receives the chunks' incoming states
int affine(tgp_qsep* q, int op, int64_t nrhs, const double* y, double* out, double* sumsq, double* keep = nullptr) {
  hipStream_t st = q->ctx->stream;
  const int64_t nc = q->nchunks, ncg = ceil_div(nrhs, 8);
  TGP_TRY(grow(&q->work, &q->work_elems, scan_work<ScanAffine>(nc, ncg)));
  double* prefix = nullptr;
  TGP_TRY(launch_affine(single(q), st, op, q->model, q->c, q->w, nrhs, y, q->work, out, sumsq ? q->red : nullptr,
                        &prefix));
  if (keep)
    TGP_HIP_TRY(hipMemcpyAsync(keep, prefix, size_t(nc * ncg) * WAVE * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (sumsq) {
    qs_finish<<<1, WAVE, 0, st>>>(q->red, nullptr, nullptr, q->red + 2 * nc * ncg, nullptr,
                                  UniformSums{nc * ncg, 0, 0, 0}, 0);
    TGP_HIP_TRY(hipMemcpyAsync(sumsq, q->red + 2 * nc * ncg, sizeof(double), hipMemcpyDeviceToHost, st));
  }
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

int host_affine(tgp_qsep* q, int op, int64_t nrhs, const void* y_host, void* out_host, double* sumsq) {
  TGP_ARG_CHECK(nrhs >= 1, "need at least one right-hand side (got %lld)", (long long)nrhs);
  TGP_ARG_CHECK(y_host && out_host, "null array");
  TGP_ARG_CHECK(q->factored, "the quasiseparable factor has not been computed (call tgp_qsep_factor first)");
  hipStream_t st = q->ctx->stream;
  const int64_t elems = q->n * nrhs;
  TGP_TRY(grow(&q->io, &q->io_elems, elems));
  TGP_TRY(grow(&q->io2, &q->io2_elems, elems));
  const int64_t nc_all = q->nchunks * ceil_div(nrhs, 8);
  TGP_TRY(grow(&q->red, &q->red_elems, 2 * nc_all + 2));
  TGP_HIP_TRY(hipMemcpyAsync(q->io, y_host, size_t(elems) * sizeof(double), hipMemcpyHostToDevice, st));
  TGP_TRY(affine(q, op, nrhs, q->io, q->io2, sumsq));
  TGP_HIP_TRY(hipMemcpyAsync(out_host, q->io2, size_t(elems) * sizeof(double), hipMemcpyDeviceToHost, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  return TGP_OK;
}

// Conditional mean and variance at m test points for each of nterms test-side vectors (gv, device, nterms x 8).
// `v_host`: the residual (alpha = K^-1 r is then computed by the two solves) or, with v_is_alpha, alpha itself; only
// read when the mean is wanted.  xtest_host == nullptr: the test points are the resident t (m == n); they are sorted,
// so their intervals need no sort and nothing goes through the host.
int predict(tgp_qsep* q, const double* v_host, int v_is_alpha, int64_t m, const double* xtest_host, int nterms,
            const double* gv, double* mean_host, double* var_host) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, nc = q->nchunks;
  const int want_mean = mean_host != nullptr, want_var = var_host != nullptr;
  // pred: xt (m) | pt (m x nterms x PT) | mean (nterms x m) | var (nterms x m);  pidx: idx (m) | sidx (m) | order (m)
  TGP_TRY(grow(&q->pred, &q->pred_elems, m * (1 + int64_t(nterms) * (PT + 2))));
  TGP_TRY(grow(&q->pidx, &q->pidx_elems, 3 * m));
  double *pt = q->pred + m, *mean = pt + m * nterms * PT, *var = mean + m * nterms;
  const double* xt = xtest_host ? q->pred : q->t;
  int64_t *idx = q->pidx, *sidx = idx + m, *order = sidx + m;
  const unsigned mblocks = unsigned((m + 255) / 256);
  if (xtest_host)
    TGP_HIP_TRY(hipMemcpyAsync(q->pred, xtest_host, size_t(m) * sizeof(double), hipMemcpyHostToDevice, st));
  qs_pred_locate<<<mblocks, 256, 0, st>>>(q->t, n, xt, m, idx);
  TGP_HIP_TRY(hipGetLastError());
  const size_t um = xtest_host ? size_t(m) : 0;
  std::vector<int64_t> h_idx(um), h_order(um), h_sidx(um);
  if (xtest_host)
    TGP_HIP_TRY(hipMemcpyAsync(h_idx.data(), idx, size_t(m) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  else
    qs_pred_identity<<<mblocks, 256, 0, st>>>(idx, m, sidx, order);
  const double* alpha = nullptr;
  if (want_mean) {  // alpha stays on the device, in io
    TGP_TRY(grow(&q->io, &q->io_elems, n));
    TGP_TRY(grow(&q->io2, &q->io2_elems, n));
    TGP_HIP_TRY(hipMemcpyAsync(q->io, v_host, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
    if (!v_is_alpha) {
      TGP_TRY(affine(q, TGP_QS_FWD, 1, q->io, q->io2, nullptr));
      TGP_TRY(affine(q, TGP_QS_BWD, 1, q->io2, q->io, nullptr));
    }
    alpha = q->io;
  }
  if (xtest_host) {
    TGP_HIP_TRY(hipStreamSynchronize(st));
    for (int64_t j = 0; j < m; ++j) h_order[size_t(j)] = j;
    std::stable_sort(h_order.begin(), h_order.end(),
                     [&](int64_t a, int64_t b) { return h_idx[size_t(a)] < h_idx[size_t(b)]; });
    for (int64_t j = 0; j < m; ++j) h_sidx[size_t(j)] = h_idx[size_t(h_order[size_t(j)])];
    TGP_HIP_TRY(hipMemcpyAsync(sidx, h_sidx.data(), size_t(m) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    TGP_HIP_TRY(hipMemcpyAsync(order, h_order.data(), size_t(m) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  }
  TGP_TRY(grow(&q->work, &q->work_elems, scan_work<ScanPred>(nc, 1)));
  for (int dir = 0; dir < 2; ++dir) {
    qs_pred_fold<<<blocks_for(nc), WAVE * WPB, 0, st>>>(dir, want_mean, want_var, q->model, q->t, q->c, q->w, alpha,
                                                        UniformGExtent{n, q->lc, nc, 0, 0, 0, 0}, q->work);
    double* prefix = nullptr;
    TGP_TRY(run_scan<ScanPred>(q->model, st, nc, 1, q->work, &prefix));
    qs_pred_emit<<<blocks_for(nc), WAVE * WPB, 0, st>>>(dir, want_mean, want_var, q->model, q->t, q->c, q->w, alpha,
                                                        UniformPExtent{n, q->lc, nc, m}, prefix, xt, sidx, order, gv,
                                                        nterms, pt, mean, var);
  }
  TGP_HIP_TRY(hipGetLastError());
  const size_t out_bytes = size_t(m) * size_t(nterms) * sizeof(double);
  if (want_mean) TGP_HIP_TRY(hipMemcpyAsync(mean_host, mean, out_bytes, hipMemcpyDeviceToHost, st));
  if (want_var) TGP_HIP_TRY(hipMemcpyAsync(var_host, var, out_bytes, hipMemcpyDeviceToHost, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  return TGP_OK;
}

// Directions are processed in passes of at most GRAD_MAX_BATCH (the grid's y extent) and of at most GRAD_SCRATCH_BYTES
// of dc, dw scratch (n (1 + J) doubles per direction), whatever the number of parameters.
constexpr int64_t GRAD_MAX_BATCH = 8;
constexpr int64_t GRAD_SCRATCH_BYTES = int64_t(1) << 30;
constexpr int64_t DIR_DOUBLES = sizeof(QDir) / sizeof(double);
static_assert(sizeof(QDir) % sizeof(double) == 0, "directions are laid out in a buffer of doubles");

// directions [d0, d0 + nd) of one model's host tangents (dleaves: ndir x nl x 4, dh: ndir x J, dPinf: ndir x J x J)
void pack_dirs(QDir* out, int64_t d0, int64_t nd, int64_t nl, int64_t J, const double* dleaves, const double* dh,
               const double* dPinf) {
  for (int64_t b = 0; b < nd; ++b) {
    QDir x{};
    const int64_t d = d0 + b;
    for (int64_t l = 0; l < nl; ++l)
      for (int p = 0; p < 4; ++p) x.dpar[l][p] = dleaves[(d * nl + l) * 4 + p];
    for (int64_t r = 0; r < J; ++r) {
      x.dh[r] = dh[d * J + r];
      for (int64_t c = 0; c < J; ++c) x.dP[r * QJ + c] = dPinf[(d * J + r) * J + c];
    }
    out[b] = x;
  }
}

// the derivative along one direction from its two sums; one function, so that single and batched calls round alike
__attribute__((noinline)) double grad_value(const double* sums) { return -0.5 * sums[0] - sums[1]; }

// After factor() and the forward solve of the residual (q->io: r, q->io2: z; gkeep: both scans' chunk prefixes):
// the derivative of the log-likelihood along each of ndir directions, -1/2 sum dc/c - sum z dz.
int grad_directions(tgp_qsep* q, int32_t ndir, const double* dleaves, const double* dh, const double* dPinf,
                    double* dout) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, nc = q->nchunks, J = q->J, nl = q->host_model.nleaves;
  const int64_t per_dir = n * (1 + J);
  TGP_ARG_CHECK(per_dir * int64_t(sizeof(double)) <= GRAD_SCRATCH_BYTES,
                "the gradient's scratch for one direction (n (1 + J) doubles) exceeds its cap of %lld bytes",
                (long long)GRAD_SCRATCH_BYTES);
  const int64_t batch =
      std::min<int64_t>({int64_t(ndir), GRAD_MAX_BATCH, GRAD_SCRATCH_BYTES / (per_dir * int64_t(sizeof(double)))});
  TGP_TRY(grow(&q->gdir, &q->gdir_elems, batch * DIR_DOUBLES));
  TGP_TRY(grow(&q->gtan, &q->gtan_elems, batch * per_dir));
  TGP_TRY(grow(&q->gred, &q->gred_elems, batch * (2 * nc + 2)));
  TGP_TRY(grow(&q->work, &q->work_elems, scan_work<ScanCong>(nc, batch)));
  const QDir* dirs = reinterpret_cast<const QDir*>(q->gdir);
  std::vector<QDir> hd(size_t(batch), QDir{});
  std::vector<double> sums(size_t(2 * batch));
  for (int64_t d0 = 0; d0 < ndir; d0 += batch) {
    const int64_t nb = std::min<int64_t>(batch, ndir - d0);
    pack_dirs(hd.data(), d0, nb, nl, J, dleaves, dh, dPinf);
    TGP_HIP_TRY(hipMemcpyAsync(q->gdir, hd.data(), size_t(nb) * sizeof(QDir), hipMemcpyHostToDevice, st));
    double* res = q->gred + 2 * nb * nc;
    TGP_TRY(launch_tangents(single(q), st, q->model, dirs, nb, q->noise, q->c, q->w, q->io, q->gkeep, q->work, q->gtan,
                            q->gred, res));
    // the host vectors are reused by the next batch: wait for this one
    TGP_HIP_TRY(hipMemcpyAsync(sums.data(), res, size_t(2 * nb) * sizeof(double), hipMemcpyDeviceToHost, st));
    TGP_HIP_TRY(hipStreamSynchronize(st));
    for (int64_t b = 0; b < nb; ++b) dout[d0 + b] = grad_value(&sums[size_t(2 * b)]);
  }
  return TGP_OK;
}

// alpha = K^-1 r (q->io2: z -> q->io) and, when wanted, 1/2 (alpha^2 - diag K^-1)
int grad_vectors(tgp_qsep* q, double* gnoise_host, double* alpha_host) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, nc = q->nchunks;
  TGP_TRY(affine(q, TGP_QS_BWD, 1, q->io2, q->io, nullptr));
  if (alpha_host)
    TGP_HIP_TRY(hipMemcpyAsync(alpha_host, q->io, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (gnoise_host) {
    TGP_TRY(grow(&q->gout, &q->gout_elems, n));
    TGP_TRY(grow(&q->work, &q->work_elems, scan_work<ScanPred>(nc, 1)));
    TGP_TRY(launch_invdiag(single(q), st, q->model, q->c, q->w, q->io, q->work, q->gout));
    TGP_HIP_TRY(hipMemcpyAsync(gnoise_host, q->gout, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  TGP_HIP_TRY(hipStreamSynchronize(st));
  return TGP_OK;
}

// the log-probability from sum z^2 and sum log c; one function, so that single and batched calls round alike
__attribute__((noinline)) double logprob_value(double zz, double logdet, int64_t n) {
  return -0.5 * zz - 0.5 * logdet - 0.5 * double(n) * kLog2Pi;
}

// what qs_finish leaves per member of a chain -- (sum log c, sum z^2, first bad pivot), the third an int64 in a double's
// slot -- as that member's info and value; one function, so that every kind of chain decodes alike
__attribute__((noinline)) void member_value(const double* got, int64_t n, int32_t* info, double* out) {
  int64_t first_bad;
  memcpy(&first_bad, &got[2], sizeof(first_bad));
  *info = first_bad == INT64_MAX ? 0 : int32_t(first_bad + 1);
  *out = *info ? NAN : logprob_value(got[1], got[0], n);
}

// ---- launch chains: many models over one series, or a set of series -----------------------------------------------------
// A launch chain evaluates up to BATCH_MAX_MEMBERS members in one sequence of launches with one synchronisation, in a
// buffer of at most BATCH_SCRATCH_BYTES: the value (log-probability) of each, its value and gradient, or (sets of series)
// its value and the conditional mean and variance at test points of its own.  Who the members
// are is a UniformMembers (models of a batch over the handle's series) or a TableMembers (series of a set); the sequence
// is written once (chain).  The buffer, in doubles, with the totals over the members it is carved for (Totals: N points,
// C chunks, W primal and T tangent scan work space, B members), P directions per member and D of them per pass:
//   fixed          BATCH_MAX_MEMBERS models | value and gradient: BATCH_MAX_MEMBERS x GRAD_MAX_BATCH directions (one pass's)
//   value          noise | residual (N each; n where a batch shares one) | c (N) | w (N J) | z (N) | scan work space (W) |
//                  per-chunk sums of log c | of z^2 | bad-pivot slots (C each) | results (3 B)
//   and gradient   both primal scans' chunk prefixes (2 x 64 C, before the work space) | results (2 P B) | with the
//                  vectors: alpha | noise gradient (N each) | dc, dw (D N (1 + J)) | tangent scan work space (T) |
//                  per-chunk tangent sums (2 D C)
//   and prediction (sets of series; M test points in the chain) with the mean: alpha (N) | the members' QTest table (3 B) |
//                  xt | sidx | order (M each) | pt (PT M) | with the mean: means (M) | with the variance: variances (M)
// W holds the largest of the scans that share it (Riccati and affine: 4 lane-blocks per element and level; with the
// vectors or a prediction the prediction's: 6), T the congruence scan's (3 per direction).
constexpr int64_t BATCH_MAX_MEMBERS = 64;
constexpr int64_t BATCH_SCRATCH_BYTES = int64_t(1) << 30;
static_assert(sizeof(QModel) % sizeof(double) == 0, "models are laid out in a buffer of doubles");
constexpr int64_t MODEL_DOUBLES = sizeof(QModel) / sizeof(double);
constexpr int64_t BATCH_BUDGET = BATCH_SCRATCH_BYTES / int64_t(sizeof(double));

// One call's host arrays from a chain's first member on, and what the call wants
struct ChainCall {
  bool grad;      // value and gradient (also with no direction and no vector: the prefixes are kept all the same)
  int64_t nl, J;
  int64_t P, D;   // directions per member, per pass
  const QModel* models;
  const double *noise, *resid;         // a batch's shared ones are on the device already
  const double *dleaves, *dh, *dPinf;  // P per member
  int32_t* info;
  double *out, *dout, *gnoise, *alpha;  // the last two may be null
  // value and prediction (sets of series): member b's test points are [test_offsets[b], test_offsets[b + 1]) - test_offsets[0]
  // of xtest, mean and var (either may be null); at_data[b] (the array may be null): they are its own data, xtest is not read
  const int64_t* test_offsets;
  const double* xtest;
  const int32_t* at_data;
  double *mean, *var;
  // value and posterior draws (sets of series): nrhs columns of standard normals, xi ((N + M) J x nrhs, member after
  // member, each [data; test points]) and eps (N x nrhs), and of draws at the data (N x nrhs) and at the test points
  // (M x nrhs; either may be null)
  int64_t nrhs;
  const double *xi, *eps;
  double *data, *test;
  bool vectors() const { return gnoise || alpha; }
  bool predicts() const { return test_offsets && (mean || var); }
  // how many test points its first k members hold, and whether alpha is made on the device
  int64_t tests(int64_t k) const { return test_offsets ? test_offsets[k] - test_offsets[0] : 0; }
  bool needs_alpha() const { return vectors() || (predicts() && mean); }

  // the same call from member b0 on, whose points start `at`, whose noise and residual noise_at and resid_at doubles in
  ChainCall from(int64_t b0, int64_t at, int64_t noise_at, int64_t resid_at) const {
    auto adv = [](auto* p, int64_t k) { return p ? p + k : p; };
    ChainCall c = *this;
    c.models += b0, c.noise += noise_at, c.resid += resid_at;
    c.dleaves = adv(dleaves, b0 * P * nl * 4), c.dh = adv(dh, b0 * P * J), c.dPinf = adv(dPinf, b0 * P * J * J);
    c.info += b0, c.out += b0, c.dout = adv(dout, b0 * P);
    c.gnoise = adv(gnoise, at), c.alpha = adv(alpha, at);
    const int64_t tests_at = tests(b0);
    c.test_offsets = adv(test_offsets, b0), c.at_data = adv(at_data, b0);
    c.xtest = adv(xtest, tests_at), c.mean = adv(mean, tests_at), c.var = adv(var, tests_at);
    c.xi = adv(xi, (at + tests_at) * J * nrhs), c.eps = adv(eps, at * nrhs);
    c.data = adv(data, at * nrhs), c.test = adv(test, tests_at * nrhs);
    return c;
  }
};

struct ChainArrays {
  QModel* models;
  QDir* dirs;
  double *noise, *resid, *c, *w, *z, *keep, *work, *logsum, *sumsq;
  int64_t* bad;
  double *res, *dres, *alpha, *gnoise, *tan, *twork, *tred;
  // prediction: the members' QTest table, then per test point of the chain xt | sidx | order | pt (PT) | mean | var
  QTest* tests;
  double *xt, *pt, *mean, *var;
  int64_t *sidx, *order;
  double* end;  // where a call that needs more goes on carving
};

// the chain's buffer, carved for the members it has room for
template <class M>
ChainArrays carve(const M& m, double* buf, const ChainCall& a) {
  const Totals r = m.room();
  const int64_t J = a.J, vec = a.vectors() ? r.points : 0;
  const bool pred = a.predicts();
  const int64_t mt = pred ? a.tests(r.members) : 0;  // a predicting chain's buffer is carved for the members it holds
  double* p = buf;
  auto take = [&](int64_t len) {
    double* got = p;
    p += len;
    return got;
  };
  ChainArrays A{};
  A.models = reinterpret_cast<QModel*>(take(BATCH_MAX_MEMBERS * MODEL_DOUBLES));
  A.dirs = reinterpret_cast<QDir*>(take(a.grad ? BATCH_MAX_MEMBERS * GRAD_MAX_BATCH * DIR_DOUBLES : 0));
  A.noise = take(m.own_noise() ? r.points : m.n_of(0));
  A.resid = take(m.own_resid() ? r.points : m.n_of(0));
  A.c = take(r.points), A.w = take(r.points * J), A.z = take(r.points);
  A.keep = take(a.grad ? 2 * r.chunks * WAVE : 0);
  A.work = take(r.work);
  A.logsum = take(r.chunks), A.sumsq = take(r.chunks), A.bad = reinterpret_cast<int64_t*>(take(r.chunks));
  A.res = take(3 * r.members), A.dres = take(2 * a.P * r.members);
  A.alpha = take(a.needs_alpha() ? r.points : 0), A.gnoise = take(vec);
  A.tan = take(a.D * r.points * (1 + J)), A.twork = take(r.twork), A.tred = take(a.D * 2 * r.chunks);
  static_assert(sizeof(QTest) == 3 * sizeof(double), "a member's test points are three slots of the buffer");
  A.tests = reinterpret_cast<QTest*>(take(pred ? 3 * r.members : 0));
  A.xt = take(mt), A.sidx = reinterpret_cast<int64_t*>(take(mt)), A.order = reinterpret_cast<int64_t*>(take(mt));
  A.pt = take(mt * PT), A.mean = take(a.mean ? mt : 0), A.var = take(a.var ? mt : 0);
  A.end = p;
  return A;
}

// The value part of a chain: the members' models, noise and residual go up, then factor, forward solve and one qs_finish
// block per member, which leaves (sum log c, sum z^2, first bad pivot) at res[3 member], the third an int64 in a double's
// slot.  Value and gradient: each scan's chunk prefixes are set aside before the next scan writes there.
template <class M>
int chain_value(const M& m, hipStream_t st, const ChainArrays& A, const ChainCall& a) {
  const Totals h = m.held();
  TGP_HIP_TRY(hipMemcpyAsync(A.models, a.models, size_t(h.members) * sizeof(QModel), hipMemcpyHostToDevice, st));
  if (m.own_noise())
    TGP_HIP_TRY(hipMemcpyAsync(A.noise, a.noise, size_t(h.points) * sizeof(double), hipMemcpyHostToDevice, st));
  if (m.own_resid())
    TGP_HIP_TRY(hipMemcpyAsync(A.resid, a.resid, size_t(h.points) * sizeof(double), hipMemcpyHostToDevice, st));
  double* prefix = nullptr;
  TGP_TRY(launch_factor(m, st, A.models, A.noise, A.work, A.c, A.w, A.logsum, A.bad, &prefix));
  if (a.grad) m.template set_aside<ScanRiccati>(st, prefix, A.keep, 0);
  TGP_TRY(launch_affine(m, st, TGP_QS_FWD, A.models, A.c, A.w, 1, A.resid, A.work, A.z, A.sumsq, &prefix));
  if (a.grad) m.template set_aside<ScanAffine>(st, prefix, A.keep, 1);
  qs_finish<<<unsigned(h.members), WAVE, 0, st>>>(A.logsum, A.sumsq, A.bad, A.res,
                                                  reinterpret_cast<int64_t*>(A.res) + 2, m.sums(1), 3);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// What a predicting chain sends up besides the value's arrays; alive until the chain's synchronisation
struct TestUpload {
  std::vector<QTest> tests;
  std::vector<int64_t> order;
};

// The prediction part of a chain of series, after its value part and (with the mean) alpha: the members' QTest table and
// test points go up -- each member's sorted by value here (stable, NaN first: place_test_points' order), those at their
// own data not at all -- qs_pred_locate_table finds the intervals, then per direction qs_pred_fold, the prediction's scan
// and qs_pred_emit, as the single predict() runs them; means and variances come down with the chain's other results.
int chain_predict(const TableMembers& m, hipStream_t st, const ChainArrays& A, const ChainCall& a, TestUpload* up) {
  const int64_t nb = m.count, mt = a.tests(nb);
  const int want_mean = a.mean != nullptr, want_var = a.var != nullptr;
  up->tests.resize(size_t(nb));
  up->order.resize(size_t(mt));
  int64_t most = 0;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t at = a.tests(b), cnt = a.tests(b + 1) - at;
    const bool own = a.at_data && a.at_data[b];
    up->tests[size_t(b)] = {at, cnt, own};
    most = std::max(most, cnt);
    if (own || cnt == 0) continue;
    int64_t* o = up->order.data() + at;
    const double* x = a.xtest + at;
    for (int64_t j = 0; j < cnt; ++j) o[j] = j;
    std::stable_sort(o, o + cnt, [&](int64_t p, int64_t q) { return sort_key(x[p]) < sort_key(x[q]); });
  }
  TGP_HIP_TRY(hipMemcpyAsync(A.tests, up->tests.data(), size_t(nb) * sizeof(QTest), hipMemcpyHostToDevice, st));
  if (most == 0) return TGP_OK;
  for (int64_t b = 0; b < nb;) {  // one copy per run of members that brought test points
    if (up->tests[size_t(b)].own) { ++b; continue; }
    int64_t e = b;
    while (e < nb && !up->tests[size_t(e)].own) ++e;
    const int64_t at = a.tests(b), len = a.tests(e) - at;
    if (len > 0) {
      TGP_HIP_TRY(hipMemcpyAsync(A.xt + at, a.xtest + at, size_t(len) * sizeof(double), hipMemcpyHostToDevice, st));
      TGP_HIP_TRY(hipMemcpyAsync(A.order + at, up->order.data() + at, size_t(len) * sizeof(int64_t),
                                 hipMemcpyHostToDevice, st));
    }
    b = e;
  }
  qs_pred_locate_table<<<dim3(unsigned(ceil_div(most, 256)), unsigned(nb)), 256, 0, st>>>(m.tab, A.tests, m.t, A.xt,
                                                                                          A.order, A.sidx);
  const dim3 grid(unsigned(blocks_for(m.chunks())), unsigned(nb));
  const double* alpha = want_mean ? A.alpha : nullptr;
  const double* gv = reinterpret_cast<const double*>(A.models) + offsetof(QModel, h) / sizeof(double);
  for (int dir = 0; dir < 2; ++dir) {
    qs_pred_fold<<<grid, WAVE * WPB, 0, st>>>(dir, want_mean, want_var, A.models, m.t, A.c, A.w, alpha, m.gext(false),
                                              A.work);
    double* prefix = nullptr;
    TGP_TRY(m.template scan<ScanPred>(st, A.models, A.work, 1, false, &prefix));
    qs_pred_emit<<<grid, WAVE * WPB, 0, st>>>(dir, want_mean, want_var, A.models, m.t, A.c, A.w, alpha,
                                              TablePExtent{m.tab, A.tests}, prefix, A.xt, A.sidx, A.order, gv, 1, A.pt,
                                              A.mean, A.var);
  }
  TGP_HIP_TRY(hipGetLastError());
  if (want_mean) TGP_HIP_TRY(hipMemcpyAsync(a.mean, A.mean, size_t(mt) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (want_var) TGP_HIP_TRY(hipMemcpyAsync(a.var, A.var, size_t(mt) * sizeof(double), hipMemcpyDeviceToHost, st));
  return TGP_OK;
}

// batches of models over one series do not predict: no entry point sets their call's test points
int chain_predict(const UniformMembers&, hipStream_t, const ChainArrays&, const ChainCall&, TestUpload*) {
  return TGP_OK;
}

// One launch chain over the members m in `buf`: the value part; value and gradient: the direction passes, then, with
// the vectors, the backward solve and the noise gradient; value and prediction: the backward solve when the mean is
// wanted, then chain_predict; one stream synchronisation; the results decoded into the call's host arrays.  A failed
// member gets NaN for everything but its info: its c and w are not a factor of anything, and what ran on them is
// overwritten.
template <class M>
int chain(const M& m, hipStream_t st, double* buf, const ChainCall& a, int32_t* passes) {
  const ChainArrays A = carve(m, buf, a);
  const Totals h = m.held();
  const int64_t nb = h.members, J = a.J, P = a.P, D = a.D;
  TGP_TRY(chain_value(m, st, A, a));
  // direction passes: pass k's host directions (member-major) stay alive until the synchronisation below, its results
  // land after those of the passes before it (2 nb d0 doubles)
  std::vector<QDir> hd(size_t(nb * P));
  for (int64_t d0 = 0; d0 < P; d0 += D, ++*passes) {
    const int64_t nd = std::min<int64_t>(D, P - d0);
    QDir* h0 = hd.data() + nb * d0;
    for (int64_t b = 0; b < nb; ++b)
      pack_dirs(h0 + b * nd, d0, nd, a.nl, J, a.dleaves + b * P * a.nl * 4, a.dh + b * P * J, a.dPinf + b * P * J * J);
    TGP_HIP_TRY(hipMemcpyAsync(A.dirs, h0, size_t(nb * nd) * sizeof(QDir), hipMemcpyHostToDevice, st));
    TGP_TRY(launch_tangents(m, st, A.models, A.dirs, nd, A.noise, A.c, A.w, A.resid, A.keep, A.twork, A.tan, A.tred,
                            A.dres + 2 * nb * d0));
  }
  TestUpload up;
  if (a.needs_alpha()) {
    double* prefix = nullptr;
    TGP_TRY(launch_affine(m.own_rhs(), st, TGP_QS_BWD, A.models, A.c, A.w, 1, A.z, A.work, A.alpha, nullptr, &prefix));
  }
  if (a.predicts()) TGP_TRY(chain_predict(m, st, A, a, &up));
  if (a.vectors()) {
    if (a.alpha)
      TGP_HIP_TRY(hipMemcpyAsync(a.alpha, A.alpha, size_t(h.points) * sizeof(double), hipMemcpyDeviceToHost, st));
    if (a.gnoise) {
      TGP_TRY(launch_invdiag(m, st, A.models, A.c, A.w, A.alpha, A.work, A.gnoise));
      TGP_HIP_TRY(hipMemcpyAsync(a.gnoise, A.gnoise, size_t(h.points) * sizeof(double), hipMemcpyDeviceToHost, st));
    }
  }
  std::vector<double> got(size_t(3 * nb)), dgot(size_t(2 * nb * P));
  TGP_HIP_TRY(hipMemcpyAsync(got.data(), A.res, got.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (P > 0) TGP_HIP_TRY(hipMemcpyAsync(dgot.data(), A.dres, dgot.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t n = m.n_of(b), lo = m.off_of(b);
    member_value(&got[size_t(3 * b)], n, &a.info[b], &a.out[b]);
    const bool failed = a.info[b] != 0;
    for (int64_t d0 = 0; d0 < P; d0 += D) {
      const int64_t nd = std::min<int64_t>(D, P - d0);
      for (int64_t d = 0; d < nd; ++d)
        a.dout[b * P + d0 + d] = failed ? NAN : grad_value(&dgot[size_t(2 * (nb * d0 + b * nd + d))]);
    }
    for (int64_t i = 0; failed && i < n; ++i) {
      if (a.gnoise) a.gnoise[lo + i] = NAN;
      if (a.alpha) a.alpha[lo + i] = NAN;
    }
    for (int64_t j = a.tests(b); failed && j < a.tests(b + 1); ++j) {  // as predict_guard answers for the single call
      if (a.mean) a.mean[j] = NAN;
      if (a.var) a.var[j] = NAN;
    }
  }
  return TGP_OK;
}

// checks `nb` models' host arrays and packs them (leaves: nb x nleaves x 5, hvec: nb x J, Pinf: nb x J x J; one state map)
int pack_models(std::vector<QModel>* out, int64_t nb, const double* leaves, int32_t nleaves, const int32_t* state_map,
                int32_t J, const double* hvec, const double* Pinf) {
  out->assign(size_t(nb), QModel{});
  for (int64_t b = 0; b < nb; ++b)
    TGP_TRY(pack_model(&(*out)[size_t(b)], leaves + b * nleaves * 5, nleaves, state_map, J, hvec + b * J,
                       Pinf + b * J * J));
  return TGP_OK;
}

// ---- batches of models over the one series: how many members a chain holds --------------------------------------------
// Value: as many members as keep the buffer under the cap.  Per member, in doubles: noise, if its own (n) | residual, if
// its own (n) | c (n) | w (n J) | z (n) | scan work space (W) | per-chunk sums and bad-pivot slots (3 nchunks) | results (3).
struct BatchLayout {
  int64_t fixed, per_member, work;  // doubles
};

BatchLayout batch_layout(int64_t n, int64_t nc, int64_t J, bool own_noise, bool own_resid) {
  BatchLayout l;
  l.work = std::max(scan_work<ScanRiccati>(nc, 1), scan_work<ScanAffine>(nc, 1));
  l.fixed = BATCH_MAX_MEMBERS * MODEL_DOUBLES + (own_noise ? 0 : n) + (own_resid ? 0 : n);
  l.per_member = (own_noise ? n : 0) + (own_resid ? n : 0) + n * (2 + J) + l.work + 3 * nc + 3;
  return l;
}

// Value and gradient: with P directions per member and S the sum of the scan's level sizes, per member the above and
// both primal scans' chunk prefixes (2 x 64 nchunks) | results (2 P) | with the vectors: alpha (n) | noise gradient (n),
// the work space 384 S instead of 256 S; per member and direction of a pass dc, dw (n (1 + J)) | scan work space (192 S) |
// per-chunk sums (2 nchunks).  The split (grad_split): as many members as fit with one direction each, then as many
// directions per pass as the rest holds.  A function of (n, J, P, B, own or shared noise and residual, vectors or not)
// alone.
struct GradLayout {
  int64_t fixed, per_member, per_dir, work, twork;  // doubles; twork: the tangent scans' work space per direction
  int64_t members, dirs;                            // per chain, per pass; members == 0: one member does not fit
};

GradLayout grad_split(int64_t n, int64_t nc, int64_t J, int64_t P, int64_t B, bool own_noise, bool own_resid,
                      bool vectors) {
  GradLayout l;
  // the larger need of the scans that share it, as in batch_layout; the prediction scan joins them with the vectors
  l.work = std::max(scan_work<ScanRiccati>(nc, 1), scan_work<ScanAffine>(nc, 1));
  if (vectors) l.work = std::max(l.work, scan_work<ScanPred>(nc, 1));
  l.twork = scan_work<ScanCong>(nc, 1);
  l.fixed = BATCH_MAX_MEMBERS * (MODEL_DOUBLES + GRAD_MAX_BATCH * DIR_DOUBLES) + (own_noise ? 0 : n) + (own_resid ? 0 : n);
  l.per_member = (own_noise ? n : 0) + (own_resid ? n : 0) + n * (2 + J) + 2 * nc * WAVE + l.work + 3 * nc + 3 + 2 * P +
                 (vectors ? 2 * n : 0);
  l.per_dir = n * (1 + J) + l.twork + 2 * nc;
  const int64_t budget = BATCH_BUDGET - l.fixed;
  const int64_t one = l.per_member + (P > 0 ? l.per_dir : 0);
  l.members = budget < one ? 0 : std::min<int64_t>({B, BATCH_MAX_MEMBERS, budget / one});
  l.dirs = 0;
  if (l.members > 0 && P > 0)
    l.dirs = std::min<int64_t>({P, GRAD_MAX_BATCH, (budget - l.members * l.per_member) / (l.members * l.per_dir)});
  return l;
}

// The chains of one call on a batch: nb models in chains of m.cap members, in a buffer of `need` doubles that is carved
// once, for m.cap members, so that a shared noise or residual goes up once and stays where every chain looks for it.
int batch_chains(tgp_qsep* q, UniformMembers m, int64_t nb, int64_t need, const ChainCall& a, int32_t* nchains,
                 int32_t* npasses) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n;
  TGP_TRY(grow(&q->bat, &q->bat_elems, need));
  const ChainArrays A = carve(m, q->bat, a);
  if (!m.own_noise())
    TGP_HIP_TRY(hipMemcpyAsync(A.noise, a.noise, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
  if (!m.own_resid())
    TGP_HIP_TRY(hipMemcpyAsync(A.resid, a.resid, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
  int32_t chains = 0, passes = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += m.cap, ++chains) {
    m.count = std::min<int64_t>(m.cap, nb - b0);
    TGP_TRY(chain(m, st, q->bat, a.from(b0, b0 * n, b0 * m.noise_stride, b0 * m.y_stride), &passes));
  }
  if (nchains) *nchains = chains;
  if (npasses) *npasses = passes;
  return TGP_OK;
}

// ---- sets of series: which members a chain holds -------------------------------------------------------------------------
// Chains are filled in the order given (series_fill); a chain ends at BATCH_MAX_MEMBERS members or before the member
// whose need would take it past the cap less the fixed part.  With S4_b the sizes of series b's MAXLEV table levels
// summed (1 beyond its own depth), series b needs, in doubles,
//   value          need_b = N_b (4 + J) + 256 S4_b + 3 nchunks_b + 3
//   and gradient   member_b = need_b + 2 x 64 nchunks_b + 2 P, with the vectors + 2 N_b and 384 S4_b for 256 S4_b
//                  dir_b    = N_b (1 + J) + 192 S4_b + 2 nchunks_b per direction of a pass
// and value and gradient count sum (member_b + [P > 0] dir_b) against the cap; per chain,
// D = min(P, GRAD_MAX_BATCH, (cap - fixed - sum member_b) / sum dir_b).  A function of (N_0 .. N_{B-1}, J, P, vectors
// wanted or not) alone.
constexpr int64_t SERIES_BLOCKS = std::max(ScanRiccati::ESZ + ScanRiccati::PSZ, ScanAffine::ESZ + ScanAffine::PSZ);

int64_t series_levels(const QExtent& x) {
  int64_t s = 0;
  for (int l = 0; l < MAXLEV; ++l) s += x.lev[l];
  return s;
}
int64_t series_work(const QExtent& x, bool vectors) {
  const int64_t blocks = vectors ? std::max<int64_t>(SERIES_BLOCKS, ScanPred::ESZ + ScanPred::PSZ) : SERIES_BLOCKS;
  return series_levels(x) * blocks * WAVE;
}
int64_t series_twork(const QExtent& x) { return series_levels(x) * (ScanCong::ESZ + ScanCong::PSZ) * WAVE; }

int64_t series_need(const QExtent& x, int64_t J) { return x.n * (4 + J) + series_work(x, false) + 3 * x.nchunks + 3; }
int64_t series_grad_member(const QExtent& x, int64_t J, int64_t P, bool vectors) {
  return x.n * (4 + J) + 2 * x.nchunks * WAVE + series_work(x, vectors) + 3 * x.nchunks + 3 + 2 * P +
         (vectors ? 2 * x.n : 0);
}
int64_t series_grad_dir(const QExtent& x, int64_t J) { return x.n * (1 + J) + series_twork(x) + 2 * x.nchunks; }

constexpr int64_t SERIES_GRAD_FIXED = BATCH_MAX_MEMBERS * (MODEL_DOUBLES + GRAD_MAX_BATCH * DIR_DOUBLES);

// Cuts the set into chains for `cut` and makes the resident table say where each member lies in its chain.  member(x),
// dir(x): what series x needs by itself and per direction of a pass; fixed: the fixed part of the buffer; tangent_work(x):
// what its `twork` steps by (the tangent scans' work space per direction; posterior draws: per column group).
template <class Member, class Dir, class Twork = int64_t (*)(const QExtent&)>
int series_fill(tgp_qsep_series* s, const tgp_qsep_series::Cut& cut, int64_t fixed, Member member, Dir dir,
                Twork tangent_work = series_twork) {
  if (s->cut == cut) return TGP_OK;
  const int64_t budget = BATCH_BUDGET - fixed, P = cut.P;
  auto one = [&](const QExtent& x) { return member(x) + (P > 0 ? dir(x) : 0); };
  for (int64_t b = 0; b < s->nseries; ++b)
    TGP_ARG_CHECK(one(s->ext[size_t(b)]) <= budget,
                  "series %lld (n = %lld) needs %lld doubles of scratch and exceeds its cap of %lld bytes", (long long)b,
                  (long long)s->ext[size_t(b)].n, (long long)one(s->ext[size_t(b)]), (long long)BATCH_SCRATCH_BYTES);
  s->cut = {};
  s->chain0.assign(1, 0);
  s->chain_d.clear();
  int64_t used = 0, count = 0, largest = 0, mem = 0, dsum = 0, off = 0, work = 0, chunks = 0, twork = 0;
  auto close = [&]() {  // the chain that ends here: its directions per pass and its need
    const int64_t d = P > 0 ? std::min<int64_t>({P, GRAD_MAX_BATCH, (budget - mem) / dsum}) : 0;
    s->chain_d.push_back(d);
    largest = std::max(largest, mem + d * dsum);
  };
  for (int64_t b = 0; b < s->nseries; ++b) {
    QExtent& x = s->ext[size_t(b)];
    if (count == BATCH_MAX_MEMBERS || used + one(x) > budget) {
      close();
      s->chain0.push_back(b);
      used = count = mem = dsum = off = work = chunks = twork = 0;
    }
    x.off = off, x.work = work, x.chunks = chunks, x.keep = 2 * chunks * WAVE, x.twork = twork;
    off += x.n, work += series_work(x, cut.vectors != 0), chunks += x.nchunks, twork += tangent_work(x);
    mem += member(x), dsum += dir(x);
    used += one(x), ++count;
  }
  close();
  s->chain0.push_back(s->nseries);
  s->buf_need = fixed + largest;
  hipStream_t st = s->ctx->stream;
  TGP_HIP_TRY(hipMemcpyAsync(s->tab, s->ext.data(), s->ext.size() * sizeof(QExtent), hipMemcpyHostToDevice, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  s->cut = cut;
  return TGP_OK;
}

int series_split(tgp_qsep_series* s, int32_t J) {
  return series_fill(s, {1, J, 0, 0}, BATCH_MAX_MEMBERS * MODEL_DOUBLES,
                     [&](const QExtent& x) { return series_need(x, J); }, [](const QExtent&) { return int64_t(0); });
}

int series_grad_split(tgp_qsep_series* s, int32_t J, int32_t P, bool vectors) {
  return series_fill(s, {2, J, P, int32_t(vectors)}, SERIES_GRAD_FIXED,
                     [&](const QExtent& x) { return series_grad_member(x, J, P, vectors); },
                     [&](const QExtent& x) { return series_grad_dir(x, J); });
}

// Value and prediction: series b with M_b test points needs, in doubles, what the value takes with the prediction scan's
// work space (384 S4_b for 256 S4_b), its QTest entry (3), with the mean alpha (N_b), and per test point xt, sidx, order
// (1 each), pt (PT), with the mean its mean, with the variance its variance (1 each):
//   pred_b = N_b (4 + J) + 384 S4_b + 3 nchunks_b + 6 + [mean] N_b + M_b (3 + PT + [mean] + [var])
// A member at its own data counts its M_b = N_b like any other.  A function of (N_b, M_b, J, mean and variance wanted
// or not) alone; the chains are the value's fill over it.
int64_t series_predict_need(const QExtent& x, int64_t J, int64_t mt, bool want_mean, bool want_var) {
  return x.n * (4 + J) + series_work(x, true) + 3 * x.nchunks + 6 + (want_mean ? x.n : 0) +
         mt * (3 + PT + (want_mean ? 1 : 0) + (want_var ? 1 : 0));
}

int series_predict_split(tgp_qsep_series* s, int32_t J, bool want_mean, bool want_var, const int64_t* test_offsets) {
  tgp_qsep_series::Cut cut{3, J, 0, 1, int32_t(want_mean) + 2 * int32_t(want_var), {}};
  cut.tests.resize(size_t(s->nseries));
  for (int64_t b = 0; b < s->nseries; ++b) cut.tests[size_t(b)] = test_offsets[b + 1] - test_offsets[b];
  const QExtent* first = s->ext.data();  // series_fill hands the set's own extents over: x is series x - first
  auto need = [&](const QExtent& x) {
    return series_predict_need(x, J, cut.tests[size_t(&x - first)], want_mean, want_var);
  };
  return series_fill(s, cut, BATCH_MAX_MEMBERS * MODEL_DOUBLES, need, [](const QExtent&) { return int64_t(0); });
}

// members [b0, b0 + nb) of the set as the chain the resident table was cut for, with D directions per pass
TableMembers table_members(const tgp_qsep_series* s, int64_t b0, int64_t nb, int64_t D) {
  TableMembers m{s->t + s->offsets[size_t(b0)], s->tab + b0, &s->ext[size_t(b0)], nb};
  m.tot.members = nb;
  for (int64_t b = 0; b < nb; ++b) {
    const QExtent& x = m.mine[b];
    m.tot.points += x.n, m.tot.chunks += x.nchunks;
    m.tot.work += series_work(x, s->cut.vectors != 0), m.tot.twork += D * series_twork(x);
    for (int l = 0; l <= MAXLEV; ++l) m.top[l] = std::max(m.top[l], x.lev[l]);
  }
  while (m.top[m.depth - 1] > GROUP) ++m.depth;
  return m;
}

// the chains of one call on a set, after its split
int series_chains(tgp_qsep_series* s, const ChainCall& a, int32_t* nchains, int32_t* npasses) {
  TGP_TRY(grow(&s->buf, &s->buf_elems, s->buf_need));
  const size_t chains = s->chain0.size() - 1;
  int32_t passes = 0;
  for (size_t k = 0; k < chains; ++k) {
    const int64_t b0 = s->chain0[k], at = s->offsets[size_t(b0)];
    ChainCall c = a.from(b0, at, at, at);
    c.D = s->chain_d[k];
    TGP_TRY(chain(table_members(s, b0, s->chain0[k + 1] - b0, c.D), s->ctx->stream, s->buf, c, &passes));
  }
  if (nchains) *nchains = int32_t(chains);
  if (npasses) *npasses = passes;
  return TGP_OK;
}

// checks and the failed-factor answer shared by both prediction entry points; *done: nothing is left to compute
int predict_guard(tgp_qsep* q, const double* v_host, int64_t m, bool xtest_ok, int32_t nterms, double* mean_host,
                  double* var_host, bool* done) {
  *done = true;
  TGP_ARG_CHECK(q->factored, "the quasiseparable factor has not been computed (call tgp_qsep_factor first)");
  TGP_ARG_CHECK(m >= 0, "negative number of test points (%lld)", (long long)m);
  if (m == 0 || (!mean_host && !var_host)) return TGP_OK;
  TGP_ARG_CHECK(xtest_ok, "null test points");
  TGP_ARG_CHECK(!mean_host || v_host, "the mean needs the residual or alpha");
  if (q->info != 0) {  // failed factor: c and w are not a factor of anything
    for (int64_t j = 0; j < m * nterms; ++j) {
      if (mean_host) mean_host[j] = NAN;
      if (var_host) var_host[j] = NAN;
    }
    return TGP_OK;
  }
  *done = false;
  return TGP_OK;
}

// ---- posterior samples and the conditional mean of many columns ------------------------------------------------------
// Columns are served in passes of at most SAMPLE_MAX_COLS; a pass holds, in doubles per column, xi (G J, later z and
// alpha: J counts as at least 2 so that both fit), f (G) and eps, later v (G): G (max(J, 2) + 2) with G = n + m, and is
// made smaller until that and the scans' work space stay under SAMPLE_SCRATCH_BYTES.  A function of (n, m, J, nrhs).
constexpr int64_t SAMPLE_MAX_COLS = 64;
constexpr int64_t SAMPLE_SCRATCH_BYTES = int64_t(1) << 30;

int64_t sample_pass_doubles(int64_t G, int64_t nchunks, int64_t J, int64_t cols) {
  return G * (std::max<int64_t>(J, 2) + 2) * cols + scan_work<ScanAffine>(nchunks, ceil_div(cols, 8));
}

// columns per pass; 0: one column alone exceeds the cap
int64_t sample_pass_cols(int64_t G, int64_t nchunks, int64_t J, int64_t nrhs) {
  const int64_t cap = SAMPLE_SCRATCH_BYTES / int64_t(sizeof(double));
  int64_t cols = std::min(nrhs, SAMPLE_MAX_COLS);
  while (cols > 0 && sample_pass_doubles(G, nchunks, J, cols) > cap) cols -= cols > 8 ? (cols % 8 ? cols % 8 : 8) : 1;
  return cols;
}

// columns [c0, c0 + cols) of a host array of `rows` x nrhs to / from a device array of rows x cols
int copy_cols(hipStream_t st, bool up, double* dev, const double* host, int64_t rows, int64_t nrhs, int64_t c0,
              int64_t cols) {
  if (rows == 0 || cols == 0) return TGP_OK;
  const size_t hp = size_t(nrhs) * sizeof(double), dp = size_t(cols) * sizeof(double);
  if (cols == nrhs) {  // the whole array: one contiguous copy
    if (up)
      TGP_HIP_TRY(hipMemcpyAsync(dev, host, size_t(rows) * dp, hipMemcpyHostToDevice, st));
    else
      TGP_HIP_TRY(hipMemcpyAsync(const_cast<double*>(host), dev, size_t(rows) * dp, hipMemcpyDeviceToHost, st));
    return TGP_OK;
  }
  if (up)
    TGP_HIP_TRY(hipMemcpy2DAsync(dev, dp, host + c0, hp, dp, size_t(rows), hipMemcpyHostToDevice, st));
  else
    TGP_HIP_TRY(hipMemcpy2DAsync(const_cast<double*>(host) + c0, hp, dev, dp, dp, size_t(rows), hipMemcpyDeviceToHost,
                                 st));
  return TGP_OK;
}

// The test points of one call on the device: pred: xt (m) | gt (G, with a grid) | `extra` doubles for the caller;
// pidx: sidx (m) | order (m) | gp (G).
// They are sorted by value on the host (stable; NaN first), their intervals located on the device; with `grid` the
// merged grid of data and test points is built too.
struct TestPoints {
  double *xt = nullptr, *gt = nullptr;
  int64_t *sidx = nullptr, *order = nullptr, *gp = nullptr;
};

int place_test_points(tgp_qsep* q, int64_t m, const double* xtest_host, bool grid, int64_t extra, TestPoints* tp) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, G = n + m;
  TGP_TRY(grow(&q->pred, &q->pred_elems, m + (grid ? G : 0) + extra));
  TGP_TRY(grow(&q->pidx, &q->pidx_elems, 2 * m + (grid ? G : 0)));
  tp->xt = q->pred, tp->gt = grid ? q->pred + m : nullptr;
  tp->sidx = q->pidx, tp->order = q->pidx + m, tp->gp = grid ? q->pidx + 2 * m : nullptr;
  if (m == 0) return TGP_OK;
  std::vector<int64_t> h_order(static_cast<size_t>(m));
  for (int64_t j = 0; j < m; ++j) h_order[size_t(j)] = j;
  std::stable_sort(h_order.begin(), h_order.end(), [&](int64_t a, int64_t b) {
    return sort_key(xtest_host[a]) < sort_key(xtest_host[b]);
  });
  TGP_HIP_TRY(hipMemcpyAsync(tp->xt, xtest_host, size_t(m) * sizeof(double), hipMemcpyHostToDevice, st));
  TGP_HIP_TRY(hipMemcpyAsync(tp->order, h_order.data(), size_t(m) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));  // h_order leaves scope
  const UniformSExtent ext{n, q->lc, q->nchunks, m, 0, 0, 0};
  qs_smp_locate<<<unsigned((m + 255) / 256), 256, 0, st>>>(ext, q->t, tp->xt, tp->order, tp->sidx, tp->gt, tp->gp);
  if (grid) qs_smp_place<<<unsigned((n + 255) / 256), 256, 0, st>>>(ext, q->t, tp->xt, tp->order, tp->gt, tp->gp);
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

// out (m x cols) = (accumulate ? out : 0) + k(x, X) alpha for the cols columns of alpha (n x cols); q->work is grown
int cond_mean_cols(tgp_qsep* q, const double* alpha, int64_t cols, int64_t m, const TestPoints& tp, int accumulate,
                   double* out) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, nc = q->nchunks, ncg = ceil_div(cols, 8);
  TGP_TRY(grow(&q->work, &q->work_elems, scan_work<ScanAffine>(nc, ncg)));
  const unsigned blocks = unsigned(blocks_for(nc * ncg));
  const UniformSExtent ext{n, q->lc, nc, m, 0, 0, 0};
  for (int dir = 0; dir < 2; ++dir) {
    qs_cm_fold<<<blocks, WAVE * WPB, 0, st>>>(dir, q->model, q->t, alpha, ext, cols, ncg, q->work);
    double* prefix = nullptr;
    TGP_TRY(run_scan<ScanAffine>(q->model, st, nc, ncg, q->work, &prefix));
    qs_cm_emit<<<blocks, WAVE * WPB, 0, st>>>(dir, accumulate, q->model, q->t, alpha, ext, cols, ncg, prefix, tp.xt,
                                              tp.sidx, tp.order, out);
  }
  TGP_HIP_TRY(hipGetLastError());
  return TGP_OK;
}

void fill_nan(double* a, int64_t len) {
  for (int64_t j = 0; a && j < len; ++j) a[j] = NAN;
}

int sample(tgp_qsep* q, const double* resid_host, int64_t m, const double* xtest_host, int64_t nrhs,
           const double* xi_host, const double* eps_host, double* data_host, double* test_host, int32_t* npasses) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, J = q->J, G = n + m;
  const int64_t lcG = chunk_length(G), ncG = ceil_div(G, lcG);
  const int64_t pc = sample_pass_cols(G, std::max(ncG, q->nchunks), J, nrhs);
  TGP_ARG_CHECK(pc >= 1, "one column of samples at %lld points needs %lld doubles of scratch and exceeds its cap of %lld "
                "bytes", (long long)G, (long long)sample_pass_doubles(G, std::max(ncG, q->nchunks), J, 1),
                (long long)SAMPLE_SCRATCH_BYTES);
  for (int64_t j = 0; j < m; ++j)
    TGP_ARG_CHECK(std::isfinite(xtest_host[j]), "test point %lld is not finite: a sample is a recurrence over all points",
                  (long long)j);
  TestPoints tp;
  TGP_TRY(place_test_points(q, m, xtest_host, m > 0, n, &tp));
  double* resid = q->pred + m + (m > 0 ? G : 0);
  const double* gt = m > 0 ? tp.gt : q->t;
  TGP_HIP_TRY(hipMemcpyAsync(resid, resid_host, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
  const int64_t Jp = std::max<int64_t>(J, 2);
  TGP_TRY(grow(&q->smp, &q->smp_elems, G * (Jp + 2) * pc));
  TGP_TRY(grow(&q->work, &q->work_elems, scan_work<ScanAffine>(std::max(ncG, q->nchunks), ceil_div(pc, 8))));
  int32_t passes = 0;
  for (int64_t c0 = 0; c0 < nrhs; c0 += pc, ++passes) {
    const int64_t cols = std::min(pc, nrhs - c0), ncg = ceil_div(cols, 8);
    double *xi = q->smp, *f = xi + G * Jp * cols, *e = f + G * cols;  // z and alpha take xi's place once it is read
    double *z = xi, *alpha = xi + n * cols;
    TGP_TRY(copy_cols(st, true, xi, xi_host, G * J, nrhs, c0, cols));
    TGP_TRY(copy_cols(st, true, e, eps_host, n, nrhs, c0, cols));
    const unsigned blocks = unsigned(blocks_for(ncG * ncg)), eblocks = unsigned((n * cols + 255) / 256);
    const UniformSExtent ext{n, q->lc, q->nchunks, m, G, lcG, ncG};
    qs_prior<<<blocks, WAVE * WPB, 0, st>>>(0, q->model, gt, tp.gp, ext, xi, cols, ncg, nullptr, q->work, nullptr,
                                            nullptr);
    double* prefix = nullptr;
    TGP_TRY(run_scan<ScanAffine>(q->model, st, ncG, ncg, q->work, &prefix));
    qs_prior<<<blocks, WAVE * WPB, 0, st>>>(1, q->model, gt, tp.gp, ext, xi, cols, ncg, prefix, nullptr, f,
                                            f + n * cols);
    qs_smp_resid<<<eblocks, 256, 0, st>>>(resid, q->noise, f, e, n, cols);
    TGP_HIP_TRY(hipGetLastError());
    TGP_TRY(affine(q, TGP_QS_FWD, cols, e, z, nullptr));
    TGP_TRY(affine(q, TGP_QS_BWD, cols, z, alpha, nullptr));
    if (test_host && m > 0) {
      TGP_TRY(cond_mean_cols(q, alpha, cols, m, tp, 1, f + n * cols));
      TGP_TRY(copy_cols(st, false, f + n * cols, test_host, m, nrhs, c0, cols));
    }
    if (data_host) {
      qs_smp_data<<<eblocks, 256, 0, st>>>(q->noise, f, alpha, e, n, cols);
      TGP_HIP_TRY(hipGetLastError());
      TGP_TRY(copy_cols(st, false, e, data_host, n, nrhs, c0, cols));
    }
  }
  TGP_HIP_TRY(hipStreamSynchronize(st));
  if (npasses) *npasses = passes;
  return TGP_OK;
}

int predict_mean(tgp_qsep* q, int64_t nrhs, const double* v_host, int v_is_alpha, int64_t m, const double* xtest_host,
                 double* mean_host) {
  hipStream_t st = q->ctx->stream;
  const int64_t n = q->n, J = q->J;
  const int64_t pc = sample_pass_cols(n + m, q->nchunks, J, nrhs);
  TGP_ARG_CHECK(pc >= 1, "one column of the conditional mean at %lld points exceeds the scratch cap of %lld bytes",
                (long long)(n + m), (long long)SAMPLE_SCRATCH_BYTES);
  TestPoints tp;
  TGP_TRY(place_test_points(q, m, xtest_host, false, 0, &tp));
  TGP_TRY(grow(&q->smp, &q->smp_elems, (3 * n + m) * pc));
  for (int64_t c0 = 0; c0 < nrhs; c0 += pc) {
    const int64_t cols = std::min(pc, nrhs - c0);
    double *a = q->smp, *z = a + n * cols, *alpha = z + n * cols, *mean = alpha + n * cols;
    TGP_TRY(copy_cols(st, true, v_is_alpha ? alpha : a, v_host, n, nrhs, c0, cols));
    if (!v_is_alpha) {
      TGP_TRY(affine(q, TGP_QS_FWD, cols, a, z, nullptr));
      TGP_TRY(affine(q, TGP_QS_BWD, cols, z, alpha, nullptr));
    }
    TGP_TRY(cond_mean_cols(q, alpha, cols, m, tp, 0, mean));
    TGP_TRY(copy_cols(st, false, mean, mean_host, m, nrhs, c0, cols));
  }
  TGP_HIP_TRY(hipStreamSynchronize(st));
  return TGP_OK;
}

// ---- sets of series: value and posterior draws ------------------------------------------------------------------------------
// A chain draws for its members as sample() does for one series, every step one series per grid row: the value part, the
// members' merged grids (their test points sorted by value on the host, as place_test_points sorts them), then per pass of
// columns the prior scan over the grids, v, both solves, the conditional-mean scans and the data side.  After the value's
// arrays (carve) the chain's buffer holds, with N data and M test points in the chain, G = N + M, c columns per pass in
// g = ceil(c / 8) groups:
//   the grids' extent table (13 B) | xt | sidx | order (M each) | gt | gp (G each) |
//   xi (G max(J, 2) c; later z and alpha, N c each) | f at the data | eps, later v and the draws at the data (N c each) |
//   with the test side wanted: f at the test points, later the draws there (M c) | scan work space (g sum wk_b)
// Every array of a pass has member b's rows after member b - 1's and one pitch, so each goes up or comes down in one copy
// (copy_cols).  With S4 the sum of a series' MAXLEV table levels, of its data (S4_b) and of its grid (S4G_b), series b
// with M_b test points needs, in doubles,
//   fixed_b  = N_b (4 + J) + 256 S4_b + 3 nchunks_b + 3  (the value's)  + 13 + 3 M_b + 2 G_b
//   col_b(c) = c (G_b max(J, 2) + 2 N_b + [test side] M_b) + ceil(c / 8) wk_b,   wk_b = 192 max(S4_b, S4G_b)
// Chains are the value's fill over fixed_b + col_b(1); a chain's columns per pass are the most -- at most SAMPLE_MAX_COLS,
// stepping down as sample_pass_cols does -- with sum fixed_b + sum col_b(c) under the cap less the fixed part.  A function
// of (N_b, M_b, J, nrhs, which sides are wanted) alone.
constexpr int64_t EXT_DOUBLES = sizeof(QExtent) / sizeof(double);
static_assert(sizeof(QExtent) % sizeof(double) == 0, "the grids' extents are laid out in a buffer of doubles");

int64_t series_sample_work(const QExtent& x, const QExtent& g) {
  return std::max(series_levels(x), series_levels(g)) * (ScanAffine::ESZ + ScanAffine::PSZ) * WAVE;
}
int64_t series_sample_fixed(const QExtent& x, const QExtent& g, int64_t J) {
  return series_need(x, J) + EXT_DOUBLES + 3 * (g.n - x.n) + 2 * g.n;
}
int64_t series_sample_cols(const QExtent& x, const QExtent& g, int64_t J, bool want_test, int64_t cols) {
  return cols * (g.n * std::max<int64_t>(J, 2) + 2 * x.n + (want_test ? g.n - x.n : 0)) +
         ceil_div(cols, 8) * series_sample_work(x, g);
}

int series_sample_split(tgp_qsep_series* s, int32_t J, int64_t nrhs, bool want_data, bool want_test,
                        const int64_t* test_offsets) {
  tgp_qsep_series::Cut cut{4, J, 0, 0, int32_t(want_data) + 2 * int32_t(want_test), {}, nrhs};
  cut.tests.resize(size_t(s->nseries));
  for (int64_t b = 0; b < s->nseries; ++b) cut.tests[size_t(b)] = test_offsets[b + 1] - test_offsets[b];
  if (s->cut == cut) return TGP_OK;
  std::vector<QExtent> grid(size_t(s->nseries));
  for (int64_t b = 0; b < s->nseries; ++b) {
    grid[size_t(b)] = extent_of(s->ext[size_t(b)].n + cut.tests[size_t(b)]);
    TGP_ARG_CHECK(grid[size_t(b)].lev[MAXLEV - 1] <= GROUP, "the merged grid of series %lld (%lld points) needs more "
                  "than %d scan levels", (long long)b, (long long)grid[size_t(b)].n, MAXLEV);
  }
  const QExtent* first = s->ext.data();  // series_fill hands the set's own extents over: x is series x - first
  auto fixed = [&](const QExtent& x) { return series_sample_fixed(x, grid[size_t(&x - first)], J); };
  auto percol = [&](const QExtent& x, int64_t c) {
    return series_sample_cols(x, grid[size_t(&x - first)], J, want_test, c);
  };
  TGP_TRY(series_fill(
      s, cut, BATCH_MAX_MEMBERS * MODEL_DOUBLES, [&](const QExtent& x) { return fixed(x) + percol(x, 1); },
      [](const QExtent&) { return int64_t(0); },
      [&](const QExtent& x) { return series_sample_work(x, grid[size_t(&x - first)]); }));
  const int64_t budget = BATCH_BUDGET - BATCH_MAX_MEMBERS * MODEL_DOUBLES;
  int64_t largest = 0;
  for (size_t k = 0; k + 1 < s->chain0.size(); ++k) {
    auto need = [&](int64_t c) {
      int64_t sum = 0;
      for (int64_t b = s->chain0[k]; b < s->chain0[k + 1]; ++b) sum += fixed(s->ext[size_t(b)]) + percol(s->ext[size_t(b)], c);
      return sum;
    };
    int64_t cols = std::min(nrhs, SAMPLE_MAX_COLS);
    while (cols > 1 && need(cols) > budget) cols -= cols > 8 ? (cols % 8 ? cols % 8 : 8) : 1;
    s->chain_d[k] = cols;
    largest = std::max(largest, need(cols));
  }
  s->buf_need = BATCH_MAX_MEMBERS * MODEL_DOUBLES + largest;
  return TGP_OK;
}

// the series of a chain with nrhs right-hand sides each, as launch_affine takes its members
struct ColsMembers {
  const double* t;
  const QExtent* tab;
  int64_t count;
  const int64_t* top;
  int depth;
  int64_t nrhs, ncg;
  int64_t chunks() const { return top[0]; }
  TableColsExtent ext() const { return {tab, nrhs, ncg}; }
  template <class S>
  int scan(hipStream_t st, const QModel* models, double* work, int64_t width, bool, double** prefix) const {
    *prefix = work;
    return run_scan_table<S>(models, st, tab, count, top, depth, work, width);
  }
};

// One launch chain of value and draws over the members m in `buf`, pc columns per pass; one stream synchronisation.  A
// failed member gets NaN for everything but its info.
int chain_samples(const TableMembers& m, hipStream_t st, double* buf, const ChainCall& a, int64_t pc, int32_t* passes) {
  const ChainArrays A = carve(m, buf, a);
  const Totals h = m.held();
  const int64_t nb = h.members, N = h.points, J = a.J, Jp = std::max<int64_t>(J, 2), nrhs = a.nrhs;
  const int64_t Mt = a.tests(nb), Gt = N + Mt;
  TGP_TRY(chain_value(m, st, A, a));
  // the members' grids and their test points in sorted order; alive until the synchronisation
  std::vector<QExtent> grid(static_cast<size_t>(nb));
  std::vector<int64_t> order(static_cast<size_t>(Mt));
  int64_t gtop[MAXLEV + 1] = {}, most = 0, longest = 0, wsum = 0;
  for (int64_t b = 0; b < nb; ++b) {
    const QExtent& x = m.mine[b];
    const int64_t at = a.tests(b), cnt = a.tests(b + 1) - at;
    QExtent& g = grid[size_t(b)];
    g = extent_of(x.n + cnt);
    g.off = x.off + at, g.twork = x.twork;
    wsum += series_sample_work(x, g);
    for (int l = 0; l <= MAXLEV; ++l) gtop[l] = std::max(gtop[l], g.lev[l]);
    most = std::max(most, cnt), longest = std::max(longest, x.n);
    int64_t* o = order.data() + at;
    const double* xs = a.xtest + at;
    for (int64_t j = 0; j < cnt; ++j) o[j] = j;
    std::stable_sort(o, o + cnt, [&](int64_t p, int64_t q) { return sort_key(xs[p]) < sort_key(xs[q]); });
  }
  int gdepth = 1;
  while (gtop[gdepth - 1] > GROUP) ++gdepth;
  double* p = A.end;
  auto take = [&](int64_t len) {
    double* got = p;
    p += len;
    return got;
  };
  QExtent* gtab = reinterpret_cast<QExtent*>(take(nb * EXT_DOUBLES));
  double* xt = take(Mt);
  int64_t *sidx = reinterpret_cast<int64_t*>(take(Mt)), *ord = reinterpret_cast<int64_t*>(take(Mt));
  double* gt = take(Gt);
  int64_t* gp = reinterpret_cast<int64_t*>(take(Gt));
  double *xi = take(Gt * Jp * pc), *fdata = take(N * pc), *e = take(N * pc), *ftest = take(a.test ? Mt * pc : 0);
  double* work = take(ceil_div(pc, 8) * wsum);
  if (a.data || a.test) {
    const TableSExtent sext{m.tab, gtab};
    TGP_HIP_TRY(hipMemcpyAsync(gtab, grid.data(), size_t(nb) * sizeof(QExtent), hipMemcpyHostToDevice, st));
    if (Mt > 0) {
      TGP_HIP_TRY(hipMemcpyAsync(xt, a.xtest, size_t(Mt) * sizeof(double), hipMemcpyHostToDevice, st));
      TGP_HIP_TRY(hipMemcpyAsync(ord, order.data(), size_t(Mt) * sizeof(int64_t), hipMemcpyHostToDevice, st));
      qs_smp_locate<<<dim3(unsigned(ceil_div(most, 256)), unsigned(nb)), 256, 0, st>>>(sext, m.t, xt, ord, sidx, gt, gp);
    }
    qs_smp_place<<<dim3(unsigned(ceil_div(longest, 256)), unsigned(nb)), 256, 0, st>>>(sext, m.t, xt, ord, gt, gp);
    TGP_HIP_TRY(hipGetLastError());
    for (int64_t c0 = 0; c0 < nrhs; c0 += pc, ++*passes) {
      const int64_t cols = std::min(pc, nrhs - c0), ncg = ceil_div(cols, 8);
      double *z = xi, *alpha = xi + N * cols;  // take xi's place once it is read
      TGP_TRY(copy_cols(st, true, xi, a.xi, Gt * J, nrhs, c0, cols));
      TGP_TRY(copy_cols(st, true, e, a.eps, N, nrhs, c0, cols));
      const dim3 ggrid(unsigned(blocks_for(gtop[0] * ncg)), unsigned(nb));
      const dim3 dgrid(unsigned(blocks_for(m.chunks() * ncg)), unsigned(nb));
      const unsigned eblocks = unsigned(ceil_div(N * cols, 256));
      qs_prior<<<ggrid, WAVE * WPB, 0, st>>>(0, A.models, gt, gp, sext, xi, cols, ncg, nullptr, work, nullptr, nullptr);
      TGP_TRY(run_scan_table<ScanAffine>(A.models, st, gtab, nb, gtop, gdepth, work, ncg));
      qs_prior<<<ggrid, WAVE * WPB, 0, st>>>(1, A.models, gt, gp, sext, xi, cols, ncg, work, nullptr, fdata, ftest);
      qs_smp_resid<<<eblocks, 256, 0, st>>>(A.resid, A.noise, fdata, e, N, cols);
      TGP_HIP_TRY(hipGetLastError());
      const ColsMembers cm{m.t, m.tab, nb, m.top, m.depth, cols, ncg};
      double* prefix = nullptr;
      TGP_TRY(launch_affine(cm, st, TGP_QS_FWD, A.models, A.c, A.w, cols, e, work, z, nullptr, &prefix));
      TGP_TRY(launch_affine(cm, st, TGP_QS_BWD, A.models, A.c, A.w, cols, z, work, alpha, nullptr, &prefix));
      if (a.test && Mt > 0) {
        for (int dir = 0; dir < 2; ++dir) {
          qs_cm_fold<<<dgrid, WAVE * WPB, 0, st>>>(dir, A.models, m.t, alpha, sext, cols, ncg, work);
          TGP_TRY(run_scan_table<ScanAffine>(A.models, st, m.tab, nb, m.top, m.depth, work, ncg));
          qs_cm_emit<<<dgrid, WAVE * WPB, 0, st>>>(dir, 1, A.models, m.t, alpha, sext, cols, ncg, work, xt, sidx, ord,
                                                   ftest);
        }
        TGP_HIP_TRY(hipGetLastError());
        TGP_TRY(copy_cols(st, false, ftest, a.test, Mt, nrhs, c0, cols));
      }
      if (a.data) {
        qs_smp_data<<<eblocks, 256, 0, st>>>(A.noise, fdata, alpha, e, N, cols);
        TGP_HIP_TRY(hipGetLastError());
        TGP_TRY(copy_cols(st, false, e, a.data, N, nrhs, c0, cols));
      }
    }
  }
  std::vector<double> got(size_t(3 * nb));
  TGP_HIP_TRY(hipMemcpyAsync(got.data(), A.res, got.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  for (int64_t b = 0; b < nb; ++b) {
    member_value(&got[size_t(3 * b)], m.n_of(b), &a.info[b], &a.out[b]);
    if (a.info[b] == 0) continue;
    if (a.data) fill_nan(a.data + m.off_of(b) * nrhs, m.n_of(b) * nrhs);
    if (a.test) fill_nan(a.test + a.tests(b) * nrhs, (a.tests(b + 1) - a.tests(b)) * nrhs);
  }
  return TGP_OK;
}

#define QS_GUARD(q)                                                                 \
  TGP_ARG_CHECK((q) != nullptr && (q)->ctx != nullptr, "null quasiseparable handle"); \
  std::unique_lock<std::recursive_mutex> _tgp_lock((q)->ctx->mu);                     \
  TGP_HIP_TRY(hipSetDevice((q)->ctx->device))

// in the two constructors: a failed HIP call ends with `fail`, which destroys the half-built handle
#define Q_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) {                \
    set_error("%s failed: %s", #expr, hipGetErrorString(_e));                          \
    return fail(_e == hipErrorOutOfMemory ? TGP_E_NOMEM : TGP_E_HIP); } } while (0)

}  // namespace

extern "C" {

int tgp_qsep_create(tgp_ctx* ctx, int64_t n, const double* t_host, tgp_qsep** out) {
  TGP_ARG_CHECK(ctx != nullptr, "null context");
  std::unique_lock<std::recursive_mutex> lock(ctx->mu);
  TGP_HIP_TRY(hipSetDevice(ctx->device));
  TGP_ARG_CHECK(out != nullptr && t_host != nullptr, "null argument");
  TGP_ARG_CHECK(n >= 1, "need at least one data point (n = %lld)", (long long)n);
  tgp_qsep* q = new tgp_qsep();
  q->ctx = ctx;
  q->n = n;
  q->lc = chunk_length(n);
  q->nchunks = ceil_div(n, q->lc);
  auto fail = [&](int code) { tgp_qsep_destroy(q); return code; };
  Q_TRY(hipMalloc(&q->model, sizeof(QModel)));
  Q_TRY(hipMalloc(&q->t, size_t(n) * sizeof(double)));
  Q_TRY(hipMalloc(&q->noise, size_t(n) * sizeof(double)));
  Q_TRY(hipMalloc(&q->c, size_t(n) * sizeof(double)));
  Q_TRY(hipMalloc(&q->w, size_t(n) * QJ * sizeof(double)));
  Q_TRY(hipMalloc(&q->bad, size_t(q->nchunks + 1) * sizeof(int64_t)));
  Q_TRY(hipMalloc(&q->gvec, sizeof(q->host_g)));
  Q_TRY(hipMemcpyAsync(q->t, t_host, size_t(n) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  Q_TRY(hipStreamSynchronize(ctx->stream));
  if (int s = grow(&q->red, &q->red_elems, 2 * q->nchunks + 2); s < 0) return fail(s);
  *out = q;
  return TGP_OK;
}

int tgp_qsep_destroy(tgp_qsep* q) {
  if (!q) return TGP_OK;
  if (q->ctx) {
    hipSetDevice(q->ctx->device);
    hipStreamSynchronize(q->ctx->stream);
  }
  void* bufs[] = {q->model, q->t,    q->noise, q->c,     q->w,    q->io,   q->io2,  q->work, q->red,
                  q->bad,   q->pred, q->pidx,  q->gkeep, q->gdir, q->gtan, q->gred, q->gout, q->gvec,
                  q->bat,   q->smp};
  for (void* b : bufs)
    if (b) hipFree(b);
  delete q;
  return TGP_OK;
}

int tgp_qsep_factor(tgp_qsep* q, const double* leaves, int32_t nleaves, const int32_t* state_map, int32_t J,
                    const double* hvec, const double* Pinf, const double* noise_host, int32_t* info) {
  QS_GUARD(q);
  TGP_TRY(set_model(q, leaves, nleaves, state_map, J, hvec, Pinf));
  TGP_TRY(factor(q, noise_host));
  if (info) *info = q->info;
  return TGP_OK;
}

int tgp_qsep_factor_logprob(tgp_qsep* q, const double* leaves, int32_t nleaves, const int32_t* state_map,
                            int32_t J, const double* hvec, const double* Pinf, const double* noise_host,
                            const double* resid_host, int32_t* info, double* out) {
  QS_GUARD(q);
  TGP_ARG_CHECK(resid_host && out, "null argument");
  TGP_TRY(set_model(q, leaves, nleaves, state_map, J, hvec, Pinf));
  TGP_TRY(factor(q, noise_host));
  if (info) *info = q->info;
  TGP_TRY(grow(&q->io, &q->io_elems, q->n));
  TGP_TRY(grow(&q->io2, &q->io2_elems, q->n));
  hipStream_t st = q->ctx->stream;
  double zz = 0.0;
  TGP_HIP_TRY(hipMemcpyAsync(q->io, resid_host, size_t(q->n) * sizeof(double), hipMemcpyHostToDevice, st));
  TGP_TRY(affine(q, TGP_QS_FWD, 1, q->io, q->io2, &zz));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  *out = logprob_value(zz, q->logdet, q->n);
  return TGP_OK;
}

int tgp_qsep_grad(tgp_qsep* q, const double* leaves, int32_t nleaves, const int32_t* state_map, int32_t J,
                  const double* hvec, const double* Pinf, const double* noise_host, const double* resid_host,
                  int32_t ndir, const double* dleaves, const double* dh, const double* dPinf, int32_t* info,
                  double* out, double* dout, double* gnoise_host, double* alpha_host) {
  QS_GUARD(q);
  TGP_ARG_CHECK(resid_host && out, "null argument");
  TGP_ARG_CHECK(ndir >= 0, "negative number of directions (%d)", ndir);
  TGP_ARG_CHECK(ndir == 0 || (dleaves && dh && dPinf && dout), "null direction array");
  TGP_TRY(set_model(q, leaves, nleaves, state_map, J, hvec, Pinf));
  const int64_t n = q->n, nc = q->nchunks;
  TGP_TRY(grow(&q->gkeep, &q->gkeep_elems, 2 * nc * WAVE));
  TGP_TRY(factor(q, noise_host, q->gkeep));
  if (info) *info = q->info;
  TGP_TRY(grow(&q->io, &q->io_elems, n));
  TGP_TRY(grow(&q->io2, &q->io2_elems, n));
  hipStream_t st = q->ctx->stream;
  double zz = 0.0;
  TGP_HIP_TRY(hipMemcpyAsync(q->io, resid_host, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
  TGP_TRY(affine(q, TGP_QS_FWD, 1, q->io, q->io2, &zz, q->gkeep + nc * WAVE));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  *out = logprob_value(zz, q->logdet, n);
  if (q->info != 0) {  // failed factor: c and w are not a factor of anything
    for (int32_t d = 0; d < ndir; ++d) dout[d] = NAN;
    for (int64_t i = 0; i < n; ++i) {
      if (gnoise_host) gnoise_host[i] = NAN;
      if (alpha_host) alpha_host[i] = NAN;
    }
    return TGP_OK;
  }
  if (ndir > 0) TGP_TRY(grad_directions(q, ndir, dleaves, dh, dPinf, dout));
  if (gnoise_host || alpha_host) TGP_TRY(grad_vectors(q, gnoise_host, alpha_host));
  return TGP_OK;
}

int tgp_qsep_logprob_batch(tgp_qsep* q, int32_t nb, const double* leaves, int32_t nleaves, const int32_t* state_map,
                           int32_t J, const double* hvec, const double* Pinf, const double* noise_host,
                           int64_t noise_stride, const double* resid_host, int64_t resid_stride, int32_t* info,
                           double* out, int32_t* nchains) {
  QS_GUARD(q);
  TGP_ARG_CHECK(nb >= 0, "negative number of models (%d)", nb);
  if (nchains) *nchains = 0;
  if (nb == 0) return TGP_OK;
  const int64_t n = q->n, nc = q->nchunks;
  TGP_ARG_CHECK(leaves && state_map && hvec && Pinf, "null model array");
  TGP_ARG_CHECK(noise_host && resid_host && info && out, "null argument");
  TGP_ARG_CHECK(noise_stride == 0 || noise_stride == n, "the noise stride must be 0 (shared) or n (got %lld)",
                (long long)noise_stride);
  TGP_ARG_CHECK(resid_stride == 0 || resid_stride == n, "the residual stride must be 0 (shared) or n (got %lld)",
                (long long)resid_stride);
  std::vector<QModel> models;
  TGP_TRY(pack_models(&models, nb, leaves, nleaves, state_map, J, hvec, Pinf));
  const BatchLayout lay = batch_layout(n, nc, J, noise_stride != 0, resid_stride != 0);
  const int64_t budget = BATCH_BUDGET - lay.fixed;
  TGP_ARG_CHECK(budget >= lay.per_member,
                "the batch's scratch for one model (%lld doubles, %lld shared) exceeds its cap of %lld bytes",
                (long long)lay.per_member, (long long)lay.fixed, (long long)BATCH_SCRATCH_BYTES);
  const int64_t cap = std::min<int64_t>({int64_t(nb), BATCH_MAX_MEMBERS, budget / lay.per_member});
  const UniformMembers m{q->t, n, q->lc, nc, 0, cap, noise_stride, resid_stride, lay.work, 0};
  ChainCall a{};
  a.nl = nleaves, a.J = J, a.models = models.data(), a.noise = noise_host, a.resid = resid_host;
  a.info = info, a.out = out;
  return batch_chains(q, m, nb, lay.fixed + cap * lay.per_member, a, nchains, nullptr);
}

int tgp_qsep_grad_batch(tgp_qsep* q, int32_t nb, const double* leaves, int32_t nleaves, const int32_t* state_map,
                        int32_t J, const double* hvec, const double* Pinf, const double* noise_host,
                        int64_t noise_stride, const double* resid_host, int64_t resid_stride, int32_t ndir,
                        const double* dleaves, const double* dh, const double* dPinf, int32_t* info, double* out,
                        double* dout, double* gnoise_host, double* alpha_host, int32_t* nchains, int32_t* npasses) {
  QS_GUARD(q);
  TGP_ARG_CHECK(nb >= 0, "negative number of models (%d)", nb);
  TGP_ARG_CHECK(ndir >= 0, "negative number of directions (%d)", ndir);
  if (nchains) *nchains = 0;
  if (npasses) *npasses = 0;
  if (nb == 0) return TGP_OK;
  const int64_t n = q->n, nc = q->nchunks;
  TGP_ARG_CHECK(leaves && state_map && hvec && Pinf, "null model array");
  TGP_ARG_CHECK(noise_host && resid_host && info && out, "null argument");
  TGP_ARG_CHECK(ndir == 0 || (dleaves && dh && dPinf && dout), "null direction array");
  TGP_ARG_CHECK(noise_stride == 0 || noise_stride == n, "the noise stride must be 0 (shared) or n (got %lld)",
                (long long)noise_stride);
  TGP_ARG_CHECK(resid_stride == 0 || resid_stride == n, "the residual stride must be 0 (shared) or n (got %lld)",
                (long long)resid_stride);
  std::vector<QModel> models;
  TGP_TRY(pack_models(&models, nb, leaves, nleaves, state_map, J, hvec, Pinf));
  const bool vectors = gnoise_host || alpha_host;
  const GradLayout lay = grad_split(n, nc, J, ndir, nb, noise_stride != 0, resid_stride != 0, vectors);
  TGP_ARG_CHECK(lay.members > 0,
                "the gradient batch's scratch for one model and one direction (%lld + %lld doubles, %lld shared) "
                "exceeds its cap of %lld bytes",
                (long long)lay.per_member, (long long)lay.per_dir, (long long)lay.fixed,
                (long long)BATCH_SCRATCH_BYTES);
  const int64_t cap = lay.members, P = ndir;
  const UniformMembers m{q->t, n, q->lc, nc, 0, cap, noise_stride, resid_stride, lay.work, lay.dirs * lay.twork};
  ChainCall a{};
  a.grad = true, a.nl = nleaves, a.J = J, a.P = P, a.D = lay.dirs;
  a.models = models.data(), a.noise = noise_host, a.resid = resid_host;
  if (P > 0) a.dleaves = dleaves, a.dh = dh, a.dPinf = dPinf, a.dout = dout;
  a.info = info, a.out = out, a.gnoise = gnoise_host, a.alpha = alpha_host;
  return batch_chains(q, m, nb, lay.fixed + cap * (lay.per_member + lay.dirs * lay.per_dir), a, nchains, npasses);
}

int tgp_qsep_series_create(tgp_ctx* ctx, int32_t nseries, const int64_t* offsets, const double* t_concat,
                           tgp_qsep_series** out) {
  TGP_ARG_CHECK(ctx != nullptr, "null context");
  std::unique_lock<std::recursive_mutex> lock(ctx->mu);
  TGP_HIP_TRY(hipSetDevice(ctx->device));
  TGP_ARG_CHECK(out != nullptr && offsets != nullptr && t_concat != nullptr, "null argument");
  TGP_ARG_CHECK(nseries >= 1, "need at least one series (nseries = %d)", nseries);
  TGP_ARG_CHECK(offsets[0] == 0, "the offsets start at 0 (got %lld)", (long long)offsets[0]);
  for (int32_t b = 0; b < nseries; ++b) {
    TGP_ARG_CHECK(offsets[b + 1] >= offsets[b], "the offsets must not decrease (series %d: %lld after %lld)", b,
                  (long long)offsets[b + 1], (long long)offsets[b]);
    TGP_ARG_CHECK(offsets[b + 1] > offsets[b], "series %d is empty: every series needs at least one data point", b);
  }
  std::vector<QExtent> ext(size_t(nseries), QExtent{});
  for (int32_t b = 0; b < nseries; ++b) {
    QExtent& x = ext[size_t(b)];
    x = extent_of(offsets[b + 1] - offsets[b]);
    TGP_ARG_CHECK(x.lev[MAXLEV - 1] <= GROUP, "series %d (n = %lld) needs more than %d scan levels", b,
                  (long long)x.n, MAXLEV);
  }
  tgp_qsep_series* s = new tgp_qsep_series();
  s->ctx = ctx;
  s->nseries = nseries;
  s->offsets.assign(offsets, offsets + nseries + 1);
  s->ext = std::move(ext);
  auto fail = [&](int code) { tgp_qsep_series_destroy(s); return code; };
  const size_t total = size_t(offsets[nseries]);
  Q_TRY(hipMalloc(&s->t, total * sizeof(double)));
  Q_TRY(hipMalloc(&s->tab, size_t(nseries) * sizeof(QExtent)));
  Q_TRY(hipMemcpyAsync(s->t, t_concat, total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  Q_TRY(hipStreamSynchronize(ctx->stream));
  *out = s;
  return TGP_OK;
}

int tgp_qsep_series_destroy(tgp_qsep_series* s) {
  if (!s) return TGP_OK;
  if (s->ctx) {
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
  }
  void* bufs[] = {s->t, s->tab, s->buf};
  for (void* b : bufs)
    if (b) hipFree(b);
  delete s;
  return TGP_OK;
}

int tgp_qsep_series_logprob(tgp_qsep_series* s, const double* leaves, int32_t nleaves, const int32_t* state_map,
                            int32_t J, const double* hvec, const double* Pinf, const double* noise_concat,
                            const double* resid_concat, int32_t* info, double* out, int32_t* nchains) {
  QS_GUARD(s);
  if (nchains) *nchains = 0;
  TGP_ARG_CHECK(leaves && state_map && hvec && Pinf, "null model array");
  TGP_ARG_CHECK(noise_concat && resid_concat && info && out, "null argument");
  std::vector<QModel> models;
  TGP_TRY(pack_models(&models, s->nseries, leaves, nleaves, state_map, J, hvec, Pinf));
  TGP_TRY(series_split(s, J));
  ChainCall a{};
  a.nl = nleaves, a.J = J, a.models = models.data(), a.noise = noise_concat, a.resid = resid_concat;
  a.info = info, a.out = out;
  return series_chains(s, a, nchains, nullptr);
}

int tgp_qsep_series_grad(tgp_qsep_series* s, const double* leaves, int32_t nleaves, const int32_t* state_map,
                         int32_t J, const double* hvec, const double* Pinf, const double* noise_concat,
                         const double* resid_concat, int32_t ndir, const double* dleaves, const double* dh,
                         const double* dPinf, int32_t* info, double* out, double* dout, double* gnoise_concat,
                         double* alpha_concat, int32_t* nchains, int32_t* npasses) {
  QS_GUARD(s);
  if (nchains) *nchains = 0;
  if (npasses) *npasses = 0;
  TGP_ARG_CHECK(ndir >= 0, "negative number of directions (%d)", ndir);
  TGP_ARG_CHECK(leaves && state_map && hvec && Pinf, "null model array");
  TGP_ARG_CHECK(noise_concat && resid_concat && info && out, "null argument");
  TGP_ARG_CHECK(ndir == 0 || (dleaves && dh && dPinf && dout), "null direction array");
  std::vector<QModel> models;
  TGP_TRY(pack_models(&models, s->nseries, leaves, nleaves, state_map, J, hvec, Pinf));
  TGP_TRY(series_grad_split(s, J, ndir, gnoise_concat || alpha_concat));
  ChainCall a{};
  a.grad = true, a.nl = nleaves, a.J = J, a.P = ndir;  // D: each chain's own
  a.models = models.data(), a.noise = noise_concat, a.resid = resid_concat;
  a.dleaves = dleaves, a.dh = dh, a.dPinf = dPinf, a.dout = dout;
  a.info = info, a.out = out, a.gnoise = gnoise_concat, a.alpha = alpha_concat;
  return series_chains(s, a, nchains, npasses);
}

int tgp_qsep_series_predict(tgp_qsep_series* s, const double* leaves, int32_t nleaves, const int32_t* state_map,
                            int32_t J, const double* hvec, const double* Pinf, const double* noise_concat,
                            const double* resid_concat, const int64_t* test_offsets, const double* xtest_concat,
                            const int32_t* at_data, int32_t* info, double* out, double* mean_concat,
                            double* var_concat, int32_t* nchains) {
  QS_GUARD(s);
  if (nchains) *nchains = 0;
  TGP_ARG_CHECK(leaves && state_map && hvec && Pinf, "null model array");
  TGP_ARG_CHECK(noise_concat && resid_concat && info && out, "null argument");
  TGP_ARG_CHECK(test_offsets != nullptr, "null test offsets");
  TGP_ARG_CHECK(test_offsets[0] == 0, "the test offsets start at 0 (got %lld)", (long long)test_offsets[0]);
  for (int64_t b = 0; b < s->nseries; ++b) {
    const int64_t cnt = test_offsets[b + 1] - test_offsets[b], n = s->ext[size_t(b)].n;
    TGP_ARG_CHECK(cnt >= 0, "the test offsets must not decrease (series %lld: %lld after %lld)", (long long)b,
                  (long long)test_offsets[b + 1], (long long)test_offsets[b]);
    const bool own = at_data && at_data[b];
    TGP_ARG_CHECK(!own || cnt == n, "series %lld predicts at its own %lld data points: its count of test points must "
                  "be that (got %lld)", (long long)b, (long long)n, (long long)cnt);
    TGP_ARG_CHECK(own || cnt == 0 || xtest_concat, "null test points (series %lld brings %lld)", (long long)b,
                  (long long)cnt);
  }
  std::vector<QModel> models;
  TGP_TRY(pack_models(&models, s->nseries, leaves, nleaves, state_map, J, hvec, Pinf));
  TGP_TRY(series_predict_split(s, J, mean_concat != nullptr, var_concat != nullptr, test_offsets));
  ChainCall a{};
  a.nl = nleaves, a.J = J, a.models = models.data(), a.noise = noise_concat, a.resid = resid_concat;
  a.info = info, a.out = out;
  a.test_offsets = test_offsets, a.xtest = xtest_concat, a.at_data = at_data, a.mean = mean_concat, a.var = var_concat;
  return series_chains(s, a, nchains, nullptr);
}

int tgp_qsep_series_sample(tgp_qsep_series* s, const double* leaves, int32_t nleaves, const int32_t* state_map,
                           int32_t J, const double* hvec, const double* Pinf, const double* noise_concat,
                           const double* resid_concat, const int64_t* test_offsets, const double* xtest_concat,
                           const int32_t* at_data, int64_t nrhs, const double* xi_concat, const double* eps_concat,
                           int32_t* info, double* out, double* data_concat, double* test_concat, int32_t* nchains,
                           int32_t* npasses) {
  QS_GUARD(s);
  if (nchains) *nchains = 0;
  if (npasses) *npasses = 0;
  TGP_ARG_CHECK(leaves && state_map && hvec && Pinf, "null model array");
  TGP_ARG_CHECK(noise_concat && resid_concat && info && out, "null argument");
  TGP_ARG_CHECK(nrhs >= 1, "need at least one column of draws (got %lld)", (long long)nrhs);
  TGP_ARG_CHECK(test_offsets != nullptr, "null test offsets");
  TGP_ARG_CHECK(test_offsets[0] == 0, "the test offsets start at 0 (got %lld)", (long long)test_offsets[0]);
  const bool draws = data_concat || test_concat;
  TGP_ARG_CHECK(!draws || (xi_concat && eps_concat), "null standard normals");
  for (int64_t b = 0; b < s->nseries; ++b) {
    const int64_t lo = test_offsets[b], cnt = test_offsets[b + 1] - lo;
    TGP_ARG_CHECK(cnt >= 0, "the test offsets must not decrease (series %lld: %lld after %lld)", (long long)b,
                  (long long)test_offsets[b + 1], (long long)lo);
    TGP_ARG_CHECK(!(at_data && at_data[b]) || cnt == 0, "series %lld draws at its own data, which the data side "
                  "returns: its count of test points must be 0 (got %lld)", (long long)b, (long long)cnt);
    TGP_ARG_CHECK(cnt == 0 || xtest_concat, "null test points (series %lld brings %lld)", (long long)b, (long long)cnt);
    for (int64_t j = 0; j < cnt; ++j)
      TGP_ARG_CHECK(std::isfinite(xtest_concat[lo + j]), "test point %lld of series %lld is not finite: a sample is a "
                    "recurrence over all points", (long long)j, (long long)b);
  }
  std::vector<QModel> models;
  TGP_TRY(pack_models(&models, s->nseries, leaves, nleaves, state_map, J, hvec, Pinf));
  TGP_TRY(series_sample_split(s, J, nrhs, data_concat != nullptr, test_concat != nullptr, test_offsets));
  ChainCall a{};
  a.nl = nleaves, a.J = J, a.models = models.data(), a.noise = noise_concat, a.resid = resid_concat;
  a.info = info, a.out = out;
  a.test_offsets = test_offsets, a.xtest = xtest_concat;
  a.nrhs = nrhs, a.xi = xi_concat, a.eps = eps_concat, a.data = data_concat, a.test = test_concat;
  TGP_TRY(grow(&s->buf, &s->buf_elems, s->buf_need));
  const size_t chains = s->chain0.size() - 1;
  int32_t passes = 0;
  for (size_t k = 0; k < chains; ++k) {
    const int64_t b0 = s->chain0[k], at = s->offsets[size_t(b0)];
    TGP_TRY(chain_samples(table_members(s, b0, s->chain0[k + 1] - b0, 0), s->ctx->stream, s->buf, a.from(b0, at, at, at),
                          s->chain_d[k], &passes));
  }
  if (nchains) *nchains = int32_t(chains);
  if (npasses) *npasses = passes;
  return TGP_OK;
}

int tgp_qsep_normalization(tgp_qsep* q, double* out) {
  QS_GUARD(q);
  TGP_ARG_CHECK(out != nullptr, "null argument");
  TGP_ARG_CHECK(q->factored, "the quasiseparable factor has not been computed (call tgp_qsep_factor first)");
  *out = 0.5 * q->logdet + 0.5 * double(q->n) * kLog2Pi;
  return TGP_OK;
}

int tgp_qsep_solve_tri(tgp_qsep* q, int transpose, int64_t nrhs, const double* y_host, double* out_host) {
  QS_GUARD(q);
  return host_affine(q, transpose ? TGP_QS_BWD : TGP_QS_FWD, nrhs, y_host, out_host, nullptr);
}

int tgp_qsep_dot_tri(tgp_qsep* q, int64_t nrhs, const double* y_host, double* out_host) {
  QS_GUARD(q);
  return host_affine(q, TGP_QS_DOT, nrhs, y_host, out_host, nullptr);
}

int tgp_qsep_factor_data(tgp_qsep* q, double* c_host, double* w_host) {
  QS_GUARD(q);
  TGP_ARG_CHECK(q->factored, "the quasiseparable factor has not been computed (call tgp_qsep_factor first)");
  hipStream_t st = q->ctx->stream;
  if (c_host) TGP_HIP_TRY(hipMemcpyAsync(c_host, q->c, size_t(q->n) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (w_host)
    TGP_HIP_TRY(hipMemcpyAsync(w_host, q->w, size_t(q->n) * q->J * sizeof(double), hipMemcpyDeviceToHost, st));
  TGP_HIP_TRY(hipStreamSynchronize(st));
  return TGP_OK;
}

int tgp_qsep_predict(tgp_qsep* q, const double* v_host, int32_t v_is_alpha, int64_t m, const double* xtest_host,
                     double* mean_host, double* var_host) {
  QS_GUARD(q);
  bool done;
  TGP_TRY(predict_guard(q, v_host, m, xtest_host != nullptr, 1, mean_host, var_host, &done));
  if (done) return TGP_OK;
  // one term, g = h: the model's own (zero-padded) h on the device
  return predict(q, v_host, v_is_alpha, m, xtest_host, 1, q->model->h, mean_host, var_host);
}

int tgp_qsep_predict_terms(tgp_qsep* q, const double* v_host, int32_t v_is_alpha, int64_t m,
                           const double* xtest_host, int32_t nterms, const double* g_host, double* mean_host,
                           double* var_host) {
  QS_GUARD(q);
  TGP_ARG_CHECK(nterms >= 1 && nterms <= QJ, "one call predicts 1..%d terms (got %d)", QJ, nterms);
  TGP_ARG_CHECK(g_host != nullptr, "null term vectors");
  TGP_ARG_CHECK(xtest_host || m == q->n, "without test points the prediction is at the %lld data points (m = %lld)",
                (long long)q->n, (long long)m);
  bool done;
  TGP_TRY(predict_guard(q, v_host, m, true, nterms, mean_host, var_host, &done));
  if (done) return TGP_OK;
  const int J = q->J;
  std::fill(q->host_g, q->host_g + QJ * QJ, 0.0);
  for (int k = 0; k < nterms; ++k)
    for (int j = 0; j < J; ++j) q->host_g[k * QJ + j] = g_host[k * J + j];
  TGP_HIP_TRY(hipMemcpyAsync(q->gvec, q->host_g, sizeof(q->host_g), hipMemcpyHostToDevice, q->ctx->stream));
  return predict(q, v_host, v_is_alpha, m, xtest_host, nterms, q->gvec, mean_host, var_host);
}

int tgp_qsep_sample(tgp_qsep* q, const double* resid_host, int64_t m, const double* xtest_host, int64_t nrhs,
                    const double* xi_host, const double* eps_host, double* data_host, double* test_host,
                    int32_t* npasses) {
  QS_GUARD(q);
  TGP_ARG_CHECK(q->factored, "the quasiseparable factor has not been computed (call tgp_qsep_factor first)");
  TGP_ARG_CHECK(m >= 0 && nrhs >= 0, "negative number of test points or columns (%lld, %lld)", (long long)m,
                (long long)nrhs);
  if (npasses) *npasses = 0;
  if (nrhs == 0 || (!data_host && (!test_host || m == 0))) return TGP_OK;
  TGP_ARG_CHECK(m == 0 || xtest_host, "null test points");
  TGP_ARG_CHECK(resid_host && xi_host && eps_host, "null array");
  if (q->info != 0) {  // failed factor: c and w are not a factor of anything
    fill_nan(data_host, q->n * nrhs);
    fill_nan(test_host, m * nrhs);
    return TGP_OK;
  }
  return sample(q, resid_host, m, xtest_host, nrhs, xi_host, eps_host, data_host, test_host, npasses);
}

int tgp_qsep_predict_mean(tgp_qsep* q, int64_t nrhs, const double* v_host, int32_t v_is_alpha, int64_t m,
                          const double* xtest_host, double* mean_host) {
  QS_GUARD(q);
  TGP_ARG_CHECK(q->factored, "the quasiseparable factor has not been computed (call tgp_qsep_factor first)");
  TGP_ARG_CHECK(m >= 0 && nrhs >= 0, "negative number of test points or columns (%lld, %lld)", (long long)m,
                (long long)nrhs);
  if (nrhs == 0 || m == 0) return TGP_OK;
  TGP_ARG_CHECK(v_host && xtest_host && mean_host, "null array");
  if (q->info != 0) {
    fill_nan(mean_host, m * nrhs);
    return TGP_OK;
  }
  return predict_mean(q, nrhs, v_host, v_is_alpha, m, xtest_host, mean_host);
}

}  // extern "C"
