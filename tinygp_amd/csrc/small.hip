// small.hip -- batches of SMALL dense problems, one workgroup each (tgp_small_logprob).
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
struct SmallRow {
  int64_t x_off, noise_off, resid_off;
  int32_t n, d, prog, pad;
};
static_assert(sizeof(SmallRow) == 40 && sizeof(KProg) % 8 == 0, "the staging buffer is carved in 8-byte units");

__host__ __device__ constexpr int64_t small_lds_doubles(int64_t n) { return n * (n + 1) / 2 + n; }
static_assert(small_lds_doubles(TGP_SMALL_MAX_N) * 8 + 2 * SMALL_THREADS * 8 <= 163840,
              "a member at the cap, with the reduction scratch, fits the 160 KiB of one workgroup");

__device__ __forceinline__ int col_off(int j, int n) { return j * (n + 1) - j * (j - 1) / 2; }

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
  const double* x = X + row.x_off * d;
  const double* nz = noise + row.noise_off;
  const double* rs = resid + row.resid_off;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

  // 1 + 2: wave w assembles columns w, w + 4, ..; lane l their rows j + l, j + l + 64, ..; row n is the residual
  for (int j = wave; j < n; j += SMALL_WAVES) {
    double* col = A + col_off(j, n);
    for (int i = j + lane; i <= n; i += 64) {
      double v;
      if (i == n) {
        v = rs[j];
      } else {
        double r1, r2, r3;
        pair_dist<double, 2, 0>(x + int64_t(i) * d, x + int64_t(j) * d, d, r1, r2, r3);
        v = eval_kprog<double, 2>(kp, r1, r2, r3);
        if (i == j) v += nz[j];  // noise.py:77-78 fused, as in kmat_kernel
      }
      col[i - j] = v;
    }
  }
  __syncthreads();

  // 3 + 4: right-looking, column by column.  The pivot is read by every thread from the same LDS word: the decision to
  // leave is the workgroup's, no barrier sits under divergent control flow.
  int fail = 0;
  for (int p = 0; p < n; ++p) {
    double* cp = A + col_off(p, n);
    const double pivot = cp[0];
    if (!(pivot > 0.0)) {
      fail = p + 1;
      break;
    }
    // (the diagonal word keeps the pivot L_pp^2: a thread may still be reading it while the column is scaled)
    const double lpp = sqrt(pivot);
    for (int i = p + 1 + int(threadIdx.x); i <= n; i += SMALL_THREADS) cp[i - p] = cp[i - p] / lpp;
    __syncthreads();
    for (int j = p + 1 + wave; j < n; j += SMALL_WAVES) {
      double* col = A + col_off(j, n);
      const double ljp = cp[j - p];
      for (int i = j + lane; i <= n; i += 64) col[i - j] = __builtin_fma(-cp[i - p], ljp, col[i - j]);
    }
    __syncthreads();
  }

  // 5: sum log L_pp and sum z_p^2 (one term per thread: n < 256), a fixed tree
  double sl = 0.0, sz = 0.0;
  if (fail == 0 && int(threadIdx.x) < n) {
    const double* cp = A + col_off(int(threadIdx.x), n);
    const double z = cp[n - int(threadIdx.x)];
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
  if (threadIdx.x == 0) {
    const double v = -0.5 * red[1][0] - red[0][0] - 0.5 * double(n) * 1.8378770664093453;  // log(2 pi)
    out[blockIdx.x] = fail ? __builtin_nan("") : v;
    info[blockIdx.x] = fail;
  }
}
static_assert(TGP_SMALL_MAX_N < SMALL_THREADS, "one reduction term per thread");

// what members [b0, b1) need in the staging buffer, and where
struct SmallLaunch {
  int64_t b0 = 0, b1 = 0, max_n = 0;
  int64_t x_doubles = 0, vec_doubles = 0;
  std::vector<char> host;  // rows | programs | X | noise | residual, as on the device
};

int64_t launch_bytes(int64_t nb, int64_t x_doubles, int64_t vec_doubles) {
  return nb * int64_t(sizeof(SmallRow) + sizeof(KProg)) + (x_doubles + 2 * vec_doubles) * 8 + nb * 8 + round_up(nb * 4, 8);
}

// enqueues every launch; the host buffers in `launches` must outlive the join
int small_enqueue(tgp_ctx* ctx, const std::vector<SmallLaunch>& launches, int32_t* info_host, double* out_host) {
  hipStream_t st = ctx->stream;
  if (!ctx->small_lds_raised) {
    TGP_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(small_logprob_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    int(small_lds_doubles(TGP_SMALL_MAX_N) * 8)));
    ctx->small_lds_raised = true;
  }
  int64_t need = 0;
  for (const SmallLaunch& l : launches) need = std::max(need, launch_bytes(l.b1 - l.b0, l.x_doubles, l.vec_doubles));
  TGP_TRY(ensure_work(ctx, size_t(need)));
  for (const SmallLaunch& l : launches) {
    const int64_t nb = l.b1 - l.b0;
    char* base = static_cast<char*>(ctx->d_work);
    const SmallRow* rows = reinterpret_cast<const SmallRow*>(base);
    const KProg* progs = reinterpret_cast<const KProg*>(base + nb * sizeof(SmallRow));
    const double* X = reinterpret_cast<const double*>(base + nb * (sizeof(SmallRow) + sizeof(KProg)));
    const double* noise = X + l.x_doubles;
    const double* resid = noise + l.vec_doubles;
    double* out = const_cast<double*>(resid) + l.vec_doubles;
    int32_t* info = reinterpret_cast<int32_t*>(out + nb);
    TGP_HIP_TRY(hipMemcpyAsync(base, l.host.data(), l.host.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(small_logprob_kernel, dim3(unsigned(nb)), dim3(SMALL_THREADS),
                       size_t(small_lds_doubles(l.max_n) * 8), st, rows, progs, X, noise, resid, out, info);
    TGP_HIP_TRY(hipGetLastError());
    TGP_HIP_TRY(hipMemcpyAsync(out_host + l.b0, out, size_t(nb) * 8, hipMemcpyDeviceToHost, st));
    TGP_HIP_TRY(hipMemcpyAsync(info_host + l.b0, info, size_t(nb) * 4, hipMemcpyDeviceToHost, st));
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
  TGP_ARG_CHECK(ctx != nullptr, "null context");
  TGP_ARG_CHECK(nb >= 0, "negative number of members (%d)", nb);
  if (nb == 0) return TGP_OK;
  std::unique_lock<std::recursive_mutex> lock(ctx->mu);
  TGP_HIP_TRY(hipSetDevice(ctx->device));
  TGP_ARG_CHECK(progs && prog_off && x_off && n && X_host && vec_off && noise_host && resid_host && info_host && out_host,
                "null argument");
  TGP_ARG_CHECK(d >= 1 && d <= TGP_MAX_DIM, "the input dimension must be 1 .. %d (got %d)", TGP_MAX_DIM, d);
  TGP_ARG_CHECK(x_rows >= 0, "negative number of coordinate rows (%lld)", (long long)x_rows);
  std::vector<KProg> kps(size_t(nb), KProg{});
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
  }
  // the split: launches are filled in the order given and end before the member that would take the staging buffer
  // past its cap; coordinates that several members of a launch share (same offset, same length) are staged once
  std::vector<SmallLaunch> launches;
  for (int64_t b0 = 0; b0 < nb;) {
    SmallLaunch l;
    l.b0 = b0;
    std::map<std::pair<int64_t, int32_t>, int64_t> seen;  // (x_off, n) -> first row in the launch's X
    std::vector<SmallRow> rows;
    int64_t b = b0;
    for (; b < nb; ++b) {
      const auto key = std::make_pair(x_off[b], n[b]);
      const bool fresh = seen.find(key) == seen.end();
      const int64_t xd = l.x_doubles + (fresh ? int64_t(n[b]) * d : 0), vd = l.vec_doubles + n[b];
      if (b > b0 && launch_bytes(b - b0 + 1, xd, vd) > SMALL_STAGE_BYTES) break;
      if (fresh) seen[key] = l.x_doubles / d;
      rows.push_back(SmallRow{seen[key], l.vec_doubles, l.vec_doubles, n[b], d, int32_t(b - b0), 0});
      l.x_doubles = xd, l.vec_doubles = vd;
      l.max_n = std::max<int64_t>(l.max_n, n[b]);
    }
    l.b1 = b;
    const int64_t cnt = b - b0;
    l.host.resize(size_t(cnt * int64_t(sizeof(SmallRow) + sizeof(KProg)) + (l.x_doubles + 2 * l.vec_doubles) * 8));
    char* w = l.host.data();
    std::memcpy(w, rows.data(), size_t(cnt) * sizeof(SmallRow));
    w += cnt * sizeof(SmallRow);
    std::memcpy(w, &kps[size_t(b0)], size_t(cnt) * sizeof(KProg));
    w += cnt * sizeof(KProg);
    double* xs = reinterpret_cast<double*>(w);
    double* nzs = xs + l.x_doubles;
    double* rss = nzs + l.vec_doubles;
    for (const auto& kv : seen)
      std::memcpy(xs + kv.second * d, X_host + kv.first.first * d, size_t(kv.first.second) * d * 8);
    for (int64_t m = 0; m < cnt; ++m) {
      const SmallRow& r = rows[size_t(m)];
      std::memcpy(nzs + r.noise_off, noise_host + vec_off[b0 + m], size_t(r.n) * 8);
      std::memcpy(rss + r.resid_off, resid_host + vec_off[b0 + m], size_t(r.n) * 8);
    }
    launches.push_back(std::move(l));
    b0 = b;
  }
  // one host join, on every path: the host buffers above are read by the copies that were enqueued
  const int status = small_enqueue(ctx, launches, info_host, out_host);
  const hipError_t joined = hipStreamSynchronize(ctx->stream);
  TGP_TRY(status);
  TGP_HIP_TRY(joined);
  return TGP_OK;
}
