// Triplets baseline loss (KL(pos || orig) - KL(neg || orig), both "elementwise_mean") and its three gradients.
//
// Replaces code/utils/cluster/baselines/triplets.py:231-238 -- in torch a chain of about fifteen launches (log_softmax,
// two softmax, two kl_div and their backward nodes) over three [N, k] matrices -- with two launches.
//
// Logits a (orig), b (pos), c (neg), all [N, k].  With lo = a - lse(a), lp = b - lse(b), lq = c - lse(c), p = exp(lp),
// q = exp(lq), tp_n = sum_j p (lp - lo), tq_n = sum_j q (lq - lo):
//   loss = sum_n (tp_n - tq_n) / (N k)
//   d_a  = (q - p) / (N k)
//   d_b  =  p ((lp - lo) - tp_n) / (N k)
//   d_c  = -q ((lq - lo) - tq_n) / (N k)
// The log-space form IS the specification: log p is b - lse(b), never log(exp(..)).  torch's own gradient of the
// target is 0 * (-inf) = NaN as soon as a softmax entry underflows (float64: at a logit spread of about 750); here such
// an entry contributes its finite limit, 0.
//
//   triplets_rows_kernel    one 64-lane wave owns a row, lane j holds classes j, j + 64, .. (T <= 16 per matrix, all three
//                           rows are read once and stay in registers); max, sum, tp, tq are wave reductions in float64.
//                           A workgroup of TR_ROWS waves adds its rows' tp - tq in wave order and writes ONE float64
//                           partial.  Both KL terms come from tr_kl_row: b == c bit for bit gives tp == tq, d_a == 0
//                           and d_b == -d_c exactly.
//   triplets_finish_kernel  one workgroup: thread t adds a contiguous run of partials in index order, thread 0 adds the
//                           256 runs in index order, divides by N k and rounds to fp32 once.
// No float atomics, no "last workgroup finalises": the order of every sum is a function of (N, k) alone.
//
// Non-finite logits.  A term with lp = -inf (b_j = -inf: p_j is an exact zero) contributes 0 * lo, as torch's
// xlogy(0, 0) - 0 * lo does, so the loss is non-finite exactly when torch's is.  Every gradient of a row that holds a
// non-finite logit in ANY of the three inputs is NaN (torch keeps some of them finite); other rows are not affected.
#include "common.h"
#include "../../include/iic_hip.h"

#define TR_ROWS 4                        // rows (= waves) per workgroup
#define TR_THREADS (64 * TR_ROWS)
#define TR_MAXK 1024
#define TR_FIN_THREADS 256

static bool tr_supported(long N, int k) {
  return k >= 1 && k <= TR_MAXK && N >= 1 && N < (1L << 31) && N * (long)k < (1L << 31);
}
static long tr_partials(long N) { return (N + TR_ROWS - 1) / TR_ROWS; }

// lse(x) of one row, T values per lane (class lane + 64 t where it is below k).  All lanes return the same bits.
template <int T>
__device__ __forceinline__ double tr_lse(const float (&x)[T], int lane, int k) {
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < T; ++t)
    if (lane + 64 * t < k) m = fmaxf(m, x[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < T; ++t)
    if (lane + 64 * t < k) s += exp((double)x[t] - (double)m);      // a NaN or +inf logit, or a row of -inf: NaN
  s = wave_sum_d(s);
  return (double)m + log(s);
}

// One KL term of a row: d[t] = lt - lo and w[t] = exp(lt) per class, returns sum_j w (lt - lo) (the same bits in every lane)
template <int T>
__device__ __forceinline__ double tr_kl_row(const float (&a)[T], double lse_a, const float (&x)[T], double lse_x, int lane,
                                            int k, double (&d)[T], double (&w)[T]) {
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    d[t] = w[t] = 0.0;
    if (lane + 64 * t < k) {
      const double lo = (double)a[t] - lse_a, lt = (double)x[t] - lse_x;
      d[t] = lt - lo;
      w[t] = exp(lt);
      s += lt == -INFINITY ? 0.0 * lo : w[t] * d[t];
    }
  }
  return wave_sum_d(s);
}

template <int T>
__global__ __launch_bounds__(TR_THREADS) void triplets_rows_kernel(
    const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ C, long ld, long N, int k,
    float* __restrict__ d_a, float* __restrict__ d_b, float* __restrict__ d_c, double* __restrict__ part) {
  __shared__ double s_row[TR_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * TR_ROWS + wv;
  double r = 0.0;
  if (row < N) {      // wave-uniform
    float a[T], b[T], c[T];
    bool finite = true;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int j = lane + 64 * t;
      a[t] = b[t] = c[t] = 0.f;
      if (j < k) {
        a[t] = A[row * ld + j];
        b[t] = B[row * ld + j];
        c[t] = C[row * ld + j];
        finite = finite && isfinite(a[t]) && isfinite(b[t]) && isfinite(c[t]);
      }
    }
    const bool poison = __any(!finite);
    const double la = tr_lse<T>(a, lane, k), lb = tr_lse<T>(b, lane, k), lc = tr_lse<T>(c, lane, k);
    double dp[T], p[T], dq[T], q[T];
    const double tp = tr_kl_row<T>(a, la, b, lb, lane, k, dp, p);
    const double tq = tr_kl_row<T>(a, la, c, lc, lane, k, dq, q);
    r = tp - tq;
    if (d_a) {
      const double nk = (double)N * (double)k;
      const float bad = __builtin_nanf("");
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int j = lane + 64 * t;
        if (j < k) {
          const long o = row * k + j;
          d_a[o] = poison ? bad : (float)((q[t] - p[t]) / nk);
          if (d_b) {
            const double gb = p[t] * (dp[t] - tp) / nk, gc = q[t] * (dq[t] - tq) / nk;
            d_b[o] = poison ? bad : (float)gb;
            d_c[o] = poison ? bad : -(float)gc;
          }
        }
      }
    }
  }
  if (lane == 0) s_row[wv] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < TR_ROWS; ++i) s += s_row[i];
    part[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(TR_FIN_THREADS) void triplets_finish_kernel(const double* __restrict__ part, long W, long N,
                                                                         int k, float* __restrict__ loss) {
  __shared__ double s_run[TR_FIN_THREADS];
  const long per = (W + TR_FIN_THREADS - 1) / TR_FIN_THREADS;
  const long lo = (long)threadIdx.x * per, hi = lo + per < W ? lo + per : W;
  double s = 0.0;
  for (long i = lo; i < hi; ++i) s += part[i];
  s_run[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < TR_FIN_THREADS; ++i) t += s_run[i];
    loss[0] = (float)(t / ((double)N * (double)k));
  }
}

template <int T>
static void tr_launch(const float* a, const float* b, const float* c, long ld, long N, int k, float* d_a, float* d_b,
                      float* d_c, double* part, hipStream_t s) {
  hipLaunchKernelGGL(triplets_rows_kernel<T>, dim3((unsigned)tr_partials(N)), dim3(TR_THREADS), 0, s, a, b, c, ld, N, k,
                     d_a, d_b, d_c, part);
}

extern "C" {

int iic_triplets_supported(long N, int k) { return tr_supported(N, k) ? 1 : 0; }

long iic_triplets_workspace_bytes(long N, int k) {
  if (!tr_supported(N, k)) return 0;
  return (tr_partials(N) * 8 + 255) & ~255L;
}

int iic_triplets_loss(const float* a, const float* b, const float* c, long ld, long N, int k, float* loss, float* d_a,
                      float* d_b, float* d_c, void* ws, void* stream) {
  if (!tr_supported(N, k)) return IIC_ERR_UNSUPPORTED;
  if (!a || !b || !c || !loss || !ws || ld < k) return IIC_ERR_ARG;
  if ((d_b == nullptr) != (d_c == nullptr) || (d_b && !d_a)) return IIC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  if (k <= 64) tr_launch<1>(a, b, c, ld, N, k, d_a, d_b, d_c, part, s);
  else if (k <= 128) tr_launch<2>(a, b, c, ld, N, k, d_a, d_b, d_c, part, s);
  else if (k <= 256) tr_launch<4>(a, b, c, ld, N, k, d_a, d_b, d_c, part, s);
  else if (k <= 512) tr_launch<8>(a, b, c, ld, N, k, d_a, d_b, d_c, part, s);
  else tr_launch<16>(a, b, c, ld, N, k, d_a, d_b, d_c, part, s);
  hipLaunchKernelGGL(triplets_finish_kernel, dim3(1), dim3(TR_FIN_THREADS), 0, s, part, tr_partials(N), N, k, loss);
  return iic_launch_status();
}

}  // extern "C"
