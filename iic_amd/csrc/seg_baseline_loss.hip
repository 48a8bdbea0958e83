// Losses of the Isola and Doersch segmentation baselines for gfx950: value and gradient from ONE launch each, nothing
// read back to the host.
//
// Replaces code/utils/segmentation/baselines/isola_utils.py:27-72 (isola_loss: two mask gathers, the per-row mask, its
// sum fetched with .item() every step, the EPS replacement, log, the masked sum and their backward nodes) and
// code/utils/segmentation/baselines/doersch_utils.py:55-66 (doersch_loss: the same mask and .item(), the constant target
// vector, nn.CrossEntropyLoss(reduction="none"), the masked mean and their backward nodes).
//
// Both read mask_u8 [N][S][S] at the two points (cy, cx), (oy, ox) of the device coordinate block (clamped into the map):
//   m_n = (mask[n][cy][cx] + mask[n][oy][ox]) > 0,   norm = sum_n m_n   (an integer count: exact).
// One workgroup.  Row arithmetic is float64; the row terms are added in ROW ORDER, n = 0, 1, ..., by one thread, 256 rows
// staged through LDS at a time; every output is rounded to fp32 once.  Two calls give the same bits.
#include "common.h"
#include "../../include/iic_hip.h"

namespace {

constexpr int BL_MAXK = 32;
constexpr double BL_EPS = 2.220446049250313e-16;      // sys.float_info.epsilon = 2^-52 (isola_utils.py:11)

struct bl_points {
  long a, b;      // offsets of the two points inside one [S][S] map
  int label;
};
__device__ __forceinline__ bl_points bl_read(const int* __restrict__ blk, int S) {
  bl_points p;
  const int cy = min(max(blk[0], 0), S - 1), cx = min(max(blk[1], 0), S - 1);
  const int oy = min(max(blk[2], 0), S - 1), ox = min(max(blk[3], 0), S - 1);
  p.a = (long)cy * S + cx;
  p.b = (long)oy * S + ox;
  p.label = blk[4];
  return p;
}
__device__ __forceinline__ int bl_row_mask(const uint8_t* __restrict__ mask, long n, int S, const bl_points& p) {
  const uint8_t* m = mask + n * S * S;
  return ((int)m[p.a] + (int)m[p.b]) > 0 ? 1 : 0;
}
// norm = sum_n m_n: integer, so any order is exact
__device__ __forceinline__ int bl_norm(const uint8_t* __restrict__ mask, int N, int S, const bl_points& p, int* s_cnt) {
  if (threadIdx.x == 0) *s_cnt = 0;
  __syncthreads();
  int c = 0;
  for (int r = threadIdx.x; r < N; r += 256) c += bl_row_mask(mask, r, S, p);
  if (c) atomicAdd(s_cnt, c);
  __syncthreads();
  return *s_cnt;
}
// adds term(r0 .. r0 + 255) to *tot in row order; s_term holds this thread's term on entry
__device__ __forceinline__ void bl_fold_rows(double term, double* s_term, double* tot, int rows) {
  s_term[threadIdx.x] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = *tot;
    for (int i = 0; i < rows; ++i) t += s_term[i];
    *tot = t;
  }
  __syncthreads();
}

// prob fp32 [N] (already through the sigmoid).  t = p (label != 0: adjacent) or fl32(1 - p); dropped iff t < EPS;
// loss = -(1 / norm) sum_n m_n keep_n log(t_n) -- the reference's expression evaluated literally in float64 (a dropped
// row contributes m_n * 0 * log(EPS) = 0; 0 * inf and 0 * NaN are NaN as they are there);
// dp_n = -+ (m_n / norm) / t_n for kept rows, 0 for dropped ones (norm == 0: NaN for every row).
__global__ __launch_bounds__(256) void isola_loss_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ mask,
                                                         const int* __restrict__ blk, float* __restrict__ loss,
                                                         float* __restrict__ dprob, int N, int S) {
#pragma clang fp contract(off)
  __shared__ double s_term[256], s_tot;
  __shared__ int s_cnt;
  const bl_points pts = bl_read(blk, S);
  const bool adjacent = pts.label != 0;
  const int cnt = bl_norm(mask, N, S, pts, &s_cnt);
  const double norm = (double)cnt, rnorm = 1.0 / norm;
  if (threadIdx.x == 0) s_tot = 0.0;
  __syncthreads();
  for (int r0 = 0; r0 < N; r0 += 256) {
    const int r = r0 + threadIdx.x;
    double term = 0.0;
    if (r < N) {
      const float pv = prob[r];
      const float tf = adjacent ? pv : 1.f - pv;
      const double m = (double)bl_row_mask(mask, r, S, pts);
      const bool drop = tf < (float)BL_EPS;      // EPS = 2^-52 is an fp32 value: the comparison torch makes
      const double t = drop ? BL_EPS : (double)tf;
      term = m * (drop ? 0.0 : 1.0) * log(t);
      double g = 0.0;
      if (cnt == 0) g = __builtin_nan("");
      else if (!drop) g = (adjacent ? -1.0 : 1.0) * (m * rnorm) / t;
      if (dprob) dprob[r] = (float)g;
    }
    bl_fold_rows(term, s_term, &s_tot, min(256, N - r0));
  }
  if (threadIdx.x == 0) *loss = (float)(-rnorm * s_tot);
}

// logits fp32 [N][k], target = the block's label for every row.  ce_n = log sum_j exp(x_j - max) - (x_label - max);
// loss = (sum_n m_n ce_n) / norm; dlogits = (m_n / norm) (softmax - onehot).
__global__ __launch_bounds__(256) void doersch_loss_kernel(const float* __restrict__ logits,
                                                           const uint8_t* __restrict__ mask, const int* __restrict__ blk,
                                                           float* __restrict__ loss, float* __restrict__ dlogits, int N,
                                                           int k, int S) {
#pragma clang fp contract(off)
  __shared__ double s_term[256], s_tot;
  __shared__ int s_cnt;
  const bl_points pts = bl_read(blk, S);
  const int label = min(max(pts.label, 0), k - 1);
  const int cnt = bl_norm(mask, N, S, pts, &s_cnt);
  const double norm = (double)cnt;
  if (threadIdx.x == 0) s_tot = 0.0;
  __syncthreads();
  for (int r0 = 0; r0 < N; r0 += 256) {
    const int r = r0 + threadIdx.x;
    double term = 0.0;
    if (r < N) {
      const float* xr = logits + (long)r * k;
      const double m = (double)bl_row_mask(mask, r, S, pts);
      double x[BL_MAXK];
      double mx = -__builtin_inf();
#pragma unroll
      for (int j = 0; j < BL_MAXK; ++j)
        if (j < k) {
          x[j] = (double)xr[j];
          mx = (x[j] > mx || x[j] != x[j]) ? x[j] : mx;      // a NaN logit poisons the row, as torch's max does
        }
      double s = 0.0, xl = 0.0;
#pragma unroll
      for (int j = 0; j < BL_MAXK; ++j)
        if (j < k) {
          x[j] = exp(x[j] - mx);
          s += x[j];
          if (j == label) xl = (double)xr[j] - mx;
        }
      term = m * (log(s) - xl);
      if (dlogits) {
        const double f = m / norm;
#pragma unroll
        for (int j = 0; j < BL_MAXK; ++j)
          if (j < k) dlogits[(long)r * k + j] = (float)(f * (x[j] / s - (j == label ? 1.0 : 0.0)));
      }
    }
    bl_fold_rows(term, s_term, &s_tot, min(256, N - r0));
  }
  if (threadIdx.x == 0) *loss = (float)(s_tot / norm);
}

}  // namespace

extern "C" {

int iic_isola_loss(const float* prob, const unsigned char* mask_u8, const int* coords, float* loss, float* dprob, int N,
                   int S, void* stream) {
  if (!prob || !mask_u8 || !coords || !loss || N < 1 || S < 1) return IIC_ERR_ARG;
  hipLaunchKernelGGL(isola_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, prob, (const uint8_t*)mask_u8, coords,
                     loss, dprob, N, S);
  return iic_launch_status();
}

int iic_doersch_loss(const float* logits, const unsigned char* mask_u8, const int* coords, float* loss, float* dlogits,
                     int N, int k, int S, void* stream) {
  if (!logits || !mask_u8 || !coords || !loss || N < 1 || S < 1 || k < 1) return IIC_ERR_ARG;
  if (k > BL_MAXK) return IIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(doersch_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, (const uint8_t*)mask_u8,
                     coords, loss, dlogits, N, k, S);
  return iic_launch_status();
}

}  // extern "C"
