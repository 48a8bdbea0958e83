// Device-side evaluation counts.
//
// Replaces the k_pred x k_gt masked sums of
//   /root/reference/code/utils/cluster/eval_metrics.py:18-24 (_original_match) and :42-46
//   (_hungarian_match): `int(((flat_preds == c1) * (flat_targets == c2)).sum())` per pair -- 1 400
//   tiny kernels each ending in a host sync at k = 140, gt_k = 10 -- by ONE contingency-matrix
//   kernel, and `int((preds == targets).sum())` of _acc (:69) by a counting kernel.
// Integer work: per-workgroup LDS histogram (k_pred * k_gt <= 16384 bins) merged with 64-bit
// global atomics; labels outside [0, k) match no pair, exactly like the reference's comparisons.
//
// cluster_argmax_acc_kernel is the other half of that survey entry, for the clustering scripts
// (code/utils/cluster/cluster_eval.py): it replaces
//   :55-63   torch.argmax of every sub-head (int64 out) and the slice assignments into flat int32 arrays that span
//            the whole data set
//   :128-132 and :212-228  the reorder loops `reordered_preds[flat_preds == pred_i] = target_i` (2 launches per
//            output cluster and sub-head) and _acc: all of it is a function of one k x gt_k count matrix per sub-head
// by ONE launch per batch.  One wave per (sample, sub-head) row: the lanes stride over the k probabilities, a 64-lane
// butterfly on (value, index) finds torch.argmax's answer -- NaN is maximal, the first maximal index wins -- and lane 0
// stores the label and issues the 64-bit integer atomics into bins that live in global memory (no LDS histogram, no
// k * gt_k cap: a batch is a few thousand rows).  Integer adds commute: the result does not depend on arrival order.
#include "common.h"
#include "../../include/iic_hip.h"

#define EV_MAXBINS 16384

__global__ __launch_bounds__(256) void contingency_kernel(const long long* __restrict__ preds,
                                                          const long long* __restrict__ targets,
                                                          long n, int kp, int kt,
                                                          unsigned long long* __restrict__ counts) {
  __shared__ unsigned int bins[EV_MAXBINS];
  const int nb = kp * kt;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) bins[i] = 0u;
  __syncthreads();
  // a workgroup handles < 2^32 samples (grid-stride over at most n / gridDim), 32-bit bins suffice
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long long p = preds[i], t = targets[i];
    if (p >= 0 && p < kp && t >= 0 && t < kt) atomicAdd(&bins[(int)p * kt + (int)t], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += blockDim.x)
    if (bins[i]) atomicAdd(&counts[i], (unsigned long long)bins[i]);
}

__global__ __launch_bounds__(256) void count_equal_kernel(const long long* __restrict__ a,
                                                          const long long* __restrict__ b, long n,
                                                          unsigned long long* __restrict__ out) {
  unsigned int c = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    c += (a[i] == b[i]) ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// does (av, ai) come before (bv, bi) in torch.argmax's order?  NaN above every number, then the larger value, then the
// lower index (-0.0 == 0.0, all NaNs alike).  ai != bi for any two candidates, so this is a strict total order.
__device__ __forceinline__ bool ca_before(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an != bn) return an;
  if (!an && av != bv) return av > bv;
  return ai < bi;
}

#define CA_WAVES 4

__global__ __launch_bounds__(64 * CA_WAVES) void cluster_argmax_acc_kernel(
    const float* __restrict__ probs, long ld, long head_stride, long rows, int H, int k,
    const long long* __restrict__ targets, int gt_k, unsigned long long* __restrict__ counts, int* __restrict__ labels,
    long label_stride) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * CA_WAVES + (threadIdx.x >> 6);      // row = sample * H + sub-head: uniform per wave
  if (r >= rows) return;
  const long i = r / H;
  const int h = (int)(r - i * H);
  const float* row = probs + i * ld + (long)h * head_stride;
  // a lane without an element holds (-inf, INT_MAX): it loses to every real element, an all -inf row included
  float bv = -__builtin_inff();
  int bi = 0x7fffffff;
  for (int c = lane; c < k; c += 64) {
    const float v = row[c];
    if (ca_before(v, c, bv, bi)) {
      bv = v;
      bi = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ca_before(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane != 0) return;
  if (labels) labels[(long)h * label_stride + i] = bi;
  if (counts) {
    const long nb = (long)k * gt_k;
    unsigned long long* c = counts + (long)h * (nb + 1);
    atomicAdd(&c[nb], 1ull);
    const long long t = targets[i];
    if (t >= 0 && t < gt_k) atomicAdd(&c[(long)bi * gt_k + t], 1ull);
  }
}

extern "C" {

int iic_cluster_argmax_acc(const float* probs, long ld, long head_stride, long n, int H, int k,
                           const long long* targets, int gt_k, long long* counts, int* labels, long label_stride,
                           void* stream) {
  if (!probs || n < 0 || H <= 0 || k <= 0) return IIC_ERR_ARG;
  if (!counts && !labels) return IIC_ERR_ARG;
  if (counts && (!targets || gt_k <= 0)) return IIC_ERR_ARG;
  if (n == 0) return IIC_OK;
  const long rows = n * (long)H;
  const long grid = (rows + CA_WAVES - 1) / CA_WAVES;
  if (grid > 0x7fffffffL) return IIC_ERR_ARG;
  hipLaunchKernelGGL(cluster_argmax_acc_kernel, dim3((unsigned)grid), dim3(64 * CA_WAVES), 0, (hipStream_t)stream, probs,
                     ld, head_stride, rows, H, k, targets, gt_k, (unsigned long long*)counts, labels, label_stride);
  return iic_launch_status();
}

int iic_contingency(const long long* preds, const long long* targets, long n, int k_pred, int k_gt,
                    long long* counts, void* stream) {
  if (!preds || !targets || !counts || n < 0 || k_pred <= 0 || k_gt <= 0) return IIC_ERR_ARG;
  if ((long)k_pred * k_gt > EV_MAXBINS) return IIC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (iic_zero_async(counts, sizeof(long long) * k_pred * k_gt, s) != IIC_OK) return IIC_ERR_LAUNCH;
  if (n == 0) return IIC_OK;
  long blocks = (n + 255) / 256;
  int grid = (int)(blocks < 1024 ? blocks : 1024);
  hipLaunchKernelGGL(contingency_kernel, dim3(grid), dim3(256), 0, s, preds, targets, n, k_pred, k_gt,
                     (unsigned long long*)counts);
  return iic_launch_status();
}

int iic_count_equal(const long long* a, const long long* b, long n, long long* count, void* stream) {
  if (!a || !b || !count || n < 0) return IIC_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (iic_zero_async(count, sizeof(long long), s) != IIC_OK) return IIC_ERR_LAUNCH;
  if (n == 0) return IIC_OK;
  long blocks = (n + 255) / 256;
  int grid = (int)(blocks < 1024 ? blocks : 1024);
  hipLaunchKernelGGL(count_equal_kernel, dim3(grid), dim3(256), 0, s, a, b, n, (unsigned long long*)count);
  return iic_launch_status();
}

}  // extern "C"
