// The Linear over bf16 PT activations for gfx950, one family for one or two operands: Linear(C H W -> F) on layer 3's PT
// tensor (the supervised head of the semi-supervised fine-tuning step, iic_sup_*) and the joint Linear(2 C p p -> F) over
// the two patch activations of the Isola / Doersch baselines' heads (iic_pair_*); then the rest of the supervised head:
// BatchNorm1d + ReLU, cross-entropy, and the ten-crop accuracy count.
//
// Replaces code/archs/semisup/sup_head5.py:12-19,33-37 (nn.Linear + nn.BatchNorm1d + nn.ReLU over
// net5g.py:56's flatten of layer 3), the nn.CrossEntropyLoss of code/scripts/semisup/IID_semisup_STL10.py and
// code/utils/semisup/general.py:46-93 (assess_acc_block).
//
// The three products of the first Linear run on the bf16 MFMA pipe (v_mfma_f32_32x32x16_bf16, fp32 accumulation):
//   forward        y[n][f]  = sum_k x[n][k] wb[f][k] + b[f]        A = the PT interior in place, B = wb [F][K]
//   backward-data  dx[n][k] = sum_f dyb[n][f] wt[k][f]             A = bf16(dy) [N][F],          B = wt [K][F]
//   weight grad    dW[f][k] = sum_n dyt[f][n] x[n][k]              A = bf16(dy)^T [F][Np],       B = the PT interior,
//                                                                  transposed on its way into LDS
// k runs over the PT interior in (h, w, c) order: K = H W C, row h of an image is W C contiguous bf16, so a K-tile of 64
// never leaves a row (C % 64 == 0) and its address is a division per tile, no index table.  wb / wt are the fp32 parameter
// rounded to bf16 with its (c, h, w) columns permuted to that order (sup_weight_prep_*); dW is written straight back in the
// parameter's (c, h, w) order.  One block = 4 waves = a 128 x 128 output tile (2 x 2 MFMA tiles of 32 x 32 per wave), K-tiles
// of 64 through double-buffered LDS at a 144-byte row pitch.  No float atomics anywhere: the forward's K split writes
// partial matrices that sup_fold_kernel adds in index order, so two runs give equal bits.
// With two operands the forward's K axis covers both PT activations, one after the other, and each column half of the
// weight is a matrix whose rows are 2 K apart: the same kernels, driven by one set of host routines (lin_*, below the
// kernels) that the iic_sup_* and iic_pair_* entries call with an operand count of 1 or 2.
#include "common.h"
#include "../../include/iic_hip.h"

namespace {

constexpr int TM = 128, TN = 128, BK = 64;
constexpr int PITCH = BK + 8;                       // bf16 elements: 144-byte rows, 16-byte aligned
constexpr int TILE_ELEMS = TM * PITCH;              // one operand tile
constexpr size_t GEMM_LDS = (size_t)4 * TILE_ELEMS * sizeof(bf16_t);   // A and B, two buffers each

// A bf16 matrix whose row r, column k lives at p[r * ld + (k / seg) * segstride + k % seg]: a plain row-major matrix
// (seg = number of columns) or the interior of a PT tensor (seg = W C, segstride = (W + 2) C, p at the first interior
// element, ld = (H + 2)(W + 2) C).
struct sup_mat {
  const bf16_t* p;
  long ld;
  int seg;
  long segstride;
  int rows;
};

__device__ __forceinline__ long sup_koff(const sup_mat& m, int k) {
  const int s = k / m.seg;
  return (long)s * m.segstride + (k - s * m.seg);
}

// 128 rows x 64 k of a sup_mat -> registers (4 x 16 bytes per thread: chunk id = tid + 256 i, row = id >> 3, 8 k each)
__device__ __forceinline__ void sup_gload(const sup_mat& m, int row0, int k0, u32x4 (&r)[4]) {
  const long koff = sup_koff(m, k0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + 256 * i, row = row0 + (id >> 3);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < m.rows) v = *reinterpret_cast<const u32x4*>(m.p + (long)row * m.ld + koff + (id & 7) * 8);
    r[i] = v;
  }
}
__device__ __forceinline__ void sup_lstore(bf16_t* s, const u32x4 (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + 256 * i;
    *reinterpret_cast<u32x4*>(s + (id >> 3) * PITCH + (id & 7) * 8) = r[i];
  }
}

// one K-tile of 64: wave (wm, wn) multiplies its 64 rows of sA with its 64 rows of sB.  Fragment of lane l for k-step s:
// row l & 31, k = 16 s + 8 (l >> 5) ... + 7 (16 bytes), for A and B alike.
__device__ __forceinline__ void sup_compute(const bf16_t* sA, const bf16_t* sB, int wm, int wn, f32x16 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const bf16_t* pa = sA + (wm * 64 + r) * PITCH + 8 * h;
  const bf16_t* pb = sB + (wn * 64 + r) * PITCH + 8 * h;
#pragma unroll
  for (int s = 0; s < BK / 16; ++s) {
    const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(pa + s * 16);
    const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(pa + 32 * PITCH + s * 16);
    const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(pb + s * 16);
    const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(pb + 32 * PITCH + s * 16);
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
  }
}

__device__ __forceinline__ void sup_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// out[m][n] = sum_k A[m][k] B[n][k]  (both operands k-contiguous).  blockIdx = (row tile, column tile, K slice).
// A is two matrices side by side along k: K-tiles 0 .. ka - 1 come from A, tiles ka .. K / 64 - 1 from A2 (its columns
// from 0) -- the two patch activations of the baselines' joint Linear; ka = K / 64 for a single operand.
// OUT_BF16 = false: fp32 out + z * M * ldc (+ bias[n] when given) at [m * ldc + n];
// OUT_BF16 = true:  bf16 RNE into the sup_mat `o` (row m, column n) -- the interior of a PT tensor, border untouched.
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void sup_gemm_kernel(sup_mat A, sup_mat A2, int ka, sup_mat B, int K,
                                                        const float* __restrict__ bias, float* __restrict__ out, long ldc,
                                                        sup_mat o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sup_smem[];
  bf16_t* const sA = reinterpret_cast<bf16_t*>(sup_smem);     // [2][TILE_ELEMS]
  bf16_t* const sB = sA + 2 * TILE_ELEMS;                     // [2][TILE_ELEMS]
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, lane = threadIdx.x & 63;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  const int ntiles = K / BK, S = gridDim.z, z = blockIdx.z;
  const int per = (ntiles + S - 1) / S;
  const int t0 = z * per, t1 = min(ntiles, t0 + per);
  f32x16 acc[2][2];
  sup_zero(acc);
  u32x4 ra[4], rb[4];
  auto load_a = [&](int t) {
    if (t < ka) sup_gload(A, m0, t * BK, ra);
    else sup_gload(A2, m0, (t - ka) * BK, ra);
  };
  if (t0 < t1) {
    load_a(t0);
    sup_gload(B, n0, t0 * BK, rb);
    sup_lstore(sA, ra);
    sup_lstore(sB, rb);
    if (t0 + 1 < t1) {
      load_a(t0 + 1);
      sup_gload(B, n0, (t0 + 1) * BK, rb);
    }
  }
  for (int t = t0; t < t1; ++t) {
    const int cur = (t - t0) & 1;
    __syncthreads();               // buffer `cur` complete; everyone is done reading the other one
    if (t + 1 < t1) {
      sup_lstore(sA + (cur ^ 1) * TILE_ELEMS, ra);
      sup_lstore(sB + (cur ^ 1) * TILE_ELEMS, rb);
    }
    if (t + 2 < t1) {
      load_a(t + 2);
      sup_gload(B, n0, (t + 2) * BK, rb);
    }
    sup_compute(sA + cur * TILE_ELEMS, sB + cur * TILE_ELEMS, wm, wn, acc);
  }
  const int M = A.rows, Nn = B.rows;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = n0 + wn * 64 + b * 32 + (lane & 31);
      if (col >= Nn) continue;
      if (OUT_BF16) {
        const long coff = sup_koff(o, col);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * 64 + a * 32 + mfma32_row(r, lane);
          if (row < M) const_cast<bf16_t*>(o.p)[(long)row * o.ld + coff] = f32_to_bf16(acc[a][b][r]);
        }
      } else {
        const float bv = bias ? bias[col] : 0.f;
        float* const op = out + (long)z * M * ldc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * 64 + a * 32 + mfma32_row(r, lane);
          if (row < M) op[(long)row * ldc + col] = acc[a][b][r] + bv;
        }
      }
    }
}

// y[i] = ws[0][i] + ws[1][i] + ... + ws[S-1][i] + bias[i % F]: index order, no atomics
__global__ __launch_bounds__(256) void sup_fold_kernel(const float* __restrict__ ws, int S, const float* __restrict__ bias,
                                                        float* __restrict__ y, long mn, int F) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= mn) return;
  float v = ws[i];
  for (int q = 1; q < S; ++q) v += ws[(long)q * mn + i];
  if (bias) v += bias[i % F];
  y[i] = v;
}

// Weight gradient.  blockIdx = (128 rows f, 8 channels c0 ..., 16 pixels p0 ...): the tile's 128 columns are
// j = 16 cc + pp <-> channel c0 + cc, pixel p0 + pp, so that a lane group of 16 stores 64 contiguous bytes of the
// parameter's (c, h, w) row and a loader thread reads the 8 channels of one pixel in one 16-byte load.
// A = dyt [F][Np] (Np = N rounded up to 64, zero padded), K = Np.  B[j][n] = x[n][pixel][channel]: the loader takes two
// images n, n + 1 per item and writes 8 packed pairs into the [j][n] LDS image (conflict-free: banks 36 pp + np).
// dW rows are ldw floats apart (ldw = K, or 2 K for one column half of the baselines' joint Linear).
__device__ __forceinline__ void sup_wg_bload(const bf16_t* __restrict__ x, long ldn, long poff, int N, int k0,
                                             u32x4 (&r)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int np = (threadIdx.x >> 4) + 16 * i, n = k0 + 2 * np;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (poff >= 0 && n + q < N) v = *reinterpret_cast<const u32x4*>(x + (long)(n + q) * ldn + poff);
      r[i][q] = v;
    }
  }
}
__device__ __forceinline__ void sup_wg_bstore(bf16_t* s, const u32x4 (&r)[2][2]) {
  const int pp = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int np = (threadIdx.x >> 4) + 16 * i;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t lo = r[i][0][w], hi = r[i][1][w];
      // channels 2 w and 2 w + 1 of images n (low half) and n + 1 (high half)
      *reinterpret_cast<uint32_t*>(s + ((2 * w) * 16 + pp) * PITCH + 2 * np) = (lo & 0xffffu) | (hi << 16);
      *reinterpret_cast<uint32_t*>(s + ((2 * w + 1) * 16 + pp) * PITCH + 2 * np) = (lo >> 16) | (hi & 0xffff0000u);
    }
  }
}

__global__ __launch_bounds__(256) void sup_wgrad_kernel(sup_mat A, const bf16_t* __restrict__ x, long ldn, int N, int H,
                                                         int W, int C, float* __restrict__ dW, long ldw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sup_smem[];
  bf16_t* const sA = reinterpret_cast<bf16_t*>(sup_smem);
  bf16_t* const sB = sA + 2 * TILE_ELEMS;
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, lane = threadIdx.x & 63;
  const int f0 = blockIdx.x * TM, c0 = blockIdx.y * 8, p0 = blockIdx.z * 16;
  const int HW = H * W;
  // this thread's pixel: offset of its 8 channels inside an image of the PT tensor, -1 beyond the last pixel
  long poff = -1;
  {
    const int p = p0 + (threadIdx.x & 15);
    if (p < HW) poff = ((long)(p / W + 1) * (W + 2) + (p % W + 1)) * C + c0;
  }
  const int ntiles = A.seg / BK;      // Np / 64
  f32x16 acc[2][2];
  sup_zero(acc);
  u32x4 ra[4], rb[2][2];
  sup_gload(A, f0, 0, ra);
  sup_wg_bload(x, ldn, poff, N, 0, rb);
  sup_lstore(sA, ra);
  sup_wg_bstore(sB, rb);
  if (1 < ntiles) {
    sup_gload(A, f0, BK, ra);
    sup_wg_bload(x, ldn, poff, N, BK, rb);
  }
  for (int t = 0; t < ntiles; ++t) {
    const int cur = t & 1;
    __syncthreads();
    if (t + 1 < ntiles) {
      sup_lstore(sA + (cur ^ 1) * TILE_ELEMS, ra);
      sup_wg_bstore(sB + (cur ^ 1) * TILE_ELEMS, rb);
    }
    if (t + 2 < ntiles) {
      sup_gload(A, f0, (t + 2) * BK, ra);
      sup_wg_bload(x, ldn, poff, N, (t + 2) * BK, rb);
    }
    sup_compute(sA + cur * TILE_ELEMS, sB + cur * TILE_ELEMS, wm, wn, acc);
  }
  const int F = A.rows;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = wn * 64 + b * 32 + (lane & 31);
      const int c = c0 + (j >> 4), p = p0 + (j & 15);
      if (p >= HW) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = f0 + wm * 64 + a * 32 + mfma32_row(r, lane);
        if (row < F) dW[(long)row * ldw + (long)c * HW + p] = acc[a][b][r];
      }
    }
}

// wb[f][p C + c] = bf16(w[f][c HW + p]): per row f the [C][HW] slab transposed to [HW][C], 64 channels x 64 pixels
// through LDS -- reads run along p, writes are 128-byte runs of packed channel pairs.  blockIdx = (pixel tile, channel
// tile, f).  Rows of w and wb are ld floats / bf16 apart (ld = K, or 2 K for one column half of the joint Linear).
__global__ __launch_bounds__(256) void sup_weight_prep_fwd_kernel(const float* __restrict__ w, bf16_t* __restrict__ wb,
                                                                   int C, int HW, long ld) {
  __shared__ float tile[64][65];
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const float* src = w + (long)blockIdx.z * ld;
  uint32_t* dst = reinterpret_cast<uint32_t*>(wb + (long)blockIdx.z * ld);
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int cl = e >> 6, pl = e & 63;
    tile[cl][pl] = (p0 + pl < HW) ? src[(long)(c0 + cl) * HW + p0 + pl] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 32; e += 256) {
    const int pl = e >> 5, c2 = e & 31;
    if (p0 + pl < HW) dst[((long)(p0 + pl) * C + c0) / 2 + c2] = pack_bf16x2(tile[2 * c2][pl], tile[2 * c2 + 1][pl]);
  }
}
// wt[p C + c][f] = bf16(w[f][c HW + p]): 64 f x 64 source columns through LDS, 128-byte runs on both sides; rows of
// w are ld floats apart
__global__ __launch_bounds__(256) void sup_weight_prep_bwd_kernel(const float* __restrict__ w, bf16_t* __restrict__ wt,
                                                                   int F, int C, int HW, long ld) {
  __shared__ float tile[64][65];
  const long K = (long)C * HW;
  const int f0 = blockIdx.y * 64;
  const long s0 = (long)blockIdx.x * 64;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int fl = e >> 6, sl = e & 63;
    tile[fl][sl] = (f0 + fl < F && s0 + sl < K) ? w[(long)(f0 + fl) * ld + s0 + sl] : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int sl = e >> 6, fl = e & 63;
    const long s = s0 + sl;
    if (s < K && f0 + fl < F) {
      const int c = (int)(s / HW), p = (int)(s - (long)c * HW);
      wt[((long)p * C + c) * F + f0 + fl] = f32_to_bf16(tile[fl][sl]);
    }
  }
}

// dyb[n][f] = bf16(dy[n][f]); dyt[f][n] = the same, n < Np, zero for n >= N.  32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void sup_dy_cast_kernel(const float* __restrict__ dy, bf16_t* __restrict__ dyb,
                                                           bf16_t* __restrict__ dyt, int N, int F, int Np) {
  __shared__ bf16_t tile[32][33];
  const int f0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  for (int e = threadIdx.x; e < 32 * 32; e += 256) {
    const int nl = e >> 5, fl = e & 31, n = n0 + nl, f = f0 + fl;
    bf16_t v = 0;
    if (n < N && f < F) {
      v = f32_to_bf16(dy[(long)n * F + f]);
      dyb[(long)n * F + f] = v;
    }
    tile[nl][fl] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 32 * 32; e += 256) {
    const int fl = e >> 5, nl = e & 31, n = n0 + nl, f = f0 + fl;
    if (n < Np && f < F) dyt[(long)f * Np + n] = tile[nl][fl];
  }
}

// ---- BatchNorm1d + ReLU over fp32 [N][F] ---------------------------------------------------------------------------
// A block owns 32 columns; its 8 row groups (r = g, g + 8, ...) accumulate in double and are folded through LDS in group
// order: a fixed order, whatever else runs.  The element-wise arithmetic is fp32.
__device__ __forceinline__ double sup_col_fold(double v, double (*part)[32], int g, int cl) {
  __syncthreads();
  part[g][cl] = v;
  __syncthreads();
  double t = part[0][cl];
#pragma unroll
  for (int q = 1; q < 8; ++q) t += part[q][cl];
  return t;
}

__global__ __launch_bounds__(256) void sup_bn_relu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ rmean,
                                                               float* __restrict__ rvar, float* __restrict__ y,
                                                               float* __restrict__ smean, float* __restrict__ sinv, int N,
                                                               int F, int training, float momentum, float eps) {
  __shared__ double part[8][32];
  const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const bool vc = c < F;
  float mean, inv;
  if (training) {
    double s = 0.0;
    if (vc)
      for (int r = g; r < N; r += 8) s += (double)x[(long)r * F + c];
    const double m = sup_col_fold(s, part, g, cl) / (double)N;
    double q = 0.0;
    if (vc)
      for (int r = g; r < N; r += 8) {
        const double d = (double)x[(long)r * F + c] - m;
        q += d * d;
      }
    const double var = sup_col_fold(q, part, g, cl) / (double)N;      // biased
    mean = (float)m;
    inv = (float)(1.0 / sqrt(var + (double)eps));
    if (vc && g == 0 && rmean) {
      const double mo = (double)momentum;
      rmean[c] = (float)((1.0 - mo) * (double)rmean[c] + mo * m);
      rvar[c] = (float)((1.0 - mo) * (double)rvar[c] + mo * var * ((double)N / (double)(N - 1)));   // unbiased
    }
  } else {
    mean = vc ? rmean[c] : 0.f;
    inv = vc ? (float)(1.0 / sqrt((double)rvar[c] + (double)eps)) : 0.f;
  }
  if (!vc) return;
  if (g == 0) {
    smean[c] = mean;
    sinv[c] = inv;
  }
  const float ga = gamma[c], be = beta[c];
  for (int r = g; r < N; r += 8) {
    const float xh = (x[(long)r * F + c] - mean) * inv;
    y[(long)r * F + c] = iic_relu(xh * ga + be);
  }
}

// g = dout where y > 0, else 0; dgamma = sum g xhat, dbeta = sum g;
// batch statistics: dx = gamma inv (g - dbeta / N - xhat dgamma / N); running statistics: dx = gamma inv g
__global__ __launch_bounds__(256) void sup_bn_relu_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                               const float* __restrict__ y, const float* __restrict__ gamma,
                                                               const float* __restrict__ smean, const float* __restrict__ sinv,
                                                               float* __restrict__ dx, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, int N, int F, int training) {
  __shared__ double part[8][32];
  const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  const bool vc = c < F;
  const float mean = vc ? smean[c] : 0.f, inv = vc ? sinv[c] : 0.f;
  double s1 = 0.0, s2 = 0.0;
  if (vc)
    for (int r = g; r < N; r += 8) {
      const long i = (long)r * F + c;
      const float gz = y[i] > 0.f ? dout[i] : 0.f;
      const float xh = (x[i] - mean) * inv;
      s1 += (double)gz;
      s2 += (double)gz * (double)xh;
    }
  const double S1 = sup_col_fold(s1, part, g, cl);
  const double S2 = sup_col_fold(s2, part, g, cl);
  if (!vc) return;
  if (g == 0) {
    dgamma[c] = (float)S2;
    dbeta[c] = (float)S1;
  }
  const float k = gamma[c] * inv;
  const float m1 = training ? (float)(S1 / (double)N) : 0.f, m2 = training ? (float)(S2 / (double)N) : 0.f;
  for (int r = g; r < N; r += 8) {
    const long i = (long)r * F + c;
    const float gz = y[i] > 0.f ? dout[i] : 0.f;
    const float xh = (x[i] - mean) * inv;
    dx[i] = k * (gz - m1 - xh * m2);
  }
}

// ---- cross-entropy: mean loss and dlogits = (softmax - onehot) / N from one launch (one block: the row losses are
// summed in double per thread and folded in wave order) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void sup_cross_entropy_kernel(const float* __restrict__ logits,
                                                                 const long long* __restrict__ targets,
                                                                 float* __restrict__ loss, float* __restrict__ dlogits,
                                                                 int N, int k) {
  __shared__ double red[32];
  const float invn = 1.f / (float)N;
  double acc = 0.0;
  for (int r = threadIdx.x; r < N; r += 256) {
    const float* xr = logits + (long)r * k;
    float* dr = dlogits + (long)r * k;
    const int t = (int)targets[r];
    float m = -INFINITY;
    for (int j = 0; j < k; ++j) m = fmaxf(m, xr[j]);
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += expf(xr[j] - m);
    const float inv = 1.f / s;
    for (int j = 0; j < k; ++j) dr[j] = (expf(xr[j] - m) * inv - (j == t ? 1.f : 0.f)) * invn;
    acc += (double)(logf(s) - (xr[t] - m));
  }
  const double tot = block_sum_d(acc, red);
  if (threadIdx.x == 0) *loss = (float)(tot / (double)N);
}

// ---- ten-crop accuracy: one thread per image; the `crops` rows of a class are added in float64 in row order and divided
// by `crops`, the first maximal class wins (np.argmax: a NaN counts as maximal); counts += (correct, images) ------------
__global__ __launch_bounds__(256) void sup_tencrop_acc_kernel(const float* __restrict__ logits,
                                                               const long long* __restrict__ targets,
                                                               unsigned long long* __restrict__ counts, int B, int k,
                                                               int crops) {
  __shared__ unsigned int s_ok, s_n;
  if (threadIdx.x == 0) s_ok = s_n = 0u;
  __syncthreads();
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) {
    const float* base = logits + (long)b * crops * k;
    int best = 0;
    double bv = 0.0;
    for (int j = 0; j < k; ++j) {
      double s = 0.0;
      for (int q = 0; q < crops; ++q) s += (double)base[(long)q * k + j];
      s /= (double)crops;
      if (j == 0 || (!(bv != bv) && (s > bv || s != s))) {
        best = j;
        bv = s;
      }
    }
    atomicAdd(&s_n, 1u);
    if ((long long)best == targets[b]) atomicAdd(&s_ok, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(counts, (unsigned long long)s_ok);
    atomicAdd(counts + 1, (unsigned long long)s_n);
  }
}

bool sup_shape_ok(int N, int F, int C, int H, int W) {
  return N >= 1 && F >= 64 && C >= 64 && H >= 1 && W >= 1 && (F % 64) == 0 && (C % 64) == 0 &&
         (long)N * (H + 2) * (W + 2) * C < (1L << 40) && (long)H * W * C < (1L << 30);
}
sup_mat sup_pt(const void* pt, int N, int H, int W, int C) {
  sup_mat m;
  m.p = (const bf16_t*)pt + (long)(W + 2 + 1) * C;
  m.ld = (long)(H + 2) * (W + 2) * C;
  m.seg = W * C;
  m.segstride = (long)(W + 2) * C;
  m.rows = N;
  return m;
}
sup_mat sup_flat(const void* p, int rows, int cols) {
  sup_mat m;
  m.p = (const bf16_t*)p;
  m.ld = cols;
  m.seg = cols;
  m.segstride = 0;
  m.rows = rows;
  return m;
}

// ---- host side of the Linear over Q = 1 or 2 PT operands -------------------------------------------------------------
// y[n][f] = sum_q sum_k a_q[n][k] w[f][q K + k] + b[f], K = H W C per operand: iic_sup_* is Q = 1, iic_pair_* (the joint
// Linear of the Isola / Doersch heads over the two p x p patch activations) Q = 2 with H = W = p.  The forward runs its K
// axis over both activations (sup_gemm_kernel's A, A2); everywhere else the column halves of w are handled one after
// the other by the same kernels: a half of w, wb or dW is a matrix whose rows are Q K apart.
struct lin_shape {
  int N, F, C, H, W, Q;
};
bool lin_shape_ok(const lin_shape& s) {
  if (!sup_shape_ok(s.N, s.F, s.C, s.H, s.W)) return false;
  return s.Q == 1 || (s.H == s.W && (s.H & 1) == 1 && 2L * s.H * s.W * s.C < (1L << 30));
}
// K slices of the forward: enough workgroups for two per CU (their LDS: 72 KB each) over the row x column tiles, at
// least 8 K-tiles per slice, at most 16 slices for one operand and 64 for two.  The pair forward has a fraction of one
// 128-row tile of images and reads every weight element once, so it is bound by streaming w and the slices are what
// fills the chip -- at the Potsdam shape (N = 75, F = 1024, C = 1024, p = 11: 8 column tiles, 3872 K-tiles) 64 slices
// of 60 or 61 K-tiles, whose partial matrices (64 x 75 x 1024 fp32, 20 MB) are 4 % of the 507 MB of weights read.
int lin_nsplit(const lin_shape& s) {
  const long tiles = (long)((s.N + TM - 1) / TM) * ((s.F + TN - 1) / TN);
  const int ktiles = s.Q * s.H * s.W * s.C / BK, cap = s.Q == 1 ? 16 : 64;
  long n = (2L * iic_num_cus() + tiles - 1) / tiles;
  if (n > ktiles / 8) n = ktiles / 8;
  if (n > cap) n = cap;
  return n < 1 ? 1 : (int)n;
}

// wb, wt of w [F][Q K]; per half: the forward operand, then the backward one
int lin_weight_prep(const float* w, void* wb, void* wt, const lin_shape& s, void* stream) {
  if (!lin_shape_ok(s)) return IIC_ERR_UNSUPPORTED;
  const int F = s.F, C = s.C, HW = s.H * s.W;
  const long K = (long)C * HW;
  if (F > 65535 || C / 64 > 65535) return IIC_ERR_UNSUPPORTED;
  for (int q = 0; q < s.Q; ++q) {
    int rc = iic_launch_lds<sup_weight_prep_fwd_kernel>(dim3((HW + 63) / 64, C / 64, F), dim3(256), 0, (hipStream_t)stream,
                                                        w + q * K, (bf16_t*)wb + q * K, C, HW, s.Q * K);
    if (rc) return rc;
    rc = iic_launch_lds<sup_weight_prep_bwd_kernel>(dim3((unsigned)((K + 63) / 64), (F + 63) / 64), dim3(256), 0,
                                                    (hipStream_t)stream, w + q * K, (bf16_t*)wt + q * K * F, F, C, HW,
                                                    s.Q * K);
    if (rc) return rc;
  }
  return iic_launch_status();
}

// a1_pt is read at Q = 2 only
int lin_fwd(const void* a0_pt, const void* a1_pt, const void* wb, const float* bias, float* y, float* ws,
            const lin_shape& s, void* stream) {
  if (!lin_shape_ok(s)) return IIC_ERR_UNSUPPORTED;
  const int N = s.N, F = s.F, K = s.H * s.W * s.C;
  const int S = lin_nsplit(s);
  if (S > 1 && !ws) return IIC_ERR_ARG;
  const sup_mat A = sup_pt(a0_pt, N, s.H, s.W, s.C), A2 = s.Q == 2 ? sup_pt(a1_pt, N, s.H, s.W, s.C) : A,
                B = sup_flat(wb, F, s.Q * K), none = sup_flat(nullptr, 0, 1);
  dim3 grid((N + TM - 1) / TM, (F + TN - 1) / TN, S);
  int rc = iic_launch_lds<sup_gemm_kernel<false>>(grid, dim3(256), GEMM_LDS, (hipStream_t)stream, A, A2, K / BK, B,
                                                  s.Q * K, S > 1 ? (const float*)nullptr : bias, S > 1 ? ws : y, (long)F,
                                                  none);
  if (rc) return rc;
  if (S > 1) {
    const long mn = (long)N * F;
    rc = iic_launch_lds<sup_fold_kernel>(dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                         (const float*)ws, S, bias, y, mn, F);
    if (rc) return rc;
  }
  return iic_launch_status();
}

// dx1_pt is written at Q = 2 only
int lin_bwd_dx(const void* dyb, const void* wt, void* dx0_pt, void* dx1_pt, const lin_shape& s, void* stream) {
  if (!lin_shape_ok(s)) return IIC_ERR_UNSUPPORTED;
  const int N = s.N, F = s.F, K = s.H * s.W * s.C;
  const sup_mat A = sup_flat(dyb, N, F);
  dim3 grid((N + TM - 1) / TM, (K + TN - 1) / TN, 1);
  for (int q = 0; q < s.Q; ++q) {
    const sup_mat B = sup_flat((const bf16_t*)wt + (long)q * K * F, K, F),
                  o = sup_pt(q ? dx1_pt : dx0_pt, N, s.H, s.W, s.C);
    int rc = iic_launch_lds<sup_gemm_kernel<true>>(grid, dim3(256), GEMM_LDS, (hipStream_t)stream, A, A, F / BK, B, F,
                                                   (const float*)nullptr, (float*)nullptr, 0L, o);
    if (rc) return rc;
  }
  return iic_launch_status();
}

// a1_pt is read at Q = 2 only
int lin_wgrad(const void* dyt, const void* a0_pt, const void* a1_pt, float* dW, const lin_shape& s, void* stream) {
  if (!lin_shape_ok(s)) return IIC_ERR_UNSUPPORTED;
  const int N = s.N, F = s.F, C = s.C, Np = (N + 63) / 64 * 64, HW = s.H * s.W;
  const long K = (long)HW * C;
  if ((HW + 15) / 16 > 65535 || C / 8 > 65535) return IIC_ERR_UNSUPPORTED;
  const sup_mat A = sup_flat(dyt, F, Np);
  dim3 grid((F + TM - 1) / TM, C / 8, (HW + 15) / 16);
  for (int q = 0; q < s.Q; ++q) {
    int rc = iic_launch_lds<sup_wgrad_kernel>(grid, dim3(256), GEMM_LDS, (hipStream_t)stream, A,
                                              (const bf16_t*)(q ? a1_pt : a0_pt), (long)(s.H + 2) * (s.W + 2) * C, N, s.H,
                                              s.W, C, dW + q * K, s.Q * K);
    if (rc) return rc;
  }
  return iic_launch_status();
}

}  // namespace

extern "C" {

int iic_sup_weight_prep(const float* w, void* wb, void* wt, int F, int C, int H, int W, void* stream) {
  if (!w || !wb || !wt) return IIC_ERR_ARG;
  return lin_weight_prep(w, wb, wt, lin_shape{1, F, C, H, W, 1}, stream);
}

int iic_sup_fwd_nsplit(int N, int F, int C, int H, int W) {
  const lin_shape s{N, F, C, H, W, 1};
  return lin_shape_ok(s) ? lin_nsplit(s) : 0;
}

int iic_sup_linear_fwd(const void* x_pt, const void* wb, const float* bias, float* y, float* ws, int N, int F, int C, int H,
                       int W, void* stream) {
  if (!x_pt || !wb || !y) return IIC_ERR_ARG;
  return lin_fwd(x_pt, nullptr, wb, bias, y, ws, lin_shape{N, F, C, H, W, 1}, stream);
}

int iic_sup_dy_cast(const float* dy, void* dyb, void* dyt, int N, int F, void* stream) {
  if (!dy || !dyb || !dyt || N < 1 || F < 1) return IIC_ERR_ARG;
  const int Np = (N + 63) / 64 * 64;
  int rc = iic_launch_lds<sup_dy_cast_kernel>(dim3((F + 31) / 32, Np / 32), dim3(256), 0, (hipStream_t)stream, dy,
                                              (bf16_t*)dyb, (bf16_t*)dyt, N, F, Np);
  if (rc) return rc;
  return iic_launch_status();
}

int iic_sup_linear_bwd_dx(const void* dyb, const void* wt, void* dx_pt, int N, int F, int C, int H, int W, void* stream) {
  if (!dyb || !wt || !dx_pt) return IIC_ERR_ARG;
  return lin_bwd_dx(dyb, wt, dx_pt, nullptr, lin_shape{N, F, C, H, W, 1}, stream);
}

int iic_sup_linear_wgrad(const void* dyt, const void* x_pt, float* dW, int N, int F, int C, int H, int W, void* stream) {
  if (!dyt || !x_pt || !dW) return IIC_ERR_ARG;
  return lin_wgrad(dyt, x_pt, nullptr, dW, lin_shape{N, F, C, H, W, 1}, stream);
}

int iic_sup_bn_relu_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float* y, float* save_mean, float* save_invstd, int N, int F, int training, float momentum,
                        float eps, void* stream) {
  if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || N < 1 || F < 1) return IIC_ERR_ARG;
  if (training && N < 2) return IIC_ERR_ARG;                 // one value per channel: no batch variance
  if (!training && (!running_mean || !running_var)) return IIC_ERR_ARG;
  if ((running_mean == nullptr) != (running_var == nullptr)) return IIC_ERR_ARG;
  int rc = iic_launch_lds<sup_bn_relu_fwd_kernel>(dim3((F + 31) / 32), dim3(256), 0, (hipStream_t)stream, x, gamma, beta,
                                                  running_mean, running_var, y, save_mean, save_invstd, N, F, training,
                                                  momentum, eps);
  if (rc) return rc;
  return iic_launch_status();
}

int iic_sup_bn_relu_bwd(const float* dout, const float* x, const float* y, const float* gamma, const float* save_mean,
                        const float* save_invstd, float* dx, float* dgamma, float* dbeta, int N, int F, int training,
                        void* stream) {
  if (!dout || !x || !y || !gamma || !save_mean || !save_invstd || !dx || !dgamma || !dbeta || N < 1 || F < 1)
    return IIC_ERR_ARG;
  int rc = iic_launch_lds<sup_bn_relu_bwd_kernel>(dim3((F + 31) / 32), dim3(256), 0, (hipStream_t)stream, dout, x, y, gamma,
                                                  save_mean, save_invstd, dx, dgamma, dbeta, N, F, training);
  if (rc) return rc;
  return iic_launch_status();
}

int iic_sup_cross_entropy(const float* logits, const long long* targets, float* loss, float* dlogits, int N, int k,
                          void* stream) {
  if (!logits || !targets || !loss || !dlogits || N < 1 || k < 1) return IIC_ERR_ARG;
  int rc = iic_launch_lds<sup_cross_entropy_kernel>(dim3(1), dim3(256), 0, (hipStream_t)stream, logits, targets, loss,
                                                    dlogits, N, k);
  if (rc) return rc;
  return iic_launch_status();
}

int iic_sup_tencrop_acc(const float* logits, const long long* targets, long long* counts, int B, int k, int crops,
                        void* stream) {
  if (!logits || !targets || !counts || B < 1 || k < 1 || crops < 1) return IIC_ERR_ARG;
  int rc = iic_launch_lds<sup_tencrop_acc_kernel>(dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, logits, targets,
                                                  (unsigned long long*)counts, B, k, crops);
  if (rc) return rc;
  return iic_launch_status();
}

// ---- the joint Linear of the Isola / Doersch heads (iic_hip.h: iic_pair_*): the same routines at Q = 2, H = W = p ----

int iic_pair_weight_prep(const float* w, void* wb, void* wt, int F, int C, int p, void* stream) {
  if (!w || !wb || !wt) return IIC_ERR_ARG;
  return lin_weight_prep(w, wb, wt, lin_shape{1, F, C, p, p, 2}, stream);
}

int iic_pair_linear_fwd_nsplit(int N, int F, int C, int p) {
  const lin_shape s{N, F, C, p, p, 2};
  return lin_shape_ok(s) ? lin_nsplit(s) : 0;
}

int iic_pair_linear_fwd(const void* a0_pt, const void* a1_pt, const void* wb, const float* bias, float* y, float* ws, int N,
                        int F, int C, int p, void* stream) {
  if (!a0_pt || !a1_pt || !wb || !y) return IIC_ERR_ARG;
  return lin_fwd(a0_pt, a1_pt, wb, bias, y, ws, lin_shape{N, F, C, p, p, 2}, stream);
}

int iic_pair_linear_bwd_dx(const void* dyb, const void* wt, void* dx0_pt, void* dx1_pt, int N, int F, int C, int p,
                           void* stream) {
  if (!dyb || !wt || !dx0_pt || !dx1_pt) return IIC_ERR_ARG;
  return lin_bwd_dx(dyb, wt, dx0_pt, dx1_pt, lin_shape{N, F, C, p, p, 2}, stream);
}

int iic_pair_linear_wgrad(const void* dyt, const void* a0_pt, const void* a1_pt, float* dW, int N, int F, int C, int p,
                          void* stream) {
  if (!dyt || !a0_pt || !a1_pt || !dW) return IIC_ERR_ARG;
  return lin_wgrad(dyt, a0_pt, a1_pt, dW, lin_shape{N, F, C, p, p, 2}, stream);
}

}  // extern "C"
