// General affine warp + whole-batch integer shift of the segmentation loss's second view:
//   perform_affine_tf          /root/reference/code/utils/segmentation/transforms.py:131-143
//                              (F.affine_grid + F.grid_sample, bilinear, zero padding)
//   random_translation_multiple  transforms.py:145-165 (zero pad + crop = shift with zero fill)
// Every published run uses identity / x-flip matrices and no sparse shift; those stay folded into
// the joint / gradient kernels' index arithmetic (seg_loss.hip).  This file is the general case.
//
// The host converts theta (normalised coordinates) to a pixel-space matrix per sample
// (iic_amd/seg_losses.py::_pixel_matrices): source pixel (ix, iy) = M * (ox, oy, 1).
//   out[n][k][oy][ox] = 0                                   if (oy + sy, ox + sx) is outside the image
//                     = bilinear(x[n][k], M_n * (ox + sx, oy + sy, 1))  otherwise (zeros outside)
// NCHW fp32 (the loss inputs are the fp32 softmax maps).  HBM-bound: one read + one write per element.
//
// Two backward kernels.  affine_warp_bwd_gather_kernel (the product path, seg_losses._AffineWarpFn): one thread per
// source pixel gathers its contributors in ascending (oy, ox), acc = fl32(acc + fl32(w g)) from +0.0f, no atomics --
// bit-reproducible; it serves matrices whose search box is at most IIC_WARP_GATHER_CAP = 8 positions in each direction
// (include/iic_hip.h has the condition; every matrix of the reference's random_affine qualifies).
// affine_warp_bwd_kernel: zero-fill + float-atomic scatter, any matrix; the backward of what the gather kernel refuses.
#include "common.h"
#include "../../include/iic_hip.h"

struct WarpTap {
  int o00, o01, o10, o11;      // offsets inside one (n, k) plane, -1 = outside
  float w00, w01, w10, w11;
};

// The bilinear taps of the sampling point M (qx, qy, 1), (qx, qy) inside the image: the one routine of the forward, of the
// atomic backward and of the gather backward's membership test.  m = the sample's row of six.
__device__ __forceinline__ void warp_taps_at(const float* __restrict__ m, int qx, int qy, int H, int W, WarpTap& t) {
  // coordinates in double: the reference's float64 runs are the parity target.  A float32 entry times a pixel index is
  // exact in double, so the value is round(round(m0 qx + m1 qy) + m2) with or without fused multiply-adds as long as the
  // sum keeps this association; contraction off pins it (the host emulation of tests/warp_gather_cases.py follows it)
#pragma clang fp contract(off)
  const double fx = (double)m[0] * qx + (double)m[1] * qy + (double)m[2];
  const double fy = (double)m[3] * qx + (double)m[4] * qy + (double)m[5];
  const double x0d = floor(fx), y0d = floor(fy);
  // no tap inside the image (a NaN coordinate included): all four outside, weights 0.  One straight line of selects --
  // an early return here made the compiler keep two of the weights in a stack slot.
  const bool any = x0d >= -1.0 && x0d < (double)W && y0d >= -1.0 && y0d < (double)H;
  const int x0 = any ? (int)x0d : -1, y0 = any ? (int)y0d : -1;
  const float ax = (float)(fx - x0d), ay = (float)(fy - y0d);
  const bool vx0 = any && x0 >= 0, vx1 = any && x0 + 1 < W, vy0 = y0 >= 0, vy1 = y0 + 1 < H;
  t.o00 = (vx0 && vy0) ? y0 * W + x0 : -1;
  t.o01 = (vx1 && vy0) ? y0 * W + x0 + 1 : -1;
  t.o10 = (vx0 && vy1) ? (y0 + 1) * W + x0 : -1;
  t.o11 = (vx1 && vy1) ? (y0 + 1) * W + x0 + 1 : -1;
  t.w00 = any ? (1.f - ax) * (1.f - ay) : 0.f;
  t.w01 = any ? ax * (1.f - ay) : 0.f;
  t.w10 = any ? (1.f - ax) * ay : 0.f;
  t.w11 = any ? ax * ay : 0.f;
}

__device__ __forceinline__ bool warp_taps(const float* __restrict__ M, int n, int oy, int ox, int H, int W,
                                          int sx, int sy, WarpTap& t) {
  const int qx = ox + sx, qy = oy + sy;
  if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
  warp_taps_at(M + (long)n * 6, qx, qy, H, W, t);
  return true;
}

__global__ __launch_bounds__(256) void affine_warp_fwd_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ M,
                                                              float* __restrict__ out, int N, int K, int H,
                                                              int W, int sx, int sy) {
  const long hw = (long)H * W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * hw) return;
  const int n = (int)(i / hw);
  const int r = (int)(i - (long)n * hw);
  const int oy = r / W, ox = r - oy * W;
  WarpTap t;
  const bool inside = warp_taps(M, n, oy, ox, H, W, sx, sy, t);
  const float* xp = x + (long)n * K * hw;
  float* op = out + (long)n * K * hw + r;
  for (int k = 0; k < K; ++k) {
    float v = 0.f;
    if (inside) {
      if (t.o00 >= 0) v += t.w00 * xp[t.o00];
      if (t.o01 >= 0) v += t.w01 * xp[t.o01];
      if (t.o10 >= 0) v += t.w10 * xp[t.o10];
      if (t.o11 >= 0) v += t.w11 * xp[t.o11];
    }
    op[(long)k * hw] = v;
    xp += hw;
  }
}

// dx (zeroed here) += scatter of dout through the same taps.  Float atomics: the order of the
// (at most a few) contributions to one source pixel is not fixed -- the one kernel of the library
// whose result is not bit-reproducible; the loss reaches it only for matrices the gather kernel below refuses.
__global__ __launch_bounds__(256) void affine_warp_bwd_kernel(const float* __restrict__ dout,
                                                              const float* __restrict__ M,
                                                              float* __restrict__ dx, int N, int K, int H,
                                                              int W, int sx, int sy) {
  const long hw = (long)H * W;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * hw) return;
  const int n = (int)(i / hw);
  const int r = (int)(i - (long)n * hw);
  const int oy = r / W, ox = r - oy * W;
  WarpTap t;
  if (!warp_taps(M, n, oy, ox, H, W, sx, sy, t)) return;
  const float* gp = dout + (long)n * K * hw + r;
  float* dp = dx + (long)n * K * hw;
  for (int k = 0; k < K; ++k) {
    const float g = gp[(long)k * hw];
    if (g != 0.f) {
      if (t.o00 >= 0) atomicAdd(dp + t.o00, t.w00 * g);
      if (t.o01 >= 0) atomicAdd(dp + t.o01, t.w01 * g);
      if (t.o10 >= 0) atomicAdd(dp + t.o10, t.w10 * g);
      if (t.o11 >= 0) atomicAdd(dp + t.o11, t.w11 * g);
    }
    dp += hw;
  }
}

// ---- the same adjoint as a gather: fixed summation order, no atomics, no zero-fill -------------------------------------------
// One thread owns the source pixel (n, v, u) and writes dx[n][k][v][u] for every k.  The output pixels that tap it have
// their sampling point M (qx, qy, 1) in [u-1, u+1) x [v-1, v+1); the preimage of that square is a parallelogram whose
// bounding box follows from the inverse of M's 2x2 part (include/iic_hip.h states the formulas and the cap).  The box only
// bounds the search: at each of its positions the forward's own warp_taps_at decides whether one of the four taps IS this
// pixel, and with which float32 weight.  The geometry does not depend on k, so it is found once -- a 64-bit membership
// mask and CAP x CAP weights, held in registers (every index below is a compile-time constant: no scratch) -- and the
// channel loop streams dout through it: contributors in ascending (oy, ox), acc = +0.0f, acc = fl32(acc + fl32(w g)).
// Neighbouring threads own neighbouring pixels: their boxes are translates of one another by the columns of the inverse,
// so one row of a wave's boxes reads a near-contiguous span of dout, and the dx stores are coalesced.
static constexpr int WARP_CAP = IIC_WARP_GATHER_CAP;
static constexpr double WARP_SLACK = 1.0 / 64;
static_assert(WARP_CAP == 8, "one byte of the membership mask per row of the box");

// Half-extents of the box, slack included; false for a matrix the gather kernel does not serve (singular, non-finite,
// or a box beyond the cap).  Host and device: the launch's refusal and the kernel's box are the same arithmetic.
__host__ __device__ inline bool warp_gather_extents(const float* m, double& ex, double& ey) {
  const double a = m[0], b = m[1], c = m[3], d = m[4];
  const double det = a * d - b * c;
  ex = (fabs(d) + fabs(b)) / fabs(det) + WARP_SLACK;
  ey = (fabs(c) + fabs(a)) / fabs(det) + WARP_SLACK;
  // (written so that a NaN anywhere refuses)
  return det != 0.0 && 2.0 * ex + 1.0 < (double)WARP_CAP && 2.0 * ey + 1.0 < (double)WARP_CAP &&
         fabs((double)m[2]) <= 3.0e38 && fabs((double)m[5]) <= 3.0e38;
}

// acc = fl32(acc + fl32(w g)): two roundings.  (__fmul_rn / __fadd_rn are plain * and + to this compiler and fuse into
// one v_fma_f32 like any other; the pragma is what keeps them apart.)
__device__ __forceinline__ float warp_gather_step(float acc, float w, float g) {
#pragma clang fp contract(off)
  const float p = w * g;
  return acc + p;
}

__global__ __launch_bounds__(256) void affine_warp_bwd_gather_kernel(const float* __restrict__ dout,
                                                                     const float* __restrict__ M,
                                                                     float* __restrict__ dx, int N, int K, int H,
                                                                     int W, int sx, int sy) {
  const long hw = (long)H * W;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)N * hw) return;
  const int n = (int)(idx / hw);
  const int r = (int)(idx - (long)n * hw);
  const int v = r / W, u = r - v * W;
  const float* m = M + (long)n * 6;
  double ex, ey;
  warp_gather_extents(m, ex, ey);        // (the launch has refused what this refuses)
  const double det = (double)m[0] * m[4] - (double)m[1] * m[3];
  const double du = (double)u - (double)m[2], dv = (double)v - (double)m[5];
  const double cx = ((double)m[4] * du - (double)m[1] * dv) / det;
  const double cy = ((double)m[0] * dv - (double)m[3] * du) / det;
  // positions q whose output pixel q - (sx, sy) exists: the clamp of the box.  An empty box has lo = hi + 1.
  const int qx_min = max(0, sx), qx_max = min(W - 1, W - 1 + sx);
  const int qy_min = max(0, sy), qy_max = min(H - 1, H - 1 + sy);
  const int x_lo = (int)fmin(fmax(ceil(cx - ex), (double)qx_min), (double)qx_max + 1.0);
  const int y_lo = (int)fmin(fmax(ceil(cy - ey), (double)qy_min), (double)qy_max + 1.0);
  const int x_hi = min((int)fmax(fmin(floor(cx + ex), (double)qx_max), (double)x_lo - 1.0), x_lo + WARP_CAP - 1);
  const int y_hi = min((int)fmax(fmin(floor(cy + ey), (double)qy_max), (double)y_lo - 1.0), y_lo + WARP_CAP - 1);

  float wgt[WARP_CAP * WARP_CAP];
  unsigned rows[WARP_CAP];              // bit i of rows[j]: box position (x_lo + i, y_lo + j) taps this pixel
#pragma unroll
  for (int j = 0; j < WARP_CAP; ++j) {
    rows[j] = 0u;
#pragma unroll
    for (int i = 0; i < WARP_CAP; ++i) wgt[j * WARP_CAP + i] = 0.f;
  }
  // a rolled loop over the rows (sixty-four unrolled copies of the double-precision taps keep hundreds of registers
  // live); j is uniform, so filing a row under its compile-time index below is a scalar choice
#pragma unroll 1
  for (int j = 0; j < WARP_CAP; ++j) {
    float w[WARP_CAP];
    unsigned bits = 0u;
#pragma unroll
    for (int i = 0; i < WARP_CAP; ++i) {
      w[i] = 0.f;
      if (y_lo + j <= y_hi && x_lo + i <= x_hi) {
        WarpTap t;
        warp_taps_at(m, x_lo + i, y_lo + j, H, W, t);
        const bool hit = t.o00 == r || t.o01 == r || t.o10 == r || t.o11 == r;
        w[i] = t.o00 == r ? t.w00 : t.o01 == r ? t.w01 : t.o10 == r ? t.w10 : t.w11;
        if (hit) bits |= 1u << i;
      }
    }
#pragma unroll
    for (int jj = 0; jj < WARP_CAP; ++jj) {
      if (jj == j) {
        rows[jj] = bits;
#pragma unroll
        for (int i = 0; i < WARP_CAP; ++i) wgt[jj * WARP_CAP + i] = w[i];
      }
    }
  }

  // Offset, inside a plane, of the output pixel of box position (0, 0).  Every position of the clamped box has its output
  // pixel inside the image, and a row with members is a row of the box: its loads are unconditional, columns past the
  // box's last re-read that one (col[]), and issue together; what a non-member reads is not used.
  const long base = (long)(y_lo - sy) * W + (x_lo - sx);
  int col[WARP_CAP];
#pragma unroll
  for (int i = 0; i < WARP_CAP; ++i) col[i] = min(i, x_hi - x_lo);
  long plane = (long)n * K * hw;
  for (int k = 0; k < K; ++k) {
    // the box's origin in this plane, opaque to the optimiser: left to itself it carries the sixty-four addresses of
    // the box through the loop, 128 registers, instead of adding a row and a column offset per load
    long origin = plane + base;
    asm volatile("" : "+v"(origin));
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < WARP_CAP; ++j) {
      if (rows[j]) {
        const float* rp = dout + (origin + (long)j * W);
        float g[WARP_CAP];
#pragma unroll
        for (int i = 0; i < WARP_CAP; ++i) g[i] = rp[col[i]];
#pragma unroll
        for (int i = 0; i < WARP_CAP; ++i)
          if (rows[j] >> i & 1u) acc = warp_gather_step(acc, wgt[j * WARP_CAP + i], g[i]);
      }
    }
    dx[plane + r] = acc;
    plane += hw;
  }
}

extern "C" {

int iic_affine_warp_gather_supported(const float* host_mats, int N) {
  if (!host_mats || N <= 0) return 0;
  for (int n = 0; n < N; ++n) {
    double ex, ey;
    if (!warp_gather_extents(host_mats + (long)n * 6, ex, ey)) return 0;
  }
  return 1;
}

int iic_affine_warp_bwd_gather(const float* dout, const float* pixel_mats, const float* host_mats, float* dx, int N,
                               int K, int H, int W, int shift_x, int shift_y, void* stream) {
  if (!dout || !pixel_mats || !host_mats || !dx || N <= 0 || K <= 0 || H <= 0 || W <= 0) return IIC_ERR_ARG;
  if (!iic_affine_warp_gather_supported(host_mats, N)) return IIC_ERR_UNSUPPORTED;
  const long total = (long)N * H * W;
  hipLaunchKernelGGL(affine_warp_bwd_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, dout, pixel_mats, dx, N, K, H, W, shift_x, shift_y);
  return iic_launch_status();
}

int iic_affine_warp_fwd(const float* x, const float* pixel_mats, float* out, int N, int K, int H, int W,
                        int shift_x, int shift_y, void* stream) {
  if (!x || !pixel_mats || !out || N <= 0 || K <= 0 || H <= 0 || W <= 0) return IIC_ERR_ARG;
  const long total = (long)N * H * W;
  hipLaunchKernelGGL(affine_warp_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, x, pixel_mats, out, N, K, H, W, shift_x, shift_y);
  return iic_launch_status();
}

int iic_affine_warp_bwd(const float* dout, const float* pixel_mats, float* dx, int N, int K, int H, int W,
                        int shift_x, int shift_y, void* stream) {
  if (!dout || !pixel_mats || !dx || N <= 0 || K <= 0 || H <= 0 || W <= 0) return IIC_ERR_ARG;
  const long total = (long)N * H * W;
  if (iic_zero_async(dx, (size_t)total * K * sizeof(float), (hipStream_t)stream) != IIC_OK) return IIC_ERR_LAUNCH;
  hipLaunchKernelGGL(affine_warp_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, dout, pixel_mats, dx, N, K, H, W, shift_x, shift_y);
  return iic_launch_status();
}

}  // extern "C"
