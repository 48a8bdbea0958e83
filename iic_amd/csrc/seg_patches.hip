// Patch sampler of the Isola and Doersch segmentation baselines for gfx950: the two p x p patches of the bilinearly
// up-sampled trunk features, interpolated pixel by pixel from the PT feature tensor, and the adjoint.
//
// Replaces, in code/archs/segmentation/baselines/net10a_isola.py:91-96 and net10a_doersch.py:84-89,
//   x = F.interpolate(x, size=self.input_sz, mode="bilinear")          -- fp32 [N][512][S][S], 6.1 GB per Potsdam batch
//   patches1, patches2 = get_patches(x, centre, other, patch_side)     -- code/utils/segmentation/baselines/general.py:4-18
// and their backward nodes (the slice's zero-filled [N][512][S][S] gradient and the interpolation's backward over it).
// Only the 2 p p pixels per image that the patches hold are interpolated; the up-sampled map exists in neither direction.
//
//   seg_patch_fwd_kernel  a workgroup per output row (image q N + n, row i of p + 2): the four PT neighbours of every
//       patch pixel blended with the operations of bilinear_fwd_kernel (seg_bilinear.h), stored in the source's dtype
//       (bf16: one round-to-nearest-even); border rows and columns are written as zeros.
//   seg_patch_bwd_kernel  a workgroup per source row (n, ys), a thread per two channels of a source pixel: a GATHER.  The
//       coefficient of source pixel (ys, xs) in patch pixel (i, j) is wy(i) wx(j),
//           wy(i) = [y0(i) == ys] (1 - ly(i)) + [y1(i) == ys] ly(i),     wx(j) likewise,
//       each a single fp32 sum (both taps fall on one row / column where the clamp at the far edge folds them), their
//       product rounded once, and   acc <- acc + g[q][i][j] * (wy(i) wx(j))   with product and sum rounded separately, in
//       the FIXED ORDER: centre patch (q = 0) before other patch (q = 1), inside a patch the pixels in ascending (i, j).
//       Patch pixels whose taps do not touch (ys, xs) are skipped, not added as zeros.  Every interior element is written
//       exactly once (zeros outside both footprints), the border never.  No atomics: two calls give the same bits.
// The coordinate block lives on the device -- a captured step can be replayed with new patches -- so the kernels clamp
// the centres into [d, S - 1 - d], d = p / 2; the host wrapper (iic_amd/archs/seg_baselines.py) validates and raises.
#include "common.h"
#include "../../include/iic_hip.h"
#include "seg_bilinear.h"

namespace {

constexpr int SP_PMAX = 127;      // patch side served (odd)

template <typename T>
__device__ __forceinline__ void sp_st(T* p, float v);
template <>
__device__ __forceinline__ void sp_st<bf16_t>(bf16_t* p, float v) { *p = f32_to_bf16(v); }
template <>
__device__ __forceinline__ void sp_st<float>(float* p, float v) { *p = v; }

template <typename T>
__device__ __forceinline__ void sp_st2(T* p, float a, float b);
template <>
__device__ __forceinline__ void sp_st2<bf16_t>(bf16_t* p, float a, float b) {
  *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(a, b);
}
template <>
__device__ __forceinline__ void sp_st2<float>(float* p, float a, float b) {
  const f32x2 v = {a, b};
  *reinterpret_cast<f32x2*>(p) = v;
}

__device__ __forceinline__ int sp_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <typename T>
__global__ __launch_bounds__(256) void seg_patch_fwd_kernel(const T* __restrict__ pt, const int* __restrict__ blk,
                                                            T* __restrict__ out, int N, int Hl, int Wl, int Hp, int Wp,
                                                            int off, int C, int S, int p) {
  const int pp = p + 2, d = p >> 1;
  const int i = blockIdx.x % pp, qn = blockIdx.x / pp;
  const int q = qn >= N ? 1 : 0, n = qn - q * N;
  T* const orow = out + ((long)qn * pp + i) * pp * C;
  const int run = pp * C;
  if (i == 0 || i == pp - 1) {
    for (int e = threadIdx.x; e < run; e += 256) sp_st<T>(orow + e, 0.f);
    return;
  }
  const float sy = (float)Hl / (float)S, sx = (float)Wl / (float)S;
  const int cy = sp_clamp(blk[2 * q], d, S - 1 - d), cx = sp_clamp(blk[2 * q + 1], d, S - 1 - d);
  int y0, y1;
  float ly;
  sk_src(cy - d + i - 1, sy, Hl, y0, y1, ly);
  const T* const r0 = pt + ((long)n * Hp + y0 + off) * Wp * C;
  const T* const r1 = pt + ((long)n * Hp + y1 + off) * Wp * C;
  for (int e = threadIdx.x; e < run; e += 256) {
    const int j = e / C, c = e - j * C;
    float v = 0.f;
    if (j != 0 && j != pp - 1) {
      int x0, x1;
      float lx;
      sk_src(cx - d + j - 1, sx, Wl, x0, x1, lx);
      const long c0 = (long)(x0 + off) * C + c, c1 = (long)(x1 + off) * C + c;
      v = sk_blend(sk_ld<T>(r0 + c0), sk_ld<T>(r0 + c1), sk_ld<T>(r1 + c0), sk_ld<T>(r1 + c1), lx, ly);
    }
    sp_st<T>(orow + e, v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void seg_patch_bwd_kernel(const T* __restrict__ dc, const T* __restrict__ dother,
                                                            const int* __restrict__ blk, T* __restrict__ dx, int N, int Hl,
                                                            int Wl, int Hp, int Wp, int off, int C, int S, int p) {
#pragma clang fp contract(off)
  __shared__ float s_wy[2][SP_PMAX + 1], s_lx[2][SP_PMAX + 1];
  __shared__ int s_x0[2][SP_PMAX + 1], s_x1[2][SP_PMAX + 1];
  __shared__ int s_rows[2][SP_PMAX + 1], s_nrows[2];
  __shared__ unsigned char s_my[2][SP_PMAX + 1];
  const int pp = p + 2, d = p >> 1;
  const int n = blockIdx.x / Hl, ys = blockIdx.x - n * Hl;
  const float sy = (float)Hl / (float)S, sx = (float)Wl / (float)S;
  for (int t = threadIdx.x; t < 2 * p; t += 256) {
    const int q = t / p, i = t - q * p;
    const int cy = sp_clamp(blk[2 * q], d, S - 1 - d), cx = sp_clamp(blk[2 * q + 1], d, S - 1 - d);
    int y0, y1, x0, x1;
    float ly, lx;
    sk_src(cy - d + i, sy, Hl, y0, y1, ly);
    sk_src(cx - d + i, sx, Wl, x0, x1, lx);
    s_wy[q][i] = (y0 == ys ? 1.f - ly : 0.f) + (y1 == ys ? ly : 0.f);
    s_my[q][i] = (y0 == ys || y1 == ys) ? 1 : 0;
    s_x0[q][i] = x0;
    s_x1[q][i] = x1;
    s_lx[q][i] = lx;
  }
  __syncthreads();
  if (threadIdx.x < 2) {      // the patch rows that touch this source row, ascending
    const int q = threadIdx.x;
    int cnt = 0;
    for (int i = 0; i < p; ++i)
      if (s_my[q][i]) s_rows[q][cnt++] = i;
    s_nrows[q] = cnt;
  }
  __syncthreads();
  const int half = C >> 1, items = Wl * half;
  T* const orow = dx + (((long)n * Hp + ys + off) * Wp + off) * C;
  for (int e = threadIdx.x; e < items; e += 256) {
    const int xs = e / half, c = 2 * (e - xs * half);
    float a0 = 0.f, a1 = 0.f;
    for (int q = 0; q < 2; ++q) {
      const int nr = s_nrows[q];
      if (nr == 0 || xs < s_x0[q][0] || xs > s_x1[q][p - 1]) continue;
      const T* const g = (q ? dother : dc) + (long)n * pp * pp * C + c;
      for (int r = 0; r < nr; ++r) {
        const int i = s_rows[q][r];
        const float wy = s_wy[q][i];
        for (int j = 0; j < p; ++j) {
          const int x0 = s_x0[q][j], x1 = s_x1[q][j];
          if (x0 != xs && x1 != xs) continue;
          const float lx = s_lx[q][j];
          const float wx = (x0 == xs ? 1.f - lx : 0.f) + (x1 == xs ? lx : 0.f);
          const float w = wy * wx;
          const T* const gp = g + ((long)(i + 1) * pp + (j + 1)) * C;
          a0 = a0 + sk_ld<T>(gp) * w;
          a1 = a1 + sk_ld<T>(gp + 1) * w;
        }
      }
    }
    sp_st2<T>(orow + (long)xs * C + c, a0, a1);
  }
}

bool sp_shape_ok(int N, int Hl, int Wl, int Hp, int Wp, int off, int C, int S, int p) {
  return N >= 1 && Hl >= 1 && Wl >= 1 && C >= 2 && (C & 1) == 0 && off >= 0 && S >= 1 && p >= 1 && (p & 1) == 1 &&
         p <= SP_PMAX && p <= S && (long)2 * N * (p + 2) < 0x7fffffffL && (long)N * Hl < 0x7fffffffL &&
         (long)(p + 2) * C < 0x7fffffffL && (long)Wl * C < 0x7fffffffL;
}

}  // namespace

extern "C" {

int iic_seg_patch_sample_fwd(const void* pt, int pt_is_f32, const int* coords, void* patches, int N, int Hl, int Wl, int Hp,
                             int Wp, int off, int C, int S, int p, void* stream) {
  if (!pt || !coords || !patches || off < 0 || Hl + off > Hp || Wl + off > Wp) return IIC_ERR_ARG;
  if (!sp_shape_ok(N, Hl, Wl, Hp, Wp, off, C, S, p)) return IIC_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(2 * N * (p + 2)));
  if (pt_is_f32)
    hipLaunchKernelGGL(seg_patch_fwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)pt, coords,
                       (float*)patches, N, Hl, Wl, Hp, Wp, off, C, S, p);
  else
    hipLaunchKernelGGL(seg_patch_fwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pt, coords,
                       (bf16_t*)patches, N, Hl, Wl, Hp, Wp, off, C, S, p);
  return iic_launch_status();
}

int iic_seg_patch_sample_bwd(const void* dcentre, const void* dother, int pt_is_f32, const int* coords, void* dx_pt, int N,
                             int Hl, int Wl, int Hp, int Wp, int off, int C, int S, int p, void* stream) {
  if (!dcentre || !dother || !coords || !dx_pt || off < 0 || Hl + off > Hp || Wl + off > Wp) return IIC_ERR_ARG;
  if (!sp_shape_ok(N, Hl, Wl, Hp, Wp, off, C, S, p)) return IIC_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(N * Hl));
  if (pt_is_f32)
    hipLaunchKernelGGL(seg_patch_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dcentre,
                       (const float*)dother, coords, (float*)dx_pt, N, Hl, Wl, Hp, Wp, off, C, S, p);
  else
    hipLaunchKernelGGL(seg_patch_bwd_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dcentre,
                       (const bf16_t*)dother, coords, (bf16_t*)dx_pt, N, Hl, Wl, Hp, Wp, off, C, S, p);
  return iic_launch_status();
}

}  // extern "C"
