// The bilinear up-sampling arithmetic of bilinear_fwd_kernel (seg_head.hip), shared by the kernels that interpolate
// single pixels of a PT feature tensor: seg_kmeans.hip (sampled rows, label maps) and seg_patches.hip (the baselines'
// patch sampler).
#pragma once
#include "common.h"

// The interpolated numbers must be the very ones bilinear_fwd_kernel stores: pinned operation by operation as
// seg_eval.hip pins them (see the note there), not left to -ffp-contract.
__device__ __forceinline__ void sk_src(int d, float scale, int in, int& i0, int& i1, float& lam) {
#pragma clang fp contract(off)
  float s = __builtin_fmaf((float)d + 0.5f, scale, -0.5f);
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = s - (float)i0;
}

__device__ __forceinline__ float sk_blend(float v00, float v01, float v10, float v11, float lx, float ly) {
#pragma clang fp contract(off)
  const float top = __builtin_fmaf(v01, lx, v00 * (1.f - lx));
  const float bot = __builtin_fmaf(v10, 1.f - lx, v11 * lx);
  return (1.f - ly) * top + ly * bot;
}

template <typename T>
__device__ __forceinline__ float sk_ld(const T* p);
template <>
__device__ __forceinline__ float sk_ld<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }
template <>
__device__ __forceinline__ float sk_ld<float>(const float* p) { return *p; }

