// The arithmetic of OpenCV 3.x's resize (modules/imgproc/src/resize.cpp) that the segmentation kernels share:
// seg_augment.hip multiplies and adds host-built taps, seg_prescale.hip also computes the coefficients itself.
// Every operation is rounded on its own, as cv2's scalar code does: contraction is off from here to the end of the
// including file (augment.hip explains why a fused multiply-add changes the bytes).
#pragma once
#include <stdint.h>

#pragma clang fp contract(off)

// (a * wa + b * wb), every operation rounded to float32
__device__ __forceinline__ float seg_lerp(float a, float wa, float b, float wb) { return a * wa + b * wb; }

__device__ __forceinline__ int seg_trunc_u8(float v) {
  const int i = (int)v;          // toward zero, as astype(np.uint8) of a value in [0, 256)
  return i < 0 ? 0 : (i > 255 ? 255 : i);
}

// INTER_LINEAR along one side of `len` source pixels for destination index d >= 0, inv = 1. / scale in double:
// f = float32((d + 0.5) * inv - 0.5), the product and the difference in double; floor, the low and high clamps and
// a0 = 1.f - f in float32 -- bit-equal to iic_amd/seg_ragged.py::linear_taps.  1 <= len <= 16384.
struct seg_linear_tap {
  int i0, i1;
  float a0, a1;
};
__device__ __forceinline__ seg_linear_tap seg_linear_coeff(int d, double inv, int len) {
  float f = (float)(((double)d + 0.5) * inv - 0.5);
  const float fl = floorf(f);
  f = f - fl;
  int s;
  if (fl < 0.f) {
    s = 0; f = 0.f;
  } else if (fl >= (float)(len - 1)) {         // also every position too large for an int
    s = len - 1; f = 0.f;
  } else {
    s = (int)fl;
  }
  seg_linear_tap t;
  t.i0 = s;
  t.i1 = s + 1 < len ? s + 1 : len - 1;
  t.a0 = 1.f - f;
  t.a1 = f;
  return t;
}

// INTER_NEAREST along one side: min(floor(d * inv), len - 1) in double (seg_ragged.py::nearest_index)
__device__ __forceinline__ int seg_nearest_coeff(int d, double inv, int len) {
  const double v = floor((double)d * inv);
  return v >= (double)(len - 1) ? len - 1 : (int)v;
}
