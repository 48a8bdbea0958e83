// ColorJitter arithmetic of PIL on uint8 RGB, shared by augment.hip (clustering pipelines) and
// seg_augment.hip (segmentation pipelines): ImageEnhance's blend, the L conversion, and the
// RGB -> HSV -> RGB round trip of torchvision's adjust_hue.  Bit for bit PIL's results; the
// specification is oracle/augment_oracle.py.
#pragma once
#include <hip/hip_runtime.h>

// PIL's C code runs as separate IEEE multiplies and adds: no contraction in any file that includes this
// (see augment.hip).
#pragma clang fp contract(off)

__device__ __forceinline__ int aug_luma(int r, int g, int b) {
  return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
}
// ImagingBlend for one channel value
__device__ __forceinline__ int aug_blend(int in1, int in2, float alpha) {
  const float t = (float)in1 + alpha * (float)(in2 - in1);
  if (t <= 0.f) return 0;
  if (t >= 255.f) return 255;
  return (int)t;
}
__device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow Convert.c rgb2hsv_row / hsv2rgb_row with the hue shift in between
__device__ __forceinline__ void aug_hue(int& r, int& g, int& b, int delta) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr;
    const float gc = (float)(maxc - g) / cr;
    const float bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = (float)((double)bc - (double)gc);
    else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double x = (double)h / 6.0 + 1.0;     // in [5/6, 11/6]
    h = (float)(x - floor(x));                                       // fmod(x, 1.0), exact
    uh = aug_clip8((int)((double)h * 255.0));
    us = aug_clip8((int)((double)s * 255.0));
  }
  uh = (uh + delta) & 255;
  if (us == 0) {
    r = g = b = uv;
    return;
  }
  const double hh = (double)uh * 6.0 / 255.0;
  const int i = (int)floor(hh);
  const double f = (double)(float)(hh - (double)i);
  const double fs = (double)(float)((double)us / 255.0);
  const double v = (double)uv;
  const int p = aug_clip8((int)round(v * (1.0 - fs)));
  const int q = aug_clip8((int)round(v * (1.0 - fs * f)));
  const int t = aug_clip8((int)round(v * (1.0 - fs * (1.0 - f))));
  switch (i % 6) {
    case 0: r = uv; g = t; b = p; break;
    case 1: r = q; g = uv; b = p; break;
    case 2: r = p; g = uv; b = t; break;
    case 3: r = p; g = q; b = uv; break;
    case 4: r = t; g = p; b = uv; break;
    default: r = uv; g = p; b = q; break;
  }
}
