// The stages of the clustering augmentation kernels, shared by augment.hip (iic_augment) and augment_affine.hip
// (iic_augment_affine): the parameter row, Pillow's two resampling passes with the cutout test, the ColorJitter ops, the
// tensor conversion, and -- for the affine entry only -- the crop gather and Pillow's bilinear affine on an LDS plane.
// A workgroup of 256 threads produces one output image; every function below is called by all of its threads.
// Specification: oracle/augment_oracle.py::np_pipeline, and tests/augment_affine_cases.py::np_affine_bilinear for the affine.
#pragma once
#include "common.h"
#include "aug_jitter.h"
#include "../../include/iic_hip.h"

// PIL's C code runs as separate IEEE multiplies and adds: no contraction in any file that includes this (see augment.hip).
#pragma clang fp contract(off)

#define AUG_PREC 22
#define AUG_IP 20      // ints per output image:  src, x0, y0, flip, nops, op[4], hue_delta, table,
                       //                         switches (bit 0: rotate the whole image before the crop; bit 1, read by
                       //                         iic_augment_affine only: RandomAffine on the crop), a0..a5 (16.16 fixed point),
                       //                         cutout box (left | upper << 16), (right | lower << 16)
                       //                         in crop coordinates (custom_cutout, transforms.py:28-44:
                       //                         img.paste(0, box) on the cropped image; right == left: none)
#define AUG_FP 4       // floats per output image: factor of op 0 (brightness), 1 (contrast), 2 (saturation), -
#define AUG_AP 6       // doubles per output image (iic_augment_affine): the inverse matrix Image.transform receives

struct AugTabs {           // one entry per crop size: Pillow coefficient table of crop -> S
  int crop[IIC_AUG_MAX_TABLES], ksize[IIC_AUG_MAX_TABLES], boff[IIC_AUG_MAX_TABLES], koff[IIC_AUG_MAX_TABLES];
};

// tables_host [n_tables][4] (include/iic_hip.h) -> the kernel argument (unused entries repeat the first) and the largest
// crop; false for a table count or an entry out of range
static inline bool aug_read_tables(const int* tables_host, int n_tables, int H, int W, AugTabs* tabs, int* max_crop) {
  if (n_tables < 1 || n_tables > IIC_AUG_MAX_TABLES) return false;
  *max_crop = 0;
  for (int t = 0; t < IIC_AUG_MAX_TABLES; ++t) {
    const int* e = tables_host + 4 * (t < n_tables ? t : 0);
    if (e[0] <= 0 || e[0] > H || e[0] > W || e[1] <= 0 || e[2] < 0 || e[3] < 0) return false;
    tabs->crop[t] = e[0]; tabs->ksize[t] = e[1]; tabs->boff[t] = e[2]; tabs->koff[t] = e[3];
    *max_crop = e[0] > *max_crop ? e[0] : *max_crop;
  }
  return true;
}

// LDS of one workgroup: the horizontal pass's plane at 0, the vertical pass's 16-byte aligned behind it.  The affine
// entry keeps the raw crop in the first region and the affined crop in the second until the passes overwrite them (each
// plane is dead by then), so a region is as large as the larger of its two tenants.
static constexpr size_t AUG_LDS_LIMIT = 150 * 1024;   // below IIC_LDS_BYTES: the kernels' static s_red comes on top
static inline size_t aug_lds_bytes(int crop, int S, int ch, bool affine) {
  const size_t first = (size_t)crop * (affine && crop > S ? crop : S) * ch;
  const size_t second = affine && crop > S ? (size_t)crop * crop * ch : (size_t)S * S * ch;
  return ((first + 15) & ~(size_t)15) + second;
}
__device__ __forceinline__ int aug_lds_second(int crop, int S, int ch, bool affine) {
  return (crop * (affine && crop > S ? crop : S) * ch + 15) & ~15;
}

// ---- horizontal pass: image `im` [H][W][CH] (global memory, or a crop plane in LDS) [-> rotation gather] -> sB
// [crop][S][CH].  (x0, y0): the crop's origin in `im`; a0..a5 are read only with rot.
template <int CH>
__device__ __forceinline__ void aug_hpass(const uint8_t* im, int H, int W, int x0, int y0, bool rot, const int* ip,
                                          int crop, int S, const int* bnd, const int* kt, int KS, uint8_t* sB, int tid) {
  const int a0 = ip[12], a1 = ip[13], a2 = ip[14], a3 = ip[15], a4 = ip[16], a5 = ip[17];
  const int bx0 = ip[18] & 0xffff, by0 = (ip[18] >> 16) & 0xffff;
  const int bx1 = ip[19] & 0xffff, by1 = (ip[19] >> 16) & 0xffff;
  for (int idx = tid; idx < crop * S * CH; idx += 256) {
    const int c = idx % CH, xo = (idx / CH) % S, y = idx / (CH * S);
    const int xmin = bnd[xo * 2], cnt = bnd[xo * 2 + 1];
    int ss = 1 << (AUG_PREC - 1);
    const int Y = y0 + y, X = x0 + xmin;
    const bool cut_row = y >= by0 && y < by1;       // cutout: crop pixels inside the box read as 0
    if (rot) {
      int xx = a2 + a1 * Y + a0 * X, yy = a5 + a4 * Y + a3 * X;
      for (int k = 0; k < cnt; ++k) {
        const int xin = xx >> 16, yin = yy >> 16;
        int v = (xin >= 0 && xin < W && yin >= 0 && yin < H) ? (int)im[((long)yin * W + xin) * CH + c] : 0;
        if (cut_row && xmin + k >= bx0 && xmin + k < bx1) v = 0;
        ss += v * kt[xo * KS + k];
        xx += a0;
        yy += a3;
      }
    } else {
      const uint8_t* row = im + ((long)Y * W + X) * CH + c;
      for (int k = 0; k < cnt; ++k) {
        int v = (int)row[k * CH];
        if (cut_row && xmin + k >= bx0 && xmin + k < bx1) v = 0;
        ss += v * kt[xo * KS + k];
      }
    }
    sB[idx] = (uint8_t)aug_clip8(ss >> AUG_PREC);
  }
}

// ---- vertical pass (sB -> sC [S][S][CH])
template <int CH>
__device__ __forceinline__ void aug_vpass(const uint8_t* sB, int S, const int* bnd, const int* kt, int KS, uint8_t* sC,
                                          int tid) {
  for (int idx = tid; idx < S * S * CH; idx += 256) {
    const int c = idx % CH, xo = (idx / CH) % S, yo = idx / (CH * S);
    const int ymin = bnd[yo * 2], cnt = bnd[yo * 2 + 1];
    int ss = 1 << (AUG_PREC - 1);
    for (int k = 0; k < cnt; ++k) ss += (int)sB[((ymin + k) * S + xo) * CH + c] * kt[yo * KS + k];
    sC[idx] = (uint8_t)aug_clip8(ss >> AUG_PREC);
  }
}

// ---- ColorJitter ops in their shuffled order (pointwise on whole pixels, in place); s_red: 4 ints of LDS.  Ends with
// the workgroup synchronised.
template <int CH>
__device__ __forceinline__ void aug_jitter_ops(uint8_t* sC, int S, const int* ip, const float* fp, int* s_red, int tid) {
  const int nops = ip[4], hdelta = ip[9];
  for (int o = 0; o < nops; ++o) {
    const int op = ip[5 + o];
    if (CH == 1 && op >= 2) continue;                // saturation / hue: identities on an L image
    int mean = 0;
    if (op == 1) {                                   // contrast: rounded mean of the L image
      int part = 0;
      for (int px = tid; px < S * S; px += 256)
        part += CH == 1 ? (int)sC[px] : aug_luma(sC[px * 3], sC[px * 3 + 1], sC[px * 3 + 2]);
#pragma unroll
      for (int sft = 32; sft > 0; sft >>= 1) part += __shfl_xor(part, sft, 64);
      if ((tid & 63) == 0) s_red[tid >> 6] = part;
      __syncthreads();
      const int tot = s_red[0] + s_red[1] + s_red[2] + s_red[3];
      mean = (int)((double)tot / (double)(S * S) + 0.5);
      __syncthreads();
    }
    const float alpha = op < 3 ? fp[op] : 0.f;
    for (int px = tid; px < S * S; px += 256) {
      if (CH == 1) {
        sC[px] = (uint8_t)aug_blend(op == 0 ? 0 : mean, sC[px], alpha);
        continue;
      }
      int r = sC[px * 3], g = sC[px * 3 + 1], b = sC[px * 3 + 2];
      if (op == 0) {
        r = aug_blend(0, r, alpha); g = aug_blend(0, g, alpha); b = aug_blend(0, b, alpha);
      } else if (op == 1) {
        r = aug_blend(mean, r, alpha); g = aug_blend(mean, g, alpha); b = aug_blend(mean, b, alpha);
      } else if (op == 2) {
        const int L = aug_luma(r, g, b);
        r = aug_blend(L, r, alpha); g = aug_blend(L, g, alpha); b = aug_blend(L, b, alpha);
      } else {
        aug_hue(r, g, b, hdelta);
      }
      sC[px * 3] = (uint8_t)r; sC[px * 3 + 1] = (uint8_t)g; sC[px * 3 + 2] = (uint8_t)b;
    }
    __syncthreads();
  }
}

// ---- custom_greyscale_to_tensor / ToTensor (+ the horizontal flip, which commutes with the ops above): sC -> `on`
// float [C][S][S], C = 1 for CH == 1, else 4 with INC_RGB and 1 without
template <int CH, bool INC_RGB>
__device__ __forceinline__ void aug_to_tensor(const uint8_t* sC, int S, int flip, const float* __restrict__ lut,
                                              const float* __restrict__ norm, float* __restrict__ on, int tid) {
  constexpr int C = CH == 1 ? 1 : (INC_RGB ? 4 : 1);
  for (int px = tid; px < S * S; px += 256) {
    const int y = px / S, x = px - y * S;
    const int sp = (y * S + (flip ? S - 1 - x : x)) * CH;
    // norm (nullable): torchvision Normalize after the tensor conversion, (v - mean[c]) / std[c]
    // as two float32 operations (t.sub_(m).div_(s)); norm = [C means][C stds]
    if (CH == 1) {
      float v = lut[sC[sp]];
      if (norm) v = (v - norm[0]) / norm[1];
      on[px] = v;
      continue;
    }
    const int r = sC[sp], g = sC[sp + 1], b = sC[sp + 2];
    if (INC_RGB) {
      float vr = lut[r], vg = lut[g], vb = lut[b];
      if (norm) {
        vr = (vr - norm[0]) / norm[C + 0];
        vg = (vg - norm[1]) / norm[C + 1];
        vb = (vb - norm[2]) / norm[C + 2];
      }
      on[px] = vr;
      on[S * S + px] = vg;
      on[2 * S * S + px] = vb;
    }
    float vl = lut[aug_luma(r, g, b)];
    if (norm) vl = (vl - norm[C - 1]) / norm[2 * C - 1];
    on[(C - 1) * S * S + px] = vl;
  }
}

// ---- the raw crop as an image of its own (iic_augment_affine): im [H][W][CH] [-> rotation gather] -> sA [crop][crop][CH].
// The rotation is the horizontal pass's: source x = (a2 + a1 Y + a0 X) >> 16, zero outside the image.
template <int CH>
__device__ __forceinline__ void aug_crop_gather(const uint8_t* __restrict__ im, int H, int W, int x0, int y0, bool rot,
                                                const int* ip, int crop, uint8_t* sA, int tid) {
  const int a0 = ip[12], a1 = ip[13], a2 = ip[14], a3 = ip[15], a4 = ip[16], a5 = ip[17];
  for (int idx = tid; idx < crop * crop * CH; idx += 256) {
    const int c = idx % CH, x = (idx / CH) % crop, y = idx / (CH * crop);
    const int Y = y0 + y, X = x0 + x;
    int xin = X, yin = Y;
    bool in = true;
    if (rot) {
      xin = (a2 + a1 * Y + a0 * X) >> 16;
      yin = (a5 + a4 * Y + a3 * X) >> 16;
      in = xin >= 0 && xin < W && yin >= 0 && yin < H;
    }
    sA[idx] = in ? im[((long)yin * W + xin) * CH + c] : (uint8_t)0;
  }
}

// ---- Pillow's Image.transform(size, AFFINE, m, BILINEAR, fillcolor=0) of the w x w crop plane sA -> sT (Geometry.c:
// ImagingGenericTransform with affine_transform and bilinear_filter32RGB), in IEEE double, every multiply and add on its
// own.  The range test is on the UNSHIFTED coordinates and written so that a NaN fails it; behind it xf, yf are in
// [-1, w - 1] and every index is clamped: nothing outside the plane is read, whatever m holds.
template <int CH>
__device__ __forceinline__ void aug_affine_bilinear(const uint8_t* sA, int w, const double* __restrict__ m, uint8_t* sT,
                                                    int tid) {
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  const double lim = (double)w;
  for (int px = tid; px < w * w; px += 256) {
    const int y = px / w, x = px - y * w;
    const double xin = (double)x + 0.5, yin = (double)y + 0.5;
    double X = (m0 * xin + m1 * yin) + m2;
    double Y = (m3 * xin + m4 * yin) + m5;
    uint8_t* o = sT + px * CH;
    if (!(X >= 0.0 && X < lim && Y >= 0.0 && Y < lim)) {
#pragma unroll
      for (int c = 0; c < CH; ++c) o[c] = 0;
      continue;
    }
    X -= 0.5;
    Y -= 0.5;
    const double fx = floor(X), fy = floor(Y);
    const double dx = X - fx, dy = Y - fy;
    const int xf = (int)fx, yf = (int)fy;            // may be -1
    const int xa = min(max(xf, 0), w - 1), xb = min(max(xf + 1, 0), w - 1), yc = min(max(yf, 0), w - 1);
    const bool below = yf + 1 >= 0 && yf + 1 < w;
    const uint8_t* r1 = sA + yc * w * CH;
    const uint8_t* r2 = sA + (below ? yf + 1 : yc) * w * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int p0 = r1[xa * CH + c], p1 = r1[xb * CH + c];
      const double v1 = (double)p0 + (double)(p1 - p0) * dx;
      double v2 = v1;
      if (below) {
        const int q0 = r2[xa * CH + c], q1 = r2[xb * CH + c];
        v2 = (double)q0 + (double)(q1 - q0) * dx;
      }
      const double v = v1 + (v2 - v1) * dy;
      o[c] = (uint8_t)(int)v;                        // truncation; 0 <= v <= 255
    }
  }
}
