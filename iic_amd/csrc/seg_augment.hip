// GPU-side paired augmentation for the segmentation scripts: what the training __getitem__ of the
// reference's Potsdam and COCO-Stuff datasets returns, for a whole batch in one launch.
//
// Replaces, per sample,
//   /root/reference/code/datasets/segmentation/potsdam.py:95-216    (_Potsdam._prepare_train)
//   /root/reference/code/datasets/segmentation/cocostuff.py:104-230 (_Coco._prepare_train)
// which run on the host, one image at a time:
//   pad_if_too_small + pad_and_or_crop (code/utils/segmentation/transforms.py:23-88): sources smaller
//     than S are centred in zeros (int(x / 2.) arithmetic), then an S x S window is cut;
//   img1 = the crop as uint8; img2 = torchvision ColorJitter of its RGB part (never of IR,
//     potsdam.py:147-156) -- PIL arithmetic, aug_jitter.h;
//   custom_greyscale_numpy (transforms.py:7-20) unless no_sobel: grey appended after RGB
//     (include_rgb) or instead of it; IR, when the source has it, comes last;
//   astype(float32) / 255. (the 256-entry table of the clustering augmenter);
//   torch.flip(img2, dims=[2]) and the negated top row of affine2_to_1 (potsdam.py:194-202);
//   mask_img1: ones (Potsdam) or _filter_label's mask (cocostuff.py:137-141) as a 256-entry table
//     of the fine label, 255 standing for -1; padded label pixels are fine-label 0.
// The random affine of img2 (transforms.py:91-128) is NOT in this kernel: the host warps the batch
// with iic_affine_warp_fwd afterwards and folds the mirror into the warp's matrix (flip bit 1 below).
//
// Grey is OpenCV's 8-bit COLOR_RGB2GRAY, not PIL's "L": restated here from OpenCV 3.x's source
// (fixed point, 14 fractional bits), NOT compared against a cv2 binary -- cv2 is not installable
// where this is built and tested.  Newer OpenCV builds use a 15-bit variant that can differ by one
// grey level.  The formula lives in seg_grey() alone.
//
// Shape: a streaming kernel, one workgroup per sample.  A thread owns four consecutive output x of
// one row: it reads the four source pixels once for both views and writes every planar fp32
// channel with one 16-byte store (S % 4 == 0).  The only LDS is the reduction of ColorJitter's
// contrast mean (the rounded mean of the L image the preceding ops produced), which needs one
// extra pass over the crop for the samples whose op list holds contrast.  No atomics: two calls
// with the same parameters give identical bytes.
//
// seg_prepare_test_kernel (below the training kernel) is the test-time twin, `_prepare_test`
// (potsdam.py:295-350, cocostuff.py:309-358): the centre crop, one view, no jitter, plus the
// filtered label map; it shares seg_load, seg_grey and seg_pad_offset with the training kernel.
//
// seg_augment_ragged_kernel (between the two) is the training kernel for a dataset whose images differ in size
// (COCO-Stuff): images packed without padding, every sample padded and cropped by its own extent, optionally resampled
// through host-built tables (use_random_scale; or, from the original-resolution images, pre_scale_all followed by
// use_random_scale as two resampling stages); it shares seg_load, seg_grey, seg_jitter and seg_pad_offset.
#include "common.h"
#include "aug_jitter.h"
#include "seg_resample.h"
#include "../../include/iic_hip.h"

#pragma clang fp contract(off)

#define SEG_IP IIC_SEG_AUG_IPARAMS   // src, x0, y0, flip bits, nops, op[4], hue_delta, -, -
#define SEG_FP IIC_SEG_AUG_FPARAMS   // brightness, contrast, saturation, (hue), affine2_to_1 before the flip [6]
#define SEG_THREADS 512

// OpenCV 3.x RGB2Gray for 8-bit images (modules/imgproc/src/color.cpp: yuv_shift = 14, R2Y = 4899,
// G2Y = 9617, B2Y = 1868, CV_DESCALE rounds to nearest)
#define SEG_GREY_R 4899
#define SEG_GREY_G 9617
#define SEG_GREY_B 1868
#define SEG_GREY_SHIFT 14
__device__ __forceinline__ int seg_grey(int r, int g, int b) {
  return (r * SEG_GREY_R + g * SEG_GREY_G + b * SEG_GREY_B + (1 << (SEG_GREY_SHIFT - 1))) >> SEG_GREY_SHIFT;
}

// pad_if_too_small (transforms.py:34-41): offset of a source side of `len` pixels inside the padded side of
// max(len, S), int(x / 2.) arithmetic; 0 for a side that is not padded
__host__ __device__ __forceinline__ int seg_pad_offset(int len, int S) {
  const int padded = len > S ? len : S;
  return padded / 2 - len / 2;
}

// ops [first, last) of the shuffled ColorJitter list on one pixel; opsw holds op o in bits 4o..4o+3
__device__ __forceinline__ void seg_jitter(int& r, int& g, int& b, int opsw, int first, int last, float f_b,
                                           float f_c, float f_s, int mean, int hdelta) {
  for (int o = first; o < last; ++o) {
    const int op = (opsw >> (4 * o)) & 15;
    if (op == 0) {
      r = aug_blend(0, r, f_b); g = aug_blend(0, g, f_b); b = aug_blend(0, b, f_b);
    } else if (op == 1) {
      r = aug_blend(mean, r, f_c); g = aug_blend(mean, g, f_c); b = aug_blend(mean, b, f_c);
    } else if (op == 2) {
      const int L = aug_luma(r, g, b);
      r = aug_blend(L, r, f_s); g = aug_blend(L, g, f_s); b = aug_blend(L, b, f_s);
    } else {
      aug_hue(r, g, b, hdelta);
    }
  }
}

// one source pixel of the padded image at crop position (y, x): zeros outside the source
template <int CS>
__device__ __forceinline__ void seg_load(const uint8_t* __restrict__ im, int sy, int sx, int H, int W, int& r,
                                         int& g, int& b, int& ir) {
  r = g = b = ir = 0;
  if (im != nullptr && sy >= 0 && sy < H && sx >= 0 && sx < W) {
    const uint8_t* p = im + ((long)sy * W + sx) * CS;
    if (CS == 4) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
      r = v & 255; g = (v >> 8) & 255; b = (v >> 16) & 255; ir = v >> 24;
    } else {
      r = p[0]; g = p[1]; b = p[2];
    }
  }
}

// MODE 0: no_sobel, RGB(+IR); 1: RGB, grey(, IR); 2: grey(, IR)
template <int CS, int MODE>
__global__ __launch_bounds__(SEG_THREADS) void seg_augment_kernel(
    const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ labels, const uint8_t* __restrict__ table, int B,
    int H, int W, int pad_y, int pad_x, const int* __restrict__ iparams, const float* __restrict__ fparams, int S,
    const float* __restrict__ lut, float* __restrict__ img1, float* __restrict__ img2, uint8_t* __restrict__ mask,
    float* __restrict__ aff) {
  __shared__ int s_red[SEG_THREADS / 64];
  constexpr int C = (MODE == 0 ? 3 : (MODE == 1 ? 4 : 1)) + (CS == 4 ? 1 : 0);
  constexpr int CG = MODE == 1 ? 3 : 0;              // grey's channel (IR, when present, is C - 1)
  const int n = blockIdx.x, tid = threadIdx.x;
  const int* ip = iparams + (long)n * SEG_IP;
  const float* fp = fparams + (long)n * SEG_FP;
  const int src = ip[0], x0 = ip[1] - pad_x, y0 = ip[2] - pad_y, flip = ip[3] & 1, defer = (ip[3] >> 1) & 1;
  int nops = ip[4];
  nops = nops < 0 ? 0 : (nops > 4 ? 4 : nops);
  const int opsw = (ip[5] & 3) | ((ip[6] & 3) << 4) | ((ip[7] & 3) << 8) | ((ip[8] & 3) << 12);
  const int hdelta = ip[9] & 255;
  const float f_b = fp[0], f_c = fp[1], f_s = fp[2];
  const bool valid = src >= 0 && src < B;           // an index outside the dataset reads as a black image
  const uint8_t* im = valid ? imgs + (long)src * H * W * CS : nullptr;
  const uint8_t* lb = (labels != nullptr && valid) ? labels + (long)src * H * W : nullptr;
  const int Q = S >> 2, nquads = S * Q;

  // ---- affine2_to_1: the given rows, top row negated when flipped (potsdam.py:202)
  if (tid < 6) {
    const float v = fp[4 + tid];
    aff[(long)n * 6 + tid] = (flip && tid < 3) ? v * -1.f : v;
  }

  // ---- contrast: rounded mean of the L image after the ops that precede it
  int cpos = -1;
  for (int o = 0; o < nops; ++o)
    if (((opsw >> (4 * o)) & 15) == 1 && cpos < 0) cpos = o;
  int mean = 0;
  if (cpos >= 0) {                                   // uniform over the workgroup
    int part = 0;
    for (int q = tid; q < nquads; q += SEG_THREADS) {
      const int y = q / Q, xq = (q - y * Q) << 2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int r, g, b, ir;
        seg_load<CS>(im, y0 + y, x0 + xq + j, H, W, r, g, b, ir);
        seg_jitter(r, g, b, opsw, 0, cpos, f_b, f_c, f_s, 0, hdelta);
        part += aug_luma(r, g, b);
      }
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) part += __shfl_xor(part, sft, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = part;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < SEG_THREADS / 64; ++w) tot += s_red[w];
    mean = (int)((double)tot / (double)(S * S) + 0.5);
  }

  // ---- both views
  const long plane = (long)S * S;
  float* o1 = img1 + (long)n * C * plane;
  float* o2 = img2 + (long)n * C * plane;
  uint8_t* om = mask + (long)n * plane;
  const bool mirror = flip && !defer;
  for (int q = tid; q < nquads; q += SEG_THREADS) {
    const int y = q / Q, xq = (q - y * Q) << 2;
    f32x4 v1[C], v2[C];
    uint32_t mk = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int r, g, b, ir;
      const int sy = y0 + y, sx = x0 + xq + j;
      seg_load<CS>(im, sy, sx, H, W, r, g, b, ir);
      int m = 1;
      if (labels != nullptr) {
        const int l = (lb != nullptr && sy >= 0 && sy < H && sx >= 0 && sx < W) ? (int)lb[(long)sy * W + sx] : 0;
        m = table[l];
      }
      mk |= (uint32_t)(m & 255) << (8 * j);
      int r2 = r, g2 = g, b2 = b;
      seg_jitter(r2, g2, b2, opsw, 0, nops, f_b, f_c, f_s, mean, hdelta);
      if (MODE != 2) {
        v1[0][j] = lut[r]; v1[1][j] = lut[g]; v1[2][j] = lut[b];
        v2[0][j] = lut[r2]; v2[1][j] = lut[g2]; v2[2][j] = lut[b2];
      }
      if (MODE != 0) {
        v1[CG][j] = lut[seg_grey(r, g, b)];
        v2[CG][j] = lut[seg_grey(r2, g2, b2)];
      }
      if (CS == 4) {
        v1[C - 1][j] = lut[ir];
        v2[C - 1][j] = lut[ir];
      }
    }
    const long off1 = (long)y * S + xq;
    const long off2 = (long)y * S + (mirror ? S - 4 - xq : xq);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      *reinterpret_cast<f32x4*>(o1 + c * plane + off1) = v1[c];
      const f32x4 m2 = {v2[c][3], v2[c][2], v2[c][1], v2[c][0]};     // torch.flip(img2, dims=[2]) within the run
      *reinterpret_cast<f32x4*>(o2 + c * plane + off2) = mirror ? m2 : v2[c];
    }
    *reinterpret_cast<uint32_t*>(om + off1) = mk;
  }
}

// ---- datasets whose images differ in size (COCO-Stuff), optionally with use_random_scale: the packed twin of
// seg_augment_kernel.  Image i is h_i x w_i x CS at pixel offset offsets[i] of one packed array, row pitch w_i; pad
// offsets and the inside test come from the sample's own extent (cocostuff.py:133-135 over transforms.py:23-88).
// RS = 1 (cocostuff.py:123-130, potsdam.py:109-114): every crop row and column carries a host-built resampling tap
// (iic_seg_resample_tap: OpenCV 3.x's INTER_LINEAR coefficients for the float image, INTER_NEAREST's index for the
// label); the kernel only multiplies and adds, in cv2's order (horizontal pass, then vertical), each operation rounded
// to float32 on its own, and truncates RGB to uint8 as `img.astype(np.uint8)` does after the crop.  With RS = 0 no
// tap is read.
// RS = 2 (pre_scale_all, then use_random_scale, on the ORIGINAL images: cocostuff.py:113-130, potsdam.py:103-114): the
// reference resizes twice and never truncates in between.  Every crop row and column carries the two taps of the second
// resize on the pre-scaled side and, for each of them, the two taps of the first resize on the source side
// (iic_seg_resample_tap2); the four intermediate pixels are computed as above, kept in float32, and combined by the
// same formula with the second stage's weights.  RS = 0 is no resampling, RS = 1 the single stage.
struct seg_ragged_src {
  const uint8_t* im;             // nullptr: a black image
  const uint8_t* lb;             // nullptr: no labels, or a black image
  int h, w;                      // the stored extent; w is the row pitch
  int x0, y0;                    // crop origin in source coordinates (RS = 0)
  const iic_seg_resample_tap* ty;   // S row taps, then S column taps (RS = 1)
  const iic_seg_resample_tap* tx;
  const iic_seg_resample_tap2* ty2;  // the same for the two-stage tables (RS = 2)
  const iic_seg_resample_tap2* tx2;
};

__device__ __forceinline__ int seg_clamp_index(int i, int len) { return i < 0 ? 0 : (i >= len ? len - 1 : i); }

// cv2's INTER_LINEAR pixel on the uint8 source: (p00 ax0 + p01 ax1) by0 + (p10 ax0 + p11 ax1) by1 per channel, every
// operation rounded to float32 (seg_lerp; contraction is off in this file).  Indices are clamped to the image.
template <int CS>
__device__ __forceinline__ void seg_bilinear(const seg_ragged_src& s, int y0, int y1, int x0, int x1, float ax0,
                                             float ax1, float by0, float by1, float v[4]) {
  const int ya = seg_clamp_index(y0, s.h), yb = seg_clamp_index(y1, s.h);
  const int xa = seg_clamp_index(x0, s.w), xb = seg_clamp_index(x1, s.w);
  int p00[4], p01[4], p10[4], p11[4];
  seg_load<CS>(s.im, ya, xa, s.h, s.w, p00[0], p00[1], p00[2], p00[3]);
  seg_load<CS>(s.im, ya, xb, s.h, s.w, p01[0], p01[1], p01[2], p01[3]);
  seg_load<CS>(s.im, yb, xa, s.h, s.w, p10[0], p10[1], p10[2], p10[3]);
  seg_load<CS>(s.im, yb, xb, s.h, s.w, p11[0], p11[1], p11[2], p11[3]);
#pragma unroll
  for (int c = 0; c < CS; ++c) {
    const float top = seg_lerp((float)p00[c], ax0, (float)p01[c], ax1);
    const float bot = seg_lerp((float)p10[c], ax0, (float)p11[c], ax1);
    v[c] = seg_lerp(top, by0, bot, by1);
  }
}

// one pixel of the crop at (y, x): r, g, b, ir and the fine label l (0 in the padding).  RS != 0: irf is the resampled
// IR value BEFORE truncation -- the reference truncates only the RGB part it hands to PIL (potsdam.py:148-151), IR goes
// on as the float image / 255. (potsdam.py:170)
template <int CS, int RS>
__device__ __forceinline__ void seg_ragged_fetch(const seg_ragged_src& s, int y, int x, bool want_label, int& r, int& g,
                                                 int& b, int& ir, float& irf, int& l) {
  l = 0;
  irf = 0.f;
  if (RS == 0) {
    const int sy = s.y0 + y, sx = s.x0 + x;
    seg_load<CS>(s.im, sy, sx, s.h, s.w, r, g, b, ir);
    if (want_label && s.lb != nullptr && sy >= 0 && sy < s.h && sx >= 0 && sx < s.w) l = s.lb[(long)sy * s.w + sx];
  } else if (RS == 1) {
    r = g = b = ir = 0;
    const iic_seg_resample_tap ty = s.ty[y], tx = s.tx[x];
    if (s.im == nullptr || !ty.inside || !tx.inside) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    seg_bilinear<CS>(s, ty.i0, ty.i1, tx.i0, tx.i1, tx.a0, tx.a1, ty.a0, ty.a1, v);
    r = seg_trunc_u8(v[0]); g = seg_trunc_u8(v[1]); b = seg_trunc_u8(v[2]);
    if (CS == 4) {
      ir = seg_trunc_u8(v[3]);
      irf = v[3];
    }
    if (want_label && s.lb != nullptr)
      l = s.lb[(long)seg_clamp_index(ty.nearest, s.h) * s.w + seg_clamp_index(tx.nearest, s.w)];
  } else {
    r = g = b = ir = 0;
    const iic_seg_resample_tap2 ty = s.ty2[y], tx = s.tx2[x];
    if (s.im == nullptr || !ty.inside || !tx.inside) return;
    float m[2][2][4];              // the pre-scaled image at the second stage's four taps, untruncated
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        m[i][j][3] = 0.f;
        seg_bilinear<CS>(s, ty.i0[i], ty.i1[i], tx.i0[j], tx.i1[j], tx.a0[j], tx.a1[j], ty.a0[i], ty.a1[i], m[i][j]);
      }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < CS; ++c) {
      const float top = seg_lerp(m[0][0][c], tx.b0, m[0][1][c], tx.b1);
      const float bot = seg_lerp(m[1][0][c], tx.b0, m[1][1][c], tx.b1);
      v[c] = seg_lerp(top, ty.b0, bot, ty.b1);
    }
    r = seg_trunc_u8(v[0]); g = seg_trunc_u8(v[1]); b = seg_trunc_u8(v[2]);
    if (CS == 4) {
      ir = seg_trunc_u8(v[3]);
      irf = v[3];
    }
    if (want_label && s.lb != nullptr)
      l = s.lb[(long)seg_clamp_index(ty.nearest, s.h) * s.w + seg_clamp_index(tx.nearest, s.w)];
  }
}

// MODE as above.  One workgroup per sample, a thread per four consecutive output x of one row, as seg_augment_kernel.
template <int CS, int MODE, int RS>
__global__ __launch_bounds__(SEG_THREADS) void seg_augment_ragged_kernel(
    const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ labels, const uint8_t* __restrict__ table,
    const long* __restrict__ offsets, const int* __restrict__ sizes, int B, long total_px,
    const int* __restrict__ iparams, const float* __restrict__ fparams, const iic_seg_resample_tap* __restrict__ taps,
    const iic_seg_resample_tap2* __restrict__ taps2, int S, const float* __restrict__ lut, float* __restrict__ img1, float* __restrict__ img2, uint8_t* __restrict__ mask,
    float* __restrict__ aff) {
  __shared__ int s_red[SEG_THREADS / 64];
  constexpr int C = (MODE == 0 ? 3 : (MODE == 1 ? 4 : 1)) + (CS == 4 ? 1 : 0);
  constexpr int CG = MODE == 1 ? 3 : 0;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int* ip = iparams + (long)n * SEG_IP;
  const float* fp = fparams + (long)n * SEG_FP;
  const int src = ip[0], flip = ip[3] & 1, defer = (ip[3] >> 1) & 1;
  int nops = ip[4];
  nops = nops < 0 ? 0 : (nops > 4 ? 4 : nops);
  const int opsw = (ip[5] & 3) | ((ip[6] & 3) << 4) | ((ip[7] & 3) << 8) | ((ip[8] & 3) << 12);
  const int hdelta = ip[9] & 255;
  const float f_b = fp[0], f_c = fp[1], f_s = fp[2];
  // an index outside the dataset, or an image whose extent or offset would leave the pack, reads as a black image
  seg_ragged_src s = {nullptr, nullptr, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr};
  if (src >= 0 && src < B) {
    const int h = sizes[2 * src], w = sizes[2 * src + 1];
    const long off = offsets[src];
    if (h >= 1 && h <= 16384 && w >= 1 && w <= 16384 && off >= 0 && off <= total_px && (long)h * w <= total_px - off) {
      s.im = imgs + off * CS;
      s.lb = labels != nullptr ? labels + off : nullptr;
      s.h = h; s.w = w;
      s.x0 = ip[1] - seg_pad_offset(w, S);
      s.y0 = ip[2] - seg_pad_offset(h, S);
    }
  }
  if (RS == 1) {
    s.ty = taps + (long)n * 2 * S;
    s.tx = s.ty + S;
  } else if (RS == 2) {
    s.ty2 = taps2 + (long)n * 2 * S;
    s.tx2 = s.ty2 + S;
  }
  const int Q = S >> 2, nquads = S * Q;

  // ---- affine2_to_1: the given rows, top row negated when flipped (cocostuff.py:220)
  if (tid < 6) {
    const float v = fp[4 + tid];
    aff[(long)n * 6 + tid] = (flip && tid < 3) ? v * -1.f : v;
  }

  // ---- contrast: rounded mean of the L image after the ops that precede it, over all S * S pixels, padding included
  int cpos = -1;
  for (int o = 0; o < nops; ++o)
    if (((opsw >> (4 * o)) & 15) == 1 && cpos < 0) cpos = o;
  int mean = 0;
  if (cpos >= 0) {                                   // uniform over the workgroup
    int part = 0;
    for (int q = tid; q < nquads; q += SEG_THREADS) {
      const int y = q / Q, xq = (q - y * Q) << 2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int r, g, b, ir, l;
        float irf;
        seg_ragged_fetch<CS, RS>(s, y, xq + j, false, r, g, b, ir, irf, l);
        seg_jitter(r, g, b, opsw, 0, cpos, f_b, f_c, f_s, 0, hdelta);
        part += aug_luma(r, g, b);
      }
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) part += __shfl_xor(part, sft, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = part;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < SEG_THREADS / 64; ++w) tot += s_red[w];
    mean = (int)((double)tot / (double)(S * S) + 0.5);
  }

  // ---- both views
  const long plane = (long)S * S;
  float* o1 = img1 + (long)n * C * plane;
  float* o2 = img2 + (long)n * C * plane;
  uint8_t* om = mask + (long)n * plane;
  const bool mirror = flip && !defer;
  for (int q = tid; q < nquads; q += SEG_THREADS) {
    const int y = q / Q, xq = (q - y * Q) << 2;
    f32x4 v1[C], v2[C];
    uint32_t mk = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int r, g, b, ir, l;
      float irf;
      seg_ragged_fetch<CS, RS>(s, y, xq + j, labels != nullptr, r, g, b, ir, irf, l);
      const int m = labels != nullptr ? (int)table[l] : 1;
      mk |= (uint32_t)(m & 255) << (8 * j);
      int r2 = r, g2 = g, b2 = b;
      seg_jitter(r2, g2, b2, opsw, 0, nops, f_b, f_c, f_s, mean, hdelta);
      if (MODE != 2) {
        v1[0][j] = lut[r]; v1[1][j] = lut[g]; v1[2][j] = lut[b];
        v2[0][j] = lut[r2]; v2[1][j] = lut[g2]; v2[2][j] = lut[b2];
      }
      if (MODE != 0) {
        v1[CG][j] = lut[seg_grey(r, g, b)];
        v2[CG][j] = lut[seg_grey(r2, g2, b2)];
      }
      if (CS == 4) {
        const float vir = RS != 0 ? irf / 255.f : lut[ir];
        v1[C - 1][j] = vir;
        v2[C - 1][j] = vir;
      }
    }
    const long off1 = (long)y * S + xq;
    const long off2 = (long)y * S + (mirror ? S - 4 - xq : xq);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      *reinterpret_cast<f32x4*>(o1 + c * plane + off1) = v1[c];
      const f32x4 m2 = {v2[c][3], v2[c][2], v2[c][1], v2[c][0]};     // torch.flip(img2, dims=[2]) within the run
      *reinterpret_cast<f32x4*>(o2 + c * plane + off2) = mirror ? m2 : v2[c];
    }
    *reinterpret_cast<uint32_t*>(om + off1) = mk;
  }
}

// ---- random_affine's warp of img2 for the ragged augmenter: perform_affine_tf (transforms.py:131-143), F.affine_grid +
// F.grid_sample (bilinear, zeros, align_corners false -- the convention of seg_losses.ALIGN_CORNERS), followed by
// torch.flip(dims=[2]) where flips[n], restated operation by operation so that the result is bit-identical to what the
// reference computes on a CPU (tests/golden/seg_augment_ragged.npz): the sampling position is
// fma(y_b, t01, x_b * t00) + t02 on the host-made base grid (linspace(-1, 1, S) * (S - 1) / S), un-normalised as
// fma(g + 1, S / 2, -0.5); the four taps are accumulated as nw_val * nw, then one fma per further tap in the order ne,
// sw, se, with the weights (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx.  iic_affine_warp_fwd computes the same warp
// from a pixel-space matrix in another order of operations (within 2e-6 of this one).
#define SEG_WARP_THREADS 256
__global__ __launch_bounds__(SEG_WARP_THREADS) void seg_grid_warp_kernel(
    const float* __restrict__ x, const float* __restrict__ theta, const int* __restrict__ flips,
    const float* __restrict__ base, float* __restrict__ out, int N, int C, int S) {
  const long idx = (long)blockIdx.x * SEG_WARP_THREADS + threadIdx.x;
  const long plane = (long)S * S;
  if (idx >= (long)N * plane) return;
  const int n = (int)(idx / plane);
  const int rem = (int)(idx - (long)n * plane);
  const int oy = rem / S, ox = rem - oy * S;
  const float* t = theta + (long)n * 6;
  const float xb = base[flips[n] ? S - 1 - ox : ox], yb = base[oy];
  const float gx = __fmaf_rn(yb, t[1], xb * t[0]) + t[2];
  const float gy = __fmaf_rn(yb, t[4], xb * t[3]) + t[5];
  const float half = (float)S / 2.f;
  const float fx = __fmaf_rn(gx + 1.f, half, -0.5f), fy = __fmaf_rn(gy + 1.f, half, -0.5f);
  const float* xi = x + (long)n * C * plane;
  float* o = out + (long)n * C * plane + rem;
  // a position further than one pixel outside the image (or not a number) has four zero taps
  if (!(fx > -1.f && fx < (float)S && fy > -1.f && fy < (float)S)) {
    for (int c = 0; c < C; ++c) o[c * plane] = 0.f;
    return;
  }
  const float xw = floorf(fx), yn = floorf(fy);
  const float w = fx - xw, e = 1.f - w, nn = fy - yn, s = 1.f - nn;
  const float nw = s * e, ne = s * w, sw = nn * e, se = nn * w;
  const int ix = (int)xw, iy = (int)yn;
  const bool x0 = ix >= 0, x1 = ix + 1 < S, y0 = iy >= 0, y1 = iy + 1 < S;     // ix, iy in [-1, S - 1]
  for (int c = 0; c < C; ++c) {
    const float* p = xi + c * plane;
    const float a = (y0 && x0) ? p[(long)iy * S + ix] : 0.f;
    const float b = (y0 && x1) ? p[(long)iy * S + ix + 1] : 0.f;
    const float cc = (y1 && x0) ? p[(long)(iy + 1) * S + ix] : 0.f;
    const float d = (y1 && x1) ? p[(long)(iy + 1) * S + ix + 1] : 0.f;
    float r = a * nw;
    r = __fmaf_rn(b, ne, r);
    r = __fmaf_rn(cc, sw, r);
    r = __fmaf_rn(d, se, r);
    o[c * plane] = r;
  }
}

// ---- test-time batches: `_prepare_test`, one thread per four consecutive output x of one row, no LDS
#define SEG_TEST_THREADS 256

// pad_and_or_crop(mode="centre") (transforms.py:61-63, :81-82): first source row / column of the crop.  The crop
// starts at int(padded / 2.) - int(S / 2.) in the padded side; the source starts at seg_pad_offset inside it.
__device__ __forceinline__ int seg_centre_origin(int len, int S) {
  const int padded = len > S ? len : S;
  return padded / 2 - S / 2 - seg_pad_offset(len, S);
}

// MODE as above.  sizes: (h, w) of every image, stored top-left in its [H][W] slab, or nullptr (all H x W).
template <int CS, int MODE>
__global__ __launch_bounds__(SEG_TEST_THREADS) void seg_prepare_test_kernel(
    const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ labels, const int* __restrict__ sizes,
    const uint8_t* __restrict__ ttable, const uint8_t* __restrict__ rtable, int B, int H, int W,
    const int* __restrict__ idx, int S, const float* __restrict__ lut, float* __restrict__ out,
    uint8_t* __restrict__ targets, uint8_t* __restrict__ mask) {
  constexpr int C = (MODE == 0 ? 3 : (MODE == 1 ? 4 : 1)) + (CS == 4 ? 1 : 0);
  constexpr int CG = MODE == 1 ? 3 : 0;
  const int n = blockIdx.y, Q = S >> 2;
  const int q = blockIdx.x * SEG_TEST_THREADS + threadIdx.x;
  if (q >= S * Q) return;
  const int src = idx[n];
  const bool valid = src >= 0 && src < B;           // an index outside the dataset reads as a black image, label 0
  int h = H, w = W;
  if (valid && sizes != nullptr) {                  // an extent outside the slab is clamped to it
    h = sizes[2 * src], w = sizes[2 * src + 1];
    h = h < 0 ? 0 : (h > H ? H : h);
    w = w < 0 ? 0 : (w > W ? W : w);
  }
  const uint8_t* im = valid ? imgs + (long)src * H * W * CS : nullptr;
  const uint8_t* lb = valid ? labels + (long)src * H * W : nullptr;
  const int y = q / Q, xq = (q - y * Q) << 2;
  const int sy = seg_centre_origin(h, S) + y, sx0 = seg_centre_origin(w, S) + xq;
  const bool row_in = sy >= 0 && sy < h;
  f32x4 v[C];
  uint32_t tg = 0, mk = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sx = sx0 + j;
    const bool in = row_in && sx >= 0 && sx < w;    // inside the image's own extent (h <= H, w <= W)
    int r, g, b, ir;
    seg_load<CS>(in ? im : nullptr, sy, sx, H, W, r, g, b, ir);
    const int l = (in && lb != nullptr) ? (int)lb[(long)sy * W + sx] : 0;       // padded label pixels: fine label 0
    tg |= (uint32_t)ttable[l] << (8 * j);
    mk |= (uint32_t)(rtable != nullptr ? rtable[l] : 1) << (8 * j);
    if (MODE != 2) {
      v[0][j] = lut[r]; v[1][j] = lut[g]; v[2][j] = lut[b];
    }
    if (MODE != 0) v[CG][j] = lut[seg_grey(r, g, b)];
    if (CS == 4) v[C - 1][j] = lut[ir];
  }
  const long plane = (long)S * S, off = (long)y * S + xq;
  float* o = out + (long)n * C * plane + off;
#pragma unroll
  for (int c = 0; c < C; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = v[c];
  *reinterpret_cast<uint32_t*>(targets + (long)n * plane + off) = tg;
  *reinterpret_cast<uint32_t*>(mask + (long)n * plane + off) = mk;
}

extern "C" {

int iic_seg_prepare_test(const void* imgs_u8, int B, int H, int W, int Cs, const void* labels_u8, const int* sizes,
                         const void* target_table, const void* relevance, const int* idx, int N, int S,
                         int no_sobel, int include_rgb, const float* lut, float* imgs, void* targets, void* mask,
                         void* stream) {
  if (!imgs_u8 || !labels_u8 || !target_table || !idx || !lut || !imgs || !targets || !mask) return IIC_ERR_ARG;
  if (B <= 0 || N <= 0 || S <= 0 || H <= 0 || W <= 0) return IIC_ERR_ARG;
  if (Cs != 3 && Cs != 4) return IIC_ERR_UNSUPPORTED;
  if (S % 4 != 0 || S > 4096 || H > 16384 || W > 16384 || N > 65535) return IIC_ERR_UNSUPPORTED;
  const int mode = no_sobel ? 0 : (include_rgb ? 1 : 2);
  const int nquads = S * (S >> 2);
  const dim3 grid((nquads + SEG_TEST_THREADS - 1) / SEG_TEST_THREADS, N);
  hipStream_t s = (hipStream_t)stream;
#define SEG_LAUNCH(CS_, MODE_)                                                                              \
  hipLaunchKernelGGL((seg_prepare_test_kernel<CS_, MODE_>), grid, dim3(SEG_TEST_THREADS), 0, s,             \
                     (const uint8_t*)imgs_u8, (const uint8_t*)labels_u8, sizes, (const uint8_t*)target_table, \
                     (const uint8_t*)relevance, B, H, W, idx, S, lut, imgs, (uint8_t*)targets, (uint8_t*)mask)
  if (Cs == 3) {
    if (mode == 0) SEG_LAUNCH(3, 0);
    else if (mode == 1) SEG_LAUNCH(3, 1);
    else SEG_LAUNCH(3, 2);
  } else {
    if (mode == 0) SEG_LAUNCH(4, 0);
    else if (mode == 1) SEG_LAUNCH(4, 1);
    else SEG_LAUNCH(4, 2);
  }
#undef SEG_LAUNCH
  return iic_launch_status();
}

int iic_seg_augment(const void* imgs_u8, int B, int H, int W, int Cs, const void* labels_u8,
                    const void* relevance, const int* iparams, const float* fparams, int N, int S,
                    int no_sobel, int include_rgb, const float* lut, float* img1, float* img2,
                    void* mask_img1, float* affine2_to_1, void* stream) {
  if (!imgs_u8 || !iparams || !fparams || !lut || !img1 || !img2 || !mask_img1 || !affine2_to_1) return IIC_ERR_ARG;
  if (B <= 0 || N <= 0 || S <= 0 || H <= 0 || W <= 0) return IIC_ERR_ARG;
  if ((labels_u8 == nullptr) != (relevance == nullptr)) return IIC_ERR_ARG;
  if (Cs != 3 && Cs != 4) return IIC_ERR_UNSUPPORTED;
  if (S % 4 != 0 || S > 4096 || H > 16384 || W > 16384) return IIC_ERR_UNSUPPORTED;
  const int pad_y = seg_pad_offset(H, S), pad_x = seg_pad_offset(W, S);
  const int mode = no_sobel ? 0 : (include_rgb ? 1 : 2);
  hipStream_t s = (hipStream_t)stream;
#define SEG_LAUNCH(CS_, MODE_)                                                                            \
  hipLaunchKernelGGL((seg_augment_kernel<CS_, MODE_>), dim3(N), dim3(SEG_THREADS), 0, s,                  \
                     (const uint8_t*)imgs_u8, (const uint8_t*)labels_u8, (const uint8_t*)relevance, B, H, \
                     W, pad_y, pad_x, iparams, fparams, S, lut, img1, img2, (uint8_t*)mask_img1,          \
                     affine2_to_1)
  if (Cs == 3) {
    if (mode == 0) SEG_LAUNCH(3, 0);
    else if (mode == 1) SEG_LAUNCH(3, 1);
    else SEG_LAUNCH(3, 2);
  } else {
    if (mode == 0) SEG_LAUNCH(4, 0);
    else if (mode == 1) SEG_LAUNCH(4, 1);
    else SEG_LAUNCH(4, 2);
  }
#undef SEG_LAUNCH
  return iic_launch_status();
}

// the three resampling flavours of seg_augment_ragged_kernel: no table, iic_seg_resample_tap, iic_seg_resample_tap2
static int seg_ragged_launch(const void* imgs_u8, const long* offsets, const int* sizes, int B, long total_px, int Cs,
                             const void* labels_u8, const void* relevance, const int* iparams, const float* fparams,
                             const iic_seg_resample_tap* taps, const iic_seg_resample_tap2* taps2, int N, int S,
                             int no_sobel, int include_rgb, const float* lut, float* img1, float* img2,
                             void* mask_img1, float* affine2_to_1, void* stream) {
  if (!imgs_u8 || !offsets || !sizes || !iparams || !fparams || !lut || !img1 || !img2 || !mask_img1 || !affine2_to_1)
    return IIC_ERR_ARG;
  if (B <= 0 || N <= 0 || S <= 0 || total_px <= 0) return IIC_ERR_ARG;
  if ((labels_u8 == nullptr) != (relevance == nullptr)) return IIC_ERR_ARG;
  if (Cs != 3 && Cs != 4) return IIC_ERR_UNSUPPORTED;
  if (S % 4 != 0 || S > 4096) return IIC_ERR_UNSUPPORTED;
  const int mode = no_sobel ? 0 : (include_rgb ? 1 : 2);
  hipStream_t s = (hipStream_t)stream;
#define SEG_LAUNCH(CS_, MODE_, RS_)                                                                            \
  hipLaunchKernelGGL((seg_augment_ragged_kernel<CS_, MODE_, RS_>), dim3(N), dim3(SEG_THREADS), 0, s,           \
                     (const uint8_t*)imgs_u8, (const uint8_t*)labels_u8, (const uint8_t*)relevance, offsets,   \
                     sizes, B, total_px, iparams, fparams, taps, taps2, S, lut, img1, img2,                    \
                     (uint8_t*)mask_img1, affine2_to_1)
#define SEG_LAUNCH_MODE(CS_, RS_)              \
  do {                                         \
    if (mode == 0) SEG_LAUNCH(CS_, 0, RS_);    \
    else if (mode == 1) SEG_LAUNCH(CS_, 1, RS_); \
    else SEG_LAUNCH(CS_, 2, RS_);              \
  } while (0)
  if (taps2 != nullptr) {
    if (Cs == 3) SEG_LAUNCH_MODE(3, 2);
    else SEG_LAUNCH_MODE(4, 2);
  } else if (taps == nullptr) {
    if (Cs == 3) SEG_LAUNCH_MODE(3, 0);
    else SEG_LAUNCH_MODE(4, 0);
  } else {
    if (Cs == 3) SEG_LAUNCH_MODE(3, 1);
    else SEG_LAUNCH_MODE(4, 1);
  }
#undef SEG_LAUNCH_MODE
#undef SEG_LAUNCH
  return iic_launch_status();
}

int iic_seg_augment_ragged(const void* imgs_u8, const long* offsets, const int* sizes, int B, long total_px, int Cs,
                           const void* labels_u8, const void* relevance, const int* iparams, const float* fparams,
                           const iic_seg_resample_tap* taps, int N, int S, int no_sobel, int include_rgb,
                           const float* lut, float* img1, float* img2, void* mask_img1, float* affine2_to_1,
                           void* stream) {
  return seg_ragged_launch(imgs_u8, offsets, sizes, B, total_px, Cs, labels_u8, relevance, iparams, fparams, taps,
                           nullptr, N, S, no_sobel, include_rgb, lut, img1, img2, mask_img1, affine2_to_1, stream);
}

int iic_seg_augment_ragged_prescaled(const void* imgs_u8, const long* offsets, const int* sizes, int B, long total_px,
                                     int Cs, const void* labels_u8, const void* relevance, const int* iparams,
                                     const float* fparams, const iic_seg_resample_tap2* taps2, int N, int S,
                                     int no_sobel, int include_rgb, const float* lut, float* img1, float* img2,
                                     void* mask_img1, float* affine2_to_1, void* stream) {
  if (!taps2) return IIC_ERR_ARG;
  return seg_ragged_launch(imgs_u8, offsets, sizes, B, total_px, Cs, labels_u8, relevance, iparams, fparams, nullptr,
                           taps2, N, S, no_sobel, include_rgb, lut, img1, img2, mask_img1, affine2_to_1, stream);
}

int iic_seg_augment_warp(const float* img2, const float* affine1_to_2, const int* flips, const float* base_grid,
                         float* out, int N, int C, int S, void* stream) {
  if (!img2 || !affine1_to_2 || !flips || !base_grid || !out || img2 == out) return IIC_ERR_ARG;
  if (N <= 0 || C <= 0 || S <= 0) return IIC_ERR_ARG;
  if (S > 4096 || C > 8) return IIC_ERR_UNSUPPORTED;
  const long total = (long)N * S * S;
  const long blocks = (total + SEG_WARP_THREADS - 1) / SEG_WARP_THREADS;
  if (blocks > 0x7fffffffL) return IIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(seg_grid_warp_kernel, dim3((unsigned)blocks), dim3(SEG_WARP_THREADS), 0, (hipStream_t)stream, img2,
                     affine1_to_2, flips, base_grid, out, N, C, S);
  return iic_launch_status();
}

}  // extern "C"
