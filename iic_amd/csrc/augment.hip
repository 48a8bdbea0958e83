// GPU-side paired augmentation for the clustering scripts.
//
// Replaces the per-sample PIL pipeline the reference builds in
//   /root/reference/code/utils/cluster/transforms.py:107-217 (sobel_make_transforms, default
//   branch) out of torchvision 0.2.1 transforms:
//     RandomCrop -> Resize (PIL BILINEAR) -> [RandomHorizontalFlip -> ColorJitter] ->
//     custom_greyscale_to_tensor (:12-25)
// with ONE kernel: a workgroup produces one output image entirely in LDS (crop 84x84x3 ->
// 96x96x3 is < 52 KB).  The arithmetic is PIL's, reproduced bit for bit (specification and
// cross-check: oracle/augment_oracle.py::np_pipeline):
//   * resize: Pillow's two-pass convolution resampling -- horizontal then vertical pass, 22-bit
//     fixed-point weights (computed on the host exactly like precompute_coeffs /
//     normalize_coeffs_8bpc), 8-bit rounding after each pass;
//   * brightness / contrast / saturation: ImageEnhance = ImagingBlend(degenerate, image, factor):
//     (float)in1 + factor * (float)(in2 - in1) in float32 WITHOUT fused multiply-add, truncated,
//     clipped; contrast's degenerate is the rounded mean of the L image, saturation's the L image;
//   * hue: Pillow's RGB -> HSV -> RGB round trip (float / double mix of Convert.c) with the uint8
//     wrap-around hue shift of torchvision's adjust_hue;
//   * grey: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; to_tensor: value / 255 in float32
//     (256-entry table from the host).
// The same kernel serves the greyscale scripts' pipelines (transforms.py:220-330, mode "L" images,
// CH = 1): optional RandomRotation first (PIL Image.rotate, NEAREST = ImagingTransformAffine's
// 16.16 fixed-point inverse mapping, zero fill; the coefficients come from the host), a crop size
// chosen per image out of a few (one resampling table per size), ToTensor at the end.  On an L
// image ColorJitter's saturation and hue are identities (ImageEnhance.Color blends the image with
// itself; adjust_hue returns L images unchanged).
// The random parameters (rotation, crop size and offsets, flip, jitter factors and their shuffled
// order) are inputs: iic_amd/augment.py draws them with torchvision's distributions.
// The stages themselves are in aug_stages.h: augment_affine.hip (the RandomAffine of the semi-supervised script) runs
// the same ones behind its affine.
#include "aug_stages.h"

// PIL's C code runs as separate IEEE multiplies and adds (x86-64 builds without FMA): a fused
// a*b+c rounds once instead of twice and flips truncations.  hipcc contracts by default
// (-ffp-contract=fast; the *_rn intrinsics are plain operators in its headers too), so contraction is
// switched off for this translation unit and every step (aug_stages.h, aug_jitter.h) is written as its own operation.
#pragma clang fp contract(off)

template <int CH, bool INC_RGB>
__global__ __launch_bounds__(256) void augment_kernel(
    const uint8_t* __restrict__ imgs, int H, int W, const int* __restrict__ iparams,
    const float* __restrict__ fparams, const AugTabs tabs, const int* __restrict__ bounds,
    const int* __restrict__ kk, int S, const float* __restrict__ lut, float* __restrict__ out,
    const float* __restrict__ norm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ int s_red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int* ip = iparams + (long)n * AUG_IP;
  const float* fp = fparams + (long)n * AUG_FP;
  const int src = ip[0], x0 = ip[1], y0 = ip[2], flip = ip[3], tab = ip[10], rot = ip[11];
  const int crop = tabs.crop[tab], KS = tabs.ksize[tab];
  const int* bnd = bounds + tabs.boff[tab] * 2;
  const int* kt = kk + tabs.koff[tab];
  uint8_t* sB = smem_raw;                                            // [crop][S][CH] after the horizontal pass
  uint8_t* sC = smem_raw + aug_lds_second(crop, S, CH, false);       // [S][S][CH]
  const uint8_t* im = imgs + (long)src * H * W * CH;
  constexpr int C = CH == 1 ? 1 : (INC_RGB ? 4 : 1);

  aug_hpass<CH>(im, H, W, x0, y0, rot != 0, ip, crop, S, bnd, kt, KS, sB, tid);
  __syncthreads();
  aug_vpass<CH>(sB, S, bnd, kt, KS, sC, tid);
  __syncthreads();
  aug_jitter_ops<CH>(sC, S, ip, fp, s_red, tid);
  aug_to_tensor<CH, INC_RGB>(sC, S, flip, lut, norm, out + (long)n * C * S * S, tid);
}

extern "C" {

int iic_augment(const void* imgs_u8, int B, int H, int W, int channels, const int* iparams,
                const float* fparams, int N, const int* tables_host, int n_tables,
                const int* bounds, const int* kk, int S, const float* lut, float* out,
                int include_rgb, const float* norm, void* stream) {
  if (!imgs_u8 || !iparams || !fparams || !tables_host || !bounds || !kk || !lut || !out) return IIC_ERR_ARG;
  if (B <= 0 || N <= 0 || S <= 0 || H <= 0 || W <= 0) return IIC_ERR_ARG;
  if (channels != 1 && channels != 3) return IIC_ERR_UNSUPPORTED;
  AugTabs tabs;
  int max_crop = 0;
  if (!aug_read_tables(tables_host, n_tables, H, W, &tabs, &max_crop)) return IIC_ERR_ARG;
  const size_t lds = aug_lds_bytes(max_crop, S, channels, false);
  if (lds > AUG_LDS_LIMIT) return IIC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int rc = IIC_OK;
  // (the kernel's static s_red comes on top of the dynamic LDS: lds stays below the workgroup's total, see above)
#define AUG_LAUNCH(CH_, RGB_)                                                                     \
  rc = iic_launch_lds<augment_kernel<CH_, RGB_>>(dim3(N), dim3(256), lds, s, (const uint8_t*)imgs_u8, H, W, \
                                                 iparams, fparams, tabs, bounds, kk, S, lut, out, norm)
  if (channels == 1) AUG_LAUNCH(1, false);
  else if (include_rgb) AUG_LAUNCH(3, true);
  else AUG_LAUNCH(3, false);
  return rc ? rc : iic_launch_status();
}

}  // extern "C"
