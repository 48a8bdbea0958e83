// RandomAffine of the semi-supervised script's tf2 on the device (code/utils/cluster/transforms.py:152-161;
// examples/commands.txt section 1.3, model 698: --random_affine --affine_p 0.5): iic_augment with, per output image,
//   RandomApply([RandomAffine(18, scale, translate, shear, resample=BILINEAR, fillcolor=0)], p)
// between the RandomCrop and the cutout / Resize.  torchvision 0.2.1 hands the inverse matrix to PIL's
// Image.transform(size, AFFINE, m, BILINEAR); this kernel restates that call bit for bit (aug_stages.h:
// aug_affine_bilinear; specification tests/augment_affine_cases.py::np_affine_bilinear, checked there against Pillow's
// own transform).  The affine acts on the crop as an image of its own -- extents, clamps and the zero fill are the crop's,
// never the dataset image's -- so a workgroup first puts the raw crop into LDS (through the 16.16 rotation gather when
// the whole image is rotated first: the reference allows --fluid_warp with --random_affine), resamples it into a second
// LDS plane in IEEE double, and then runs iic_augment's own stages on that plane: horizontal pass with the cutout test,
// vertical pass, ColorJitter, tensor conversion.  A row without the affine switch (bit 1 of iparams[11]) takes
// iic_augment's path from global memory and gives iic_augment's bits.
#include "aug_stages.h"

// no fused multiply-add anywhere: see augment.hip
#pragma clang fp contract(off)

template <bool INC_RGB>
__global__ __launch_bounds__(256) void augment_affine_kernel(
    const uint8_t* __restrict__ imgs, int H, int W, const int* __restrict__ iparams,
    const float* __restrict__ fparams, const double* __restrict__ aparams, const AugTabs tabs,
    const int* __restrict__ bounds, const int* __restrict__ kk, int S, const float* __restrict__ lut,
    float* __restrict__ out, const float* __restrict__ norm) {
  constexpr int CH = 3, C = INC_RGB ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ int s_red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int* ip = iparams + (long)n * AUG_IP;
  const float* fp = fparams + (long)n * AUG_FP;
  const int src = ip[0], x0 = ip[1], y0 = ip[2], flip = ip[3], tab = ip[10];
  const bool rot = ip[11] & 1, affine = ip[11] & 2;       // uniform over the workgroup
  const int crop = tabs.crop[tab], KS = tabs.ksize[tab];
  const int* bnd = bounds + tabs.boff[tab] * 2;
  const int* kt = kk + tabs.koff[tab];
  // two regions (aug_lds_bytes): raw crop, then the horizontal pass's plane | affined crop, then the vertical pass's
  uint8_t* sB = smem_raw;
  uint8_t* sC = smem_raw + aug_lds_second(crop, S, CH, true);
  const uint8_t* im = imgs + (long)src * H * W * CH;

  if (affine) {
    uint8_t *sA = sB, *sT = sC;
    aug_crop_gather<CH>(im, H, W, x0, y0, rot, ip, crop, sA, tid);
    __syncthreads();
    aug_affine_bilinear<CH>(sA, crop, aparams + (long)n * AUG_AP, sT, tid);
    __syncthreads();                                       // sA is dead: the horizontal pass may overwrite it
    aug_hpass<CH>(sT, crop, crop, 0, 0, false, ip, crop, S, bnd, kt, KS, sB, tid);
  } else {
    aug_hpass<CH>(im, H, W, x0, y0, rot, ip, crop, S, bnd, kt, KS, sB, tid);
  }
  __syncthreads();                                         // sT is dead: the vertical pass may overwrite it
  aug_vpass<CH>(sB, S, bnd, kt, KS, sC, tid);
  __syncthreads();
  aug_jitter_ops<CH>(sC, S, ip, fp, s_red, tid);
  aug_to_tensor<CH, INC_RGB>(sC, S, flip, lut, norm, out + (long)n * C * S * S, tid);
}

extern "C" {

int iic_augment_affine(const void* imgs_u8, int B, int H, int W, int channels, const int* iparams,
                       const float* fparams, const double* aparams, int N, const int* tables_host, int n_tables,
                       const int* bounds, const int* kk, int S, const float* lut, float* out,
                       int include_rgb, const float* norm, void* stream) {
  if (!imgs_u8 || !iparams || !fparams || !aparams || !tables_host || !bounds || !kk || !lut || !out) return IIC_ERR_ARG;
  if (B <= 0 || N <= 0 || S <= 0 || H <= 0 || W <= 0) return IIC_ERR_ARG;
  if (channels != 3) return IIC_ERR_UNSUPPORTED;           // greyscale_make_transforms has no affine
  AugTabs tabs;
  int max_crop = 0;
  if (!aug_read_tables(tables_host, n_tables, H, W, &tabs, &max_crop)) return IIC_ERR_ARG;
  const size_t lds = aug_lds_bytes(max_crop, S, channels, true);
  if (lds > AUG_LDS_LIMIT) return IIC_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int rc = IIC_OK;
#define AUG_AFFINE_LAUNCH(RGB_)                                                                                  \
  rc = iic_launch_lds<augment_affine_kernel<RGB_>>(dim3(N), dim3(256), lds, s, (const uint8_t*)imgs_u8, H, W, iparams, \
                                                   fparams, aparams, tabs, bounds, kk, S, lut, out, norm)
  if (include_rgb) AUG_AFFINE_LAUNCH(true);
  else AUG_AFFINE_LAUNCH(false);
  return rc ? rc : iic_launch_status();
}

}  // extern "C"
