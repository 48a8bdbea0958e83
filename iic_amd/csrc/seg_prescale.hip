// pre_scale_all of the segmentation datasets as one pass over a packed dataset: what the reference does to every image
// on EVERY access,
//   code/datasets/segmentation/cocostuff.py:113-120, :242-249, :321-328
//   code/datasets/segmentation/potsdam.py:103-106
// cv2.resize(fx = fy = pre_scale_factor) with INTER_LINEAR on the float image and INTER_NEAREST on the labels, done here
// once for the whole set; the result (truncated to uint8, as `img.astype(np.uint8)` truncates it after the crop) is what
// SegRaggedAugmenter and SegTestPreparer keep resident.  RGB only: Potsdam's IR plane is never truncated after a
// resize (potsdam.py:148-151, :170), a uint8 result cannot hold it (seg_ragged.py, source="original", serves that).
//
// Coefficients: computed IN THE KERNEL (no tables), in double with contraction off, bit-equal to
// iic_amd/seg_ragged.py::linear_taps / nearest_index (seg_resample.h); 1. / factor is divided once on the host.
// OpenCV 3.x's resize restated from its source, NOT compared against a cv2 binary (seg_ragged.py says why).
//
// Shape: the host flattens the set into work items (image, first output row, row count) -- a one-dimensional grid, the
// full COCO set has more images than a grid's y extent -- one workgroup per item.  Per output row the workgroup copies
// the two source rows it interpolates between into LDS with aligned 4-byte loads (each source byte is read once per
// output row, whatever the overlap of neighbouring taps), then a thread per output pixel reads its four taps from LDS;
// consecutive lanes store consecutive 3-byte pixels.  Rows wider than the LDS buffer are done in column chunks.
// No atomics: two calls give identical bytes.
#include "common.h"
#include "seg_resample.h"
#include "../../include/iic_hip.h"

#pragma clang fp contract(off)

#define PRE_THREADS 256
#define PRE_LDS_PX 2048                          // source pixels of one row held at a time
#define PRE_LDS_DWORDS ((PRE_LDS_PX * 3 + 3 + 3) / 4 + 1)
#define PRE_MAX_SIDE 16384

// n source pixels of one row, starting at byte pointer g, into LDS so that LDS byte (g & 3) + k holds g[k]: the
// interior as aligned dwords, the ragged ends byte by byte -- no byte outside [g, g + 3 n) is read.  Returns g & 3.
__device__ __forceinline__ int pre_stage_row(const uint8_t* __restrict__ g, int n, uint32_t* __restrict__ lds, int tid) {
  const int shift = (int)((uintptr_t)g & 3);
  const uint8_t* ga = g - shift;
  const int end = shift + n * 3;
  uint8_t* lb = reinterpret_cast<uint8_t*>(lds);
  for (int i = tid; i < ((end + 3) >> 2); i += PRE_THREADS) {
    const int lo = i << 2;
    if (lo >= shift && lo + 4 <= end) {
      lds[i] = *reinterpret_cast<const uint32_t*>(ga + lo);
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (lo + b >= shift && lo + b < end) lb[lo + b] = ga[lo + b];
    }
  }
  return shift;
}

__global__ __launch_bounds__(PRE_THREADS) void seg_prescale_kernel(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ src_lb, const long* __restrict__ src_off,
    const int* __restrict__ src_sz, int B, long total_px, double inv, uint8_t* __restrict__ dst,
    uint8_t* __restrict__ dst_lb, const long* __restrict__ dst_off, const int* __restrict__ dst_pitch,
    const int* __restrict__ dst_sz, long dst_px, const int* __restrict__ work, int xchunk) {
  __shared__ uint32_t s_row[2][PRE_LDS_DWORDS];
  const int tid = threadIdx.x;
  const int* wk = work + (long)blockIdx.x * 3;
  const int img = wk[0];
  // everything below is uniform over the workgroup.  An image whose source or destination extent would leave its pack
  // is skipped as a whole: nothing of it is read or written.
  if (img < 0 || img >= B) return;
  const int h = src_sz[2 * img], w = src_sz[2 * img + 1];
  const long so = src_off[img];
  if (h < 1 || h > PRE_MAX_SIDE || w < 1 || w > PRE_MAX_SIDE || so < 0 || so > total_px || (long)h * w > total_px - so)
    return;
  const int nh = dst_sz[2 * img], nw = dst_sz[2 * img + 1], pitch = dst_pitch[img];
  const long dof = dst_off[img];
  if (nh < 1 || nh > PRE_MAX_SIDE || nw < 1 || nw > PRE_MAX_SIDE || pitch < nw || dof < 0 || dof > dst_px) return;
  if ((long)(nh - 1) * pitch + nw > dst_px - dof) return;
  const long first = wk[1], count = wk[2];
  const int r0 = first < 0 ? 0 : (first > nh ? nh : (int)first);
  const int r1 = first + count > nh ? nh : (first + count < r0 ? r0 : (int)(first + count));
  const uint8_t* im = src + so * 3;

  for (int y = r0; y < r1; ++y) {
    const seg_linear_tap ty = seg_linear_coeff(y, inv, h);
    const long lrow = src_lb != nullptr ? so + (long)seg_nearest_coeff(y, inv, h) * w : 0;
    for (int xa = 0; xa < nw; xa += xchunk) {
      const int xb = xa + xchunk < nw ? xa + xchunk : nw;
      // taps grow with x: the chunk reads source columns [s_lo, s_lo + span)
      const int s_lo = seg_linear_coeff(xa, inv, w).i0;
      int span = seg_linear_coeff(xb - 1, inv, w).i1 - s_lo + 1;
      span = span < 1 ? 1 : (span > PRE_LDS_PX ? PRE_LDS_PX : span);      // the host sizes xchunk so that it fits
      __syncthreads();                                                     // the previous chunk has been consumed
      const int sh0 = pre_stage_row(im + ((long)ty.i0 * w + s_lo) * 3, span, s_row[0], tid);
      const int sh1 = pre_stage_row(im + ((long)ty.i1 * w + s_lo) * 3, span, s_row[1], tid);
      __syncthreads();
      const uint8_t* top = reinterpret_cast<const uint8_t*>(s_row[0]) + sh0;
      const uint8_t* bot = reinterpret_cast<const uint8_t*>(s_row[1]) + sh1;
      for (int x = xa + tid; x < xb; x += PRE_THREADS) {
        const seg_linear_tap tx = seg_linear_coeff(x, inv, w);
        int o0 = tx.i0 - s_lo, o1 = tx.i1 - s_lo;
        o0 = (o0 < 0 ? 0 : (o0 >= span ? span - 1 : o0)) * 3;
        o1 = (o1 < 0 ? 0 : (o1 >= span ? span - 1 : o1)) * 3;
        uint8_t* d = dst + (dof + (long)y * pitch + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float t = seg_lerp((float)top[o0 + c], tx.a0, (float)top[o1 + c], tx.a1);
          const float b = seg_lerp((float)bot[o0 + c], tx.a0, (float)bot[o1 + c], tx.a1);
          d[c] = (uint8_t)seg_trunc_u8(seg_lerp(t, ty.a0, b, ty.a1));
        }
        if (src_lb != nullptr) dst_lb[dof + (long)y * pitch + x] = src_lb[lrow + seg_nearest_coeff(x, inv, w)];
      }
    }
  }
}

extern "C" {

int iic_seg_prescale(const void* imgs_u8, const void* labels_u8, const long* offsets, const int* sizes, int B,
                     long total_px, double factor, void* out_u8, void* out_labels_u8, const long* out_offsets,
                     const int* out_pitch, const int* out_sizes, long out_px, const int* work, int n_work,
                     void* stream) {
  if (!imgs_u8 || !offsets || !sizes || !out_u8 || !out_offsets || !out_pitch || !out_sizes || !work) return IIC_ERR_ARG;
  if (B <= 0 || total_px <= 0 || out_px <= 0 || n_work <= 0) return IIC_ERR_ARG;
  if ((labels_u8 == nullptr) != (out_labels_u8 == nullptr)) return IIC_ERR_ARG;
  if (!(factor > 0. && factor < 1.)) return IIC_ERR_ARG;                  // cocostuff.py:114
  const double inv = 1.0 / factor;
  // columns per LDS chunk: n consecutive outputs read at most (n - 1) inv + 3 source columns
  const double fit = floor((PRE_LDS_PX - 4) * factor);
  const int xchunk = fit < 1. ? 1 : (int)fit;
  hipLaunchKernelGGL(seg_prescale_kernel, dim3((unsigned)n_work), dim3(PRE_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)imgs_u8, (const uint8_t*)labels_u8, offsets, sizes, B, total_px, inv,
                     (uint8_t*)out_u8, (uint8_t*)out_labels_u8, out_offsets, out_pitch, out_sizes, out_px, work, xchunk);
  return iic_launch_status();
}

}  // extern "C"
