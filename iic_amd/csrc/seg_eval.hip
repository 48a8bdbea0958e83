// Segmentation evaluation on the device: uint8 label maps straight from the low-resolution softmax, and a
// streaming cluster-vs-class count.
//
// Replaces, in code/utils/segmentation/segmentation_eval.py (_segmentation_get_data):
//   :84      x_outs = net(imgs)                 -- the [N][k][S][S] fp32 probability maps, written only to be
//   :100     torch.argmax(x_outs_curr, dim=1)      read once by the arg-max (int64 out)
//   :101-106 the copies into flat uint8 arrays that span the whole test set
//   :126-128 masked_select of all of them
// and, in code/utils/cluster/cluster_eval.py, everything :128-132 and :212-228 derive from those flat arrays
// (the reorder loop `reordered_preds[flat_preds == pred_i] = target_i` and _acc): all of it is a function of one
// k_pred x k_gt count matrix, which seg_contingency_acc_kernel accumulates batch by batch.
//
//   seg_label_map_kernel: labels[n][y][x] = first arg-max over c of bilinear(probs[n][.][.][c]) at (y, x).  The value
//     of every class is the fp32 number bilinear_fwd_kernel (seg_head.hip) stores: same source-index function, same
//     blend, operation by operation (see sl_src).  A workgroup owns a tile of output rows x columns and stages the source rows / columns the tile
//     touches in LDS, class-major ([row][class][column], odd column pitch: the transposing writes and the strided reads
//     both spread over the banks).  One thread owns four consecutive pixels of a row and loops over the classes; the
//     four labels leave as one 32-bit store.  A tile whose sources do not fit the LDS it was given reads global memory.
//   seg_contingency_acc_kernel: 16-byte loads of the three uint8 streams, per-workgroup LDS histogram merged with
//     64-bit integer atomics (integer adds commute: the result does not depend on arrival order).
#include "common.h"
#include "../../include/iic_hip.h"

#define SE_MAXBINS 16384            // as contingency_kernel (eval_metrics.hip)
#define SL_LDS_BUDGET (40 * 1024)   // per workgroup: Potsdam (Wl 102, k 24) stages 4 source rows in 39.6 KB
#define SL_PX 4

// The labels must be the arg-max of the very numbers bilinear_fwd_kernel stores, so the arithmetic below is pinned
// operation by operation instead of being left to -ffp-contract: the same source expression, inlined into this
// kernel's four-pixel loop, was contracted differently (the final sum became an fma).  What bilinear_fwd_kernel's code
// object computes for gfx950, read from its disassembly:
//   s   = fma(d + 0.5, scale, -0.5)
//   top = fma(v01, lx, v00 * (1 - lx)),  bot = fma(v10, 1 - lx, v11 * lx)
//   out = (1 - ly) * top + ly * bot          -- two rounded products, one add
// tests/test_gpu_seg_eval.py compares the labels with the arg-max of iic_bilinear_fwd's output and fails if a compiler
// ever contracts that kernel another way.

// the source-index function of seg_head.hip (F.interpolate, bilinear, align_corners=False)
__device__ __forceinline__ void sl_src(int d, float scale, int in, int& i0, int& i1, float& lam) {
#pragma clang fp contract(off)
  float s = __builtin_fmaf((float)d + 0.5f, scale, -0.5f);
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = s - (float)i0;
}

// p0 / p1: class 0 of source rows y0 / y1; class c of column j is at [c * cs + o0[j]] (left) and [c * cs + o1[j]] (right)
__device__ __forceinline__ uint32_t sl_argmax4(const float* __restrict__ p0, const float* __restrict__ p1, int cs, int k,
                                               const int* o0, const int* o1, const float* lxs, float ly) {
#pragma clang fp contract(off)
  float best[SL_PX];
  uint32_t lab[SL_PX];
#pragma unroll
  for (int j = 0; j < SL_PX; ++j) {
    best[j] = -__builtin_inff();
    lab[j] = 0u;
  }
  for (int c = 0; c < k; ++c) {
    const float* q0 = p0 + (long)c * cs;
    const float* q1 = p1 + (long)c * cs;
#pragma unroll
    for (int j = 0; j < SL_PX; ++j) {
      const float lx = lxs[j];
      const float v00 = q0[o0[j]], v01 = q0[o1[j]];
      const float v10 = q1[o0[j]], v11 = q1[o1[j]];
      const float top = __builtin_fmaf(v01, lx, v00 * (1.f - lx));
      const float bot = __builtin_fmaf(v10, 1.f - lx, v11 * lx);
      const float v = (1.f - ly) * top + ly * bot;
      if (v > best[j]) {          // strict: the lowest class index wins a tie
        best[j] = v;
        lab[j] = (uint32_t)c;
      }
    }
  }
  return lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
}

__global__ __launch_bounds__(256) void seg_label_map_kernel(const float* __restrict__ in, uint8_t* __restrict__ out,
                                                            int Hl, int Wl, int k, int S, int qx, int ty, int xtiles,
                                                            int ytiles, int lds_floats, int vec_store) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* L = reinterpret_cast<float*>(smem_raw);
  const float sy = (float)Hl / (float)S, sx = (float)Wl / (float)S;
  int b = blockIdx.x;
  const int xt = b % xtiles;
  b /= xtiles;
  const int yt = b % ytiles, n = b / ytiles;
  // output rows [ya, yb] x columns [xa, xb] of this tile, and the source rows / columns they blend (sl_src is monotonic)
  const int ya = yt * ty, yb = min(S, ya + ty) - 1;
  const int xa = xt * qx * SL_PX, xb = min(S, xa + qx * SL_PX) - 1;
  int ylo, yhi, xlo, xhi, t;
  float f;
  sl_src(ya, sy, Hl, ylo, t, f);
  sl_src(yb, sy, Hl, t, yhi, f);
  sl_src(xa, sx, Wl, xlo, t, f);
  sl_src(xb, sx, Wl, t, xhi, f);
  const int nrows = yhi - ylo + 1, ncols = xhi - xlo + 1, cp = ncols | 1;
  const bool staged = (long)nrows * k * cp <= (long)lds_floats;      // uniform over the workgroup
  const float* src = in + (long)n * Hl * Wl * k;
  if (staged) {
    const int run = ncols * k;                                       // contiguous in global memory
    for (int r = 0; r < nrows; ++r) {
      const float* g = src + ((long)(ylo + r) * Wl + xlo) * k;
      float* l = L + (long)r * k * cp;
      for (int i = threadIdx.x; i < run; i += blockDim.x) {
        const int x = i / k, c = i - x * k;
        l[c * cp + x] = g[i];
      }
    }
    __syncthreads();
  }
  const int ry = threadIdx.x / qx, q = threadIdx.x - ry * qx;
  const int y = ya + ry, x = xa + SL_PX * q;
  if (y > yb || x > xb) return;
  int y0, y1, x0[SL_PX], x1[SL_PX];
  float ly, lx[SL_PX];
  sl_src(y, sy, Hl, y0, y1, ly);
#pragma unroll
  for (int j = 0; j < SL_PX; ++j) sl_src(min(x + j, xb), sx, Wl, x0[j], x1[j], lx[j]);
  uint32_t labs;
  if (staged) {
#pragma unroll
    for (int j = 0; j < SL_PX; ++j) {
      x0[j] -= xlo;
      x1[j] -= xlo;
    }
    labs = sl_argmax4(L + (long)(y0 - ylo) * k * cp, L + (long)(y1 - ylo) * k * cp, cp, k, x0, x1, lx, ly);
  } else {
#pragma unroll
    for (int j = 0; j < SL_PX; ++j) {
      x0[j] *= k;
      x1[j] *= k;
    }
    labs = sl_argmax4(src + (long)y0 * Wl * k, src + (long)y1 * Wl * k, 1, k, x0, x1, lx, ly);
  }
  uint8_t* o = out + ((long)n * S + y) * S + x;
  if (vec_store && x + SL_PX - 1 <= xb) {
    *reinterpret_cast<uint32_t*>(o) = labs;       // S % 4 == 0 and a 4-byte aligned base: every quad is aligned
  } else {
    for (int j = 0; j < SL_PX && x + j <= xb; ++j) o[j] = (uint8_t)(labs >> (8 * j));
  }
}

__global__ __launch_bounds__(256) void seg_contingency_acc_kernel(const uint8_t* __restrict__ preds,
                                                                  const uint8_t* __restrict__ targets,
                                                                  const uint8_t* __restrict__ mask, long n, long nvec,
                                                                  int kp, int kt,
                                                                  unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned int* bins = reinterpret_cast<unsigned int*>(smem_raw);
  const int nb = kp * kt;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) bins[i] = 0u;
  __syncthreads();
  // a workgroup handles < 2^32 samples (grid-stride over at most n / gridDim): 32-bit bins and counters suffice
  unsigned int sel = 0u;
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
  for (long v = tid; v < nvec; v += nthr) {
    const u32x4 p = reinterpret_cast<const u32x4*>(preds)[v];
    const u32x4 g = reinterpret_cast<const u32x4*>(targets)[v];
    u32x4 m = {0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
    if (mask) m = reinterpret_cast<const u32x4*>(mask)[v];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
      for (int s = 0; s < 32; s += 8) {
        if ((m[w] >> s) & 0xffu) {
          ++sel;
          const unsigned int pi = (p[w] >> s) & 0xffu, gi = (g[w] >> s) & 0xffu;
          if (pi < (unsigned int)kp && gi < (unsigned int)kt) atomicAdd(&bins[pi * kt + gi], 1u);
        }
      }
    }
  }
  for (long i = nvec * 16 + tid; i < n; i += nthr) {      // n % 16 (or everything, for unaligned streams)
    if (!mask || mask[i]) {
      ++sel;
      const unsigned int pi = preds[i], gi = targets[i];
      if (pi < (unsigned int)kp && gi < (unsigned int)kt) atomicAdd(&bins[pi * kt + gi], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += blockDim.x)
    if (bins[i]) atomicAdd(&counts[i], (unsigned long long)bins[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sel += __shfl_xor(sel, o, 64);
  if ((threadIdx.x & 63) == 0 && sel) atomicAdd(&counts[nb], (unsigned long long)sel);
}

// LDS floats a tile of ty output rows x qx quads needs at most (the kernel re-derives the exact footprint and reads
// global memory if it was given less)
static long sl_tile_floats(int Hl, int Wl, int k, int S, int qx, int ty) {
  const double sy = (double)Hl / S, sx = (double)Wl / S;
  long rows = ty == 1 ? 2 : (long)((ty - 1) * sy + 1e-3) + 3;
  long cols = (long)((qx * SL_PX - 1) * sx + 1e-3) + 3;
  if (rows > Hl) rows = Hl;
  if (cols > Wl) cols = Wl;
  return rows * k * (cols | 1);
}

extern "C" {

int iic_seg_label_map(const float* probs_nhwc, unsigned char* labels_u8, int N, int Hl, int Wl, int k, int S,
                      void* stream) {
  if (!probs_nhwc || !labels_u8 || N <= 0 || Hl <= 0 || Wl <= 0 || S <= 0 || k < 1 || k > 255) return IIC_ERR_ARG;
  int qx = 1;
  while (qx < 64 && qx * SL_PX < S) qx <<= 1;       // quads per tile row: up to 256 pixels
  int ty = 256 / qx;
  if (ty > S) ty = S;
  const long budget = SL_LDS_BUDGET / (long)sizeof(float);
  while (sl_tile_floats(Hl, Wl, k, S, qx, ty) > budget) {
    if (ty > 1) ty = (ty + 1) / 2;
    else if (qx > 1) qx >>= 1;
    else break;
  }
  long lds_floats = sl_tile_floats(Hl, Wl, k, S, qx, ty);
  if (lds_floats > budget) lds_floats = 0;           // not even one quad's sources fit: global reads
  const int xtiles = (S + qx * SL_PX - 1) / (qx * SL_PX), ytiles = (S + ty - 1) / ty;
  const long grid = (long)N * xtiles * ytiles;
  if (grid > 0x7fffffffL) return IIC_ERR_ARG;
  const int threads = ((qx * ty + 63) / 64) * 64;
  const int vec = (S % SL_PX == 0) && (((uintptr_t)labels_u8 & 3) == 0);
  hipLaunchKernelGGL(seg_label_map_kernel, dim3((unsigned)grid), dim3(threads), (size_t)lds_floats * sizeof(float),
                     (hipStream_t)stream, probs_nhwc, (uint8_t*)labels_u8, Hl, Wl, k, S, qx, ty, xtiles, ytiles,
                     (int)lds_floats, vec);
  return iic_launch_status();
}

int iic_seg_contingency_acc(const unsigned char* preds_u8, const unsigned char* targets_u8,
                            const unsigned char* mask_u8, long n, int k_pred, int k_gt, long long* counts,
                            void* stream) {
  if (!preds_u8 || !targets_u8 || !counts || n < 0 || k_pred <= 0 || k_gt <= 0) return IIC_ERR_ARG;
  if ((long)k_pred * k_gt > SE_MAXBINS) return IIC_ERR_UNSUPPORTED;
  if (n == 0) return IIC_OK;
  const uintptr_t al = (uintptr_t)preds_u8 | (uintptr_t)targets_u8 | (uintptr_t)mask_u8;
  const long nvec = (al & 15) ? 0 : n / 16;
  const size_t lds = sizeof(unsigned int) * (size_t)k_pred * k_gt;
  const long work = nvec + (n - nvec * 16);
  long blocks = (work + 255) / 256;
  const int grid = (int)(blocks < 1024 ? blocks : 1024);
  const int rc = iic_launch_lds<seg_contingency_acc_kernel>(dim3(grid), dim3(256), lds, (hipStream_t)stream, preds_u8,
                                                            targets_u8, mask_u8, n, nvec, k_pred, k_gt,
                                                            (unsigned long long*)counts);
  return rc ? rc : iic_launch_status();
}

}  // extern "C"
