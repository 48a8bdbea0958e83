// Segmentation k-means evaluation on the device: labels and counts from low-resolution dot products, sampled pixel
// features, and the centre update of mini-batch k-means.
//
// Replaces, in code/utils/segmentation/baselines/kmeans_segmentation_eval.py:
//   :56, :141   x_out = net(imgs, penultimate=True).cpu().numpy()   -- the fp32 [N][512][S][S] up-sampled trunk features
//   :64-66      transpose, boolean mask                                (vgg.py / net10a.py: F.interpolate, bilinear),
//   :143-144                                                           copied to the host once per batch per pass
//   :78-91      the sample of feature rows MiniBatchKMeans is fitted on
//   :104        MiniBatchKMeans(n_clusters=gt_k).fit on the host (sklearn/cluster/_kmeans.py _mini_batch_step,
//               _k_means_minibatch.pyx update_center_dense, MiniBatchKMeans._mini_batch_convergence / _random_reassign)
//   :148-186    kmeans.predict of every unmasked pixel, the flat int32 arrays of the test set, the reorder loop, _acc
//
// A k-means score ||c_j||^2 - 2 x.c_j is linear in x, and so is bilinear interpolation: the dot products are taken at the
// trunk's own resolution (iic_seg_head_fwd, or gather + iic_gemm_f32) and up-sampled as k channels, not 512.
//   seg_kmeans_label_acc_kernel  seg_label_map_kernel's tiling (seg_eval.hip): a workgroup stages the source rows / columns
//       of its output tile in LDS, class-major; a thread owns four consecutive pixels, up-samples every channel with the
//       operations of bilinear_fwd_kernel (seg_head.hip), takes the arg-min of cnorm_j - 2 up_j and folds the four labels
//       with their targets and mask into an LDS histogram, merged with 64-bit integer atomics -- the layout and semantics
//       of seg_contingency_acc_kernel.  One launch per batch; the label map is written only when asked for.
//   seg_feat_sample_kernel       a wave per sampled pixel, lanes over the channels: the four PT neighbours are read
//       (bf16 or fp32) and blended with the same operations.  Only sampled pixels are interpolated.
//   mb_update_kernel / mb_finalize_kernel  c_j <- (c_j w_j + sums_j) / (w_j + counts_j) in float64, w += counts, the
//       reassignment schedule and test, and the early-stopping bookkeeping in a 128-byte state block; the latch of
//       kmeans.hip's state block, whose first four words it shares (iic_kmeans_assign is given the same block).
// No float atomics: the sums come from iic_kmeans_assign's fixed-order partials, so two fits give the same bits.
#include "common.h"
#include "../../include/iic_hip.h"
#include "kmeans_ws.h"
#include "seg_bilinear.h"

#define SK_MAXBINS 16384            // as seg_contingency_acc_kernel
#define SK_LDS_BUDGET (40 * 1024)   // staged sources per workgroup, as seg_label_map_kernel
#define SK_PX 4

// p0 / p1: channel 0 of source rows y0 / y1; channel c of column j is at [c * cs + o0[j]] (left) and [c * cs + o1[j]]
// (right).  score = cnorm - 2 up: the doubling is exact, one rounding in the subtraction.  `s < best` from +inf: a NaN
// never wins, the lowest index wins a tie, and a pixel whose scores are all NaN (or +inf) gets label 0 -- the rule of
// iic_kmeans_assign.
__device__ __forceinline__ uint32_t sk_argmin4(const float* __restrict__ p0, const float* __restrict__ p1, int cs, int k,
                                               const int* o0, const int* o1, const float* lxs, float ly,
                                               const float* __restrict__ cn) {
#pragma clang fp contract(off)
  float best[SK_PX];
  uint32_t lab[SK_PX];
#pragma unroll
  for (int j = 0; j < SK_PX; ++j) {
    best[j] = __builtin_inff();
    lab[j] = 0u;
  }
  for (int c = 0; c < k; ++c) {
    const float* q0 = p0 + (long)c * cs;
    const float* q1 = p1 + (long)c * cs;
    const float cc = cn[c];
#pragma unroll
    for (int j = 0; j < SK_PX; ++j) {
      const float v = sk_blend(q0[o0[j]], q0[o1[j]], q1[o0[j]], q1[o1[j]], lxs[j], ly);
      const float s = cc - 2.f * v;
      if (s < best[j]) {
        best[j] = s;
        lab[j] = (uint32_t)c;
      }
    }
  }
  return lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
}

// dynamic LDS: [nbpad] uint32 bins, [kpad] float cnorm, [lds_floats] staged sources (nbpad, kpad multiples of 4)
__global__ __launch_bounds__(256) void seg_kmeans_label_acc_kernel(
    const float* __restrict__ in, const float* __restrict__ cnorm, const uint8_t* __restrict__ targets,
    const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, unsigned long long* __restrict__ counts, int Hl, int Wl,
    int k, int kt, int S, int qx, int ty, int xtiles, int ytiles, int lds_floats, int vec_store) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int nb = k * kt, nbpad = (nb + 3) & ~3, kpad = (k + 3) & ~3;
  unsigned int* bins = reinterpret_cast<unsigned int*>(smem_raw);
  float* cn = reinterpret_cast<float*>(bins + nbpad);
  float* L = cn + kpad;
  const float sy = (float)Hl / (float)S, sx = (float)Wl / (float)S;
  int b = blockIdx.x;
  const int xt = b % xtiles;
  b /= xtiles;
  const int yt = b % ytiles, n = b / ytiles;
  const int ya = yt * ty, yb = min(S, ya + ty) - 1;
  const int xa = xt * qx * SK_PX, xb = min(S, xa + qx * SK_PX) - 1;
  int ylo, yhi, xlo, xhi, t;
  float f;
  sk_src(ya, sy, Hl, ylo, t, f);
  sk_src(yb, sy, Hl, t, yhi, f);
  sk_src(xa, sx, Wl, xlo, t, f);
  sk_src(xb, sx, Wl, t, xhi, f);
  const int nrows = yhi - ylo + 1, ncols = xhi - xlo + 1, cp = ncols | 1;
  const bool staged = (long)nrows * k * cp <= (long)lds_floats;      // uniform over the workgroup
  const float* src = in + (long)n * Hl * Wl * k;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) bins[i] = 0u;
  for (int i = threadIdx.x; i < k; i += blockDim.x) cn[i] = cnorm[i];
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
  }
  __syncthreads();
  const int ry = threadIdx.x / qx, q = threadIdx.x - ry * qx;
  const int y = ya + ry, x = xa + SK_PX * q;
  unsigned int sel = 0u;
  if (y <= yb && x <= xb) {
    int y0, y1, x0[SK_PX], x1[SK_PX];
    float ly, lx[SK_PX];
    sk_src(y, sy, Hl, y0, y1, ly);
#pragma unroll
    for (int j = 0; j < SK_PX; ++j) sk_src(min(x + j, xb), sx, Wl, x0[j], x1[j], lx[j]);
    uint32_t labs;
    if (staged) {
#pragma unroll
      for (int j = 0; j < SK_PX; ++j) {
        x0[j] -= xlo;
        x1[j] -= xlo;
      }
      labs = sk_argmin4(L + (long)(y0 - ylo) * k * cp, L + (long)(y1 - ylo) * k * cp, cp, k, x0, x1, lx, ly, cn);
    } else {
#pragma unroll
      for (int j = 0; j < SK_PX; ++j) {
        x0[j] *= k;
        x1[j] *= k;
      }
      labs = sk_argmin4(src + (long)y0 * Wl * k, src + (long)y1 * Wl * k, 1, k, x0, x1, lx, ly, cn);
    }
    const long p = ((long)n * S + y) * S + x;
    if (out) {
      if (vec_store && x + SK_PX - 1 <= xb) {
        *reinterpret_cast<uint32_t*>(out + p) = labs;      // S % 4 == 0 and a 4-byte aligned base: every quad is aligned
      } else {
        for (int j = 0; j < SK_PX && x + j <= xb; ++j) out[p + j] = (uint8_t)(labs >> (8 * j));
      }
    }
    for (int j = 0; j < SK_PX && x + j <= xb; ++j) {
      if (!mask || mask[p + j]) {
        ++sel;
        const unsigned int pi = (labs >> (8 * j)) & 0xffu, gi = targets[p + j];
        if (gi < (unsigned int)kt) atomicAdd(&bins[pi * kt + gi], 1u);      // pi < k always
      }
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
static long sk_tile_floats(int Hl, int Wl, int k, int S, int qx, int ty) {
  const double sy = (double)Hl / S, sx = (double)Wl / S;
  long rows = ty == 1 ? 2 : (long)((ty - 1) * sy + 1e-3) + 3;
  long cols = (long)((qx * SK_PX - 1) * sx + 1e-3) + 3;
  if (rows > Hl) rows = Hl;
  if (cols > Wl) cols = Wl;
  return rows * k * (cols | 1);
}

struct sk_plan {
  int qx, ty;
  long lds_floats;      // 0: not even one quad's sources fit the budget -- global reads
};
static sk_plan sk_plan_make(int Hl, int Wl, int k, int S) {
  sk_plan p;
  p.qx = 1;
  while (p.qx < 64 && p.qx * SK_PX < S) p.qx <<= 1;       // quads per tile row: up to 256 pixels
  p.ty = 256 / p.qx;
  if (p.ty > S) p.ty = S;
  const long budget = SK_LDS_BUDGET / (long)sizeof(float);
  while (sk_tile_floats(Hl, Wl, k, S, p.qx, p.ty) > budget) {
    if (p.ty > 1) p.ty = (p.ty + 1) / 2;
    else if (p.qx > 1) p.qx >>= 1;
    else break;
  }
  p.lds_floats = sk_tile_floats(Hl, Wl, k, S, p.qx, p.ty);
  if (p.lds_floats > budget) p.lds_floats = 0;
  return p;
}

// a wave per sampled pixel (grid-stride), lanes over the channels.  Coordinates are device data: clamped into range.
template <typename T>
__global__ __launch_bounds__(256) void seg_feat_sample_kernel(const T* __restrict__ pt, const int* __restrict__ coords,
                                                              float* __restrict__ rows, long m, int N, int Hl, int Wl,
                                                              int Hp, int Wp, int off, int C, int S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float sy = (float)Hl / (float)S, sx = (float)Wl / (float)S;
  for (long i = (long)blockIdx.x * 4 + wave; i < m; i += (long)gridDim.x * 4) {
    int n = coords[3 * i], y = coords[3 * i + 1], x = coords[3 * i + 2];
    n = min(max(n, 0), N - 1);
    y = min(max(y, 0), S - 1);
    x = min(max(x, 0), S - 1);
    int y0, y1, x0, x1;
    float ly, lx;
    sk_src(y, sy, Hl, y0, y1, ly);
    sk_src(x, sx, Wl, x0, x1, lx);
    const T* r0 = pt + ((long)n * Hp + y0 + off) * Wp * C;
    const T* r1 = pt + ((long)n * Hp + y1 + off) * Wp * C;
    const long c0 = (long)(x0 + off) * C, c1 = (long)(x1 + off) * C;
    float* o = rows + i * C;
    for (int c = lane; c < C; c += 64)
      o[c] = sk_blend(sk_ld<T>(r0 + c0 + c), sk_ld<T>(r0 + c1 + c), sk_ld<T>(r1 + c0 + c), sk_ld<T>(r1 + c1 + c), lx, ly);
  }
}

// ---- mini-batch k-means: centre update, reassignment test, early-stopping bookkeeping ---------------------------------------
struct mb_state {
  int step;               // completed mini-batch steps
  int converged;          // 0 running, 1 no improvement of the smoothed inertia, 2 shift <= tol
  int pause;              // the reassignment test fired: the host reassigns, clears pause and resumes the step
  int changed;            // (written by iic_kmeans_assign, which is given this block for its latch; not read here)
  int n_since;            // samples since the last reassignment step
  int no_improvement;
  int have_ewa, have_min;
  int reassign_every;     // host: 10 k
  int max_no_improvement; // host: < 0 for None
  double inertia;         // batch inertia of the step's assignment (old centres)
  double ewa, ewa_min;
  double shift;           // squared centre shift of the step
  double tol;             // host
  double alpha;           // host: min(1, 2 batch / (n + 1))
  double ratio;           // host: reassignment_ratio
  double norm;            // host: the batch size the inertia is divided by
  double pad[3];
};
static_assert(sizeof(mb_state) == 128, "iic_hip.h documents 128 bytes");

__device__ __forceinline__ bool mb_latched(const mb_state* st) { return (st->converged | st->pause) != 0; }

__global__ __launch_bounds__(256) void mb_update_kernel(float* __restrict__ C, float* __restrict__ Cold,
                                                        const float* __restrict__ sums,
                                                        const long long* __restrict__ counts,
                                                        const double* __restrict__ w, int d, int resume,
                                                        double* __restrict__ shift_part, const mb_state* __restrict__ st) {
  __shared__ double s_red[32];
  if (mb_latched(st)) return;
  const int j = blockIdx.x;
  const long long cnt = counts[j];
  const double wj = w[j], wn = wj + (double)cnt;
  double sh = 0.0;
  for (int t = threadIdx.x; t < d; t += 256) {
    const long e = (long)j * d + t;
    float old, cn;
    if (resume) {
      old = Cold[e];
      cn = C[e];
    } else {
      old = cn = C[e];
      Cold[e] = old;
      if (cnt > 0) {
        cn = (float)(((double)old * wj + (double)sums[e]) / wn);
        C[e] = cn;
      }
    }
    const double df = (double)cn - (double)old;
    sh += df * df;
  }
  sh = block_sum_d(sh, s_red);
  if (threadIdx.x == 0) shift_part[j] = sh;
}

__global__ __launch_bounds__(256) void mb_finalize_kernel(const long long* __restrict__ counts, double* __restrict__ w,
                                                          int k, long rows, int resume,
                                                          const double* __restrict__ shift_part,
                                                          const double* __restrict__ inertia_part, long W,
                                                          mb_state* __restrict__ st) {
#pragma clang fp contract(off)
  __shared__ int s_flag;
  __shared__ double s_red[32];
  if (mb_latched(st)) return;
  if (!resume) {
    if (threadIdx.x == 0) s_flag = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 256) {
      const double wj = w[j];
      if (wj == 0.0) atomicOr(&s_flag, 1);      // _random_reassign: an empty centre always asks for a reassignment step
      w[j] = wj + (double)counts[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int ns = st->n_since + (int)rows;
      const bool rr = s_flag != 0 || ns >= st->reassign_every;
      if (rr) ns = 0;
      st->n_since = ns;
      int fire = 0;
      if (rr && st->ratio > 0.0) {
        double wmax = w[0];
        for (int j = 1; j < k; ++j) wmax = w[j] > wmax ? w[j] : wmax;
        const double thr = st->ratio * wmax;
        for (int j = 0; j < k; ++j) fire |= w[j] < thr ? 1 : 0;
      }
      s_flag = fire;
    }
    __syncthreads();
    if (s_flag) {
      if (threadIdx.x == 0) st->pause = 1;
      return;
    }
  }
  // the preceding iic_kmeans_assign's partials, in the fixed order of kmeans.hip's km_sum_fixed
  double v = 0.0;
  for (long i = threadIdx.x; i < W; i += 256) v += inertia_part[i];
  const double inertia = block_sum_d(v, s_red);
  if (threadIdx.x == 0) {
    double shift = 0.0;
    for (int j = 0; j < k; ++j) shift += shift_part[j];
    const int step = st->step + 1;
    st->step = step;
    st->shift = shift;
    st->inertia = inertia;
    const double bi = inertia / st->norm;
    if (step > 1) {      // the first step's inertia is the initialisation's
      if (!st->have_ewa) {
        st->ewa = bi;
        st->have_ewa = 1;
      } else {
        const double a = st->alpha;
        st->ewa = st->ewa * (1.0 - a) + bi * a;
      }
      if (st->tol > 0.0 && shift <= st->tol) {
        st->converged = 2;
      } else {
        if (!st->have_min || st->ewa < st->ewa_min) {
          st->no_improvement = 0;
          st->ewa_min = st->ewa;
          st->have_min = 1;
        } else {
          st->no_improvement = st->no_improvement + 1;
        }
        if (st->max_no_improvement >= 0 && st->no_improvement >= st->max_no_improvement) st->converged = 1;
      }
    }
  }
}

extern "C" {

long iic_seg_kmeans_label_lds_floats(int Hl, int Wl, int k, int S) {
  if (Hl <= 0 || Wl <= 0 || S <= 0 || k < 1 || k > 255) return -1;
  return sk_plan_make(Hl, Wl, k, S).lds_floats;
}

int iic_seg_kmeans_label_acc(const float* dots_nhwc, const float* cnorm, const unsigned char* targets_u8,
                             const unsigned char* mask_u8, int N, int Hl, int Wl, int k, int S, int k_gt,
                             long long* counts, unsigned char* labels_u8, void* stream) {
  if (!dots_nhwc || !cnorm || !targets_u8 || !counts || N <= 0 || Hl <= 0 || Wl <= 0 || S <= 0 || k_gt <= 0)
    return IIC_ERR_ARG;
  if (k < 1 || k > 255 || (long)k * k_gt > SK_MAXBINS) return IIC_ERR_UNSUPPORTED;
  const sk_plan p = sk_plan_make(Hl, Wl, k, S);
  const int xtiles = (S + p.qx * SK_PX - 1) / (p.qx * SK_PX), ytiles = (S + p.ty - 1) / p.ty;
  const long grid = (long)N * xtiles * ytiles;
  if (grid > 0x7fffffffL) return IIC_ERR_UNSUPPORTED;
  const int threads = ((p.qx * p.ty + 63) / 64) * 64;
  const int vec = (S % SK_PX == 0) && (((uintptr_t)labels_u8 & 3) == 0);
  const size_t lds = ((size_t)((k * k_gt + 3) & ~3) + (size_t)((k + 3) & ~3) + (size_t)p.lds_floats) * sizeof(float);
  const int rc = iic_launch_lds<seg_kmeans_label_acc_kernel>(
      dim3((unsigned)grid), dim3(threads), lds, (hipStream_t)stream, dots_nhwc, cnorm, (const uint8_t*)targets_u8,
      (const uint8_t*)mask_u8, (uint8_t*)labels_u8, (unsigned long long*)counts, Hl, Wl, k, k_gt, S, p.qx, p.ty, xtiles,
      ytiles, (int)p.lds_floats, vec);
  return rc ? rc : iic_launch_status();
}

int iic_seg_feat_sample(const void* pt, int pt_is_f32, const int* coords, long m, float* rows, int N, int Hl, int Wl,
                        int Hp, int Wp, int off, int C, int S, void* stream) {
  if (m == 0) return IIC_OK;
  if (!pt || !coords || !rows || m < 0 || N <= 0 || Hl <= 0 || Wl <= 0 || S <= 0 || C < 1 || off < 0 || Hl + off > Hp ||
      Wl + off > Wp)
    return IIC_ERR_ARG;
  long g = (m + 3) / 4;
  if (g > 65536) g = 65536;
  if (pt_is_f32)
    hipLaunchKernelGGL(seg_feat_sample_kernel<float>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                       (const float*)pt, coords, rows, m, N, Hl, Wl, Hp, Wp, off, C, S);
  else
    hipLaunchKernelGGL(seg_feat_sample_kernel<bf16_t>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)pt, coords, rows, m, N, Hl, Wl, Hp, Wp, off, C, S);
  return iic_launch_status();
}

int iic_kmeans_minibatch_update(float* C, float* C_old, const float* sums, const long long* counts, double* w, long n,
                                int d, int k, int resume, void* ws, void* state, void* stream) {
  if (!C || !C_old || !sums || !counts || !w || !ws || !state) return IIC_ERR_ARG;
  km_plan p;
  if (!km_plan_make(n, d, k, &p)) return IIC_ERR_UNSUPPORTED;
  const km_ws wsp = km_ws_make(ws, p, d, k);
  hipStream_t s = (hipStream_t)stream;
  mb_state* st = (mb_state*)state;
  hipLaunchKernelGGL(mb_update_kernel, dim3(k), dim3(256), 0, s, C, C_old, sums, counts, w, d, resume, wsp.shift_part, st);
  hipLaunchKernelGGL(mb_finalize_kernel, dim3(1), dim3(256), 0, s, counts, w, k, n, resume, wsp.shift_part,
                     wsp.inertia_part, p.W, st);
  return iic_launch_status();
}

}  // extern "C"
