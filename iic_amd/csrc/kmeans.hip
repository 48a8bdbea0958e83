// k-means on trunk features, on the device: Lloyd iteration, k-means++ support, convergence latch.
//
// Replaces the host-side fit of
//   code/utils/cluster/baselines/triplets.py:134-173  (features copied off the GPU batch by batch, then sklearn's
//                                                      KMeans(n_clusters=gt_k).fit on the host)
// for the features every clustering net returns under kmeans_use_features=True (net5g.py:73-78, net6c.py:52-57).
//
// One Lloyd iteration is a chain of six or seven launches on one stream:
//   km_cnorm_kernel    ||c_j||^2, one wave per centroid
//   km_assign_kernel   a workgroup owns P = 64 m consecutive rows (m tiles of 64).  Phase A, per tile: every wave takes 16
//                      rows and all ceil(k / 16) column blocks over the whole of d -- X . C^T on v_mfma_f32_16x16x4_f32 (exact
//                      fp32), x and c fragments loaded straight from global memory as float4 (the k index inside one MFMA
//                      group is permuted the same way for both operands; the next trip's fragments are in flight
//                      while this trip's MFMAs issue) -- then score = ||c||^2 - 2 x.c, arg-min with ties
//                      to the lowest j (a NaN score counts as +inf, padded columns as +inf with j >= k: a label is always
//                      in [0, k)), mind = max(0, ||x||^2 + score).  Phase B: the one-hot sums A^T X of the workgroup's P
//                      rows on the same pipe, a wave per 64-column chunk, written as ONE partial [k][d] per workgroup.
//                      X is read a second time there (from the caches when the P x d block is still in them).  A form
//                      that keeps each 64-row tile in LDS for phase B (d <= 512) was built and measured slower: LAB.md S24.
//   km_reduce_kernel   partial sums added in ascending workgroup order (two launches of fixed groups above 32 partials);
//   km_count_kernel    counts: integer sums of the per-workgroup histograms
//   km_update_kernel   c_j <- sum_j / count_j, per-centroid squared shift in float64
//   km_finalize_kernel shift, inertia (float64, fixed order), iteration counter, the `converged` latch
// No float atomics anywhere: m, the tile order and the reduction groups are functions of (n, d, k) only, so two runs give
// the same bits.  Integer atomics count changed labels.
#include "common.h"
#include "../../include/iic_hip.h"
#include "kmeans_ws.h"

__device__ __forceinline__ bool km_latched(const km_state* st) { return st && (st->converged | st->pause); }

__device__ __forceinline__ f32x4 km_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// four consecutive floats of a row at column t (zeros from d on).  VEC: the row base and t are 16-byte aligned and
// d % 4 == 0, so the four are inside or outside together.
template <bool VEC>
__device__ __forceinline__ f32x4 km_load4(const float* __restrict__ row, int t, int d) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (t < d) v = *reinterpret_cast<const f32x4*>(row + t);
  } else {
    if (t + 0 < d) v[0] = row[t + 0];
    if (t + 1 < d) v[1] = row[t + 1];
    if (t + 2 < d) v[2] = row[t + 2];
    if (t + 3 < d) v[3] = row[t + 3];
  }
  return v;
}

__global__ __launch_bounds__(64) void km_cnorm_kernel(const float* __restrict__ C, int d, float* __restrict__ cnorm,
                                                      const km_state* __restrict__ st) {
  if (km_latched(st)) return;
  const float* row = C + (long)blockIdx.x * d;
  float s = 0.f;
  for (int t = threadIdx.x; t < d; t += 64) s = fmaf(row[t], row[t], s);
  s = wave_sum(s);
  if (threadIdx.x == 0) cnorm[blockIdx.x] = s;
}

// does (av, ai) come before (bv, bi)?  lower score first, then the lower index; no NaN reaches here
__device__ __forceinline__ bool km_before(float av, int ai, float bv, int bi) { return av < bv || (av == bv && ai < bi); }

template <int KB, bool VEC>
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(
    const float* __restrict__ X, long ldx, const float* __restrict__ C, const float* __restrict__ cnorm, long n, int d,
    int k, int m, int* __restrict__ labels, float* __restrict__ mind, float* __restrict__ sum_part,
    int* __restrict__ count_part, double* __restrict__ inertia_part, km_state* __restrict__ st) {
  extern __shared__ int km_dyn[];      // [P] labels, [P] mind of the workgroup's rows: 8 P <= 32 KB
  __shared__ int s_cnt[KM_MAXK];
  __shared__ int s_changed;
  __shared__ double s_red[32];
  if (km_latched(st)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const long wg = blockIdx.x;
  const int P = m * KM_ROWS;
  const long r0 = wg * P;
  int* s_lab = km_dyn;
  float* s_mind = reinterpret_cast<float*>(km_dyn + P);
  for (int i = tid; i < KM_MAXK; i += KM_THREADS) s_cnt[i] = 0;
  if (tid == 0) s_changed = 0;
  __syncthreads();

  // ---- phase A: labels and mind of the workgroup's m tiles; this wave owns rows [16 wave, 16 wave + 16) of each ----
  for (int tile = 0; tile < m; ++tile) {
    const long rbase = r0 + (long)tile * KM_ROWS + wave * 16;      // wave-uniform
    if (rbase < n) {
      long xr = rbase + l15;
      if (xr > n - 1) xr = n - 1;      // rows past the end read the last row; their results are dropped
      const float* xrow = X + xr * ldx;
      const float* crow[KB];
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        int j = b * 16 + l15;
        if (j > k - 1) j = k - 1;      // padded columns read the last centroid; their scores are dropped
        crow[b] = C + (long)j * d;
      }
      f32x4 acc[KB];
#pragma unroll
      for (int b = 0; b < KB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      float xsq = 0.f;
      // UN steps of 16 columns per trip, the next trip's fragments loaded before this trip's MFMAs (zeros from d on)
      constexpr int UN = KB == 1 ? 4 : (KB == 2 ? 2 : 1);
      f32x4 xa[UN], cb[KB][UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        xa[u] = km_load4<VEC>(xrow, 16 * u + 4 * g, d);
#pragma unroll
        for (int b = 0; b < KB; ++b) cb[b][u] = km_load4<VEC>(crow[b], 16 * u + 4 * g, d);
      }
      for (int t0 = 0; t0 < d; t0 += 16 * UN) {
        f32x4 xn[UN], cn[KB][UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const int t = t0 + 16 * UN + 16 * u + 4 * g;
          xn[u] = km_load4<VEC>(xrow, t, d);
#pragma unroll
          for (int b = 0; b < KB; ++b) cn[b][u] = km_load4<VEC>(crow[b], t, d);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            xsq = fmaf(xa[u][e], xa[u][e], xsq);
#pragma unroll
            for (int b = 0; b < KB; ++b) acc[b] = km_mfma(xa[u][e], cb[b][u][e], acc[b]);
          }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          xa[u] = xn[u];
#pragma unroll
          for (int b = 0; b < KB; ++b) cb[b][u] = cn[b][u];
        }
      }
      // ||x||^2 of row (16 wave + l15): the four lane groups hold disjoint columns
      xsq += __shfl_xor(xsq, 16, 64);
      xsq += __shfl_xor(xsq, 32, 64);
      // accumulator register r of lane group g is row 4 g + r, column b * 16 + l15
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float bv = __builtin_inff();
        int bi = 0x7fffffff;
#pragma unroll
        for (int b = 0; b < KB; ++b) {
          const int j = b * 16 + l15;
          float s = __builtin_inff();
          if (j < k) {
            s = fmaf(-2.f, acc[b][r], cnorm[j]);
            if (s != s) s = __builtin_inff();
          }
          if (km_before(s, j, bv, bi)) {
            bv = s;
            bi = j;
          }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (km_before(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
          }
        }
        const float xn = __shfl(xsq, 4 * g + r, 64);
        const long row = rbase + 4 * g + r;
        if (l15 == 0) {
          const int li = tile * KM_ROWS + wave * 16 + 4 * g + r;
          if (row < n) {
            float md = xn + bv;
            md = md < 0.f ? 0.f : md;      // keeps NaN
            if (st && labels[row] != bi) atomicAdd(&s_changed, 1);
            labels[row] = bi;
            mind[row] = md;
            s_lab[li] = bi;
            s_mind[li] = md;
            atomicAdd(&s_cnt[bi], 1);
          } else {
            s_lab[li] = -1;
            s_mind[li] = 0.f;
          }
        }
      }
    } else {
      for (int i = lane; i < 16; i += 64) {
        s_lab[tile * KM_ROWS + wave * 16 + i] = -1;
        s_mind[tile * KM_ROWS + wave * 16 + i] = 0.f;
      }
    }
  }
  __syncthreads();
  if (st && tid == 0 && s_changed) atomicAdd(&st->changed, s_changed);
  if (count_part)
    for (int j = tid; j < k; j += KM_THREADS) count_part[wg * k + j] = s_cnt[j];
  {
    double v = 0.0;
    for (int i = tid; i < P; i += KM_THREADS) v += (double)s_mind[i];
    v = block_sum_d(v, s_red);
    if (tid == 0) inertia_part[wg] = v;
  }
  if (!sum_part) return;

  // ---- phase B: partial[j][t] = sum over the workgroup's rows i with label j of x[i][t]; a wave per 64 columns ----
  long rows = n - r0;
  if (rows > P) rows = P;
  float* part = sum_part + wg * (long)k * d;
  constexpr int BG = KB < 4 ? KB : 4;      // column blocks held in registers at a time (16 BG accumulator registers)
  for (int t0 = wave * 64; t0 < d; t0 += 4 * 64) {
    const int t = t0 + 4 * l15;
    for (int bg = 0; bg < KB && bg * 16 < k; bg += BG) {
      f32x4 acc[BG][4];
#pragma unroll
      for (int b = 0; b < BG; ++b)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[b][e] = f32x4{0.f, 0.f, 0.f, 0.f};
      // 16 rows per trip (four MFMA groups of 4 rows), the next trip's rows loaded before this trip's MFMAs
      f32x4 xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = 4 * u + g;
        xv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < rows) xv[u] = km_load4<VEC>(X + (r0 + i) * ldx, t, d);
      }
      for (int i0 = 0; i0 < rows; i0 += 16) {
        f32x4 xw[4];
        int lab[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + 16 + 4 * u + g;
          xw[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (i < rows) xw[u] = km_load4<VEC>(X + (r0 + i) * ldx, t, d);
          lab[u] = s_lab[i0 + 4 * u + g];      // i0 + 15 < P; -1 past the end matches no column
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int b = 0; b < BG; ++b) {
            const float a = (lab[u] == (bg + b) * 16 + l15) ? 1.f : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[b][e] = km_mfma(a, xv[u][e], acc[b][e]);
          }
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = xw[u];
      }
      // register r of acc[b][e]: centroid (bg + b) * 16 + 4 g + r, column t0 + 4 l15 + e
#pragma unroll
      for (int b = 0; b < BG; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = (bg + b) * 16 + 4 * g + r;
          if (j < k) {
            float* o = part + (long)j * d;
            if (VEC) {
              if (t < d) *reinterpret_cast<f32x4*>(o + t) = f32x4{acc[b][0][r], acc[b][1][r], acc[b][2][r], acc[b][3][r]};
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (t + e < d) o[t + e] = acc[b][e][r];
            }
          }
        }
    }
  }
}

// out[q][e] = in[q * group + 0][e] + in[q * group + 1][e] + ... (ascending, `win` partials in all), e < elems
__global__ __launch_bounds__(256) void km_reduce_kernel(const float* __restrict__ in, long win, int group, long elems,
                                                        float* __restrict__ out, const km_state* __restrict__ st) {
  if (km_latched(st)) return;
  const long e = (long)blockIdx.y * 256 + threadIdx.x;
  if (e >= elems) return;
  const long q = blockIdx.x;
  const long w0 = q * group;
  long w1 = w0 + group;
  if (w1 > win) w1 = win;
  float s = 0.f;
  for (long w = w0; w < w1; ++w) s += in[w * elems + e];
  out[q * elems + e] = s;
}

__global__ __launch_bounds__(256) void km_count_kernel(const int* __restrict__ count_part, long W, int k,
                                                       long long* __restrict__ counts, const km_state* __restrict__ st) {
  __shared__ unsigned long long s_total;
  if (km_latched(st)) return;
  if (threadIdx.x == 0) s_total = 0ull;
  __syncthreads();
  const int j = blockIdx.x;
  unsigned long long c = 0ull;
  for (long w = threadIdx.x; w < W; w += 256) c += (unsigned long long)count_part[w * k + j];
  atomicAdd(&s_total, c);      // integers: any order gives the same sum
  __syncthreads();
  if (threadIdx.x == 0) counts[j] = (long long)s_total;
}

__device__ __forceinline__ bool km_any_empty(const long long* __restrict__ counts, int k, int* flag) {
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += blockDim.x)
    if (counts[j] == 0) atomicOr(flag, 1);
  __syncthreads();
  return *flag != 0;
}

__global__ __launch_bounds__(256) void km_update_kernel(float* __restrict__ C, const float* __restrict__ sums,
                                                        const long long* __restrict__ counts, int d, int k, int force,
                                                        double* __restrict__ shift_part, const km_state* __restrict__ st) {
  __shared__ int s_flag;
  __shared__ double s_red[32];
  if (km_latched(st)) return;
  if (km_any_empty(counts, k, &s_flag) && !force) return;      // the host relocates first
  const int j = blockIdx.x;
  const long long cnt = counts[j];
  double sh = 0.0;
  if (cnt > 0) {
    const double inv = (double)cnt;
    for (int t = threadIdx.x; t < d; t += 256) {
      const float old = C[(long)j * d + t];
      const float cn = (float)((double)sums[(long)j * d + t] / inv);
      const double df = (double)cn - (double)old;
      sh += df * df;
      C[(long)j * d + t] = cn;
    }
  }
  sh = block_sum_d(sh, s_red);
  if (threadIdx.x == 0) shift_part[j] = sh;
}

// sum of `W` doubles in a fixed order: thread t adds elements t, t + 256, ... ascending, then the block folds
__device__ __forceinline__ double km_sum_fixed(const double* __restrict__ p, long W, double* red) {
  double v = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) v += p[w];
  return block_sum_d(v, red);
}

__global__ __launch_bounds__(256) void km_finalize_kernel(const long long* __restrict__ counts, int k, int force,
                                                          const double* __restrict__ shift_part,
                                                          const double* __restrict__ inertia_part, long W,
                                                          km_state* __restrict__ st) {
  __shared__ int s_flag;
  __shared__ double s_red[32];
  if (km_latched(st)) return;
  if (km_any_empty(counts, k, &s_flag) && !force) {
    if (threadIdx.x == 0) st->pause = 1;
    return;
  }
  const double inertia = km_sum_fixed(inertia_part, W, s_red);
  if (threadIdx.x == 0) {
    double shift = 0.0;
    for (int j = 0; j < k; ++j) shift += shift_part[j];
    st->iter = st->iter + 1;
    st->shift = shift;
    st->inertia = inertia;
    if (st->changed == 0) st->converged = 1;
    else if (shift <= st->tol) st->converged = 2;
    st->changed = 0;
  }
}

__global__ __launch_bounds__(256) void km_inertia_kernel(const double* __restrict__ inertia_part, long W,
                                                         double* __restrict__ out) {
  __shared__ double s_red[32];
  const double v = km_sum_fixed(inertia_part, W, s_red);
  if (threadIdx.x == 0) out[0] = v;
}

// k-means++ support: a wave per row, rows wg * 4 + wave, + 4 * gridDim.x, ...  dist_c = sum_t (x[t] - x_cand_c[t])^2 in
// fp32 (lanes stride the columns, then a butterfly), v_c = min(mind, dist_c); per-wave float64 sums of v_c in row order.
__global__ __launch_bounds__(256) void km_seed_kernel(const float* __restrict__ X, long ldx, long n, int d,
                                                      const long long* __restrict__ cand, int ncand,
                                                      float* __restrict__ mind, int write,
                                                      double* __restrict__ seed_part) {
  __shared__ double s_pot[4][KM_MAXCAND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* crow[KM_MAXCAND];
#pragma unroll
  for (int c = 0; c < KM_MAXCAND; ++c) {
    long long ci = c < ncand ? cand[c] : 0;
    if (ci < 0) ci = 0;
    if (ci > n - 1) ci = n - 1;
    crow[c] = X + ci * ldx;
  }
  double pot[KM_MAXCAND];
#pragma unroll
  for (int c = 0; c < KM_MAXCAND; ++c) pot[c] = 0.0;
  for (long r = (long)blockIdx.x * 4 + wave; r < n; r += (long)gridDim.x * 4) {
    const float* xrow = X + r * ldx;
    float acc[KM_MAXCAND];
#pragma unroll
    for (int c = 0; c < KM_MAXCAND; ++c) acc[c] = 0.f;
    for (int t = lane; t < d; t += 64) {
      const float x = xrow[t];
#pragma unroll
      for (int c = 0; c < KM_MAXCAND; ++c)
        if (c < ncand) {
          const float df = x - crow[c][t];
          acc[c] = fmaf(df, df, acc[c]);
        }
    }
    const float md = mind[r];
#pragma unroll
    for (int c = 0; c < KM_MAXCAND; ++c)
      if (c < ncand) {
        const float dist = wave_sum(acc[c]);
        const float v = dist < md ? dist : md;
        pot[c] += (double)v;
        if (write && c == 0 && lane == 0) mind[r] = v;
      }
  }
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < KM_MAXCAND; ++c) s_pot[wave][c] = pot[c];
  __syncthreads();
  if (threadIdx.x < KM_MAXCAND) {
    const int c = threadIdx.x;
    seed_part[(long)blockIdx.x * KM_MAXCAND + c] = ((s_pot[0][c] + s_pot[1][c]) + s_pot[2][c]) + s_pot[3][c];
  }
}

__global__ __launch_bounds__(64) void km_seed_reduce_kernel(const double* __restrict__ seed_part, int wgs, int ncand,
                                                            double* __restrict__ pot) {
  const int c = threadIdx.x;
  if (c >= ncand) return;
  double s = 0.0;
  for (int w = 0; w < wgs; ++w) s += seed_part[(long)w * KM_MAXCAND + c];
  pot[c] = s;
}

template <int KB>
static int km_launch_assign(bool vec, dim3 grid, hipStream_t s, const float* X, long ldx, const float* C,
                            const float* cnorm, long n, int d, int k, int m, int* labels, float* mind, float* sum_part,
                            int* count_part, double* inertia_part, km_state* st) {
  const size_t lds = (size_t)m * KM_ROWS * 8;      // <= 32 KB: below the 48 KB a plain launch may take
  if (vec)
    hipLaunchKernelGGL((km_assign_kernel<KB, true>), grid, dim3(KM_THREADS), lds, s, X, ldx, C, cnorm, n, d, k, m, labels,
                       mind, sum_part, count_part, inertia_part, st);
  else
    hipLaunchKernelGGL((km_assign_kernel<KB, false>), grid, dim3(KM_THREADS), lds, s, X, ldx, C, cnorm, n, d, k, m, labels,
                       mind, sum_part, count_part, inertia_part, st);
  return iic_launch_status();
}

extern "C" {

int iic_kmeans_supported(long n, int d, int k) {
  km_plan p;
  return km_plan_make(n, d, k, &p) ? 1 : 0;
}

long iic_kmeans_workspace_bytes(long n, int d, int k) {
  km_plan p;
  if (!km_plan_make(n, d, k, &p)) return 0;
  return km_ws_make(nullptr, p, d, k).bytes;
}

int iic_kmeans_assign(const float* X, long ldx, const float* C, long n, int d, int k, int* labels, float* mind,
                      float* sums, long long* counts, double* inertia, void* ws, void* state, void* stream) {
  if (!X || !C || !labels || !mind || !ws) return IIC_ERR_ARG;
  if ((sums == nullptr) != (counts == nullptr)) return IIC_ERR_ARG;
  km_plan p;
  if (!km_plan_make(n, d, k, &p)) return IIC_ERR_UNSUPPORTED;
  if (ldx < d) return IIC_ERR_ARG;
  const km_ws w = km_ws_make(ws, p, d, k);
  hipStream_t s = (hipStream_t)stream;
  km_state* st = (km_state*)state;
  hipLaunchKernelGGL(km_cnorm_kernel, dim3(k), dim3(64), 0, s, C, d, w.cnorm, st);
  const bool vec = (d % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)X | (uintptr_t)C | (uintptr_t)w.sum_part) % 16 == 0);
  const dim3 grid((unsigned)p.W);
  float* sp = sums ? w.sum_part : nullptr;
  int* cp = sums ? w.count_part : nullptr;
  int rc;
  switch (p.kb) {
    case 1: rc = km_launch_assign<1>(vec, grid, s, X, ldx, C, w.cnorm, n, d, k, p.m, labels, mind, sp, cp, w.inertia_part, st); break;
    case 2: rc = km_launch_assign<2>(vec, grid, s, X, ldx, C, w.cnorm, n, d, k, p.m, labels, mind, sp, cp, w.inertia_part, st); break;
    case 4: rc = km_launch_assign<4>(vec, grid, s, X, ldx, C, w.cnorm, n, d, k, p.m, labels, mind, sp, cp, w.inertia_part, st); break;
    case 8: rc = km_launch_assign<8>(vec, grid, s, X, ldx, C, w.cnorm, n, d, k, p.m, labels, mind, sp, cp, w.inertia_part, st); break;
    default: rc = km_launch_assign<16>(vec, grid, s, X, ldx, C, w.cnorm, n, d, k, p.m, labels, mind, sp, cp, w.inertia_part, st); break;
  }
  if (rc != IIC_OK) return rc;
  if (sums) {
    const long elems = (long)k * d;
    const unsigned gx = (unsigned)((elems + 255) / 256);
    if (p.W2) {
      hipLaunchKernelGGL(km_reduce_kernel, dim3((unsigned)p.W2, gx), dim3(256), 0, s, w.sum_part, p.W, KM_GROUP, elems,
                         w.sum_part2, st);
      hipLaunchKernelGGL(km_reduce_kernel, dim3(1, gx), dim3(256), 0, s, w.sum_part2, p.W2, (int)p.W2, elems, sums, st);
    } else {
      hipLaunchKernelGGL(km_reduce_kernel, dim3(1, gx), dim3(256), 0, s, w.sum_part, p.W, (int)p.W, elems, sums, st);
    }
    hipLaunchKernelGGL(km_count_kernel, dim3(k), dim3(256), 0, s, w.count_part, p.W, k, counts, st);
  }
  if (inertia) hipLaunchKernelGGL(km_inertia_kernel, dim3(1), dim3(256), 0, s, w.inertia_part, p.W, inertia);
  return iic_launch_status();
}

int iic_kmeans_update(float* C, const float* sums, const long long* counts, long n, int d, int k, int force, void* ws,
                      void* state, void* stream) {
  if (!C || !sums || !counts || !ws || !state) return IIC_ERR_ARG;
  km_plan p;
  if (!km_plan_make(n, d, k, &p)) return IIC_ERR_UNSUPPORTED;
  const km_ws w = km_ws_make(ws, p, d, k);
  hipStream_t s = (hipStream_t)stream;
  km_state* st = (km_state*)state;
  hipLaunchKernelGGL(km_update_kernel, dim3(k), dim3(256), 0, s, C, sums, counts, d, k, force, w.shift_part, st);
  hipLaunchKernelGGL(km_finalize_kernel, dim3(1), dim3(256), 0, s, counts, k, force, w.shift_part, w.inertia_part, p.W,
                     st);
  return iic_launch_status();
}

int iic_kmeans_seed_potential(const float* X, long ldx, long n, int d, const long long* cand, int ncand, float* mind,
                              int write, double* pot, void* ws, void* stream) {
  if (!X || !cand || !mind || !pot || !ws) return IIC_ERR_ARG;
  if (ncand < 1 || ncand > KM_MAXCAND || (write && ncand != 1)) return IIC_ERR_ARG;
  km_plan p;
  if (!km_plan_make(n, d, 1, &p)) return IIC_ERR_UNSUPPORTED;
  if (ldx < d) return IIC_ERR_ARG;
  // seed_part sits behind regions whose size depends on k: the seeding calls use the k = 1 layout of their own workspace
  const km_ws w = km_ws_make(ws, p, d, 1);
  hipStream_t s = (hipStream_t)stream;
  long wgs = (n + 3) / 4;
  if (wgs > KM_SEED_WGS) wgs = KM_SEED_WGS;
  hipLaunchKernelGGL(km_seed_kernel, dim3((unsigned)wgs), dim3(256), 0, s, X, ldx, n, d, cand, ncand, mind, write,
                     w.seed_part);
  hipLaunchKernelGGL(km_seed_reduce_kernel, dim3(1), dim3(64), 0, s, w.seed_part, (int)wgs, ncand, pot);
  return iic_launch_status();
}

}  // extern "C"
