// IID segmentation loss beyond 48 classes and 256-pixel rows: the joint and its gradient of csrc/seg_loss.hip, tiled.
//
// Replaces, in /root/reference/code/utils/segmentation/IID_losses.py:14-159, what csrc/seg_loss.hip replaces -- the
// mask multiplies (:45-47,115-117), the permutes (:51-52,121-122) and the giant-filter F.conv2d(x1, weight=x2_inv,
// padding=T) (:55,125) with its two backward convolutions -- for the shapes the reference's own overclustering rule
// (k_A = 3 gt_k: 81 for the 27 coarse COCO-Stuff labels) and --input_sz 320 / 512 produce.
//
//   R[p][q][i][j] = sum_{n,y,x} x1m[n][i][y+p-T][x+q-T] * x2m[n][j][y][x]
//   x1m = x1 * mask,  x2m = flip(x2) * mask   (zero outside the image)
//
// The kernels of seg_loss.hip keep a whole image row and every class tile of a workgroup in registers and LDS, hence
// k <= 48 and w <= 256.  Here both are cut:
//   classes -- into blocks of TK <= 3 tiles of 16 (balanced: nb = ceil(tiles / 3) blocks of TK = ceil(tiles / nb) tiles).
//     The joint gives every (i block, j block) pair a workgroup of its own: they write disjoint parts of one partial.
//     The gradient gives every block of OUTPUT classes a workgroup and walks the source classes in chunks of at most
//     SEGT_KC that are restaged in LDS.
//   columns -- into windows of ws pixels (256; 192 with three class tiles, which keeps two workgroups on a CU): x2m on
//     [x0, x0 + ws), x1m on [x0 - T, x0 + ws + T).  The joint walks the windows of a row inside the workgroup -- the
//     accumulators stay in registers, so a window costs no partial (at k = 255, T = 10 one partial is 115 MB); the
//     gradient gives every window of output pixels a workgroup, with a +-T source halo.
// Same arithmetic as seg_loss.hip: exact fp32 products on v_mfma_f32_16x16x4_f32, a fixed summation order, no float
// atomics -- bit-reproducible, and a function of the shape alone: there is ONE form, element-wise staging (coalesced
// along x, the mask read once per column), whatever the alignment of the tensors.
#include "common.h"
#include "../../include/iic_hip.h"

#define SEGT_KMAX IIC_SEG_TILED_MAX_K
#define SEGT_TMAX IIC_SEG_TILED_MAX_T
#define SEGT_WMAX IIC_SEG_TILED_MAX_W
#define SEGT_KC 48         // source classes per LDS chunk of the gradient
#define SEGT_NC 5          // columns per lane of a staged row: ceil((256 + 2 * 10 + 1) / 64)

__device__ __forceinline__ f32x4 segt_mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// pitches of the staged rows: odd (the joint reads column x + kk of row c: conflict-free), for kernels and plans alike
__host__ __device__ __forceinline__ int segt_p1(int ws, int T) { return (ws + 2 * T) | 1; }
__host__ __device__ __forceinline__ int segt_p2(int ws) { return ws | 1; }
__host__ __device__ __forceinline__ int segt_ps(int ws, int T) { return (ws + 2 * T) | 1; }

// One staged row of a masked map, window [x0 - halo, x0 - halo + P): dst[ch][xx] = src[n][c0 + ch][ys][flip(x)] *
// mask[n][ym][x] with x = x0 - halo + xx, zero where x leaves [max(0, xlo), min(w, xhi)) or the class leaves [0, k).
// Wave `wave` stages channels wave, wave + 4, ...; a lane owns columns lane + 64 j.  (ym, x): the pixel of the MASKED map;
// (ys, flip(x)): where it comes from in the source tensor -- seg_src of seg_loss.hip.
__device__ __forceinline__ void segt_stage(float* __restrict__ dst, const float* __restrict__ src,
                                           const float* __restrict__ mask, int n, int c0, int nch, int k, int h, int w,
                                           int ym, int ys, int fx, int x0, int halo, int xlo, int xhi, int P,
                                           int wave, int lane) {
  float m[SEGT_NC];
  long off[SEGT_NC];
#pragma unroll
  for (int j = 0; j < SEGT_NC; ++j) {
    const int xx = lane + 64 * j, x = x0 - halo + xx;
    const bool ok = xx < P && x >= 0 && x < w && x >= xlo && x < xhi;
    m[j] = ok ? mask[((long)n * h + ym) * w + x] : 0.f;
    off[j] = ok ? (long)ys * w + (fx ? w - 1 - x : x) : -1;
  }
  for (int ch = wave; ch < nch; ch += 4) {
    const int cls = c0 + ch;
    const float* s = src + ((long)n * k + cls) * h * w;
#pragma unroll
    for (int j = 0; j < SEGT_NC; ++j) {
      const int xx = lane + 64 * j;
      if (xx < P) dst[ch * P + xx] = (cls < k && off[j] >= 0) ? s[off[j]] * m[j] : 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------
// joint.  grid = (2T+1, groups * nb * nb, S), block = 256.  part[s][p][q][i][j].
// Workgroup = (row shift p, a group of QG column shifts, class block pair (bi, bj), a slice of the (n, y) rows).
// ------------------------------------------------------------------------------------
template <int TK, int QG>
__global__ __launch_bounds__(256) void seg_joint_tiled_kernel(
    const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ mask,
    const int* __restrict__ flips, float* __restrict__ part, int bn, int k, int h, int w, int T, int nb, int WS) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int nq = 2 * T + 1;
  const int P1 = segt_p1(WS, T), P2 = segt_p2(WS);
  float* sX1 = reinterpret_cast<float*>(smem_raw);          // [16*TK][P1]
  float* sX2 = sX1 + 16 * TK * P1;                          // [16*TK][P2]
  const int p = blockIdx.x, split = blockIdx.z, S = gridDim.z;
  const int bj = blockIdx.y % nb, t_ = blockIdx.y / nb, bi = t_ % nb, grp = t_ / nb;
  const int q0 = grp * QG, i0 = bi * 16 * TK, j0 = bj * 16 * TK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, kk = lane >> 4;
  const long rows = (long)bn * h;
  const long per = (rows + S - 1) / S;
  const long r0 = split * per, r1 = min(rows, r0 + per);

  f32x4 acc[QG][TK][TK];
#pragma unroll
  for (int a = 0; a < QG; ++a)
#pragma unroll
    for (int ti = 0; ti < TK; ++ti)
#pragma unroll
      for (int tj = 0; tj < TK; ++tj) acc[a][ti][tj] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (long r = r0; r < r1; ++r) {
    const int n = (int)(r / h), y = (int)(r - (long)n * h);
    const int y1 = y + p - T;
    if (y1 < 0 || y1 >= h) continue;                 // uniform: the shifted row is all padding
    const int fx = flips[2 * n], fy = flips[2 * n + 1];
    for (int x0 = 0; x0 < w; x0 += WS) {
      const int ws = min(WS, w - x0), ws4 = (ws + 3) & ~3;
      __syncthreads();
      // x2m on [x0, x0 + ws) (zero up to the pitch: the steps run to ws4); x1m on [x0 - T, x0 + ws4 + T)
      segt_stage(sX2, x2, mask, n, j0, 16 * TK, k, h, w, y, fy ? h - 1 - y : y, fx, x0, 0, x0, x0 + ws, P2, wave, lane);
      segt_stage(sX1, x1, mask, n, i0, 16 * TK, k, h, w, y1, y1, 0, x0, T, 0, w, P1, wave, lane);
      __syncthreads();
      for (int st = wave; st < ws4 / 4; st += 4) {
        const int xl = 4 * st + kk;
        float b[TK];
#pragma unroll
        for (int tj = 0; tj < TK; ++tj) b[tj] = sX2[(tj * 16 + c) * P2 + xl];
#pragma unroll
        for (int a = 0; a < QG; ++a) {
          if (q0 + a < nq) {
#pragma unroll
            for (int ti = 0; ti < TK; ++ti) {
              const float av = sX1[(ti * 16 + c) * P1 + xl + q0 + a];   // x + (q - T) + T
#pragma unroll
              for (int tj = 0; tj < TK; ++tj) acc[a][ti][tj] = segt_mfma16(av, b[tj], acc[a][ti][tj]);
            }
          }
        }
      }
    }
  }
  // cross-wave reduction, one shift at a time, through LDS (reuses the row buffers)
  float* red = reinterpret_cast<float*>(smem_raw);          // [4][TK*TK][256]
  constexpr int TT = TK * TK;
#pragma unroll
  for (int a = 0; a < QG; ++a) {
    const int q = q0 + a;
    if (q >= nq) break;
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < TK; ++ti)
#pragma unroll
      for (int tj = 0; tj < TK; ++tj)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          red[(wave * TT + ti * TK + tj) * 256 + lane * 4 + rr] = acc[a][ti][tj][rr];
    __syncthreads();
    float* out = part + (((long)split * nq + p) * nq + q) * k * k;
    for (int idx = tid; idx < TT * 256; idx += 256) {
      const int t = idx >> 8, e = idx & 255, ln = e >> 2, rr = e & 3;
      const int i = i0 + (t / TK) * 16 + (ln >> 4) * 4 + rr, j = j0 + (t % TK) * 16 + (ln & 15);
      if (i < k && j < k)
        out[(long)i * k + j] = red[(0 * TT + t) * 256 + e] + red[(1 * TT + t) * 256 + e] +
                               red[(2 * TT + t) * 256 + e] + red[(3 * TT + t) * 256 + e];
    }
  }
}

// ------------------------------------------------------------------------------------
// G of one gradient launch: Gp[hh][b][a (pitch KA)] = gl[hh] dR1[hh][e] + gnl[hh] dR2[hh][e], e = a*k + b (which 0) |
// b*k + a (which 1); hh = shift index p * nq + q, or 0 alone when collapsed; columns a >= k are zero.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_gprep_tiled_kernel(
    const float* __restrict__ dR1, const float* __restrict__ dR2, const float* __restrict__ gl,
    const float* __restrict__ gnl, float* __restrict__ Gp, int k, int KA, int H, int which) {
  const long total = (long)H * k * KA;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int a = (int)(idx % KA);
    const long r = idx / KA;
    const int b = (int)(r % k);
    const long hh = r / k;
    float v = 0.f;
    if (a < k) {
      const long e = which == 0 ? ((long)a * k + b) : ((long)b * k + a);
      const float w1 = gl[hh], w2 = gnl ? gnl[hh] : 0.f;
      v = w1 * dR1[hh * k * k + e] + w2 * dR2[hh * k * k + e];
    }
    Gp[idx] = v;
  }
}

// ------------------------------------------------------------------------------------
// gradient.  grid = (bn*h, windows, output class blocks), block = 256.
//   which = 0: out = d/dx1  (reads x2m rows y - (p-T), columns x - (q-T))
//   which = 1: out = d/dx2  (reads x1m rows y + (p-T), columns x + (q-T); lands at the flipped pixel, as seg_src reads)
// GEMM pixels x output classes, K = (column shift q, source class b padded to 4) per row shift p and class chunk.
// ------------------------------------------------------------------------------------
template <int TK>
__global__ __launch_bounds__(256) void seg_grad_tiled_kernel(
    const float* __restrict__ src, const float* __restrict__ mask, const int* __restrict__ flips,
    const float* __restrict__ Gp, float* __restrict__ out, int bn, int k, int h, int w, int T, int which,
    int shift_stride, int src_is_x2, int QC, int WS, int KA) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int PG = 16 * TK + 1;
  constexpr int MT = 4;                                    // pixel tiles per wave (ws <= 256)
  const int nq = 2 * T + 1;
  const int PS = segt_ps(WS, T);
  const int kcmax = min((k + 3) & ~3, SEGT_KC);
  float* sS = reinterpret_cast<float*>(smem_raw);          // [kcmax][PS]          masked source rows of a class chunk
  float* sG = sS + kcmax * PS;                             // [QC * kcmax][PG]     G slice
  const int n = blockIdx.x / h, y = blockIdx.x - n * h;
  const int x0 = blockIdx.y * WS, ws = min(WS, w - x0);
  const int a0 = blockIdx.z * 16 * TK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, kk = lane >> 4;
  const int sgn = which == 0 ? -1 : 1;
  const int fx = src_is_x2 ? flips[2 * n] : 0, fy = src_is_x2 ? flips[2 * n + 1] : 0;
  const int ntile = (ws + 15) >> 4;
  f32x4 acc[MT][TK];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < TK; ++t) acc[m][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int p = 0; p < nq; ++p) {
    const int ys = y + sgn * (p - T);
    if (ys < 0 || ys >= h) continue;                       // uniform
    for (int bc0 = 0; bc0 < k; bc0 += SEGT_KC) {
      const int kc = min(SEGT_KC, k - bc0), kc4 = (kc + 3) & ~3;
      __syncthreads();
      // classes bc0 .. bc0 + kc4 (zero past k), pixels [x0 - T, x0 - T + PS)
      segt_stage(sS, src, mask, n, bc0, kc4, k, h, w, ys, fy ? h - 1 - ys : ys, fx, x0, T, 0, w, PS, wave, lane);
      for (int qc0 = 0; qc0 < nq; qc0 += QC) {
        const int qn = min(QC, nq - qc0);
        __syncthreads();
        for (int idx = tid; idx < qn * kc4 * 16 * TK; idx += 256) {
          const int row = idx / (16 * TK), col = idx - row * (16 * TK);
          const int ql = row / kc4, bl = row - ql * kc4;
          float v = 0.f;
          if (bl < kc) v = Gp[((long)(p * nq + qc0 + ql) * shift_stride * k + bc0 + bl) * KA + a0 + col];
          sG[row * PG + col] = v;
        }
        __syncthreads();
        for (int ql = 0; ql < qn; ++ql) {
          const int xoff = sgn * (qc0 + ql - T) + T;          // wave-uniform column offset
          const float* sGq = sG + ql * kc4 * PG;
          for (int b0 = 0; b0 < kc4; b0 += 4) {
            const int b = b0 + kk;
            const float* srow = sS + b * PS + xoff + c;
            float bv[TK], av[MT];
#pragma unroll
            for (int t = 0; t < TK; ++t) bv[t] = sGq[b * PG + t * 16 + c];
#pragma unroll
            for (int m = 0; m < MT; ++m) av[m] = wave + 4 * m < ntile ? srow[(wave + 4 * m) * 16] : 0.f;
#pragma unroll
            for (int m = 0; m < MT; ++m)
              if (wave + 4 * m < ntile) {
#pragma unroll
                for (int t = 0; t < TK; ++t) acc[m][t] = segt_mfma16(av[m], bv[t], acc[m][t]);
              }
          }
        }
      }
    }
  }
  // store: D[row = pixel (lane>>4)*4 + r][col = class lane&15]; x mask; un-flip for x2
  const bool unflip = src_is_x2 == 0 && which == 1;
  const int ofx = unflip ? flips[2 * n] : 0, ofy = unflip ? flips[2 * n + 1] : 0;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int tile = wave + 4 * m;
    if (tile >= ntile) continue;
#pragma unroll
    for (int t = 0; t < TK; ++t) {
      const int a = a0 + t * 16 + c;
      if (a >= k) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int xl = tile * 16 + kk * 4 + r;
        if (xl < ws) {
          const int x = x0 + xl;
          const float v = acc[m][t][r] * mask[((long)n * h + y) * w + x];
          const int oy = ofy ? h - 1 - y : y, ox = ofx ? w - 1 - x : x;
          out[(((long)n * k + a) * h + oy) * w + ox] = v;
        }
      }
    }
  }
}

extern "C" {

// today's kernels (seg_loss.hip: seg_shape_ok, SEG_MAXW) and this file's range
static bool segt_resident_ok(int k, int w, int T) { return k >= 1 && k <= 48 && T >= 0 && T <= 10 && w >= 1 && w <= 256; }
static bool segt_shape_ok(int k, int w, int T) {
  return k >= 1 && k <= SEGT_KMAX && T >= 0 && T <= SEGT_TMAX && w >= 1 && w <= SEGT_WMAX;
}
// class blocks: nb blocks of tk tiles
static void segt_blocks(int k, int* tk, int* nb) {
  const int tiles = (k + 15) / 16;
  *nb = (tiles + 2) / 3;
  *tk = (tiles + *nb - 1) / *nb;
}
static int segt_qg(int tk) { return tk == 1 ? 21 : (tk == 2 ? 7 : 3); }      // accumulators: QG * tk * tk tiles
static int segt_ws(int tk) { return tk == 3 ? 192 : 256; }                  // window: LDS <= IIC_LDS_WG2 in both kernels

struct seg_tiled_joint_plan {
  int tk, nb;                 // class tiles per block, blocks per side
  int qg, groups;             // column shifts per workgroup, workgroups per row shift and block pair
  int ws, nwin;               // window pitch in pixels, windows per row (walked inside the workgroup)
  int gx, gy, gz, lds;
};
static bool seg_tiled_joint_make_plan(int bn, int k, int h, int w, int T, int nsplit, seg_tiled_joint_plan* P) {
  *P = seg_tiled_joint_plan{};
  if (bn <= 0 || nsplit <= 0 || h < 1 || !segt_shape_ok(k, w, T)) return false;
  const int nq = 2 * T + 1;
  segt_blocks(k, &P->tk, &P->nb);
  P->qg = segt_qg(P->tk);
  P->groups = (nq + P->qg - 1) / P->qg;
  P->ws = segt_ws(P->tk);
  P->nwin = (w + P->ws - 1) / P->ws;
  const int rows_b = 16 * P->tk * (segt_p1(P->ws, T) + segt_p2(P->ws)) * (int)sizeof(float);
  const int red_b = 4 * P->tk * P->tk * 256 * (int)sizeof(float);
  P->lds = rows_b > red_b ? rows_b : red_b;
  P->gx = nq; P->gy = P->groups * P->nb * P->nb; P->gz = nsplit;
  return P->gz <= 65535;
}

struct seg_tiled_grad_plan {
  int tk, nbo, ka;            // output class tiles per block, output class blocks, pitch of a G row (nbo * 16 * tk)
  int kc, qc;                 // source classes per staged chunk (padded to 4), column shifts per G slice
  int ws, nwin;
  int gx, gy, gz, lds;
  int prep_grid;              // the seg_gprep_tiled_kernel launch
};
static bool seg_tiled_grad_make_plan(int bn, int k, int h, int w, int T, int collapsed, seg_tiled_grad_plan* P) {
  *P = seg_tiled_grad_plan{};
  if (bn <= 0 || h < 1 || !segt_shape_ok(k, w, T)) return false;
  const int nq = 2 * T + 1;
  segt_blocks(k, &P->tk, &P->nbo);
  P->ka = P->nbo * 16 * P->tk;
  const int k4 = (k + 3) & ~3;
  P->kc = k4 < SEGT_KC ? k4 : SEGT_KC;
  P->ws = segt_ws(P->tk);
  P->nwin = (w + P->ws - 1) / P->ws;
  const int src_b = P->kc * segt_ps(P->ws, T) * (int)sizeof(float);
  const int slice_b = P->kc * (16 * P->tk + 1) * (int)sizeof(float);       // one column shift of G
  int qc = ((int)IIC_LDS_WG2 - src_b) / slice_b;                           // two workgroups per CU
  if (qc < 1) qc = 1;
  P->qc = qc > nq ? nq : qc;
  P->lds = src_b + P->qc * slice_b;
  P->gx = bn * h; P->gy = P->nwin; P->gz = P->nbo;
  const long total = (long)(collapsed ? 1 : nq * nq) * k * P->ka;
  P->prep_grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  return (long)bn * h <= 0x7fffffffL;
}

#ifdef IIC_DEBUG_HOOKS
// The plans as ints in the structs' order (host code only: needs no device).  An unsupported shape zeroes `out`.
IIC_HOOK void iic_debug_seg_tiled_joint_plan(int bn, int k, int h, int w, int T, int nsplit, int* out) {
  seg_tiled_joint_plan p;
  if (!seg_tiled_joint_make_plan(bn, k, h, w, T, nsplit, &p)) p = seg_tiled_joint_plan{};
  const int f[10] = {p.tk, p.nb, p.qg, p.groups, p.ws, p.nwin, p.gx, p.gy, p.gz, p.lds};
  for (int i = 0; i < 10; ++i) out[i] = f[i];
}
IIC_HOOK void iic_debug_seg_tiled_grad_plan(int bn, int k, int h, int w, int T, int collapsed, int* out) {
  seg_tiled_grad_plan p;
  if (!seg_tiled_grad_make_plan(bn, k, h, w, T, collapsed, &p)) p = seg_tiled_grad_plan{};
  const int f[12] = {p.tk, p.nbo, p.ka, p.kc, p.qc, p.ws, p.nwin, p.gx, p.gy, p.gz, p.lds, p.prep_grid};
  for (int i = 0; i < 12; ++i) out[i] = f[i];
}
#endif

int iic_seg_loss_path(int k, int w, int T) {
  if (segt_resident_ok(k, w, T)) return IIC_SEG_PATH_RESIDENT;
  return segt_shape_ok(k, w, T) ? IIC_SEG_PATH_TILED : IIC_SEG_PATH_NONE;
}

int iic_seg_tiled_limit(int which) {
  return which == 0 ? SEGT_KMAX : (which == 1 ? SEGT_TMAX : (which == 2 ? SEGT_WMAX : 0));
}

// A function of the shape alone (it sets the summation order).  About 2048 workgroups, at most bn h, and no more
// partials than IIC_SEG_TILED_PART_CAP_BYTES hold (never fewer than one).
int iic_seg_tiled_joint_nsplit(int bn, int h, int w, int k, int T) {
  seg_tiled_joint_plan P;
  if (!seg_tiled_joint_make_plan(bn, k, h, w, T, 1, &P)) return 1;
  const int nq = 2 * T + 1;
  long s = 2048 / ((long)nq * P.gy);
  const long one = (long)nq * nq * k * k * (long)sizeof(float);
  const long cap = IIC_SEG_TILED_PART_CAP_BYTES / one;
  if (s > cap) s = cap;
  const long rows = (long)bn * h;
  if (s > rows) s = rows;
  if (s < 1) s = 1;
  return (int)s;
}

#define SEGT_CASE(TK_, ...) \
  case TK_: rc = iic_launch_lds<__VA_ARGS__>(grid, dim3(256), (size_t)P.lds, s, SEGT_ARGS); break

int iic_seg_tiled_joint_raw(const float* x1, const float* x2, const float* mask, const int* flips, float* partials,
                            int bn, int k, int h, int w, int T, int nsplit, void* stream) {
  if (!x1 || !x2 || !mask || !flips || !partials || bn <= 0 || nsplit <= 0) return IIC_ERR_ARG;
  seg_tiled_joint_plan P;
  if (!seg_tiled_joint_make_plan(bn, k, h, w, T, nsplit, &P)) return IIC_ERR_UNSUPPORTED;
  const dim3 grid(P.gx, P.gy, P.gz);
  hipStream_t s = (hipStream_t)stream;
  int rc = IIC_ERR_UNSUPPORTED;
  switch (P.tk) {
#define SEGT_ARGS x1, x2, mask, flips, partials, bn, k, h, w, T, P.nb, P.ws
    SEGT_CASE(1, seg_joint_tiled_kernel<1, 21>);
    SEGT_CASE(2, seg_joint_tiled_kernel<2, 7>);
    SEGT_CASE(3, seg_joint_tiled_kernel<3, 3>);
#undef SEGT_ARGS
    default: break;
  }
  return rc ? rc : iic_launch_status();
}

long iic_seg_tiled_grad_workspace_bytes(int k, int T, int collapsed) {
  seg_tiled_grad_plan P;
  if (!seg_tiled_grad_make_plan(1, k, 1, 1, T, collapsed, &P)) return 0;
  const long nq = 2 * T + 1;
  return (collapsed ? 1 : nq * nq) * (long)k * P.ka * (long)sizeof(float);
}

int iic_seg_tiled_grad(const float* src, const float* mask, const int* flips, const float* dR_loss,
                       const float* dR_loss_no_lamb, const float* g_loss, const float* g_loss_no_lamb, float* out,
                       int bn, int k, int h, int w, int T, int which, int collapsed, float* workspace, void* stream) {
  if (!src || !mask || !flips || !dR_loss || !dR_loss_no_lamb || !g_loss || !out || !workspace) return IIC_ERR_ARG;
  seg_tiled_grad_plan P;
  if (!seg_tiled_grad_make_plan(bn, k, h, w, T, collapsed, &P)) return IIC_ERR_UNSUPPORTED;
  const int src_is_x2 = which == 0 ? 1 : 0;   // d/dx1 reads x2m ; d/dx2 reads x1m
  const int shift_stride = collapsed ? 0 : 1;
  const int nq = 2 * T + 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(seg_gprep_tiled_kernel, dim3(P.prep_grid), dim3(256), 0, s, dR_loss, dR_loss_no_lamb, g_loss,
                     g_loss_no_lamb, workspace, k, P.ka, collapsed ? 1 : nq * nq, which);
  const dim3 grid(P.gx, P.gy, P.gz);
  int rc = IIC_ERR_UNSUPPORTED;
  switch (P.tk) {
#define SEGT_ARGS src, mask, flips, (const float*)workspace, out, bn, k, h, w, T, which, shift_stride, src_is_x2, P.qc, \
                  P.ws, P.ka
    SEGT_CASE(1, seg_grad_tiled_kernel<1>);
    SEGT_CASE(2, seg_grad_tiled_kernel<2>);
    SEGT_CASE(3, seg_grad_tiled_kernel<3>);
#undef SEGT_ARGS
    default: break;
  }
  return rc ? rc : iic_launch_status();
}

}  // extern "C"
