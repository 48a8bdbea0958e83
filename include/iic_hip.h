/* libiic_hip.so -- C ABI of the MI355X-native (gfx950) IIC training hot path.
 *
 * The reference (xu-ji/IIC, PyTorch 0.4.1) has no FFI layer: its operator API is a
 * set of Python call signatures.  This library sits beneath Python
 * shims that reproduce those signatures (the iic_amd Python package); every entry point below names
 * the reference code it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless
 *     a parameter is documented as host;
 *   - the caller owns every buffer (workspace sizes via *_bytes helpers);
 *   - kernels are enqueued asynchronously on `stream` (a hipStream_t passed as void*),
 *     no hidden synchronisation or allocation;
 *   - return 0 on success, negative on error (IIC_ERR_*); nothing throws.
 *
 * Activation tensor format "PT" (padded tile): bf16 [N][H+2P][W+2P][C] with a ZERO
 * border of P pixels.  Kernels only ever write interior pixels, so a buffer zeroed
 * once keeps its border.  C must be a multiple of 64 for the MFMA conv kernels.
 */
#ifndef IIC_HIP_H
#define IIC_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The prototypes below are the library's WHOLE exported surface: libiic_hip.so is built with -fvisibility=hidden
 * and only what this header declares is visible (tests/test_cabi_cpu.py holds `nm -D` to it, both ways). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define IIC_OK 0
#define IIC_ERR_ARG (-1)
#define IIC_ERR_LAUNCH (-2)
#define IIC_ERR_UNSUPPORTED (-3)

int iic_version(void);

/* ---------------------------------------------------------------------------------
 * IID clustering loss -- replaces code/utils/cluster/IID_losses.py:6-47
 * (IID_loss + compute_joint).  z / zt: post-softmax fp32, element (h, n, i) at
 * z[h*head_stride + n*ld + i] (ld >= k: sub-heads may be interleaved per sample).  Two-phase so that the raw joint can be all-reduced over ranks
 *  between phase 1 and phase 2.
 * ------------------------------------------------------------------------------- */
int iic_iid_nsplit(int bn);                       /* recommended sample-splits          */
long iic_iid_workspace_bytes(int H, int k);       /* float64 scratch for phase 2        */
/* phase 1: partials[s][h][k][k] = sum over sample-split s of z^T z' (exact fp32 MFMA) */
int iic_iid_joint_raw(const float* z, const float* zt, float* partials, int H, int bn, int k,
                      long head_stride, long ld, int nsplit, void* stream);
/* phase 2: sum partials -> symmetrise, normalise, marginals, clamp (eps), the two losses
 * (IID_losses.py:21-31) and dLoss/dR, dLossNoLamb/dR ([H][k][k] fp32 each).            */
int iic_iid_loss_from_joint(const float* partials, int nparts, int H, int k, double lamb,
                            double eps, void* workspace, float* loss, float* loss_no_lamb,
                            float* dR_loss, float* dR_loss_no_lamb, void* stream);
/* phase 3: dz = (g*dR1 + gnl*dR2) applied to z' (and z for dz'); g_* are DEVICE arrays
 * [H] of upstream gradients (NULL => 1 and 0).                                        */
int iic_iid_grad(const float* z, const float* zt, const float* dR_loss,
                 const float* dR_loss_no_lamb, const float* g_loss, const float* g_loss_no_lamb,
                 float* dz, float* dzt, int H, int bn, int k, long head_stride, long ld,
                 void* stream);

/* ---------------------------------------------------------------------------------
 * IID segmentation losses -- replace code/utils/segmentation/IID_losses.py:14-159
 * (IID_segmentation_loss, IID_segmentation_loss_uncollapsed) incl. perform_affine_tf for the
 * identity / axis-flip transforms (transforms.py:131-143; `flips` = int32 [bn][2]: flip x, y).
 * x1, x2: fp32 NCHW [bn][k][h][w] (post-softmax), mask fp32 [bn][h][w], T = half_T_side_dense.
 *   partials[s][p][q][i][j] = sum over row-slice s of x1m[i](y+p-T, x+q-T) * x2m[j](y, x)
 * Exact fp32 MFMA (16x16x4).  k <= 48, T <= 10, w <= 256.  Rows with w % 4 == 0 (any served k) and
 * 16-byte aligned tensors take the streaming kernels (float4 rows prefetched under the MFMA loop);
 * anything else the element-wise generic ones -- same results (bit-identical joint).
 * iic_seg_joint_nsplit: the recommended split count, a function of the shape alone; 1 for a k or T
 * outside the served range (the launch then answers IIC_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------- */
int iic_seg_joint_nsplit(int bn, int h, int k, int T);
int iic_seg_joint_raw(const float* x1, const float* x2, const float* mask, const int* flips,
                      float* partials, int bn, int k, int h, int w, int T, int nsplit,
                      void* stream);
/* k x k stage: uncollapsed = one joint per shift (H = (2T+1)^2, nparts = nsplit);
 * collapsed = shifts summed (H = 1, nparts = nsplit*(2T+1)^2, detach_norm = 1, :60).
 * Workspace / outputs as iic_iid_loss_from_joint.                                          */
int iic_seg_loss_from_joint(const float* partials, int nparts, int H, int k, double lamb,
                            double eps, void* workspace, float* loss, float* loss_no_lamb,
                            float* dR_loss, float* dR_loss_no_lamb, int detach_norm, void* stream);
/* which = 0: out = dLoss/dx1 (src = x2);  which = 1: out = dLoss/dx2 (src = x1).
 * g_loss / g_loss_no_lamb: DEVICE arrays [H] of upstream gradients per shift ([1] if collapsed).
 * workspace: iic_seg_grad_workspace_bytes(k, T) bytes, 16-byte aligned, caller-owned scratch of
 * this launch (the per-shift gradient matrices laid out for the streaming kernel, classes padded
 * to a multiple of 4: (2T+1)^2 * roundup4(k) * 16 * ceil(k / 16) floats; 0 outside the served
 * range); NULL selects the generic kernel (any w, k <= 48), which needs none.                */
long iic_seg_grad_workspace_bytes(int k, int T);
int iic_seg_grad(const float* src, const float* mask, const int* flips, const float* dR_loss,
                 const float* dR_loss_no_lamb, const float* g_loss, const float* g_loss_no_lamb,
                 float* out, int bn, int k, int h, int w, int T, int which, int collapsed,
                 float* workspace, void* stream);
/* ---------------------------------------------------------------------------------
 * The same two contractions beyond k = 48 and w = 256 (csrc/seg_loss_tiled.hip) -- replace the same
 * lines, code/utils/segmentation/IID_losses.py:45-55 and :115-125 (mask multiplies, permutes, the
 * giant-filter F.conv2d and its backward), for the shapes the reference's overclustering rule
 * k_A = 3 gt_k and --input_sz 320 / 512 give.  Class blocks of at most 3 x 3 tiles of 16 and column
 * windows of at most 256 pixels with a +-T halo; exact fp32 MFMA (16x16x4), fixed summation order, no
 * float atomics: bit-reproducible, and ONE element-wise form whatever the alignment or w % 4.
 * Range: 1 <= k <= IIC_SEG_TILED_MAX_K, 0 <= T <= IIC_SEG_TILED_MAX_T, 1 <= w <= IIC_SEG_TILED_MAX_W,
 * any h >= 1 -- shapes the entries above serve included (same layouts, same meaning of every
 * argument; on full-mantissa operands the bits may differ from theirs: another summation order).
 * The entries above keep every answer they give, the refusals included.
 *
 * iic_seg_loss_path(k, w, T): which family serves the shape -- IIC_SEG_PATH_RESIDENT (the entries
 *   above), IIC_SEG_PATH_TILED (the entries below) or IIC_SEG_PATH_NONE.
 * iic_seg_tiled_limit(which): 0 -> the largest k, 1 -> the largest T, 2 -> the largest w (else 0).
 * iic_seg_tiled_joint_nsplit: the recommended split count, a function of the shape alone; at most
 *   bn h, and no more splits than keep the partial buffer within IIC_SEG_TILED_PART_CAP_BYTES (64 MB)
 *   -- never below 1, so the buffer is max(64 MB, one partial) at most; one partial is (2T+1)^2 k^2
 *   floats, 115 MB at k = 255, T = 10, where the answer is 1; 1 outside the range.  Windows and class
 *   blocks add no partials: partials[nsplit][(2T+1)^2][k][k], fed to iic_seg_loss_from_joint as above.
 * iic_seg_tiled_grad_workspace_bytes(k, T, collapsed): the gradient matrices G = g dR1 + gnl dR2 laid
 *   out [shift][source class][output class, padded to whole class blocks]: one shift when collapsed,
 *   (2T+1)^2 otherwise; 0 outside the range.  The workspace is mandatory here (NULL: IIC_ERR_ARG).
 * ------------------------------------------------------------------------------- */
#define IIC_SEG_TILED_MAX_K 255
#define IIC_SEG_TILED_MAX_T 10
#define IIC_SEG_TILED_MAX_W 4096
#define IIC_SEG_TILED_PART_CAP_BYTES (64L << 20)
#define IIC_SEG_PATH_NONE 0
#define IIC_SEG_PATH_RESIDENT 1
#define IIC_SEG_PATH_TILED 2
int iic_seg_loss_path(int k, int w, int T);
int iic_seg_tiled_limit(int which);
int iic_seg_tiled_joint_nsplit(int bn, int h, int w, int k, int T);
int iic_seg_tiled_joint_raw(const float* x1, const float* x2, const float* mask, const int* flips,
                            float* partials, int bn, int k, int h, int w, int T, int nsplit,
                            void* stream);
long iic_seg_tiled_grad_workspace_bytes(int k, int T, int collapsed);
int iic_seg_tiled_grad(const float* src, const float* mask, const int* flips, const float* dR_loss,
                       const float* dR_loss_no_lamb, const float* g_loss, const float* g_loss_no_lamb,
                       float* out, int bn, int k, int h, int w, int T, int which, int collapsed,
                       float* workspace, void* stream);
/* General case of the second view's warp -- perform_affine_tf (code/utils/segmentation/
 * transforms.py:131-143: affine_grid + grid_sample, bilinear, zero padding) followed by the
 * whole-batch integer shift of random_translation_multiple (transforms.py:145-165; IID_losses.py:
 * 101-104).  x, out, dout, dx: fp32 NCHW [N][K][H][W]; pixel_mats: fp32 [N][6], source pixel
 * (ix, iy) = M * (ox + shift_x, oy + shift_y, 1) (the host derives M from theta in normalised
 * coordinates); output pixels whose shifted position leaves the image are 0.  Identity / flip
 * matrices without shift never come here: they are index arithmetic inside iic_seg_joint_raw /
 * iic_seg_grad (flips).  iic_affine_warp_bwd overwrites dx.                                 */
int iic_affine_warp_fwd(const float* x, const float* pixel_mats, float* out, int N, int K, int H, int W,
                        int shift_x, int shift_y, void* stream);
int iic_affine_warp_bwd(const float* dout, const float* pixel_mats, float* dx, int N, int K, int H, int W,
                        int shift_x, int shift_y, void* stream);
/* The same backward (the adjoint of perform_affine_tf, transforms.py:131-143, and of the shift) in gather form: no
 * float atomics and no zero-fill, every element of dx written once -- bit-reproducible launch to launch and between
 * eager launches and graph replay.  One thread owns one source pixel (u, v) and sums, for every k, the output pixels
 * whose sampling point M_n (qx, qy, 1) falls in [u-1, u+1) x [v-1, v+1): it searches the bounding box of that
 * square's preimage (centre and half-extents from the inverse of M_n's 2x2 part, in double, 1/64 pixel of slack a side,
 * clamped to the image) and recomputes the forward's taps at every position of the box -- membership is decided by
 * the forward's own arithmetic, the box only bounds the search.
 *   Summation order: contributors in ascending (oy, ox); acc = +0.0f; acc = fl32(acc + fl32(w * dout)) with w the
 *   forward's float32 tap weight; no FMA contraction.  With one contributor, or with exactly representable
 *   contributions, these are iic_affine_warp_bwd's bits.  A NaN / inf of dout reaches exactly the source pixels its
 *   output pixel taps (0 x inf = NaN, as in iic_affine_warp_bwd and grid_sample).
 *   Range: matrices whose box is at most IIC_WARP_GATHER_CAP positions in each direction, i.e. with
 *   det = m0 m4 - m1 m3:  2 ((|m4| + |m1|) / |det| + 1/64) + 1 < IIC_WARP_GATHER_CAP  and the same for
 *   (|m3| + |m0|) / |det| -- every matrix the reference's random_affine draws (rotation +-30 deg, shear +-10 deg, scale
 *   0.8-1.2, flips) up to an aspect ratio of 20:9 needs at most 7, shrinking to one half needs 6.
 * iic_affine_warp_gather_supported(host_mats, N): 1 when the launch serves all N matrices, 0 when one of them is
 *   singular, non-finite or beyond the cap (or the arguments are void).  host_mats is a HOST pointer to [N][6] floats.
 * iic_affine_warp_bwd_gather: pixel_mats is the device copy of host_mats, a HOST pointer to the same [N][6] values; the
 *   launch asks the query first and answers IIC_ERR_UNSUPPORTED, with nothing enqueued, where it says 0 (no device-to-host
 *   copy anywhere).  Overwrites dx.                                                                              */
#define IIC_WARP_GATHER_CAP 8
int iic_affine_warp_gather_supported(const float* host_mats, int N);
int iic_affine_warp_bwd_gather(const float* dout, const float* pixel_mats, const float* host_mats, float* dx, int N,
                               int K, int H, int W, int shift_x, int shift_y, void* stream);

/* ---------------------------------------------------------------------------------
 * Convolution as an im2col-free implicit GEMM on bf16 MFMA (fp32 accumulate).
 * Replaces the cuDNN conv fwd / bwd-data / bwd-weight the reference reaches through
 * nn.Conv2d in code/archs/cluster/residual.py:4-7,19,22,54-55, net5g.py:21-23,
 * vgg.py:24-26.  One kernel serves forward and backward-data: the geometry maps GEMM
 * row m=(n,y,x) to an input pixel and an output pixel, and lists the taps.
 * ------------------------------------------------------------------------------- */
#define IIC_MAX_TAPS 32
typedef struct {
  int32_t N, MY, MX;            /* GEMM rows M = N*MY*MX, m -> (n, y, x)                       */
  int32_t in_Hp, in_Wp, Cin;    /* input  PT tensor dims (padded)                              */
  int32_t sy, sx, oy, ox;       /* input pixel of row m, tap offset 0:                         */
                                /*   (n*in_Hp + y*sy+oy)*in_Wp + x*sx+ox                       */
  int32_t out_Hp, out_Wp, Cout; /* output PT tensor dims (padded)                              */
  int32_t ty, tx, py, px;       /* output pixel (n*out_Hp + y*ty+py)*out_Wp + x*tx+px          */
  int32_t ntaps;
  int32_t tap_off[IIC_MAX_TAPS];/* >=0, added to the input pixel index                         */
  int32_t tap_w[IIC_MAX_TAPS];  /* which [Cout][Cin] slice of the weight tensor the tap uses   */
  int32_t NP;                   /* LDS patch pixels per 128-row tile (max input span + 1)      */
  int32_t NP256;                /* same for 256-row tiles (0 = unknown: 128-row tiles only)    */
  int32_t NP64;                 /* same for 64-row tiles  (0 = unknown)                         */
  int32_t MP;                   /* GEMM rows per image: 0 = MY*MX (dense), else a multiple of   */
                                /* 256 >= MY*MX; rows r >= MY*MX of an image are invalid (never */
                                /* stored, no statistics, zero weight gradient): tiles of large */
                                /* images then never straddle two images                        */
} iic_conv_geom;

long iic_conv_lds_bytes(const iic_conv_geom* g, int BN);
/* out[pout(m)][co] = sum_t sum_ci in[pin(m)+tap_off[t]][ci] * w[tap_w[t]][co][ci]
 * w: bf16 [wtaps][Cout][Cin].  stats (nullable): a statistics accumulator of iic_stat_bytes(Cout)
 * bytes, zero-initialised once by the caller (the finalisers re-zero it); += per-channel sum /
 * sum of squares of the fp32 accumulators (BatchNorm batch stats).  The accumulator is opaque:
 * [IIC_STAT_STRIPES][Cout][2][8] int64 fixed-point bins, added to with integer atomics, so the
 * result is exact and independent of the order in which workgroups arrive -- bit-reproducible
 * training (csrc/common.h).  `float*` in the signatures below is that opaque buffer.
 * res_grad/res_act (nullable, PT like out): out += res_grad where res_act > 0 (fused
 * ReLU-masked residual gradient).  accumulate is a flag word: IIC_ACC_ADD: out += previous
 * contents; IIC_ACC_PREMASK changes the meaning of res_grad / res_act (each nullable on its
 * own): out = (value [+ previous] [+ res_grad]) where res_act > 0, else 0 -- a backward-data
 * launch hands its gradient over already multiplied by the ReLU mask of the activation it
 * belongs to (res_act = the conv's input activation, archs/cluster.py PREMASK).           */
#define IIC_STAT_STRIPES 32
long iic_stat_bytes(int C);
#define IIC_ACC_ADD 1
#define IIC_ACC_PREMASK 2
int iic_conv_igemm(const iic_conv_geom* g, const void* in, const void* w, void* out,
                   float* stats, const void* res_grad, const void* res_act, int accumulate,
                   void* stream);
/* bwd-weight: partial[s][t][co][ci] (fp32) = sum over the rows of split s of
 * dy[pout(m)][co] * x[pin(m)+tap_off[t]][ci]; the geometry is the FORWARD geometry.
 * use_tr != 0 selects ds_read_b64_tr_b16 operand reads (fast); 0 = scalar LDS gathers. */
int iic_conv_wgrad_nsplit(const iic_conv_geom* g);
int iic_conv_wgrad(const iic_conv_geom* g, const void* x, const void* dy, float* partials,
                   int nsplit, int use_tr, void* stream);
/* dW[co][ci][kh][kw] (fp32 OIHW, the nn.Conv2d parameter layout) (+)= sum_s partial[s][t][co][ci] */
int iic_conv_wgrad_reduce(const float* partials, int nsplit, int T, int Cout, int Cin, float* dW,
                          int accumulate, void* stream);
/* fp32 OIHW parameter -> bf16 [T][Co][Ci] (forward operand) and [T][Ci][Co] (bwd-data operand) */
int iic_weight_prep(const float* w_oihw, void* w_fwd, void* w_bwd, int Cout, int Cin, int T,
                    void* stream);

/* Second-generation kernel for Cout % 128 == 0 (same contract as iic_conv_igemm, same
 * reference call sites): the weight operand is read straight from L2 in MFMA B-fragment order
 * and never staged in LDS; 256 x 128 workgroup tiles, barriers only per 64-channel chunk.
 *   w_frag[tap][k/64][n/32][ks][lane][e] = W[n = (n/32)*32 + (lane & 31)]
 *                                           [k = (k/64)*64 + ks*16 + (lane >> 5)*8 + e][tap]
 * with (n, k) = (cout, cin) for the forward operand (bwd = 0) and (cin, cout) for the
 * backward-data operand (bwd = 1).  iic_conv_igemm_frag_supported: 1 if the geometry can run
 * here (needs NP256), else callers use iic_conv_igemm with the row-major operand.            */
int iic_conv_igemm_frag_supported(const iic_conv_geom* g);
int iic_conv_igemm_frag(const iic_conv_geom* g, const void* in, const void* w_frag, void* out,
                        float* stats, const void* res_grad, const void* res_act, int accumulate,
                        void* stream);
/* Same launch with a fused BatchNorm-backward reduction over the tile it stores (backward-data
 * launches): the gradient g this conv produces is the upstream gradient of a BatchNorm whose
 * input y (PT, shaped like `out`) is known, so the two sums that BatchNorm's backward needs,
 *   red_stats += (sum g, sum g*y)     [red_y2 / red_stats2: (sum g, sum g*y2), downsample branch]
 * (the quantities of iic_bn_bwd_reduce, residual.py:20-41 backward) are taken in the epilogue from
 * the stored (bf16-rounded) values -- masked with (scale*y + shift > 0) when red_coef (that
 * BatchNorm's forward coefficients) is given, i.e. a ReLU sits between it and this conv -- instead
 * of in a separate HBM-bound pass over g and y.  Single-launch geometries only (stride 1).     */
int iic_conv_igemm_red_supported(const iic_conv_geom* g);
int iic_conv_igemm_frag_red(const iic_conv_geom* g, const void* in, const void* w_frag, void* out,
                            float* stats, const void* res_grad, const void* res_act, int accumulate,
                            const void* red_y, const float* red_coef, const void* red_y2,
                            float* red_stats, float* red_stats2, void* stream);
int iic_weight_prep_frag(const float* w_oihw, void* w_frag, int Cout, int Cin, int T, int bwd,
                         void* stream);
/* Every weight operand of a network in ONE launch (what the per-parameter calls above do once per conv and
 * layout after each optimiser step): `jobs_dev` = njobs records in DEVICE memory, sorted by first_block
 * (job i owns blocks [first_block, first_block + iic_weight_prep_multi_blocks(Cout, Cin, T))),
 * total_blocks = the sum.  mode: 0 / 1 = B-fragment order forward / backward-data operand
 * (iic_weight_prep_frag), 2 = [T][Co][Ci], 3 = [T][Ci][Co] (iic_weight_prep's two outputs).               */
typedef struct iic_weight_prep_job {
  const float* w;        /* fp32 OIHW parameter */
  void* out;             /* bf16 operand */
  long long first_block;
  int32_t Cout, Cin, T, mode;
} iic_weight_prep_job;
long iic_weight_prep_multi_blocks(int Cout, int Cin, int T);
int iic_weight_prep_multi(const iic_weight_prep_job* jobs_dev, int njobs, long total_blocks, void* stream);

/* ---------------------------------------------------------------------------------
 * BatchNorm2d (train / eval), ReLU, residual add -- replaces nn.BatchNorm2d / nn.ReLU /
 * `out += residual` in residual.py:20-41,56-57, vgg.py:28-30.
 * Statistics: stats stripes produced by iic_conv_igemm; finalised per channel here.
 * ------------------------------------------------------------------------------- */
/* coef[0..4][C]: scale, shift, mean, invstd, unbiased batch variance.  use_running: eval() with
 * track_running_stats.  running_* nullable (track_running_stats=False).  Re-zeroes stats.
 * unbiased_count (0 = count): sample count of the unbiased running_var factor n/(n-1); differs
 * from `count` only under replica de-duplication (cluster_sobel.py:215-226 replicates imgs_curr
 * num_dataloaders times; forwarding the unique images once leaves mean / biased variance
 * unchanged, only this factor sees the true batch size).                                    */
int iic_bn_finalize(float* stats, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, long long* num_batches_tracked, float* coef, int C,
                    long count, long unbiased_count, float eps, float momentum, int training,
                    void* stream);
/* Deferred running-statistic update: what iic_bn_finalize does to running_mean / running_var /
 * num_batches_tracked (torch.nn.BatchNorm2d, momentum 0.1, unbiased variance; residual.py:20,23)
 * when it is given them, applied later from the coefficients it saved (coef row 2 = batch mean,
 * row 4 = unbiased batch variance).  Used when two forwards of one step run concurrently on two
 * streams and must not read-modify-write the same running statistics.  n BatchNorms per call;
 * the pointer arrays are HOST arrays of device pointers.                                     */
int iic_bn_running_update(int n, const float* const* coef, float* const* running_mean,
                          float* const* running_var, long long* const* num_batches_tracked,
                          const int* C, float momentum, void* stream);
/* out = relu( scale*y+shift  [+ res]  [+ scale2*y2+shift2] ) on PT interiors.            */
int iic_bn_apply(const void* y, const float* coef, const void* res, const void* y2,
                 const float* coef2, void* out, int N, int H, int W, int P, int C, int relu,
                 void* stream);
/* sums[stripe][2][C] += sum g, sum g*y  with g = dout * (act > 0) (act nullable => g = dout);
 * second BN (y2/sums2) optional (downsample branch shares g).
 * mask_coef (nullable, exclusive with act): the forward coef of THIS BatchNorm when its
 * activation was act = relu(scale*y + shift) with nothing added: the mask is then recomputed
 * as (scale*y + shift > 0) and the activation tensor is not read at all.                  */
int iic_bn_bwd_reduce(const void* dout, const void* act, const void* y, const void* y2,
                      float* sums, float* sums2, const float* mask_coef, int N, int H, int W, int P,
                      int C, void* stream);
/* from sums -> bcoef[0..2][C] = c1,c2,c3 (dy = c1*g + c2*y + c3), dgamma, dbeta. Re-zeroes sums. */
int iic_bn_bwd_finalize(float* sums, const float* gamma, const float* coef, float* bcoef,
                        float* dgamma, float* dbeta, int C, long count, void* stream);
int iic_bn_bwd_apply(const void* dout, const void* act, const void* y, const float* bcoef,
                     void* dy, const void* y2, const float* bcoef2, void* dy2,
                     const float* mask_coef, int N, int H, int W, int P, int C, void* stream);
/* Backward of a BatchNorm that normalised with its running statistics (eval(), or a frozen layer of a
 * fine-tuning run: what torch.nn.functional.batch_norm(training=False) differentiates to; residual.py:20,23,56-57,
 * vgg.py:28-30 under net.eval()).  One pass over the PT interiors: dy = bf16(scale * g) with scale = coef row 0
 * (iic_bn_finalize(training=0)) and g as in iic_bn_bwd_reduce (act / mask_coef: the same three mask modes), and
 * sums += sum g, sum g*y into the accumulators of iic_bn_bwd_reduce.  Second BatchNorm sharing g (downsample
 * branch): y2, coef2, dy2, sums2 -- all four or none.  C: 64, 128, 256, 512, 1024, 2048 (IIC_ERR_UNSUPPORTED
 * otherwise, nothing launched).  The border of dy / dy2 is not written.                                        */
int iic_bn_bwd_frozen(const void* dout, const void* act, const void* y, const float* coef, void* dy,
                      const void* y2, const float* coef2, void* dy2, float* sums, float* sums2,
                      const float* mask_coef, int N, int H, int W, int P, int C, void* stream);
/* from sums and the forward coef -> dgamma = (sum g*y - running_mean * sum g) * invstd, dbeta = sum g (in
 * double; both nullable).  bcoef (nullable) receives (scale, 0, 0): dy = c1*g + c2*y + c3 of iic_bn_bwd_apply,
 * iic_stem_wgrad_combine and iic_stem_bwd_wgrad is then the frozen gradient.  Re-zeroes sums.  The running
 * statistics and num_batches_tracked are not touched.                                                        */
int iic_bn_bwd_finalize_frozen(float* sums, const float* coef, float* bcoef, float* dgamma, float* dbeta,
                               int C, void* stream);

/* ---------------------------------------------------------------------------------
 * Stem: conv3x3(Cin<=5 -> 64, pad 1, no bias) + BN + ReLU + MaxPool(k2,s2,p1), computed
 * from the fp32 NCHW input with exact-fp32 MFMA and RECOMPUTED in every pass instead of
 * materialising the 96x96x64 tensor.  Replaces net5g.py:21-26,42-45.
 * Shapes: 1 <= Cin <= 5, H and W even and >= 2.  Widths served (IIC_ERR_UNSUPPORTED beyond,
 * before anything is launched):
 *   iic_stem_stats, iic_stem_apply_pool, iic_stem_bwd_reduce: W <= 256 (8 waves of 32 columns);
 *   iic_stem_bwd_wgrad: the two conv rows, the transposed dy tile and four input rows must fit
 *     the workgroup's 160 KB of LDS -- W <= 204, 196, 192, 192, 186 for Cin = 1 .. 5;
 *   iic_stem_bwd_fused: W <= 254 for Cin <= 3 (register-resident kernel), else as iic_stem_bwd_wgrad.
 * ------------------------------------------------------------------------------- */
int iic_stem_stats(const float* x, const float* w, float* stats, int N, int Cin, int H, int W,
                   void* stream);
int iic_stem_apply_pool(const float* x, const float* w, const float* coef, void* out_pt, int N,
                        int Cin, int H, int W, void* stream);
int iic_stem_bwd_reduce(const float* x, const float* w, const float* coef, const void* dpool_pt,
                        float* sums, int N, int Cin, int H, int W, void* stream);
long iic_stem_wgrad_partial_floats(void);
int iic_stem_bwd_wgrad(const float* x, const float* w, const float* coef, const float* bcoef,
                       const void* dpool_pt, float* partials, float* dW, int N, int Cin, int H,
                       int W, void* stream);
/* Fused stem backward (one recompute pass instead of two): `sums` as iic_stem_bwd_reduce AND the
 * coefficient-free weight-gradient GEMMs G1 = sum g*patch, G2 = sum y*patch (+ G3 = sum patch)
 * into `partials` (iic_stem_wgrad_partial_floats() floats).  dy = c1*g + c2*y + c3 is affine
 * with per-channel coefficients, so after iic_bn_bwd_finalize
 *   dW[co][k] = c1[co]*G1[co][k] + c2[co]*G2[co][k] + c3[co]*G3[k]   (iic_stem_wgrad_combine). */
int iic_stem_bwd_fused(const float* x, const float* w, const float* coef, const void* dpool_pt,
                       float* sums, float* partials, int* nblocks_out, int N, int Cin, int H, int W,
                       void* stream);
int iic_stem_wgrad_combine(const float* partials, int nblocks, const float* bcoef, float* dW, int Cin,
                           void* stream);
/* First-layer convolution of the VGG-style trunks from the fp32 NCHW image (Cin*K*K <= 128,
 * K = 3 (pad 1) or 5 (pad 2), 64 output channels) -- replaces the first nn.Conv2d of
 * code/archs/cluster/vgg.py:24-26 (net6c.py:16-20, net10a.py:21-25).  Exact fp32 MFMA.
 * out: PT bf16 [N][H+2P][W+2P][64]; stats as for iic_conv_igemm (nullable).               */
int iic_firstconv_fwd(const float* x, const float* w, void* out_pt, float* stats, int N, int Cin,
                      int H, int W, int K, int pad, int P, void* stream);
long iic_firstconv_wgrad_partial_floats(void);
int iic_firstconv_wgrad(const float* x, const void* dy_pt, float* partials, float* dW, int N,
                        int Cin, int H, int W, int K, int pad, int P, void* stream);
/* nn.MaxPool2d(kernel_size=2, stride=2) (vgg.py:19-20) on PT tensors; backward routes to the
 * first arg-max in scan order like torch.                                                 */
int iic_maxpool2_fwd(const void* in_pt, void* out_pt, int N, int H, int W, int Pi, int Po, int C,
                     void* stream);
int iic_maxpool2_bwd(const void* in_pt, const void* dout_pt, void* din_pt, int N, int H, int W,
                     int Pi, int Po, int C, void* stream);
/* The same pool behind a BatchNorm + ReLU whose output is never stored (the pooled stages of vgg.py:19-30): y_pt is the
 * convolution output (PT bf16), coef the BatchNorm's forward coefficients (iic_bn_finalize); every element enters the
 * window as a = bf16(relu(scale*y + shift)) -- bit for bit what iic_bn_apply would have written.  Forward: out = maxpool(a)
 * (one full-tensor write and one read less per pooled stage); backward: din (gradient w.r.t. a) = dout at the first
 * arg-max of a in scan order, 0 elsewhere.                                                                            */
int iic_bn_relu_maxpool2_fwd(const void* y_pt, const float* coef, void* out_pt, int N, int H, int W, int Pi,
                             int Po, int C, void* stream);
int iic_bn_relu_maxpool2_bwd(const void* y_pt, const float* coef, const void* dout_pt, void* din_pt, int N,
                             int H, int W, int Pi, int Po, int C, void* stream);
/* Sobel pre-op -- replaces code/utils/cluster/transforms.py:47-96 (grey channel -> dx,dy;
 * other channels copied through in the reference's order).                              */
int iic_sobel(const float* imgs, float* out, int N, int C, int H, int W, int include_rgb,
              int using_IR, void* stream);

/* ---------------------------------------------------------------------------------
 * Heads: AvgPool(global) + Linear + Softmax(dim=1) per sub-head -- replaces
 * net5g.py:31-39,53,69-80.  fp32 throughout (feeds the loss).
 * ------------------------------------------------------------------------------- */
int iic_avgpool_fwd(const void* in_pt, float* feats, int N, int H, int W, int P, int C,
                    void* stream);
int iic_avgpool_bwd(const float* dfeats, void* din_pt, int N, int H, int W, int P, int C,
                    const void* mask_act_pt /* nullable: din = 0 where this activation <= 0 */,
                    void* stream);
/* C[m][n] (+)= sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] (+ bias[n]); exact fp32 MFMA      */
int iic_gemm_f32(const float* A, long sam, long sak, const float* B, long sbk, long sbn,
                 const float* bias, float* C, long scm, int M, int Nn, int K, int accumulate,
                 void* stream);
/* Same product with a caller-provided fp32 workspace of iic_gemm_f32_ws_floats(...) elements (0 = none needed):
 * launches with too few output tiles for the chip split K between blocks, partial tiles go to the workspace
 * and are folded in a fixed order (deterministic).  iic_gemm_f32 == this with ws = NULL (no split).          */
long iic_gemm_f32_ws_floats(long sam, long sak, long sbk, long sbn, int M, int Nn, int K);
int iic_gemm_f32_ws(const float* A, long sam, long sak, const float* B, long sbk, long sbn,
                    const float* bias, float* C, long scm, int M, int Nn, int K, int accumulate,
                    float* ws, long ws_floats, void* stream);
int iic_gemm_f32_splitk(const float* A, long sam, long sak, const float* B, long sbk, long sbn,
                        float* C, long scm, int M, int Nn, int K, int splitk, void* stream);
/* SegmentationNet10a head (net10a.py:44-59): PT feature window <-> fp32 matrix for the 1x1
 * conv (padding 1) GEMM, and bilinear up-sampling (align_corners=False) fwd / bwd between
 * pixel-major [N][Hl][Wl][k] and NCHW [N][k][S][S].                                        */
int iic_seg_window_gather(const void* pt, float* out, int N, int Hw, int Ww, int Hp, int Wp, int off,
                          int C, void* stream);
int iic_seg_window_scatter(const float* in, void* pt, int N, int Hw, int Ww, int Hp, int Wp, int off,
                           int C, void* stream);
/* Fused 10a head on the bf16 PT feature window (net10a.py:44-59: the 1x1 conv with padding 1, its
 * input gradient and its weight gradient) -- the window is read / written in place, W stays fp32,
 * products and sums are exact fp32 (v_mfma_f32_16x16x4_f32).  Supported: C = 256 or 512, k <= 32
 * (iic_seg_head_supported); otherwise the gather + iic_gemm_f32 + scatter chain above.
 * logits, dlog: fp32 [M][k] row-major, M = N*Hw*Ww; w: fp32 [k][C].
 * iic_seg_head_bwd_dx writes the window's interior rows of pt_dx (bf16) only -- the ring is the
 * conv's zero padding.  iic_seg_head_wgrad writes iic_seg_head_wgrad_chunks(M) partial matrices
 * [chunk][k][C]; fold them in order with iic_colsum_f32 (deterministic, no atomics).            */
int iic_seg_head_supported(int C, int k);
int iic_seg_head_wgrad_chunks(long M);
int iic_seg_head_fwd(const void* pt, const float* w, float* logits, int N, int Hw, int Ww, int Hp,
                     int Wp, int off, int C, int k, void* stream);
int iic_seg_head_bwd_dx(const float* dlog, const float* w, void* pt_dx, int N, int Hw, int Ww, int Hp,
                        int Wp, int off, int C, int k, void* stream);
int iic_seg_head_wgrad(const float* dlog, const void* pt, float* partials, int N, int Hw, int Ww,
                       int Hp, int Wp, int off, int C, int k, void* stream);
/* The head's weight gradient on the gather + GEMM chain (k > 32; net10a.py:44-48, the backward of the 1x1 conv
 * w.r.t. its weight): partials[chunk][k][C] = sum over the chunk's rows of dlog[m][j] * window[m][c], window the
 * fp32 matrix iic_seg_window_gather wrote ([M][C], 16-byte aligned), iic_seg_head_wgrad_chunks(M) chunks; fold
 * them in order with iic_colsum_f32: a fixed summation order, no float atomics.  Any k >= 1; C = 256 or 512
 * (else IIC_ERR_UNSUPPORTED: iic_gemm_f32_splitk then).                                                      */
int iic_seg_window_wgrad(const float* dlog, const float* window, float* partials, long M, int C, int k,
                         void* stream);
/* Bilinear up-sampling [N][Hl][Wl][k] -> [N][k][S][S], align_corners = False (net10a.py:55-59, F.interpolate),
 * and its adjoint.  Rows that fit 64 KB of LDS (2 Wl k floats forward, Wl k backward) run the resident-row
 * kernels; longer ones column-windowed kernels that compute every element by the same operations in the same
 * order (bit-identical).  Forward: any Hl, Wl, S, k <= 2048.  Backward: S <= 3.5 Hl and S <= 3.5 Wl, k <= 16384. */
int iic_bilinear_fwd(const float* in_nhwc, float* out_nchw, int N, int Hl, int Wl, int k, int S,
                     void* stream);
int iic_bilinear_bwd(const float* dout_nchw, float* din_nhwc, int N, int Hl, int Wl, int k, int S,
                     void* stream);
int iic_softmax_fwd(const float* logits, float* probs, int rows, int k, void* stream);
int iic_softmax_bwd(const float* probs, const float* dprobs, float* dlogits, int rows, int k,
                    void* stream);
int iic_colsum_f32(const float* A, float* out, int rows, int cols, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------
 * Adam -- replaces torch.optim.Adam as used by code/utils/cluster/general.py:5-9
 * (betas (0.9,0.999), eps 1e-8, no weight decay, no amsgrad).  Multi-tensor: `n` tensors.
 * ptrs are HOST arrays of device pointers.
 * ------------------------------------------------------------------------------- */
/* grads2: optional second gradient source (NULL, or a host array whose entries may be NULL): the
 * update uses grads[i] + grads2[i] -- the two views of a step may accumulate their parameter
 * gradients separately (iic_amd.ops.branch) and are summed here instead of by extra kernels;
 * grads[i] may then be NULL as well (a tensor that only the second view touched).           */
int iic_adam_step(int n, float* const* params, const float* const* grads, const float* const* grads2,
                  float* const* exp_avg, float* const* exp_avg_sq, const long* numel, float lr,
                  float beta1, float beta2, float eps, int step, void* stream);
/* Same update with the step count kept on the DEVICE: `steps_done` (int32) = updates already
 * applied to these tensors; the kernel derives the bias corrections from it and a trailing
 * 1-thread kernel increments it.  No launch argument changes between steps, so the optimiser
 * step can be part of a captured HIP graph (iic_amd.graph).                                  */
int iic_adam_step_dev(int n, float* const* params, const float* const* grads,
                      const float* const* grads2, float* const* exp_avg, float* const* exp_avg_sq,
                      const long* numel, float lr, float beta1, float beta2, float eps,
                      int* steps_done, void* stream);
/* ... and with the learning rate read from DEVICE memory too (lr_dev != NULL; `lr` is then ignored): the
 * reference scales param_groups[i]["lr"] in place between epochs (update_lr, general.py:12-23), and a
 * captured step must see the new rate without being re-captured.                                        */
int iic_adam_step_devlr(int n, float* const* params, const float* const* grads,
                        const float* const* grads2, float* const* exp_avg, float* const* exp_avg_sq,
                        const long* numel, const float* lr_dev, float lr, float beta1, float beta2,
                        float eps, int* steps_done, void* stream);

/* ---------------------------------------------------------------------------------
 * Exact-fp32 path (SURVEY.md 8c parity tier T2; csrc/f32_path.hip).  The same operators as above
 * on fp32 PT tensors -- same geometry descriptors, epilogue flags and statistic accumulators --
 * as plain one-thread-per-output kernels.  Selected only by iic_amd.ops.fp32_mode(): it lets a whole
 * network be compared with the reference's fp32 results to ~1e-4; never used by the product path.
 * Weights are the fp32 OIHW parameters themselves (wtaps = kh*kw); transposed = 1 for the
 * backward-data geometries (the geometry's output channels are the parameter's input channels).
 * ------------------------------------------------------------------------------- */
int iic_f32_conv(const iic_conv_geom* g, const float* in, const float* w_oihw, int wtaps, int transposed,
                 float* out, float* stats, const float* res_grad, const float* res_act, int accumulate,
                 void* stream);
int iic_f32_wgrad(const iic_conv_geom* g, const float* x, const float* dy, float* dW_oihw, int wtaps,
                  int accumulate, void* stream);
int iic_f32_bn_apply(const float* y, const float* coef, const float* res, const float* y2, const float* coef2,
                     float* out, int N, int H, int W, int P, int C, int relu, void* stream);
int iic_f32_bn_bwd_reduce(const float* dout, const float* act, const float* y, const float* y2, float* sums,
                          float* sums2, const float* mask_coef, int N, int H, int W, int P, int C,
                          void* stream);
int iic_f32_bn_bwd_apply(const float* dout, const float* act, const float* y, const float* bcoef, float* dy,
                         const float* y2, const float* bcoef2, float* dy2, const float* mask_coef, int N, int H,
                         int W, int P, int C, void* stream);
int iic_f32_avgpool_fwd(const float* in_pt, float* feats, int N, int H, int W, int P, int C, void* stream);
int iic_f32_avgpool_bwd(const float* dfeats, float* din_pt, int N, int H, int W, int P, int C,
                        const float* mask_act_pt, void* stream);
/* nn.MaxPool2d(2, 2, padding=1) of the ClusterNet5g stem (net5g.py:26), PT (P = 1) in and out */
int iic_f32_maxpool_s2p1_fwd(const float* in_pt, float* out_pt, int N, int H, int W, int C, void* stream);
int iic_f32_maxpool_s2p1_bwd(const float* in_pt, const float* dout_pt, float* din_pt, int N, int H, int W, int C,
                             void* stream);
int iic_f32_nchw_to_pt(const float* x_nchw, float* out_pt, int N, int C, int H, int W, int P, void* stream);
/* nn.MaxPool2d(2, 2) of the VGG-style trunks and the SegmentationNet10a head's window copies */
int iic_f32_maxpool2_fwd(const float* in_pt, float* out_pt, int N, int H, int W, int Pi, int Po, int C,
                         void* stream);
int iic_f32_maxpool2_bwd(const float* in_pt, const float* dout_pt, float* din_pt, int N, int H, int W, int Pi,
                         int Po, int C, void* stream);
int iic_f32_window_gather(const float* pt, float* out, int N, int Hw, int Ww, int Hp, int Wp, int off, int C,
                          void* stream);
int iic_f32_window_scatter(const float* in, float* pt, int N, int Hw, int Ww, int Hp, int Wp, int off, int C,
                           void* stream);

/* one-time device probes used by the test-suite (documented in DESIGN.md) */
int iic_probe_tr16(void* out_u16_64x4, void* stream);

/* ---------------------------------------------------------------------------------
 * Evaluation counts -- replaces the per-(cluster, class) masked sums with
 * a host sync each of code/utils/cluster/eval_metrics.py:18-24 (_original_match), :42-46
 * (_hungarian_match) and the equality count of _acc (:69).
 * preds / targets: int64 [n] (torch.long, as the reference's flat_preds / flat_targets);
 * counts int64 [k_pred][k_gt] (zeroed here): counts[c1][c2] = #{i : preds[i]==c1, targets[i]==c2}.
 * Labels outside [0, k) match nothing.  k_pred * k_gt <= 16384.
 * ------------------------------------------------------------------------------- */
int iic_contingency(const long long* preds, const long long* targets, long n, int k_pred, int k_gt,
                    long long* counts, void* stream);
int iic_count_equal(const long long* a, const long long* b, long n, long long* count, void* stream);

/* ---------------------------------------------------------------------------------
 * Clustering evaluation on the device (csrc/eval_metrics.hip) -- replaces, in
 * code/utils/cluster/cluster_eval.py, the per-sub-head torch.argmax and the copies into flat int32
 * arrays of the whole data set (:55-63), and everything :128-132 and :212-228 derive from those
 * arrays (the reorder loops, 2 launches per output cluster and sub-head, and _acc).  One launch per
 * batch, all sub-heads.
 * probs: fp32; row i of sub-head h is the k consecutive floats at probs + i*ld + h*head_stride (the
 * packed softmax output [n][H][k] has ld = H*k, head_stride = k; a padded ld works).
 * targets: int64 [n], may be NULL when counts is.
 * pred = torch.argmax of the row for EVERY input: the first maximal index wins, a NaN counts as
 * maximal and the first NaN wins.
 * counts: int64 [H][k*gt_k + 1], may be NULL, ACCUMULATED (the caller zeroes it once): for every
 * sample counts[h][k*gt_k] += 1 and, if 0 <= targets[i] < gt_k, counts[h][pred*gt_k + targets[i]] += 1.
 * labels: int32, may be NULL: labels[h*label_stride + i] = pred.
 * counts without targets, or both outputs NULL: IIC_ERR_ARG.  n = 0: no-op.  Any k >= 1; no cap on
 * k * gt_k (the bins live in global memory).  Integer atomics: the result does not depend on
 * arrival order.
 * ------------------------------------------------------------------------------- */
int iic_cluster_argmax_acc(const float* probs, long ld, long head_stride, long n, int H, int k,
                           const long long* targets, int gt_k, long long* counts, int* labels,
                           long label_stride, void* stream);

/* ---------------------------------------------------------------------------------
 * Segmentation evaluation on the device (csrc/seg_eval.hip).
 *
 * iic_seg_label_map -- replaces, for evaluation, the full-resolution probability maps of
 * code/utils/segmentation/segmentation_eval.py:84 (x_outs = net(imgs), [N][k][S][S] fp32) and their
 * torch.argmax at :100.  probs_nhwc: the low-resolution softmax [N][Hl][Wl][k] fp32 (what the head has
 * before iic_bilinear_fwd); labels_u8: uint8 [N][S][S], the arg-max over classes of the bilinear
 * up-sampling (F.interpolate, align_corners=False), lowest class index on a tie.  Every class value is
 * the fp32 number iic_bilinear_fwd stores, so the labels equal the arg-max of its output bit for bit.
 * 1 <= k <= 255 (segmentation_eval.py:49); any Hl, Wl, S.
 *
 * iic_seg_contingency_acc -- replaces the flat test-set arrays and their masked_select
 * (segmentation_eval.py:101-106, :126-128), the widening to int64 in front of iic_contingency, the
 * reorder loop of code/utils/cluster/cluster_eval.py:128-131, :216-217 and _acc (:132, :227): all of
 * these are functions of one count matrix.  preds / targets / mask: uint8 [n], mask may be NULL (every
 * sample selected).  counts: int64 [k_pred * k_gt + 1], ACCUMULATED (the caller zeroes it once): for
 * every i with mask[i] != 0, counts[k_pred * k_gt] += 1 and, if preds[i] < k_pred and
 * targets[i] < k_gt, counts[preds[i] * k_gt + targets[i]] += 1.  k_pred * k_gt <= 16384.  n = 0: no-op.
 * Integer atomics: the result does not depend on arrival order.
 * ------------------------------------------------------------------------------- */
int iic_seg_label_map(const float* probs_nhwc, unsigned char* labels_u8, int N, int Hl, int Wl, int k, int S,
                      void* stream);
int iic_seg_contingency_acc(const unsigned char* preds_u8, const unsigned char* targets_u8,
                            const unsigned char* mask_u8, long n, int k_pred, int k_gt, long long* counts,
                            void* stream);

/* ---------------------------------------------------------------------------------
 * Paired augmentation on the GPU -- replaces the per-sample PIL pipelines
 * of code/utils/cluster/transforms.py that the DataLoaders of code/utils/cluster/data.py:223-335
 * run on the host:
 *   :107-217 sobel_make_transforms, default branch (RGB sources, channels = 3): RandomCrop ->
 *            Resize(BILINEAR) -> [RandomHorizontalFlip -> ColorJitter] -> custom_greyscale_to_tensor (:12-25)
 *   :220-330 greyscale_make_transforms (mode "L" sources, channels = 1): [RandomRotation] ->
 *            crop (one of several sizes) -> Resize -> [flip] -> [ColorJitter] -> ToTensor
 * Results are bit-identical to PIL's (oracle/augment_oracle.py).
 * imgs_u8  uint8 [B][H][W][channels] (HWC, as the datasets hold them), resident in HBM.
 * iparams  int32 [N][20]: source image, crop x0, crop y0, flip, n_ops, op[4] (0 brightness,
 *          1 contrast, 2 saturation, 3 hue -- in application order), hue shift (uint8 wrap),
 *          table index, rotate flag, a0..a5 = PIL's inverse rotation matrix in 16.16 fixed point
 *          (source x = (a2 + a1*y + a0*x) >> 16, source y = (a5 + a4*y + a3*x) >> 16), then the
 *          cutout box of custom_cutout (transforms.py:28-44) in crop coordinates as
 *          (left | upper << 16), (right | lower << 16); right == left = no cutout.
 * norm     float [2][C] (means, then stds) of torchvision Normalize (--demean), or NULL.
 * fparams  float [N][4]: factor of brightness, contrast, saturation; [3] = hue factor (not read:
 *          the kernel uses the uint8 increment in iparams[9]).
 * tables_host  HOST int32 [n_tables][4] = (crop size, taps per output = row pitch of its kk table,
 *          first row of its bounds table, first int of its kk table), n_tables <= 8;
 * bounds   int32 [rows][2] (first tap, tap count), kk int32: Pillow's 22-bit resampling
 *          coefficients of crop -> S per table (square crops: both passes use the same table).
 * lut      float [256] = v / 255 as torch computes it.
 * out      float [N][C][S][S]; channels 3: C = 4 (R,G,B,grey) with include_rgb else 1 (grey);
 *          channels 1: C = 1.
 * ------------------------------------------------------------------------------- */
#define IIC_AUG_MAX_TABLES 8
int iic_augment(const void* imgs_u8, int B, int H, int W, int channels, const int* iparams,
                const float* fparams, int N, const int* tables_host, int n_tables,
                const int* bounds, const int* kk, int S, const float* lut, float* out,
                int include_rgb, const float* norm, void* stream);

/* ---------------------------------------------------------------------------------
 * iic_augment with the RandomAffine of sobel_make_transforms (code/utils/cluster/transforms.py:152-161; the
 * semi-supervised script switches it on, examples/commands.txt section 1.3 model 698):
 *   RandomApply([RandomAffine(18, scale=(0.9, 1.1), translate=(0.1, 0.1), shear=10, resample=BILINEAR, fillcolor=0)], p)
 * after the RandomCrop (and after fluid_warp's rotation of the whole image) and before the cutout and the Resize.  It
 * acts on the crop as an image of its own: img.transform(img.size, AFFINE, m, BILINEAR) of Pillow (Geometry.c:
 * affine_transform + bilinear_filter32RGB) in IEEE double, bit for bit -- coordinates (m0 (x + .5) + m1 (y + .5)) + m2,
 * zero where they leave [0, crop) BEFORE the half-pixel shift, floor, neighbours clamped to the crop, the row below
 * taken only when it exists, truncation to uint8.
 * Every argument as for iic_augment (channels = 3 only: greyscale_make_transforms has no affine), and
 * iparams[11] bit 0: rotate the whole image before the crop (iic_augment's rotate flag); bit 1: this row is affined.  A
 *          row without bit 1 gives exactly iic_augment's output.
 * aparams  double [N][6], required: the INVERSE matrix torchvision's _get_inverse_affine_matrix computes, as
 *          Image.transform receives it (output pixel -> crop coordinates); read for rows with bit 1 only.  The kernel
 *          reads nothing outside the crop for any values; a NaN coordinate reads as outside (zero).
 * IIC_ERR_UNSUPPORTED, before any launch, when the crop planes do not fit the workgroup's LDS:
 *          align16(3 crop max(crop, S)) + 3 max(crop, S)^2 bytes > 150 KB (84 -> 96: 51 KB, as iic_augment).
 * ------------------------------------------------------------------------------- */
int iic_augment_affine(const void* imgs_u8, int B, int H, int W, int channels, const int* iparams,
                       const float* fparams, const double* aparams, int N, const int* tables_host, int n_tables,
                       const int* bounds, const int* kk, int S, const float* lut, float* out,
                       int include_rgb, const float* norm, void* stream);

/* ---------------------------------------------------------------------------------
 * Paired augmentation of the segmentation datasets on the GPU -- replaces the per-sample host
 * pipeline of the training __getitem__:
 *   code/datasets/segmentation/potsdam.py:95-216    (_Potsdam._prepare_train)
 *   code/datasets/segmentation/cocostuff.py:104-230 (_Coco._prepare_train)
 * with pad_if_too_small / pad_and_or_crop / custom_greyscale_numpy of
 * code/utils/segmentation/transforms.py:7-88, for a whole batch in one launch.  The random affine
 * of the second view (transforms.py:91-128) is a following iic_affine_warp_fwd of img2.
 * imgs_u8    uint8 [B][H][W][Cs], Cs = 3 (RGB) or 4 (RGB + IR), resident in HBM.  With
 *            pre_scale_all these are the pre-scaled, truncated images (prepared once by the caller).
 * labels_u8  uint8 [B][H][W] fine labels, 255 = the reference's -1, or NULL (Potsdam: mask of ones);
 * relevance  uint8 [256]: _filter_label's mask (cocostuff.py:629-657, :734-760) as a function of the
 *            fine label; NULL exactly when labels_u8 is.  Padded label pixels are fine-label 0.
 * iparams    int32 [N][12]: source image, crop origin x0, y0 IN THE PADDED image (sources smaller
 *            than S are centred in zeros, int(x / 2.) arithmetic), flip bits (bit 0: img2 is flipped --
 *            the top row of affine2_to_1 is negated and the pixels are mirrored; bit 1: leave the
 *            mirroring of the pixels to the caller's warp), n_ops, op[4] (0 brightness, 1 contrast,
 *            2 saturation, 3 hue -- in application order), hue shift (uint8 wrap), 2 unused.
 * fparams    float [N][10]: factor of brightness, contrast, saturation, hue (not read: iparams[9]),
 *            then affine2_to_1 [2][3] before the flip (the identity without random affine).
 * lut        float [256] = v / 255 as torch computes it.
 * img1, img2 float [N][C][S][S]: no_sobel: R,G,B(,IR); else include_rgb: R,G,B,grey(,IR); else
 *            grey(,IR) -- the layouts sobel_process(..., using_IR) expects.  ColorJitter (PIL
 *            arithmetic, bit-exact) touches img2's RGB only.  grey = OpenCV 3.x's 8-bit RGB2GRAY,
 *            (R 4899 + G 9617 + B 1868 + 8192) >> 14, restated from its source (not PIL's L).
 * mask_img1  uint8 [N][S][S]; affine2_to_1 float [N][2][3].  S % 4 == 0 (16-byte stores).
 * ------------------------------------------------------------------------------- */
#define IIC_SEG_AUG_IPARAMS 12
#define IIC_SEG_AUG_FPARAMS 10
int iic_seg_augment(const void* imgs_u8, int B, int H, int W, int Cs, const void* labels_u8,
                    const void* relevance, const int* iparams, const float* fparams, int N, int S,
                    int no_sobel, int include_rgb, const float* lut, float* img1, float* img2,
                    void* mask_img1, float* affine2_to_1, void* stream);

/* ---------------------------------------------------------------------------------
 * iic_seg_augment for a dataset whose images differ in size (COCO-Stuff: every published command,
 * examples/commands.txt:74-97), optionally with use_random_scale.  The reference pads and crops each image by
 * its own extent: pad_if_too_small + pad_and_or_crop(mode="random") of
 * code/utils/segmentation/transforms.py:23-88, called from code/datasets/segmentation/cocostuff.py:133-135
 * (potsdam.py:117); the random scale is cocostuff.py:123-130 / potsdam.py:109-114.
 * imgs_u8    uint8, the images concatenated without padding: image i is [h_i][w_i][Cs] (row pitch w_i) and starts
 *            at PIXEL offsets[i]; Cs = 3 or 4 (with 4 every pixel stays 4-byte aligned).
 * offsets    int64 [B]; sizes int32 [B][2] = (h_i, w_i), 1 <= h_i, w_i <= 16384; total_px: pixels in the pack.
 *            An image with offsets[i] + h_i w_i > total_px (or an extent out of range) reads as a black image:
 *            no read leaves [0, total_px) whatever the tables hold.
 * labels_u8  uint8 at the same pixel offsets, one byte per pixel, 255 = -1, or NULL; relevance as for
 *            iic_seg_augment.  Label pixels outside the image are fine label 0 (pad_if_too_small zero-fills).
 * iparams, fparams, lut, img1, img2, mask_img1, affine2_to_1, no_sobel, include_rgb: as for iic_seg_augment;
 *            the crop origin is in THIS sample's padded image: sides of max(len, S), the source at
 *            int(max(len, S) / 2.) - int(len / 2.) inside, where len is the sample's h or w -- after the random
 *            scale, the scaled one.  ColorJitter's contrast mean divides by S * S, padding included.  A source
 *            index outside [0, B) reads as a black image.
 * taps       NULL: no random scale, no table is read.  Else iic_seg_resample_tap [N][2][S]: for sample n the S
 *            crop rows, then the S crop columns, of the crop in the image scaled by cv2.resize(fx = fy = scale)
 *            (OpenCV 3.x resize on float32, restated from its source, not compared against a cv2 binary):
 *            inside = 0 in the padding; i0, i1, a0, a1 the two INTER_LINEAR taps of the source side and their
 *            float32 weights; nearest the INTER_NEAREST source index (labels).  The kernel computes
 *            (p00 ax0 + p01 ax1) by0 + (p10 ax0 + p11 ax1) by1 on the uint8 pixels as float32, every product and
 *            sum rounded separately, and truncates R, G, B toward zero to uint8 before the jitter; IR (Cs = 4) is
 *            NOT truncated, as in the reference (potsdam.py:148-151 truncates the RGB part only, :170 divides the
 *            float IR plane): its output is value / 255.f.  With taps the crop origin in iparams is not read
 *            (the tables carry it).  Tap indices are clamped to the image.
 * The random affine of the second view is a following iic_seg_augment_warp of img2 (flip bit 1 defers the mirror).
 * One workgroup per sample, 16-byte planar stores (S % 4 == 0), no atomics: two calls give identical bytes.
 * ------------------------------------------------------------------------------- */
typedef struct iic_seg_resample_tap {
  int32_t i0, i1;
  float a0, a1;
  int32_t nearest;
  int32_t inside;
} iic_seg_resample_tap;
int iic_seg_augment_ragged(const void* imgs_u8, const long* offsets, const int* sizes, int B, long total_px,
                           int Cs, const void* labels_u8, const void* relevance, const int* iparams,
                           const float* fparams, const iic_seg_resample_tap* taps, int N, int S, int no_sobel,
                           int include_rgb, const float* lut, float* img1, float* img2, void* mask_img1,
                           float* affine2_to_1, void* stream);

/* ---------------------------------------------------------------------------------
 * iic_seg_augment_ragged on the ORIGINAL-resolution images with pre_scale_all AND use_random_scale: the reference
 * resizes the float image twice, by pre_scale_factor and then by the drawn scale, and truncates only after the crop
 * (code/datasets/segmentation/cocostuff.py:113-135, potsdam.py:103-117); the labels go through INTER_NEAREST twice.
 * A resident pre-scaled uint8 image cannot reproduce that (the truncation in between changes about half of the
 * final bytes), so this entry reads the originals and composes both stages per output pixel.
 * Every argument as for iic_seg_augment_ragged, except
 * taps2      iic_seg_resample_tap2 [N][2][S], required: for sample n the S crop rows, then the S crop columns, of the
 *            crop in the twice-resized image.  b0, b1: the INTER_LINEAR weights of the SECOND resize, whose two taps
 *            are indices k = 0, 1 on the pre-scaled side; i0[k], i1[k], a0[k], a1[k]: the two taps of the FIRST
 *            resize on the source side that produce pre-scaled index k; nearest: the source index of INTER_NEAREST
 *            applied twice; inside = 0 in the padding.  The kernel computes the four pre-scaled pixels as
 *            (p00 ax0 + p01 ax1) by0 + (p10 ax0 + p11 ax1) by1 in float32 WITHOUT truncating them, then
 *            (I00 bx0 + I01 bx1) by0' + (I10 bx0 + I11 bx1) by1' with the second stage's weights, every product and
 *            sum rounded on its own; R, G, B are truncated to uint8 before the jitter, IR (Cs = 4) leaves as
 *            value / 255.f untruncated.  Sixteen source pixels per output pixel; indices are clamped to the image.
 * pre_scale_all WITHOUT use_random_scale needs no entry of its own: it is iic_seg_augment_ragged with the taps of
 * scale = pre_scale_factor.
 * ------------------------------------------------------------------------------- */
typedef struct iic_seg_resample_tap2 {
  int32_t i0[2], i1[2];
  float a0[2], a1[2];
  float b0, b1;
  int32_t nearest;
  int32_t inside;
} iic_seg_resample_tap2;
int iic_seg_augment_ragged_prescaled(const void* imgs_u8, const long* offsets, const int* sizes, int B,
                                     long total_px, int Cs, const void* labels_u8, const void* relevance,
                                     const int* iparams, const float* fparams, const iic_seg_resample_tap2* taps2,
                                     int N, int S, int no_sobel, int include_rgb, const float* lut, float* img1,
                                     float* img2, void* mask_img1, float* affine2_to_1, void* stream);

/* ---------------------------------------------------------------------------------
 * pre_scale_all as one pass over a packed dataset -- replaces the resize the reference repeats on every access,
 *   code/datasets/segmentation/cocostuff.py:113-120, :242-249, :321-328; potsdam.py:103-106
 * cv2.resize(fx = fy = factor) with INTER_LINEAR on the float image and INTER_NEAREST on the labels (OpenCV 3.x's
 * resize restated from its source, not compared against a cv2 binary), the image truncated toward zero to uint8 as
 * `img.astype(np.uint8)` does after the crop.  RGB only (3 bytes per pixel): Potsdam's IR plane is never truncated.
 * imgs_u8, labels_u8 (or NULL), offsets, sizes, B, total_px: the source pack, as for iic_seg_augment_ragged, Cs = 3.
 * factor     0 < factor < 1 (cocostuff.py:114).  The coefficients are computed in the kernel, in double with
 *            contraction off: inv = 1. / factor, f = float32((d + 0.5) inv - 0.5), floor, clamps and 1.f - f in float32.
 * out_u8     uint8, out_px pixels of 3 bytes; out_labels_u8 uint8 [out_px], NULL exactly when labels_u8 is.
 * out_offsets int64 [B], out_pitch int32 [B], out_sizes int32 [B][2]: image i is written as [h'_i][w'_i] pixels with a
 *            row pitch of out_pitch[i] >= w'_i pixels from PIXEL out_offsets[i] -- back to back (pitch = w'), or the
 *            top-left corner of a slab; h'_i = cvRound(h_i factor), w'_i likewise, at least 1 (the caller computes
 *            them).  An image whose source extent leaves [0, total_px) or whose destination extent leaves
 *            [0, out_px) (or with an extent outside 1..16384) is skipped: nothing of it is written.
 * work       int32 [n_work][3] = (image, first output row, row count): one workgroup each, a one-dimensional grid
 *            (B exceeds a grid's y extent on the full COCO set).  Rows outside the image are ignored.
 * Pixels between the images (slab padding) are not written.  No atomics: two calls give identical bytes.
 * ------------------------------------------------------------------------------- */
int iic_seg_prescale(const void* imgs_u8, const void* labels_u8, const long* offsets, const int* sizes, int B,
                     long total_px, double factor, void* out_u8, void* out_labels_u8, const long* out_offsets,
                     const int* out_pitch, const int* out_sizes, long out_px, const int* work, int n_work,
                     void* stream);

/* random_affine's warp of the second view for iic_seg_augment_ragged (code/utils/segmentation/transforms.py:
 * 122-143: perform_affine_tf = F.affine_grid + F.grid_sample, bilinear, zero padding; then torch.flip(dims=[2]),
 * cocostuff.py:213-214), in the operation order of torch's CPU kernels, so that img2 equals the reference's bit for
 * bit on the reference-generated fixture (iic_affine_warp_fwd computes the same warp from a pixel-space matrix within
 * 2e-6 of it).  img2, out float [N][C][S][S] (out != img2); affine1_to_2 float [N][6], the matrix random_affine
 * draws, in normalised coordinates; flips int32 [N]: mirror the output row; base_grid float [S] =
 * linspace(-1, 1, S) * (S - 1) / S as F.affine_grid(align_corners=False) builds it (made by the host).            */
int iic_seg_augment_warp(const float* img2, const float* affine1_to_2, const int* flips,
                         const float* base_grid, float* out, int N, int C, int S, void* stream);

/* ---------------------------------------------------------------------------------
 * Test-time batches of the segmentation datasets on the GPU -- replaces the per-sample host pipeline of
 * the evaluation __getitem__:
 *   code/datasets/segmentation/potsdam.py:295-350   (_Potsdam._prepare_test)
 *   code/datasets/segmentation/cocostuff.py:309-358 (_Coco._prepare_test)
 * with pad_and_or_crop(mode="centre") over pad_if_too_small and custom_greyscale_numpy of
 * code/utils/segmentation/transforms.py:7-88, the per-class loop of _filter_label (potsdam.py:429-439,
 * cocostuff.py:629-657, :734-760), and the DataLoader + host-to-device copy of
 * code/utils/segmentation/data.py:129-149, for a whole batch in one launch.
 * imgs_u8, labels_u8, lut, no_sobel, include_rgb and the channel layout: as for iic_seg_augment; labels_u8
 *            is required here.
 * sizes      int32 [B][2]: (h, w) of every image, stored top-left in its [H][W] slab, each centre-cropped by
 *            its own extent; NULL: every image is H x W.
 * target_table uint8 [256]: the low 8 bits of _filter_label's returned label as a function of the fine label
 *            (entry 255: of -1).
 * relevance  uint8 [256] as for iic_seg_augment, or NULL: mask of ones (Potsdam, potsdam.py:342).
 * idx        int32 [N] source images; one outside [0, B) reads as a black image with fine label 0.
 * imgs       float [N][C][S][S]; targets, mask uint8 [N][S][S].  The source is centred in zeros of
 *            max(h, S) x max(w, S) and cut around (int(new_h / 2.), int(new_w / 2.)); padded label pixels are
 *            fine label 0.  S % 4 == 0, N <= 65535.  No atomics: two calls give identical bytes.
 * ------------------------------------------------------------------------------- */
int iic_seg_prepare_test(const void* imgs_u8, int B, int H, int W, int Cs, const void* labels_u8,
                         const int* sizes, const void* target_table, const void* relevance,
                         const int* idx, int N, int S, int no_sobel, int include_rgb, const float* lut,
                         float* imgs, void* targets, void* mask, void* stream);

/* ---------------------------------------------------------------------------------
 * Supervised head of the semi-supervised fine-tuning step (csrc/sup_head.hip) -- replaces
 *   code/archs/semisup/sup_head5.py:12-19, 33-37   (nn.Linear(dlen, 2048) + nn.BatchNorm1d + nn.ReLU on the
 *                                                   flattened layer-3 tensor of net5g.py:50-56)
 *   code/scripts/semisup/IID_semisup_STL10.py      (nn.CrossEntropyLoss on the head's logits)
 *   code/utils/semisup/general.py:46-93            (assess_acc_block: ten-crop sum, arg-max, count)
 * x_pt, dx_pt: bf16 PT tensors [N][H+2][W+2][C], border 1 (read as it is / never written).  K = C H W.
 * w: the fp32 parameter [F][K], columns in the reference's (c, h, w) flatten order (net5g.py:56).
 * Supported: N >= 1, any H, W, C % 64 == 0, F % 64 == 0; anything else returns IIC_ERR_UNSUPPORTED before a launch.
 * The three products run on the bf16 MFMA pipe with fp32 accumulation; no float atomics, every sum in a fixed order:
 * two calls give identical bits.
 * ------------------------------------------------------------------------------- */
/* wb [F][K] = bf16(w), round to nearest even, columns permuted to the PT interior order (h, w, c): the forward's
 * operand; wt [K][F]: its transpose, the backward-data operand.  Once per optimiser step. */
int iic_sup_weight_prep(const float* w, void* wb, void* wt, int F, int C, int H, int W, void* stream);
/* K slices S of the forward for this shape (0: unsupported shape): S > 1 needs ws, S * N * F floats; the slices'
 * partial matrices are added in index order, then the bias: S fp32 additions on top of the accumulator's. */
int iic_sup_fwd_nsplit(int N, int F, int C, int H, int W);
/* y[n][f] = sum_k x[n][k] wb[f][k] + bias[f] (bias nullable), y fp32 [N][F]; the PT interior is read in place
 * (sup_head5.py:35 on net5g.py:56's view) */
int iic_sup_linear_fwd(const void* x_pt, const void* wb, const float* bias, float* y, float* ws, int N, int F, int C,
                       int H, int W, void* stream);
/* dyb [N][F] = bf16(dy), dyt [F][Np] = its transpose, Np = N rounded up to a multiple of 64, zero beyond N: the
 * operands of the two backward products */
int iic_sup_dy_cast(const float* dy, void* dyb, void* dyt, int N, int F, void* stream);
/* dx[n][k] = sum_f dyb[n][f] wt[k][f], stored round-to-nearest-even as bf16 into the interior of dx_pt (the backward
 * of sup_head5.py:35 w.r.t. its input; no ReLU mask: layer 3's last block masks its own output gradient) */
int iic_sup_linear_bwd_dx(const void* dyb, const void* wt, void* dx_pt, int N, int F, int C, int H, int W, void* stream);
/* dW[f][c HW + p] = sum_n dyt[f][n] x[n][p][c]: fp32, in the parameter's own column order; db: iic_colsum_f32 */
int iic_sup_linear_wgrad(const void* dyt, const void* x_pt, float* dW, int N, int F, int C, int H, int W, void* stream);
/* nn.BatchNorm1d(F) + nn.ReLU over fp32 [N][F] (sup_head5.py:16-17).  training != 0: batch mean and biased variance,
 * running_mean / running_var (nullable pair) updated with `momentum` and the unbiased variance; N == 1 is
 * IIC_ERR_ARG, as torch raises.  training == 0: the running statistics.  save_mean / save_invstd [F]: what the
 * backward needs, in both modes. */
int iic_sup_bn_relu_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float* y, float* save_mean, float* save_invstd, int N, int F, int training, float momentum,
                        float eps, void* stream);
/* g = dout where y > 0; dgamma = sum g xhat, dbeta = sum g; dx = gamma invstd (g - dbeta / N - xhat dgamma / N)
 * on batch statistics, gamma invstd g on running statistics */
int iic_sup_bn_relu_bwd(const float* dout, const float* x, const float* y, const float* gamma, const float* save_mean,
                        const float* save_invstd, float* dx, float* dgamma, float* dbeta, int N, int F, int training,
                        void* stream);
/* loss[0] = mean_n (logsumexp(logits[n]) - logits[n][targets[n]]), dlogits = (softmax - onehot) / N, from one
 * launch, max-subtracted fp32.  targets int64 [N], each in [0, k): the caller checks that on the host. */
int iic_sup_cross_entropy(const float* logits, const long long* targets, float* loss, float* dlogits, int N, int k,
                          void* stream);
/* assess_acc_block without the host arrays: per image b the `crops` rows logits[b crops + q] are added per class in
 * float64 in row order and divided by `crops`, the first maximal class (np.argmax) is compared with targets[b]
 * (int64 [B]); counts int64 [2] += (correct, B). */
int iic_sup_tencrop_acc(const float* logits, const long long* targets, long long* counts, int B, int k, int crops,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * k-means on the nets' pre-head features (csrc/kmeans.hip) -- replaces
 *   code/utils/cluster/baselines/triplets.py:134-173  (features copied to the host batch by batch, then
 *                                                      sklearn.cluster.KMeans(n_clusters=gt_k).fit on the host)
 *   code/utils/cluster/baselines/triplets.py:176-228  (triplets_eval's k-means branch consumes the labels)
 * for the features of kmeans_use_features=True (code/archs/cluster/net5g.py:73-78, net6c.py:52-57).
 * X: fp32 [n][d] with row stride ldx >= d (floats); C: fp32 [k][d], contiguous.
 * Served: 1 <= k <= 256, 1 <= d <= 32768, 1 <= n < 2^31; anything else is IIC_ERR_UNSUPPORTED, ldx < d or a null
 * pointer IIC_ERR_ARG, before a launch.  Dot products and one-hot sums run on the exact-fp32 MFMA pipe; no float
 * atomics: per-workgroup partial sums in a tile order that depends on (n, d, k) only, added in ascending order --
 * two runs give the same bits.
 * state: 64 bytes on the device {int32 iter, converged, pause, changed; double shift, inertia, tol, pad}.  The host
 * zeroes it and writes tol (the scaled tolerance) before the first iteration.  Once `converged` (1: no label changed,
 * 2: shift <= tol) or `pause` (a cluster came out empty: the host relocates, clears pause and calls the update with
 * force = 1) is set, every launch that is given the state returns at once without writing: a host may enqueue several
 * iterations and read the state once.
 * ------------------------------------------------------------------------------- */
/* 1 when (n, d, k) is served, else 0.  Host only. */
int iic_kmeans_supported(long n, int d, int k);
/* bytes of the workspace `ws` of the three calls below for (n, d, k); 0 when unsupported.  Host only. */
long iic_kmeans_workspace_bytes(long n, int d, int k);
/* labels[i] = arg-min_j ||c_j||^2 - 2 x_i.c_j (ties to the lowest j, always in [0, k)), mind[i] = max(0, ||x_i||^2 +
 * that score); sums [k][d] fp32 / counts [k] int64 of the rows per label (both null: assignment only); inertia
 * (nullable) = sum_i mind[i] in float64.  state nullable: with it the latch is honoured and labels that differ from
 * the incoming ones are counted into state.changed (fill labels with -1 before the first iteration). */
int iic_kmeans_assign(const float* X, long ldx, const float* C, long n, int d, int k, int* labels, float* mind,
                      float* sums, long long* counts, double* inertia, void* ws, void* state, void* stream);
/* c_j <- sums_j / counts_j (a cluster with count 0 keeps its row); state.shift = sum ||c_new - c_old||^2,
 * state.inertia = the sum of mind of the preceding iic_kmeans_assign on the same ws, both float64 in a fixed order;
 * iter += 1; the latch as above.  A count of 0 with force == 0 changes nothing but state.pause = 1. */
int iic_kmeans_update(float* C, const float* sums, const long long* counts, long n, int d, int k, int force, void* ws,
                      void* state, void* stream);
/* k-means++ support.  cand: int64 [ncand] row indices on the device, 1 <= ncand <= 8 (clamped to [0, n)).
 * pot[c] = sum_i min(mind[i], ||x_i - x_cand[c]||^2), float64, fixed order.  write != 0 (ncand == 1):
 * mind[i] <- min(mind[i], distance to the candidate) as well.  ws: iic_kmeans_workspace_bytes(n, d, 1) bytes. */
int iic_kmeans_seed_potential(const float* X, long ldx, long n, int d, const long long* cand, int ncand, float* mind,
                              int write, double* pot, void* ws, void* stream);

/* ---------------------------------------------------------------------------------
 * Segmentation k-means evaluation (csrc/seg_kmeans.hip) -- replaces, in
 * code/utils/segmentation/baselines/kmeans_segmentation_eval.py:
 *   :56, :141    net(imgs, penultimate=True).cpu().numpy(): the fp32 [N][512][S][S] up-sampled trunk features
 *   :64-66, :143-144  transpose and boolean mask on the host
 *   :78-91       the sampled feature rows
 *   :104         MiniBatchKMeans(n_clusters=gt_k).fit on the host
 *   :148-186     kmeans.predict per batch, flat int32 arrays of the test set, the reorder loop, _acc
 * ------------------------------------------------------------------------------- */
/* kmeans_segmentation_eval.py:141-152 and what :162-186 derive from the flat arrays.  dots_nhwc fp32 [N][Hl][Wl][k]: the
 * products x.c_j at the trunk's resolution; cnorm fp32 [k].  Per output pixel of [N][S][S]: every channel is up-sampled
 * with the operations and order of iic_bilinear_fwd, score_j = cnorm_j - 2 up_j in fp32, label = arg-min (lowest index
 * on a tie; a NaN score never beats a number; all NaN: label 0 -- the rule of iic_kmeans_assign).  The label is folded
 * with targets_u8 / mask_u8 ([N][S][S]; mask nullable) into counts int64 [k k_gt + 1] exactly as
 * iic_seg_contingency_acc does: accumulated, integer atomics, counts[label k_gt + target] += 1 for selected pixels with
 * target < k_gt, the number of selected pixels in the last cell.  labels_u8 (nullable, any alignment): the label map.
 * Served: 1 <= k <= 255, k k_gt <= 16384, any Hl, Wl, S; otherwise IIC_ERR_UNSUPPORTED before a launch.  Source rows
 * that do not fit the LDS budget are read from global memory: the same bits. */
int iic_seg_kmeans_label_acc(const float* dots_nhwc, const float* cnorm, const unsigned char* targets_u8,
                             const unsigned char* mask_u8, int N, int Hl, int Wl, int k, int S, int k_gt,
                             long long* counts, unsigned char* labels_u8, void* stream);
/* LDS floats iic_seg_kmeans_label_acc stages its sources in for this geometry; 0: the global-read form; -1: bad
 * arguments.  Host only. */
long iic_seg_kmeans_label_lds_floats(int Hl, int Wl, int k, int S);
/* kmeans_segmentation_eval.py:56-91 for the sampled pixels only.  pt: the PT feature tensor [N][Hp][Wp][C], bf16
 * (pt_is_f32 == 0) or fp32, interior Hl x Wl at `off`; coords int32 [m][3] = (n, y, x) at resolution S on the device
 * (clamped into range).  rows fp32 [m][C]: rows[i][c] is the number iic_bilinear_fwd would store at (n, c, y, x) for
 * the fp32-converted interior.  Any C >= 1; m == 0 is a no-op. */
int iic_seg_feat_sample(const void* pt, int pt_is_f32, const int* coords, long m, float* rows, int N, int Hl, int Wl,
                        int Hp, int Wp, int off, int C, int S, void* stream);
/* The centre update of scikit-learn's dense mini-batch step (sklearn/cluster/_k_means_minibatch.pyx
 * update_center_dense; _kmeans.py _mini_batch_step, MiniBatchKMeans._mini_batch_convergence, _random_reassign), which
 * kmeans_segmentation_eval.py:104 runs on the host.  sums / counts / ws: what iic_kmeans_assign produced for the batch
 * of n rows.  counts_j > 0: c_j <- (c_j w_j + sums_j) / (w_j + counts_j) in float64, w_j += counts_j; otherwise the row
 * stays.  C_old [k][d] receives the centres before the step; w: float64 [k].
 * state: 128 bytes on the device {int32 step, converged, pause, changed, n_since, no_improvement, have_ewa, have_min,
 * reassign_every, max_no_improvement; double inertia, ewa, ewa_min, shift, tol, alpha, ratio, norm; 24 bytes pad}.  The
 * host zeroes it and writes reassign_every (10 k), max_no_improvement (< 0: none), tol, alpha = min(1, 2 batch /
 * (n_samples + 1)), ratio and norm (the batch size).  The same block is given to iic_kmeans_assign for its latch.
 * A step is a reassignment step when a w_j was 0 before it or n_since + n >= reassign_every (n_since then restarts); on
 * such a step, after the update, any w_j < ratio max w sets `pause` and leaves the bookkeeping undone: the host
 * reassigns, clears pause and calls again with resume = 1, which updates nothing and completes the step (shift from
 * C_old, inertia from ws).  Bookkeeping: step += 1; from the second step on the exponentially weighted average of
 * inertia / norm, its minimum and the no-improvement counter; converged = 2 when tol > 0 and shift <= tol, 1 when the
 * counter reaches max_no_improvement.  Once converged or pause is set every launch given the state returns at once.
 * Fixed-order sums, no float atomics. */
int iic_kmeans_minibatch_update(float* C, float* C_old, const float* sums, const long long* counts, double* w, long n,
                                int d, int k, int resume, void* ws, void* state, void* stream);

/* ---------------------------------------------------------------------------------
 * Triplets baseline loss and its gradients (csrc/triplets.hip) -- replaces
 *   code/utils/cluster/baselines/triplets.py:231-238  (triplets_loss: log_softmax, two softmax, two kl_div with
 *                                                      reduction "elementwise_mean", and their backward nodes)
 * a (orig), b (pos), c (neg): fp32 logits [N][k], rows at stride ld >= k floats (one ld for all three).  With
 * lo = a - lse(a), lp = b - lse(b), lq = c - lse(c), p = exp(lp), q = exp(lq), tp_n = sum_j p (lp - lo),
 * tq_n = sum_j q (lq - lo):
 *   loss = sum_n (tp_n - tq_n) / (N k)       d_a = (q - p) / (N k)
 *   d_b  = p ((lp - lo) - tp_n) / (N k)      d_c = -q ((lq - lo) - tq_n) / (N k)
 * Row arithmetic is float64, every output is rounded to fp32 once.  The log-space form is the specification: log p is
 * b - lse(b), never log(exp(..)).  torch's own gradient of the target is 0 * (-inf) = NaN once a softmax entry
 * underflows; this kernel keeps the finite limit (such an entry contributes 0), so its d_b and d_c stay finite at
 * logit spreads where torch's are NaN.  Both KL terms are computed by one routine: with b and c bit-identical,
 * loss == 0, d_a == 0 and d_b == -d_c exactly.  No float atomics: one float64 partial per workgroup, added in index
 * order by a second launch -- two calls give the same bits.
 * Non-finite logits: the loss is non-finite exactly when torch's is (b_j = -inf alone contributes 0, as xlogy(0, 0)
 * does); every gradient of a row with a non-finite logit in any of the three inputs is NaN, other rows are untouched.
 * Served: 1 <= k <= 1024, N >= 1, N k < 2^31.
 * ------------------------------------------------------------------------------- */
/* 1 when (N, k) is served, else 0.  Host only. */
int iic_triplets_supported(long N, int k);
/* bytes of the workspace `ws` of iic_triplets_loss for (N, k); 0 when unsupported.  Host only. */
long iic_triplets_workspace_bytes(long N, int k);
/* loss: fp32 [1].  d_a, d_b, d_c: fp32 [N][k] contiguous.  d_b and d_c may both be NULL (the targets are constants:
 * skipped), d_a may be NULL together with them (loss only); any other combination, a null input, loss or ws, or
 * ld < k: IIC_ERR_ARG.  A shape outside the served range: IIC_ERR_UNSUPPORTED.  Either way before any launch. */
int iic_triplets_loss(const float* a, const float* b, const float* c, long ld, long N, int k, float* loss, float* d_a,
                      float* d_b, float* d_c, void* ws, void* stream);

/* ---------------------------------------------------------------------------------
 * Isola and Doersch segmentation baselines: patch sampler (csrc/seg_patches.hip), joint Linear (csrc/sup_head.hip)
 * and losses (csrc/seg_baseline_loss.hip).
 * coords: int32 [8] on the device, {cy, cx, oy, ox, label, 0, 0, 0}: the centre patch's centre, the other patch's
 * centre (row, column at resolution S) and the step's label (Isola: adjacent != 0; Doersch: position 0..8).  On the
 * device so that a captured step can be replayed with new patches; the kernels clamp what they read, the host wrappers
 * validate before they upload.
 * ------------------------------------------------------------------------------- */
/* code/archs/segmentation/baselines/net10a_isola.py:92-96, net10a_doersch.py:85-89 and
 * code/utils/segmentation/baselines/general.py:4-18 (F.interpolate of all C channels to S x S, then two p x p slices)
 * for the 2 p p sampled pixels per image only.  pt: the trunk's PT feature tensor [N][Hp][Wp][C], bf16 (pt_is_f32 == 0) or
 * fp32, interior Hl x Wl at `off`.  p odd, d = p / 2; centres are clamped into [d, S - 1 - d].
 * patches: one PT tensor [2 N][p + 2][p + 2][C] of the source's dtype, border 1: images 0 .. N - 1 hold the centre patch,
 * N .. 2 N - 1 the other patch.  Interior (i, j, c) of image q N + n is the number iic_bilinear_fwd stores at
 * (n, c, y_q - d + i, x_q - d + j) for the fp32-converted interior (align_corners=False, as F.interpolate), rounded to
 * nearest even once when the output is bf16.  The border is written as zeros.
 * Served: C even, p odd, p <= min(S, 127); otherwise IIC_ERR_UNSUPPORTED before a launch. */
int iic_seg_patch_sample_fwd(const void* pt, int pt_is_f32, const int* coords, void* patches, int N, int Hl, int Wl, int Hp,
                             int Wp, int off, int C, int S, int p, void* stream);
/* The adjoint (the backward nodes of the same lines).  dcentre, dother: the two halves of dpatches
 * [2 N][p + 2][p + 2][C] -- [N][p + 2][p + 2][C] each, images 0 .. N - 1 and N .. 2 N - 1; two pointers because the two
 * siamese-stage calls hand back two tensors (dother = dcentre + N (p + 2)(p + 2) C for one tensor).  Their borders are
 * not read.  dx_pt [N][Hp][Wp][C]: every element of the Hl x Wl interior is written exactly once -- zeros outside both
 * footprints --, the border never.  A gather in a FIXED ORDER: per element one fp32 accumulator,
 *     acc <- acc + g_q[n][i][j][c] * (wy(i) wx(j)),   product and sum rounded separately,
 * centre patch (q = 0) before other patch (q = 1), inside a patch the pixels in ascending (i, j); wy(i) =
 * [y0(i) == ys] (1 - ly(i)) + [y1(i) == ys] ly(i) with (y0, y1, ly) the source rows and weight of patch row i as
 * iic_bilinear_fwd computes them, wx(j) likewise, wy wx rounded once.  Patch pixels whose taps miss the element are
 * skipped.  Overlapping footprints both contribute.  One rounding to bf16 at the store.  No float atomics: two calls give
 * the same bits. */
int iic_seg_patch_sample_bwd(const void* dcentre, const void* dother, int pt_is_f32, const int* coords, void* dx_pt, int N,
                             int Hl, int Wl, int Hp, int Wp, int off, int C, int S, int p, void* stream);
/* The joint Linear(2 C p p -> F) of net10a_isola.py:29 / net10a_doersch.py:24 over torch.cat of the two flattened
 * siamese activations (net10a_isola.py:52-58, net10a_doersch.py:46-52) and its backward nodes:
 *     y[n][f] = sum_q sum_k a_q[n][k] w[f][q K + k] + b[f],   K = C p p in the parameter's (c, h, w) column order.
 * a0_pt, a1_pt (and dx0_pt, dx1_pt): bf16 PT tensors [N][p + 2][p + 2][C], border 1 -- the siamese stage's output for
 * the centre and for the other patch, read in place.  The kernels are those of iic_sup_* (bf16 MFMA, fp32 accumulation,
 * fixed-order sums, no float atomics: two calls give identical bits).
 * Served: N >= 1, any odd p, C % 64 == 0, F % 64 == 0; anything else returns IIC_ERR_UNSUPPORTED before a launch. */
/* wb [F][2 K] = bf16(w), each column half permuted to the PT interior order (h, w, c); wt [2 K][F]: its transpose.
 * Once per optimiser step. */
int iic_pair_weight_prep(const float* w, void* wb, void* wt, int F, int C, int p, void* stream);
/* K slices S of the forward for this shape (0: unsupported): S > 1 needs ws, S * N * F floats.  Host only. */
int iic_pair_linear_fwd_nsplit(int N, int F, int C, int p);
/* y fp32 [N][F]: the 2 K / 64 K-tiles -- those of q = 0, then those of q = 1 -- are cut into S consecutive slices, the
 * slices' partial matrices are added in index order, then the bias (nullable). */
int iic_pair_linear_fwd(const void* a0_pt, const void* a1_pt, const void* wb, const float* bias, float* y, float* ws, int N,
                        int F, int C, int p, void* stream);
/* dx_q[n][k] = sum_f dyb[n][f] wt[q K + k][f], bf16 (round to nearest even) into the interior of dx0_pt / dx1_pt; no
 * ReLU mask (the siamese stage's BatchNorm backward applies its own).  dyb / dyt: iic_sup_dy_cast. */
int iic_pair_linear_bwd_dx(const void* dyb, const void* wt, void* dx0_pt, void* dx1_pt, int N, int F, int C, int p,
                           void* stream);
/* dW[f][q K + c p p + hw] = sum_n dyt[f][n] a_q[n][hw][c]: fp32 [F][2 K], in the parameter's own column order. */
int iic_pair_linear_wgrad(const void* dyt, const void* a0_pt, const void* a1_pt, float* dW, int N, int F, int C, int p,
                          void* stream);
/* code/utils/segmentation/baselines/isola_utils.py:27-72 (isola_loss) and its backward, one launch, nothing read back
 * (the reference calls norm_factor.item() every step).  prob fp32 [N]: the net's output, sigmoid applied;
 * mask_u8 [N][S][S].  m_n = (mask[n][cy][cx] + mask[n][oy][ox]) > 0, norm = sum m_n; t_n = p_n (label != 0) or
 * fl32(1 - p_n); a row is dropped iff t_n < EPS = 2^-52 (sys.float_info.epsilon);
 *     loss = -(1 / norm) sum_kept m_n log t_n      dprob_n = -+ m_n / (norm t_n), exactly 0 for dropped rows
 * log and the sum in float64, rows in index order, one rounding to fp32 each.  The expression is evaluated as the
 * reference writes it, so a non-finite p behaves as float64 torch does (0 * NaN is NaN).  norm == 0: the loss and every
 * gradient are NaN (the reference dies of ZeroDivisionError there).  dprob nullable.  Two calls give the same bits. */
int iic_isola_loss(const float* prob, const unsigned char* mask_u8, const int* coords, float* loss, float* dprob, int N,
                   int S, void* stream);
/* code/utils/segmentation/baselines/doersch_utils.py:55-66 (doersch_loss with nn.CrossEntropyLoss(reduction="none")) and
 * its backward, one launch.  logits fp32 [N][k], k <= 32 (else IIC_ERR_UNSUPPORTED); the target of every row is the
 * block's label (clamped into [0, k)).  ce_n = logsumexp(x_n) - x_n[label], max-subtracted float64;
 *     loss = sum_n m_n ce_n / norm      dlogits = (m_n / norm) (softmax(x_n) - onehot)
 * rows in index order, one rounding to fp32 each; norm == 0 makes all of them NaN, the value of the reference's
 * expression.  dlogits nullable.  Two calls give the same bits. */
int iic_doersch_loss(const float* logits, const unsigned char* mask_u8, const int* coords, float* loss, float* dlogits,
                     int N, int k, int S, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IIC_HIP_H */
