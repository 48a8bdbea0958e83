// Persistent, DMA-fed implicit-GEMM convolution for the 64 -> 64 channel 3x3 layers (ResNet
// layer1 of ClusterNet5g: /root/reference/code/archs/cluster/residual.py:4-7,19,22 at 64 planes;
// forward and backward-data).  These layers sit at the HBM/MFMA ridge (AI 288):
// 0.4 GB of activations move per launch for 117 GFLOP, so the kernel is organised around the
// memory pipeline instead of around the MFMA loop:
//   * one persistent workgroup per CU (8 waves) walks a contiguous range of 256-row tiles;
//   * the input patch of tile t+1 is fetched by LDS-DMA (global_load_lds_dwordx4: no VGPRs, every
//     piece in flight at once) into the second patch buffer while tile t computes, and the
//     output rows of tile t-1 are stored while tile t computes => HBM reads, HBM writes and MFMA
//     overlap inside ONE workgroup; two barriers per tile;
//   * the whole weight operand of the wave (9 taps x 64 k x 32 couts, MFMA B-fragment order, see
//     iic_weight_prep_frag) is loaded ONCE into 144 VGPRs and stays there for every tile;
//   * LDS patch rows are 128 B, unpadded (DMA writes lane-linear), with the 16-byte slot XOR-ed by
//     (row >> 1) & 7: the DMA applies the swizzle on its SOURCE address, ds_read_b128 of 16
//     consecutive rows is conflict-free;
//   * BatchNorm statistics are accumulated in registers across all tiles, one atomic pass at the
//     end of the kernel.
#include "common.h"
#include "conv_plan.h"
#include "conv_tile.h"
#include "../../include/iic_hip.h"

#define P64_BM 256
#define P64_BN 64
#define P64_THREADS 512
#define P64_NT 9
#define P64_CLD P64_BN               // unpadded epilogue tile: LDS is the scarce resource here
#define P64_SC_BYTES(BM_) ((BM_) * P64_CLD * 2)   // 32768 at 256 rows
#define P64_NTAB 4                   // row tables are written two tiles ahead of their use
#define P64_TAB_BYTES(BM_) (P64_NTAB * (BM_) * (4 + 2))   // s_pout (int) + s_prow (u16)

// (n, y, x) of a GEMM row, advanced by one tile (256 rows) at a time: no per-tile divisions.
struct P64Walk {
  int n, y, x;
};
__device__ __forceinline__ void p64_walk_init(P64Walk& w, const iic_conv_geom& g, int m) {
  const int plane = g.MY * g.MX;
  w.n = m / plane;
  const int r = m - w.n * plane;
  w.y = r / g.MX;
  w.x = r - w.y * g.MX;
}
__device__ __forceinline__ void p64_walk_advance(P64Walk& w, const iic_conv_geom& g, int d_y, int d_x) {
  w.x += d_x;
  w.y += d_y;
  if (w.x >= g.MX) { w.x -= g.MX; ++w.y; }
  while (w.y >= g.MY) { w.y -= g.MY; ++w.n; }
}
// input / output pixel of the row; rows past the end repeat the last row and are never stored
__device__ __forceinline__ void p64_walk_pixels(const P64Walk& w, const iic_conv_geom& g, int& pin,
                                                int& pout) {
  const bool valid = w.n < g.N;
  const int n = valid ? w.n : g.N - 1, y = valid ? w.y : g.MY - 1, x = valid ? w.x : g.MX - 1;
  pin = (n * g.in_Hp + y * g.sy + g.oy) * g.in_Wp + x * g.sx + g.ox;
  pout = valid ? (n * g.out_Hp + y * g.ty + g.py) * g.out_Wp + x * g.tx + g.px : -1;
}

// FORM 1: one table row per thread, advanced by one tile with adds and selects only.  256 = d_n planes + d_y rows +
// d_x pixels with d_y < MY, d_x < MX, so each of x and y carries at most once.  `pin` / `pout` are the unclamped
// pixels of (n, y, x); rows with n >= N repeat the last row (pin) and are never stored (pout = -1).
struct P64Row {
  int n, y, x, pin, pout;
};
struct P64Step {
  int d_n, d_y, d_x, MY, MX, pin_step, pin_xw, pin_yw, pout_step, pout_xw, pout_yw;
};
__device__ __forceinline__ void p64_row_init(P64Row& r, const iic_conv_geom& g, int m) {
  P64Walk w;
  p64_walk_init(w, g, m);
  r.n = w.n; r.y = w.y; r.x = w.x;
  r.pin = (w.n * g.in_Hp + w.y * g.sy + g.oy) * g.in_Wp + w.x * g.sx + g.ox;
  r.pout = (w.n * g.out_Hp + w.y * g.ty + g.py) * g.out_Wp + w.x * g.tx + g.px;
}
__device__ __forceinline__ void p64_row_advance(P64Row& r, const P64Step& s) {
  r.n += s.d_n; r.y += s.d_y; r.x += s.d_x; r.pin += s.pin_step; r.pout += s.pout_step;
  const bool cx = r.x >= s.MX;
  r.x -= cx ? s.MX : 0; r.y += cx ? 1 : 0; r.pin += cx ? s.pin_xw : 0; r.pout += cx ? s.pout_xw : 0;
  const bool cy = r.y >= s.MY;
  r.y -= cy ? s.MY : 0; r.n += cy ? 1 : 0; r.pin += cy ? s.pin_yw : 0; r.pout += cy ? s.pout_yw : 0;
}

// One LDS-DMA block of FORM 1: 64 lanes x 16 bytes from (wave-uniform base + 32-bit lane offset) to LDS byte lds_dst +
// lane * 16 (conv_igemm_pw.hip pw_dma16s; M0 is compiler-reserved: saved and restored inside the statement).  Inline
// asm because hipcc waits vmcnt(0) in front of every LDS read that follows a DMA it knows about: in the first form that
// wait sits between the DMA issue and the tile's first read (the fetch of tile t + 1 is waited for in front of the K loop
// of tile t, not at the top of t + 1), and with the DMA inside the K loop it would also wait for each spread store.
__device__ __forceinline__ void p64_dma16s(unsigned voff, const unsigned char* sbase, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// ABL: timing-ablation build (WRONG results): 1 = only the first patch is fetched, 2 = no output
// stores, 4 = one tap instead of nine.
// RED: fused BatchNorm-backward reduction over the stored rows (conv_tile.h); the partial sums
// stay in registers across all tiles of the workgroup.
// Eight waves, two per SIMD, wave tile 64 rows x 32 couts (one A fragment read per MFMA: the LDS read
// pipe is as busy as the matrix pipe).  Tried and rejected: four "wide" waves, one per SIMD with 64 rows x
// 64 couts -- every A fragment feeds two MFMAs (half the LDS read traffic), the whole 9 x 64 x 64 weight operand
// sits in 288 registers of the wave, the A fragments of tap t+1 are read while the MFMAs of tap t run.  Measured
// (round 3, tools/p64_phases.py, 660 x 49 x 49, forward): NW = 8 155-165 us, wide 186-199 us -- a single wave per
// SIMD does not cover its own LDS latency (K loop 9.7 k cycles per tile against 5.9 k + 1.6 k of barrier wait).
// Where a tile's cycles go at NW = 8 (matrix pipe alone: 4.6 k; LAB.md S9, same tool and shape):
//   FORM 0, 10.6 k: K loop 6.0 k, barrier B 1.6 k, row tables + DMA issue 1.5 k, accumulators -> LDS 1.0 k, waiting for
//     the patch 0.3 k -- the K-loop figure hides a compiler-made vmcnt(0) between the DMA issue and the first LDS read;
//   FORM 1,  9.3 k: K loop 6.5 k (DMA issue and row tables inside it), barrier B 0.6 k, accumulators -> LDS + the next
//     tile's patch rows 1.3 k, waiting for the patch 0.5 k, spread-store bookkeeping 0.2 k;
// the residual epilogue of backward-data adds 5.7-6.0 k in both (its 64 KB of residual-gradient / mask loads per tile
// are exposed).
template <int ABL, int RED, bool FORM>
__global__ __launch_bounds__(512) void conv_igemm_p64_kernel(
    const iic_conv_geom g, const bf16_t* __restrict__ in, const unsigned char* __restrict__ wfrag,
    bf16_t* __restrict__ out, float* __restrict__ stats, const bf16_t* __restrict__ res_grad,
    const bf16_t* __restrict__ res_act, int accumulate, int num_tiles, int pb_bytes, int max_tap_off,
    const bf16_t* __restrict__ red_y, const float* __restrict__ red_coef,
    const bf16_t* __restrict__ red_y2, float* __restrict__ red_stats, float* __restrict__ red_stats2,
    unsigned long long* __restrict__ prof) {
  // PROF (ABL bit 8, results CORRECT): wave 0 sums the cycles (s_memtime) its workgroup spends in each phase of
  // the tile loop into prof[blockIdx][8]: wait for patch + barrier A | store of tile t-1 | DMA issue + row
  // tables | K loop | barrier B | accumulators -> LDS; [6] = tiles, [7] = whole loop (tools/p64_phases.py)
  constexpr bool PROF = (ABL & 8) != 0;
  // FORM 1 = closed-form patch addresses (every build) + the bookkeeping taken off the tile's serial path (BK).  With
  // the fused reduction's sums resident there is no register room for BK -- its scalar walkers and the work moved
  // into the K loop spill (RED 2: 72 B of scratch against 8) -- so those builds keep the first form's bookkeeping.
  constexpr bool BK = FORM && RED == 0;
  constexpr int NW = 8, BM = P64_BM;
  constexpr int NWM = BM / 64;                  // 64-row groups of the tile
  constexpr int SC_BYTES = BM * P64_CLD * 2, TAB_ROWS = P64_NTAB * BM;
  unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, t_a = 0, t_b = 0, t_loop = 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  unsigned char* const sP0 = smem_raw;                    // patch buffer 0  [rows][128 B]
  unsigned char* const sP1 = smem_raw + pb_bytes;         // patch buffer 1
  bf16_t* const sC = reinterpret_cast<bf16_t*>(smem_raw + 2 * pb_bytes);   // [256][64]
  int* const s_pout = reinterpret_cast<int*>(smem_raw + 2 * pb_bytes + SC_BYTES);  // [4][256]
  // patch row (input pixel - first input pixel of the tile) of every tile row, < NP256 <= 65535
  unsigned short* const s_prow = reinterpret_cast<unsigned short*>(s_pout + TAB_ROWS);
  float* const s_red = reinterpret_cast<float*>(sC);      // [4 wm][2][64], after the last store

  // (NW / BM / NWM / SC_BYTES / TAB_ROWS: see the top of the kernel)
  constexpr int NTH = NW * 64;
  constexpr int NCO = 1;                        // 32-wide cout fragments per wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, g5 = lane >> 5;
  const uint32_t g5x = (uint32_t)g5 << 4;
  typedef const bf16x8 __attribute__((address_space(3))) * lds_frag_ptr;
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_raw);
  const int M = g.N * g.MY * g.MX;
  const int in_pixels = g.N * g.in_Hp * g.in_Wp;

  // contiguous tile range of this workgroup; workgroups of one XCD own neighbouring ranges
  const int G = gridDim.x;
  const int wl = xcd_tile_index(blockIdx.x, G);
  const int t0 = (int)(((long)wl * num_tiles) / G), t1 = (int)(((long)(wl + 1) * num_tiles) / G);
  if (t0 >= t1) return;

  const int v_tapoff = g.tap_off[lane & (IIC_MAX_TAPS - 1)];
  const int d_y = BM / g.MX, d_x = BM - d_y * g.MX;

  // walkers: `wr` = this thread's table row (row tid & 255 of the next tile to tabulate),
  // `w0` / `wl255` = first / last row of that tile (uniform): p_lo and the span the tile needs
  P64Walk wr, w0, w255;
  p64_walk_init(wr, g, t0 * BM + (tid & (BM - 1)));
  p64_walk_init(w0, g, t0 * BM);
  p64_walk_init(w255, g, t0 * BM + BM - 1);
  int plo_q[3], nblk_q[3];      // [0] = tile being tabulated next - 2 ... rotating queue
  auto tabulate = [&](int t) {  // writes table t (the tile all three walkers point at), advances
    int pin, pout, p0, p255, dummy;
    p64_walk_pixels(w0, g, p0, dummy);
    p64_walk_pixels(w255, g, p255, dummy);
    p0 = __builtin_amdgcn_readfirstlane(p0);
    p255 = __builtin_amdgcn_readfirstlane(p255);
    if (tid < BM) {
      p64_walk_pixels(wr, g, pin, pout);
      s_pout[(t & (P64_NTAB - 1)) * BM + tid] = pout;
      s_prow[(t & (P64_NTAB - 1)) * BM + tid] = (unsigned short)(pin - p0);
    }
    p64_walk_advance(wr, g, d_y, d_x);
    p64_walk_advance(w0, g, d_y, d_x);
    p64_walk_advance(w255, g, d_y, d_x);
    plo_q[0] = plo_q[1];
    nblk_q[0] = nblk_q[1];
    plo_q[1] = plo_q[2];
    nblk_q[1] = nblk_q[2];
    plo_q[2] = p0;
    // 1-KB blocks covering the rows this tile reads: (p255 + max tap offset - p0 + 1) x 128 B
    nblk_q[2] = ((p255 + max_tap_off - p0 + 1) * 128 + 1023) >> 10;
  };
  // LDS-DMA of a patch: piece q -> LDS byte q*16 (row q>>3, physical slot q&7); the source is
  // the logical slot (q&7) ^ ((row>>1)&7) of pixel plo + row.
  auto dma_issue = [&](unsigned char* dst, int plo, int nblk) {
    for (int blk = wave; blk < nblk; blk += NW) {         // 1-KB blocks, wave-uniform
      const int q = blk * 64 + lane;
      const int r = q >> 3;
      const int ls = (q & 7) ^ ((r >> 1) & 7);
      int p = plo + r;
      p = p < in_pixels ? p : in_pixels - 1;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(in + ((long)p * 64 + ls * 8)),
          (__attribute__((address_space(3))) void*)(dst + blk * 1024), 16, 0, 0);
    }
  };

  // ---- FORM 1 (BK): the same tables, queue and DMA with the bookkeeping off the tile's serial path -----------------
  //   * waves 0-3 walk one table row per thread (P64Row: adds and selects); the tile's first / last row walk in
  //     scalar registers (every input is workgroup-uniform), so waves 4-7 spend no VALU on tables at all.  (The
  //     table holds pin - p0, so p0 has to be known before the row is written: it cannot be read back from it.)
  //   * a 1-KB DMA block is 8 whole patch rows and a wave's blocks are 8 apart, so the lane's source offset
  //     (row lane >> 3, logical slot) is the same for every block: scalar base + one hoisted lane offset, the
  //     per-lane clamp only in the block that reaches the tensor's last pixel.
  P64Step stp;
  P64Row rr, r0, r255;
  int pin_last = 0;
  uint32_t lane_src = 0;
  if (BK) {
    const int plane = g.MY * g.MX;
    stp.d_n = BM / plane;
    const int rem = BM - stp.d_n * plane;
    stp.d_y = rem / g.MX;
    stp.d_x = rem - stp.d_y * g.MX;
    stp.MY = g.MY; stp.MX = g.MX;
    stp.pin_step = (stp.d_n * g.in_Hp + stp.d_y * g.sy) * g.in_Wp + stp.d_x * g.sx;
    stp.pin_xw = g.sy * g.in_Wp - g.MX * g.sx;
    stp.pin_yw = (g.in_Hp - g.MY * g.sy) * g.in_Wp;
    stp.pout_step = (stp.d_n * g.out_Hp + stp.d_y * g.ty) * g.out_Wp + stp.d_x * g.tx;
    stp.pout_xw = g.ty * g.out_Wp - g.MX * g.tx;
    stp.pout_yw = (g.out_Hp - g.MY * g.ty) * g.out_Wp;
    pin_last = ((g.N - 1) * g.in_Hp + (g.MY - 1) * g.sy + g.oy) * g.in_Wp + (g.MX - 1) * g.sx + g.ox;
    p64_row_init(rr, g, t0 * BM + (tid & (BM - 1)));
    p64_row_init(r0, g, t0 * BM);
    p64_row_init(r255, g, t0 * BM + BM - 1);
    lane_src = (uint32_t)(lane >> 3) * 128u + (uint32_t)(((lane & 7) ^ (lane >> 4) ^ ((wave & 1) << 2)) << 4);
  }
  auto tabulate1 = [&](int t) {
    const int p0 = r0.n < g.N ? r0.pin : pin_last;
    const int p255 = r255.n < g.N ? r255.pin : pin_last;
    if (wave < BM / 64) {
      const bool valid = rr.n < g.N;
      s_pout[(t & (P64_NTAB - 1)) * BM + tid] = valid ? rr.pout : -1;
      s_prow[(t & (P64_NTAB - 1)) * BM + tid] = (unsigned short)((valid ? rr.pin : pin_last) - p0);
      p64_row_advance(rr, stp);
    }
    p64_row_advance(r0, stp);
    p64_row_advance(r255, stp);
    plo_q[0] = plo_q[1];
    nblk_q[0] = nblk_q[1];
    plo_q[1] = plo_q[2];
    nblk_q[1] = nblk_q[2];
    plo_q[2] = p0;
    nblk_q[2] = ((p255 + max_tap_off - p0 + 1) * 128 + 1023) >> 10;
  };
  auto dma_issue1 = [&](uint32_t dst, int plo, int nblk) {      // dst: LDS byte address of the patch buffer
    const unsigned char* const ing = reinterpret_cast<const unsigned char*>(in);
    for (int blk = wave; blk < nblk; blk += NW) {         // 1-KB blocks = 8 patch rows, wave-uniform
      const int rb = plo + blk * 8;
      const unsigned char* src = ing + (long)rb * 128;
      uint32_t vo = lane_src;
      if (rb + 7 >= in_pixels) {                          // (uniform) rows past the tensor repeat its last pixel
        const int rc = rb < in_pixels ? rb : in_pixels - 1;
        int p = rb + (lane >> 3);
        p = p < in_pixels ? p : in_pixels - 1;
        src = ing + (long)rc * 128;
        vo = (uint32_t)(p - rc) * 128u + (lane_src & 127u);
      }
      p64_dma16s(vo, src, dst + (uint32_t)blk * 1024u);
    }
  };
  int R0[2];                     // BK: patch rows of this lane's two 32-row groups, read one tile ahead

  // ---- prologue: tables of the first two tiles, first patch in flight, resident weights -------
  if (BK) {
    tabulate1(t0);
    tabulate1(t0 + 1);
    __syncthreads();
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) R0[ms] = s_prow[(t0 & (P64_NTAB - 1)) * BM + wm * 64 + ms * 32 + l31];
    dma_issue1(lds_base, plo_q[1], nblk_q[1]);
  } else {
    tabulate(t0);
    tabulate(t0 + 1);
    // queue now: [1] = tile t0, [2] = tile t0 + 1
    dma_issue(sP0, plo_q[1], nblk_q[1]);
  }
  u32x4 Bw[P64_NT][NCO][4];
#pragma unroll
  for (int tap = 0; tap < P64_NT; ++tap)
#pragma unroll
    for (int c = 0; c < NCO; ++c) {
      const unsigned char* p = wfrag + ((long)g.tap_w[tap] * 2 + wn + c) * 4096 + lane * 16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) Bw[tap][c][ks] = *reinterpret_cast<const u32x4*>(p + ks * 1024);
    }
  f32x2 st_s[NCO], st_ss[NCO];                   // BN statistics of column (wn + c)*32 + l31
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    st_s[c] = f32x2{0.f, 0.f};
    st_ss[c] = f32x2{0.f, 0.f};
  }
  TileRed tr;
  if (RED) tile_red_zero(tr);

  // BK: what iteration t touches besides its own patch and sC, and why that is safe (A, B = the two barriers below;
  // every wave waits lgkmcnt(0) in front of B, so all LDS reads and table writes of an iteration are done at its B):
  //   * table slot (t + 2) & 3 is WRITTEN under tap 6, after A of t.  Its last readers: the patch rows of tile t - 2
  //     (read after B of t - 3) and s_pout of tile t - 2, read by the stores of iteration t - 1 -- done before B of t - 1.
  //   * the patch rows of tile t + 1 are READ after B of t; they were written under tap 6 of t - 1, before B of t - 1
  //     (tile t0 + 1: in the prologue, in front of its barrier).
  //   * patch buffer (t + 1) & 1 is WRITTEN by the DMA issued behind tap 0's reads, after A of t; its last readers are
  //     the K loop of t - 1, done before B of t - 1.  The queue is rotated after the issue, as in the first form.
  if (PROF) t_loop = __builtin_readcyclecounter();
  for (int t = t0; t < t1; ++t) {
    const int par = (t - t0) & 1;
    unsigned char* const sP = par ? sP1 : sP0;
    if (PROF) t_a = __builtin_readcyclecounter();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of patch t has landed
    __syncthreads();                                    // A: patch t + tile t-1 in sC are complete
    if (PROF) { t_b = __builtin_readcyclecounter(); ph[0] += t_b - t_a; t_a = t_b; }
    // a plain store (no residual / previous contents / fused reduction: every forward launch) is spread
    // over the taps of the K loop below instead: issued in one go, 32 KB of stores per workgroup back up in
    // the CU's memory pipeline at the speed HBM drains them, with the matrix pipe idle meanwhile (measured:
    // compute-only 108 us + stores 34 us + patch reads 22 us = the full 170 us, i.e. no overlap)
    const bool spread = RED == 0 && !res_grad && !res_act && !accumulate;
    if (t > t0 && !(ABL & 2) && !spread)
      igemm_store_tile<P64_BN, BM, NTH, 0, RED, (RED ? 1 : 4)>(sC, s_pout + ((t - 1) & (P64_NTAB - 1)) * BM,
                                                            out, res_grad, res_act, accumulate, P64_BN, 0, tid,
                                                            red_y, red_coef, red_y2, &tr);
    if (PROF) { t_b = __builtin_readcyclecounter(); ph[1] += t_b - t_a; t_a = t_b; }
    // queue: [2] = tile t + 1 (tabulated one iteration ago)
    if (!BK) {
      if (t + 1 < t1 && !(ABL & 1)) dma_issue(par ? sP0 : sP1, plo_q[2], nblk_q[2]);
      tabulate(t + 2);
    }
    if (PROF) { t_b = __builtin_readcyclecounter(); ph[2] += t_b - t_a; t_a = t_b; }
    // ---- tile t: 9 taps x 4 k-steps x (2 A reads, 2 MFMAs) --------------------------------
    if (!BK) {
#pragma unroll
      for (int ms = 0; ms < 2; ++ms)
        R0[ms] = s_prow[(t & (P64_NTAB - 1)) * BM + wm * 64 + ms * 32 + l31];
    }
    // FORM 1: the buffer's LDS address joins the tap offset on the scalar side.  A buffer starts k KB = 8 k rows into
    // LDS (this kernel has no static LDS: smem_raw is 1-KB aligned, and pb_bytes is whole KB), which moves the row's
    // swizzle key (R >> 1) & 7 by 4 k: the k-step terms undo that.
    const uint32_t pbase = lds_base + (par ? (uint32_t)pb_bytes : 0u);
    const int prow = (int)(pbase >> 7);
    const uint32_t kfix = (pbase >> 4) & 0x40u;
    f32x16 acc[2][NCO];
    constexpr int NTAPS = (ABL & 4) ? 1 : P64_NT;
    auto load_a = [&](int tap, bf16x8 (&a)[2][4]) {
      const int toff = __builtin_amdgcn_readlane(v_tapoff, tap);
      if (FORM) {
        // byte ((R << 7) | ((R << 3) & 0x70)) ^ (g5 << 4) ^ (ks << 5): slot ((ks << 1) | g5) ^ key, key << 4 = (R << 3) & 0x70
        const int toffp = toff + prow;
#pragma unroll
        for (int ms = 0; ms < 2; ++ms) {
          uint32_t tt = (uint32_t)(R0[ms] + toffp) << 3;
          asm volatile("" : "+v"(tt));                   // (keeps the compiler from splitting the sum again)
          uint32_t u = (tt << 4) | (tt & 0x70u);
          asm volatile("" : "+v"(u));
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
            a[ms][ks] = *reinterpret_cast<const lds_frag_ptr>((uintptr_t)(u ^ g5x ^ ((uint32_t)(ks << 5) ^ kfix)));
        }
        return;
      }
#pragma unroll
      for (int ms = 0; ms < 2; ++ms) {
        const int R = R0[ms] + toff;
        const int key = (R >> 1) & 7;
        const int base = R * 128 + (((g5 ^ key) & 1) << 4);
        const int kk = (key >> 1) << 5;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          a[ms][ks] = *reinterpret_cast<const bf16x8*>(sP + base + ((ks << 5) ^ kk));
      }
    };
#pragma unroll
    for (int tap = 0; tap < NTAPS; ++tap) {
      bf16x8 a[2][4];
      load_a(tap, a);
      if (BK) {
        // behind the first tap's reads: the DMA of tile t + 1 (queue [2]); under a late tap's MFMAs: table t + 2
        if (tap == 0 && t + 1 < t1 && !(ABL & 1)) dma_issue1(lds_base + (par ? 0u : (uint32_t)pb_bytes), plo_q[2], nblk_q[2]);
        if (tap == (NTAPS > 6 ? 6 : NTAPS - 1)) tabulate1(t + 2);
      }
      if (spread && t > t0 && !(ABL & 2)) {
        constexpr int SIT = BM * 8 / NTH;           // 16-byte pieces per thread and tile (4 | 8)
        constexpr int PER = (SIT + P64_NT - 2) / (P64_NT - 1);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
          const int it = (tap - 1) * PER + q;
          if (tap >= 1 && it < SIT) {
            const int idx = tid + it * NTH;
            const int row = idx >> 3, ch = idx & 7;
            const int po = s_pout[((t - 1) & (P64_NTAB - 1)) * BM + row];
            if (po >= 0)
              *reinterpret_cast<uint4*>(out + (long)po * P64_BN + ch * 8) =
                  *reinterpret_cast<const uint4*>(sC + row * P64_CLD + ch * 8);
          }
        }
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int c = 0; c < NCO; ++c) {
          const bf16x8 b = __builtin_bit_cast(bf16x8, Bw[tap][c][ks]);
          if (tap == 0 && ks == 0) {          // first MFMA of the tile: C operand = 0 (no zero-fill)
            const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[0][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][ks], b, z, 0, 0, 0);
            acc[1][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][ks], b, z, 0, 0, 0);
          } else {
            acc[0][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][ks], b, acc[0][c], 0, 0, 0);
            acc[1][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][ks], b, acc[1][c], 0, 0, 0);
          }
        }
    }
    if (stats) {
      if ((t + 1) * BM > M) {           // last tile: rows past the end do not count
#pragma unroll
        for (int ms = 0; ms < 2; ++ms)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (t * BM + wm * 64 + ms * 32 + mfma32_row(r, lane) >= M) {
#pragma unroll
              for (int c = 0; c < NCO; ++c) acc[ms][c][r] = 0.f;
            }
      }
#pragma unroll
      for (int c = 0; c < NCO; ++c)
#pragma unroll
        for (int ms = 0; ms < 2; ++ms)
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const f32x2 v = {acc[ms][c][r], acc[ms][c][r + 1]};
            st_s[c] += v;
            st_ss[c] += v * v;
          }
    }
    if (PROF) { t_b = __builtin_readcyclecounter(); ph[3] += t_b - t_a; t_a = t_b; }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // B: the stores of tile t-1 have read sC
    if (PROF) { t_b = __builtin_readcyclecounter(); ph[4] += t_b - t_a; t_a = t_b; }
#pragma unroll
    for (int c = 0; c < NCO; ++c)
#pragma unroll
      for (int ms = 0; ms < 2; ++ms)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          sC[(wm * 64 + ms * 32 + mfma32_row(r, lane)) * P64_CLD + (wn + c) * 32 + l31] = f32_to_bf16(acc[ms][c][r]);
    if (BK && t + 1 < t1) {
#pragma unroll
      for (int ms = 0; ms < 2; ++ms) R0[ms] = s_prow[((t + 1) & (P64_NTAB - 1)) * BM + wm * 64 + ms * 32 + l31];
    }
    if (PROF) { t_b = __builtin_readcyclecounter(); ph[5] += t_b - t_a; }
  }
  if (PROF && prof && tid == 0) {
    unsigned long long* q = prof + (long)blockIdx.x * 8;
#pragma unroll
    for (int i = 0; i < 6; ++i) q[i] = ph[i];
    q[6] = (unsigned long long)(t1 - t0);
    q[7] = __builtin_readcyclecounter() - t_loop;
  }

  // ---- drain: last tile's rows, then the statistics -------------------------------------------
  __syncthreads();
  if (!(ABL & 2))
    igemm_store_tile<P64_BN, BM, NTH, 0, RED, (RED ? 1 : 4)>(sC, s_pout + ((t1 - 1) & (P64_NTAB - 1)) * BM, out,
                                                          res_grad, res_act, accumulate, P64_BN, 0, tid,
                                                          red_y, red_coef, red_y2, &tr);
  if (RED)
    igemm_red_finish<P64_BN, NTH, RED>(tr, reinterpret_cast<float*>(sC), red_stats, red_stats2, P64_BN,
                                               0, tid);
  if (stats) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCO; ++c) {
      float s1 = st_s[c][0] + st_s[c][1], s2 = st_ss[c][0] + st_ss[c][1];
      s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 32, 64);
      if (lane < 32) {
        s_red[(wm * 2 + 0) * P64_BN + (wn + c) * 32 + lane] = s1;
        s_red[(wm * 2 + 1) * P64_BN + (wn + c) * 32 + lane] = s2;
      }
    }
    __syncthreads();
    if (tid < P64_BN) {
      float a0 = 0.f, a1 = 0.f;
#pragma unroll
      for (int q = 0; q < NWM; ++q) {
        a0 += s_red[(q * 2 + 0) * P64_BN + tid];
        a1 += s_red[(q * 2 + 1) * P64_BN + tid];
      }
      const int stripe = blockIdx.x % IIC_STAT_STRIPES;
      iic_stat_add(stats, stripe, P64_BN, tid, 0, a0);
      iic_stat_add(stats, stripe, P64_BN, tid, 1, a1);
    }
  }
}

#ifdef IIC_DEBUG_HOOKS
static unsigned long long* g_p64_prof = nullptr;   // ablate 8: per-workgroup phase cycle sums go here
IIC_HOOK void iic_debug_p64_prof(void* buf) { g_p64_prof = (unsigned long long*)buf; }
#else
static constexpr unsigned long long* g_p64_prof = nullptr;
#endif
IIC_SWITCH(g_p64_grid, 0, iic_debug_p64_grid)       // tests: force a small persistent grid (many tiles per workgroup)
// 1: closed-form patch addresses, bookkeeping off the tile's serial path (template FORM); 0: the first form of the
// tile loop, instantiated in the instrumented library only (A/B, tests/test_gpu_p64_forms.py)
IIC_SWITCH(g_p64_form, 1, iic_debug_p64_form)

static long p64_pb_bytes(const iic_conv_geom* g, int bm = P64_BM) {
  return (((long)(bm == 128 ? g->NP : g->NP256) * 128) + 1023) & ~1023L;
}
// Half-height tiles with two workgroups per CU (BM = 128) would let one
// workgroup's serial phases (40 % of a tile's cycles with the matrix pipe idle) run under the other's K loop, but do not fit: at layer1 of ClusterNet5g a 128-row
// tile still spans 340 patch rows (42.5 KB; 474 rows at 256), so two double-buffered workgroups need 208 KB.

// this kernel's part of conv_make_plan (conv_igemm_bd.hip)
bool iic_p64_plan(const iic_conv_geom* g, conv_plan* p) {
  if (g->Cin != 64 || g->Cout != 64 || g->ntaps != P64_NT || g->NP256 <= 0 || g->NP256 > 65535) return false;
  if (!igemm_dense_host(g)) return false;       // the row walkers assume the dense row numbering
  const long lds = 2 * p64_pb_bytes(g) + P64_SC_BYTES(P64_BM) + P64_TAB_BYTES(P64_BM);
  if (lds > IIC_LDS_BYTES) return false;
  const long nt = ((long)g->N * g->MY * g->MX + P64_BM - 1) / P64_BM;
  const int ncu = g_p64_grid > 0 ? g_p64_grid : iic_num_cus();
  p->kernel = CONV_P64;
  p->mtiles = (int)nt;
  p->grid = nt < ncu ? (int)nt : ncu;
  p->lds_a = (int)p64_pb_bytes(g);
  p->lds = lds;
  return true;
}

int iic_p64_launch(const iic_conv_geom* g, const conv_plan& p, const void* in, const void* wfrag, void* out, float* stats,
                   const void* res_grad, const void* res_act, int accumulate, const void* red_y,
                   const float* red_coef, const void* red_y2, float* red_stats, float* red_stats2,
                   void* stream) {
  const int red = red_y ? (red_y2 ? 2 : 1) : 0;
  const long M = (long)g->N * g->MY * g->MX;
  if (M <= 0) return IIC_ERR_ARG;
  if (M >= (1L << 31) - P64_BM || (long)g->N * g->in_Hp * g->in_Wp >= (1L << 31)) return IIC_ERR_UNSUPPORTED;
  int mto = 0;
  for (int i = 0; i < g->ntaps; ++i) mto = g->tap_off[i] > mto ? g->tap_off[i] : mto;
  int rc = IIC_OK;
#define P64_LAUNCH3(AB_, RD_, FM_)                                                                     \
  rc = iic_launch_lds<conv_igemm_p64_kernel<AB_, RD_, FM_>>(                                           \
      dim3(p.grid), dim3(512), p.lds, (hipStream_t)stream, *g, (const bf16_t*)in,                      \
      (const unsigned char*)wfrag, (bf16_t*)out, stats, (const bf16_t*)res_grad,                       \
      (const bf16_t*)res_act, accumulate, p.mtiles, p.lds_a, mto, (const bf16_t*)red_y, red_coef,      \
      (const bf16_t*)red_y2, red_stats, red_stats2, g_p64_prof)
#ifdef IIC_DEBUG_HOOKS
#define P64_LAUNCH2(AB_, RD_)                                                                          \
  do {                                                                                                 \
    if (g_p64_form) P64_LAUNCH3(AB_, RD_, true);                                                       \
    else P64_LAUNCH3(AB_, RD_, false);                                                                 \
  } while (0)
#else
#define P64_LAUNCH2(AB_, RD_) P64_LAUNCH3(AB_, RD_, true)
#endif
#define P64_LAUNCH(AB_) P64_LAUNCH2(AB_, 0)
  if (red == 1) P64_LAUNCH2(0, 1);
  else if (red == 2) P64_LAUNCH2(0, 2);
  else {
    switch (iic_debug_get_ablate()) {
#ifdef IIC_BD_ABLATIONS
      // timing-ablation / phase-profile instantiations (tools/p64_phases.py): `make -C iic_amd/csrc ABL=1` only
      case 1: P64_LAUNCH(1); break;
      case 2: P64_LAUNCH(2); break;
      case 3: P64_LAUNCH(3); break;
      case 4: P64_LAUNCH(4); break;
      case 7: P64_LAUNCH(7); break;
      case 8: P64_LAUNCH(8); break;
#endif
      default: P64_LAUNCH(0); break;
    }
  }
  return rc ? rc : iic_launch_status();
}
