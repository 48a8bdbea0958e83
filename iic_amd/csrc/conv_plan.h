// The launch plan of the weights-direct convolutions (conv_igemm_bd.hip, conv_igemm_pw.hip, conv_igemm_p64.hip): which
// kernel and which of its forms a geometry gets, decided ONCE by conv_make_plan (conv_igemm_bd.hip) under the switches
// in force.  iic_conv_igemm_frag_supported / _red_supported, the launch and the iic_debug_* readers all take their
// answer from it; the launch only turns its fields into template arguments.  tests/test_conv_dispatch_cpu.py pins the
// plans of the BASELINE layers (iic_debug_conv_plan, instrumented library).
//
// The weight gradient (conv_wgrad.hip, conv_wgrad_dma.hip) has the same arrangement: wgrad_make_plan (conv_wgrad.hip)
// fills a wgrad_plan once per launch, iic_conv_wgrad and iic_wgrad_dma_launch launch from it, iic_debug_wgrad_plan
// reports it, and the same test file pins it for every BASELINE layer.
#pragma once
#include "common.h"
#include "../../include/iic_hip.h"

// Block tiling of conv_igemm_bd_kernel (see conv_igemm_bd.hip): a 256-row tile as a bw x bh block of output pixels
struct bd_blk {
  int bw, bh, nbx, nby;      // bw == 0: row-major tiles
  int PW, npix, mul;         // patch width, patch pixels, ceil(65536 / PW) (patch row / PW by multiply-shift)
};

enum { CONV_NONE = 0, CONV_P64 = 1, CONV_PW = 2, CONV_BD = 3 };    // NONE: the first-generation kernel (conv_igemm.hip)

struct conv_plan {
  int kernel;         // CONV_*
  int ms, wn;         // BD: 32-row sub-tiles per wave, 64-cout column groups (PW: 4, 2 -- its 256 x 128 tile)
  bool gather, pad;   // BD: 1-tap gather form; BD / PW: 144-byte-pitch patch
  bd_blk blk;         // BD: block tiles (bw == 0: row-major)
  int mtiles, grid;   // row tiles, workgroups
  int lds_a;          // patch bytes (BD: or the epilogue tile, if larger; P64: one of its two patch buffers)
  long lds;           // dynamic LDS of the launch
  bool red_ok;        // may this launch carry the fused reduction
};

// Each persistent kernel fills the plan of a geometry it takes (under its own switches) and launches from it
bool iic_p64_plan(const iic_conv_geom* g, conv_plan* p);
bool iic_pw_plan(const iic_conv_geom* g, conv_plan* p);
int iic_p64_launch(const iic_conv_geom* g, const conv_plan& p, const void* in, const void* wfrag, void* out, float* stats,
                   const void* res_grad, const void* res_act, int accumulate, const void* red_y, const float* red_coef,
                   const void* red_y2, float* red_stats, float* red_stats2, void* stream);
int iic_pw_launch(const iic_conv_geom* g, const conv_plan& p, const void* in, const void* wfrag, void* out, float* stats,
                  const void* res_grad, const void* res_act, int accumulate, const void* red_y, const float* red_coef,
                  const void* red_y2, float* red_stats, float* red_stats2, void* stream);

// ---- weight gradient --------------------------------------------------------------------------------------------------
// Block tiling of conv_wgrad_b2d_kernel (see conv_wgrad_dma.hip): a 128-row K-tile as a bw x bh block of output pixels
struct wdb_args {
  int bw, bh, nbx, nby;           // block size, blocks per image row / column
  int PW, NPR, drow;              // patch width, patch pixels, tap-row distance in image rows
  int plane_bytes, num_tiles;
};

// in the order of preference, last first; NONE: no weight-gradient kernel takes the geometry
enum { WGRAD_NONE = 0, WGRAD_REG = 1, WGRAD_DMA = 2, WGRAD_PL = 3, WGRAD_PL2 = 4, WGRAD_B2D = 5 };

struct wgrad_plan {
  int kernel;         // WGRAD_*: conv_wgrad_kernel (register-staged), conv_wgrad_dma_kernel (first-generation DMA),
                      // conv_wgrad_pl_kernel, conv_wgrad_pl2_kernel (planar patch), conv_wgrad_b2d_kernel (block-tiled)
  bool use_tr;        // REG: transposing LDS reads (false: the scalar-gather cross-check)
  bool asm_reads;     // PL: inline-asm transposing reads
  bool gather;        // REG: 1-tap gather form
  int cot;            // couts of a workgroup's tile, 64 | 128 (64 cins)
  int bmk, nbuf;      // pixels of a K-tile, depth of the ring of K-tile buffers
  int ntab;           // DMA / PL / PL2: depth of the ring of row tables
  int txs;            // PL / PL2 / B2D: x step between the taps of a tap row, in input pixels (1 | 2; 0: irregular taps)
  int band, bstride;  // PL / PL2: LDS rows per band of the banded patch (0: contiguous patch), tap-row distance
  int mto;            // DMA / PL / PL2: largest tap offset
  int np;             // LDS rows of a K-tile's patch (PL / PL2: per plane)
  int plane;          // bytes of a patch plane (DMA: of the patch)
  int lx;             // REG: bytes of the patch
  int kt;             // K-tiles (B2D: blocks) of the launch
  int gx, gz;         // grid x (cout tiles x cin tiles) and z (REG: tap batches); y = the K-splits the caller asks for
  int nsplit;         // ... by default this many (iic_conv_wgrad_nsplit)
  int threads;
  long lds;           // dynamic LDS of the launch
  wdb_args blk;       // B2D
};

static inline int wgrad_cot(const iic_conv_geom* g) { return (g->Cout % 128 == 0) ? 128 : 64; }

// conv_wgrad_dma.hip: the DMA-fed kernels fill the plan of a geometry they take (p->cot and p->gx set by the caller) and
// launch from it
bool iic_wgrad_dma_plan(const iic_conv_geom* g, wgrad_plan* p);
int iic_wgrad_dma_launch(const iic_conv_geom* g, const wgrad_plan& p, const void* x, const void* dy, float* partials,
                         int nsplit, void* stream);
