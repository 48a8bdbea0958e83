// The launch plan of the weights-direct convolutions (conv_igemm_bd.hip, conv_igemm_pw.hip, conv_igemm_p64.hip): which
// kernel and which of its forms a geometry gets, decided ONCE by conv_make_plan (conv_igemm_bd.hip) under the switches
// in force.  iic_conv_igemm_frag_supported / _red_supported, the launch and the iic_debug_* readers all take their
// answer from it; the launch only turns its fields into template arguments.  tests/test_conv_dispatch_cpu.py pins the
// plans of the BASELINE layers (iic_debug_conv_plan, instrumented library).
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
