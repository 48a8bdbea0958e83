"""Which weights-direct conv kernel, and which of its forms, every conv layer of the five BASELINE configs gets at the
bench batch: the launch plan (csrc/conv_plan.h, conv_make_plan in conv_igemm_bd.hip) read through iic_debug_conv_plan of
the instrumented library -- host code, no device needed -- against a literal table recorded from the dispatch as it stood
before the plan existed.  One wrong byte in an LDS budget must not move a layer to another kernel, tile shape or
occupancy unnoticed.  The weight gradient of the same layers likewise: wgrad_plan (wgrad_make_plan in conv_wgrad.hip)
through iic_debug_wgrad_plan, further down."""
import ctypes
import os

import pytest

FIELDS = ("kernel", "ms", "wn", "gather", "pad", "bw", "bh", "mtiles", "grid", "lds_a", "lds", "red_ok")
NONE, P64, PW, BD = 0, 1, 2, 3
LDS_PER_CU = 160 * 1024

# layer: (cin, cout, K, stride, conv padding, dilation, N, H, PT border), then per geometry (forward, then every
# backward-data parity class) the expected (kernel, ms, wn, pad, block-tiled, workgroups per CU that the LDS allows)
_5G = lambda cin, cout, K, s, p, H: (cin, cout, K, s, p, 1, 660, H, 1)
_6C = lambda cin, cout, H: (cin, cout, 5, 1, 2, 1, 700, H, 2)
_POTSDAM = lambda cin, cout, H, d: (cin, cout, 3, 1, 1, d, 75, H, 3)
_COCO = lambda cin, cout, H, d: (cin, cout, 3, 1, 1, d, 120, H, 3)
BD4 = (BD, 4, 2, 0, 0, 2)         # 256 x 128 row-major tiles, swizzled patch (or the 1-tap gather), two per CU
BD4_PAD = (BD, 4, 2, 1, 0, 2)
BD4_BLK = (BD, 4, 2, 0, 1, 2)
BD4_BIG = (BD, 4, 2, 0, 0, 1)     # the stride-2 forwards: a patch that has the CU to itself
PW_PAD, PW_SWZ = (PW, 4, 2, 1, 0, 2), (PW, 4, 2, 0, 0, 2)
P64_ = (P64, 0, 0, 0, 0, 1)
NONE_ = (NONE, 0, 0, 0, 0, None)
TABLE = [
    ("5g layer1 3x3 64->64", _5G(64, 64, 3, 1, 1, 49), [P64_, P64_]),
    ("5g layer2.0 3x3 s2 64->128", _5G(64, 128, 3, 2, 1, 49),
     [BD4_BIG, NONE_, (BD, 2, 1, 0, 0, 3), (BD, 2, 1, 0, 0, 2), (BD, 2, 1, 0, 0, 2)]),
    ("5g layer2.0 1x1 s2 64->128", _5G(64, 128, 1, 2, 0, 49), [BD4, NONE_]),
    ("5g layer2 3x3 128->128", _5G(128, 128, 3, 1, 1, 25), [PW_PAD, PW_PAD]),
    ("5g layer3.0 3x3 s2 128->256", _5G(128, 256, 3, 2, 1, 25), [BD4_BIG, BD4, BD4_PAD, BD4_PAD, BD4_PAD]),
    ("5g layer3.0 1x1 s2 128->256", _5G(128, 256, 1, 2, 0, 25), [BD4, BD4]),
    ("5g layer3 3x3 256->256", _5G(256, 256, 3, 1, 1, 13), [BD4_PAD, BD4_PAD]),
    ("5g layer4.0 3x3 s2 256->512", _5G(256, 512, 3, 2, 1, 13),
     [BD4_BIG, BD4, (BD, 2, 2, 1, 0, 4), (BD, 2, 2, 1, 0, 4), (BD, 2, 2, 1, 0, 3)]),
    ("5g layer4.0 1x1 s2 256->512", _5G(256, 512, 1, 2, 0, 13), [BD4, BD4]),
    ("5g layer4 3x3 512->512", _5G(512, 512, 3, 1, 1, 7), [BD4_PAD, BD4_PAD]),
    # ClusterNet6c (mnist6c and cifar6c share every conv past the first)
    ("6c 5x5 64->128", _6C(64, 128, 12), [BD4_PAD, (BD, 2, 1, 0, 0, 2)]),
    ("6c 5x5 128->256", _6C(128, 256, 6), [(BD, 2, 2, 0, 0, 2), (BD, 2, 2, 0, 0, 2)]),
    ("6c 5x5 256->512", _6C(256, 512, 3), [(BD, 2, 2, 0, 0, 1), (BD, 2, 2, 0, 0, 1)]),
    # SegmentationNet10a
    ("potsdam c2", _POTSDAM(64, 128, 200, 1), [BD4_BLK, (BD, 2, 1, 0, 1, 3)]),
    ("potsdam c3", _POTSDAM(128, 256, 100, 1), [PW_SWZ, PW_SWZ]),
    ("potsdam c4", _POTSDAM(256, 256, 100, 1), [PW_SWZ, PW_SWZ]),
    ("potsdam c5", _POTSDAM(256, 512, 100, 2), [BD4_BLK, BD4_BLK]),
    ("potsdam c6", _POTSDAM(512, 512, 98, 2), [BD4_BLK, BD4_BLK]),
    ("coco c2", _COCO(64, 128, 128, 1), [BD4_BLK, (BD, 2, 1, 0, 1, 3)]),
    ("coco c3", _COCO(128, 256, 64, 1), [PW_PAD, PW_PAD]),
    ("coco c4", _COCO(256, 256, 64, 1), [PW_PAD, PW_PAD]),
    ("coco c5", _COCO(256, 512, 64, 2), [BD4_BLK, BD4]),
    ("coco c6", _COCO(512, 512, 62, 2), [BD4_BLK, BD4_BLK]),
]


@pytest.fixture(scope="module")
def L():
  from iic_amd import _lib
  dbg = os.path.join(os.path.dirname(_lib.LIB_PATH), "libiic_hip_dbg.so")
  assert os.path.exists(dbg), "build it: make -C iic_amd/csrc dbg"
  h = ctypes.CDLL(dbg)            # host-side functions of the instrumented library: no device needed
  for f in ("iic_conv_igemm_frag_supported", "iic_conv_igemm_red_supported", "iic_debug_bd_pitch144_used",
            "iic_debug_pw_grid"):
    getattr(h, f).restype = ctypes.c_int
  h.iic_debug_conv_plan.restype = None
  h.iic_debug_wgrad_plan.restype = None
  return h


def _geoms(layer):
  from iic_amd import geom
  cin, cout, K, s, p, d, N, H, P = layer
  spec = geom.ConvSpec(cin, cout, K, s, p, d)
  return [geom.fwd_geom(spec, N, H, H, P, P)] + geom.bwd_data_geoms(spec, N, H, H, P, P)


def _plan(L, g):
  out = (ctypes.c_int * len(FIELDS))()
  L.iic_debug_conv_plan(ctypes.byref(g), out)
  return dict(zip(FIELDS, out))


def test_dispatch_of_the_baseline_configs(L):
  for name, layer, want in TABLE:
    geoms = _geoms(layer)
    assert len(geoms) == len(want), (name, len(geoms))
    for i, (g, w) in enumerate(zip(geoms, want)):
      p = _plan(L, g)
      got = (p["kernel"], p["ms"], p["wn"], p["pad"], int(p["bw"] > 0), LDS_PER_CU // p["lds"] if p["lds"] else None)
      assert got == w, (name, i, p, w)
      assert p["gather"] == int(p["kernel"] == BD and g.ntaps == 1), (name, i, p)
      # the two ABI predicates and the patch-form hook read the same plan
      assert L.iic_conv_igemm_frag_supported(ctypes.byref(g)) == int(p["kernel"] != NONE), (name, i, p)
      assert L.iic_conv_igemm_red_supported(ctypes.byref(g)) == p["red_ok"], (name, i, p)
      used = (2 if p["kernel"] == PW else 1) if p["pad"] else 0
      assert L.iic_debug_bd_pitch144_used(ctypes.byref(g)) == used, (name, i, p)
      if p["kernel"] != NONE:
        assert 0 < p["lds_a"] <= p["lds"] <= LDS_PER_CU and p["mtiles"] > 0 and p["grid"] > 0, (name, i, p)


# ---- weight gradient: wgrad_plan (csrc/conv_plan.h, wgrad_make_plan in conv_wgrad.hip) through iic_debug_wgrad_plan ----
WFIELDS = ("kernel", "banded", "asm_reads", "gather", "cot", "bmk", "nbuf", "ntab", "txs", "band", "bstride", "mto", "np",
           "plane", "lx", "kt", "gx", "nsplit", "gz", "threads", "lds", "bw", "bh", "nbx", "nby", "PW", "NPR", "drow")
W_NONE, W_REG, W_DMA, W_PL, W_PL2, W_B2D = range(6)   # register-staged, first-generation DMA, planar, pipelined planar, block-tiled
WPINNED = ("kernel", "cot", "bmk", "nbuf", "ntab", "band", "bw", "bh", "gx", "gz", "kt", "lds", "nsplit")
# The forward geometry of every TABLE layer at the bench batch (the weight gradient runs on it), in TABLE's order: the
# WPINNED fields as the dispatch stood before the plan existed -- read from that commit's instrumented library
# (iic_debug_wgrad_config's packed code, iic_conv_wgrad_nsplit) and, for the fields the code did not carry, from that
# commit's launch formulas.  nsplit is also the launch's grid y.
WTABLE = [
    (W_PL2, 64, 128, 2, 8, 0, 0, 0, 1, 1, 12381, 131072, 224),      # 5g layer1
    (W_PL, 128, 64, 2, 8, 0, 0, 0, 1, 1, 6446, 151552, 224),        # 5g layer2.0 3x3 s2: planar, 64-pixel ring
    (W_REG, 128, 128, 1, 0, 0, 0, 0, 1, 1, 3223, 57344, 224),       # 5g layer2.0 1x1 s2: the 1-tap gather
    (W_PL, 128, 128, 2, 8, 0, 0, 0, 2, 1, 3223, 139264, 112),       # 5g layer2
    (W_PL, 128, 64, 2, 8, 0, 0, 0, 4, 1, 1743, 126976, 56),         # 5g layer3.0 3x3 s2
    (W_REG, 128, 128, 1, 0, 0, 0, 0, 4, 1, 872, 57344, 56),         # 5g layer3.0 1x1 s2
    (W_PL, 128, 128, 2, 8, 0, 0, 0, 8, 1, 872, 131072, 28),         # 5g layer3
    (W_PL, 128, 64, 2, 8, 0, 0, 0, 16, 1, 506, 122880, 14),         # 5g layer4.0 3x3 s2
    (W_REG, 128, 128, 1, 0, 0, 0, 0, 16, 1, 253, 57344, 14),        # 5g layer4.0 1x1 s2
    (W_PL, 128, 128, 2, 8, 0, 0, 0, 32, 1, 253, 135168, 7),         # 5g layer4
    (W_REG, 128, 128, 1, 0, 0, 0, 0, 1, 3, 788, 82688, 74),         # 6c 5x5: register-staged, 25 taps in 3 batches
    (W_REG, 128, 128, 1, 0, 0, 0, 0, 4, 3, 197, 98816, 18),
    (W_REG, 128, 128, 1, 0, 0, 0, 0, 16, 3, 50, 147200, 4),
    (W_B2D, 128, 128, 2, 0, 0, 5, 25, 1, 1, 24000, 114688, 224),    # potsdam c2 .. c6
    (W_B2D, 128, 128, 2, 0, 0, 5, 25, 4, 1, 6000, 114688, 56),
    (W_B2D, 128, 128, 2, 0, 0, 5, 25, 8, 1, 6000, 114688, 28),
    (W_B2D, 128, 128, 2, 0, 0, 9, 14, 16, 1, 5775, 126976, 14),
    (W_B2D, 128, 128, 2, 0, 0, 8, 16, 32, 1, 5400, 126976, 7),
    (W_B2D, 128, 128, 2, 0, 0, 8, 16, 1, 1, 15360, 114688, 224),    # coco c2 .. c6
    (W_B2D, 128, 128, 2, 0, 0, 8, 16, 4, 1, 3840, 114688, 56),
    (W_B2D, 128, 128, 2, 0, 0, 8, 16, 8, 1, 3840, 114688, 28),
    (W_B2D, 128, 128, 2, 0, 0, 8, 16, 16, 1, 3840, 126976, 14),
    (W_B2D, 128, 128, 2, 0, 0, 10, 12, 32, 1, 3600, 122880, 7),
]


def _wplan(L, g, use_tr=1):
  out = (ctypes.c_int * len(WFIELDS))()
  L.iic_debug_wgrad_plan(ctypes.byref(g), use_tr, out)
  return dict(zip(WFIELDS, out))


def test_weight_gradient_dispatch_of_the_baseline_configs(L):
  """Every conv layer's weight gradient of the five BASELINE configs runs on the kernel, in the layout, that LAB.md
  R6.8 / R6.12 / R6.13 measured: a few bytes of LDS must not drop a layer back to an older kernel unnoticed
  (SegmentationNet10a c3 / c4 once did, by 64)."""
  assert len(WTABLE) == len(TABLE)
  for (name, layer, _), want in zip(TABLE, WTABLE):
    g = _geoms(layer)[0]
    p = _wplan(L, g)
    assert tuple(p[f] for f in WPINNED) == want, (name, p, want)
    assert L.iic_conv_wgrad_nsplit(ctypes.byref(g)) == p["nsplit"], (name, p)
    assert 0 < p["lds"] <= LDS_PER_CU and p["gx"] > 0 and p["nsplit"] > 0 and p["gz"] > 0 and p["kt"] > 0, (name, p)
    assert p["threads"] == (256 if p["gather"] else 768) and p["gather"] == int(g.ntaps == 1), (name, p)
    assert p["banded"] == int(p["band"] > 0) and p["asm_reads"] == int(p["kernel"] == W_PL), (name, p)
    if layer[2:6] == (3, 1, 1, 1) and layer[6] == 660:
      # the four stride-1 3 x 3 layers of ClusterNet5g: planar, contiguous patch, 128-pixel tiles, 2 buffers, 8 tables
      assert p["kernel"] in (W_PL, W_PL2) and (p["band"], p["bmk"], p["nbuf"], p["ntab"]) == (0, 128, 2, 8), (name, p)
    if layer[6] in (75, 120):
      # SegmentationNet10a: every 3 x 3 layer on the block-tiled kernel, two buffers of 128-row blocks
      assert (p["kernel"], p["bmk"], p["nbuf"]) == (W_B2D, 128, 2) and 0 < p["bw"] * p["bh"] <= 128, (name, p)
      assert p["kt"] == layer[6] * p["nbx"] * p["nby"] and p["NPR"] == p["PW"] * (p["bh"] + 2 * p["drow"]), (name, p)
  out = (ctypes.c_int * len(WFIELDS))()
  L.iic_debug_wgrad_plan(None, 1, out)
  assert list(out) == [0] * len(WFIELDS)


def test_weight_gradient_switches_the_gpu_tests_rely_on(L):
  """iic_debug_enable_wgrad_dma 3 = 64-pixel K-tiles, 0 = the register-staged kernel; iic_debug_wgrad_planar 0 = the first
  generation (tests/test_gpu_kernels.py reaches those kernels through them) -- on a ClusterNet5g layer and on a layer
  with padded row numbering (200 x 200, 64 couts: the block-tiled kernel, which no switch but 0 takes a layer from,
  wants 128).  Expected (kernel, bmk, nbuf, ntab, kt, lds) recorded like WTABLE."""
  l1 = _geoms(_5G(64, 64, 3, 1, 1, 49))[0]
  big = _geoms((64, 64, 3, 1, 1, 1, 2, 200, 3))[0]
  assert big.MP > big.MY * big.MX and big.MP % 256 == 0
  cases = [   # geometry, enable_wgrad_dma, wgrad_planar, expected
      (l1, 1, 5, (W_PL2, 128, 2, 8, 12381, 131072)),
      (l1, 3, 5, (W_PL2, 64, 3, 8, 24761, 139264)),
      (l1, 0, 5, (W_REG, 128, 1, 0, 12381, 69440)),
      (l1, 1, 0, (W_DMA, 128, 2, 8, 12381, 127040)),
      (l1, 3, 0, (W_DMA, 64, 3, 8, 24761, 135232)),
      (big, 1, 5, (W_REG, 128, 1, 0, 628, 99392)),         # by default the register-staged kernel keeps this one
      (big, 3, 5, (W_PL2, 64, 2, 8, 1256, 147456)),
      (big, 0, 5, (W_REG, 128, 1, 0, 628, 99392)),
      (big, 1, 0, (W_REG, 128, 1, 0, 628, 99392)),
      (big, 3, 0, (W_DMA, 64, 2, 8, 1256, 144448)),
  ]
  try:
    for g, dma, planar, want in cases:
      L.iic_debug_enable_wgrad_dma(dma)
      L.iic_debug_wgrad_planar(planar)
      p = _wplan(L, g)
      assert tuple(p[f] for f in ("kernel", "bmk", "nbuf", "ntab", "kt", "lds")) == want, (dma, planar, p, want)
      assert p["nsplit"] == 224 == L.iic_conv_wgrad_nsplit(ctypes.byref(g)), (dma, planar, p)   # the switches leave it alone
      # the scalar-gather cross-check (use_tr = 0) exists in the register-staged kernel only
      q = _wplan(L, g, 0)
      assert (q["kernel"], q["bmk"], q["nbuf"], q["kt"]) == (W_REG, 128, 1, (g.N * max(g.MP, g.MY * g.MX) + 127) // 128), q
  finally:
    L.iic_debug_enable_wgrad_dma(1)
    L.iic_debug_wgrad_planar(5)


def test_persistent_kernel_grid_of_shapes_it_does_not_run(L):
  """iic_debug_pw_grid: 0 for a geometry conv_igemm_pw_kernel does not run (it used to divide by Cout / 128 == 0), and
  the plan of such a geometry is another kernel's or none."""
  l1 = _geoms(_5G(64, 64, 3, 1, 1, 49))[0]                    # 64 -> 64: the persistent 64 -> 64 kernel
  bwd = _geoms(_5G(64, 128, 3, 2, 1, 49))                     # backward-data of 64 -> 128: 64 couts
  for g, kernel in ((l1, P64), (bwd[1], NONE), (bwd[2], BD)):
    assert g.Cout == 64
    assert L.iic_debug_pw_grid(ctypes.byref(g)) == 0
    assert _plan(L, g)["kernel"] == kernel
  assert L.iic_debug_pw_grid(None) == 0
  out = (ctypes.c_int * len(FIELDS))()
  L.iic_debug_conv_plan(None, out)
  assert list(out) == [0] * len(FIELDS)
  # a shape it does run: two workgroups per CU, 256 CUs where there is no device to ask
  g = _geoms(_5G(128, 128, 3, 1, 1, 25))[0]
  assert L.iic_debug_pw_grid(ctypes.byref(g)) == _plan(L, g)["grid"] > 0
