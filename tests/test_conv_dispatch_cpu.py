"""Which weights-direct conv kernel, and which of its forms, every conv layer of the five BASELINE configs gets at the
bench batch: the launch plan (csrc/conv_plan.h, conv_make_plan in conv_igemm_bd.hip) read through iic_debug_conv_plan of
the instrumented library -- host code, no device needed -- against a literal table recorded from the dispatch as it stood
before the plan existed.  One wrong byte in an LDS budget must not move a layer to another kernel, tile shape or
occupancy unnoticed."""
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
