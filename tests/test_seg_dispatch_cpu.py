"""Which kernel, in which form, on which grid and with how much LDS the segmentation loss gives the shapes the project
runs: the two launch plans of csrc/seg_loss.hip (seg_joint_make_plan, seg_grad_make_plan) read through
iic_debug_seg_joint_plan / iic_debug_seg_grad_plan of the instrumented library -- host code, no device needed -- against
a literal table recorded from the dispatch as it stood before the plans existed: a line-by-line port of that commit's
launch formulas, itself checked against that commit's library where the library could be asked (split count, workspace
bytes; LAB.md S17).  One wrong byte in an LDS count must not move a shape to another kernel unnoticed."""
import ctypes
import os

import pytest

JFIELDS = ("kernel", "tk", "mt", "lw", "qg", "groups", "gx", "gy", "gz", "lds")
GFIELDS = ("kernel", "tk", "lw", "kpad", "rowsP", "qc", "grid", "lds", "prep_gx", "prep_gy")
J_GENERIC, J_STREAM, J_BF16 = 1, 2, 3     # seg_joint_kernel, seg_joint_stream_kernel, seg_joint_bf16_kernel
G_GENERIC, G_STREAM, G_STREAM3 = 1, 2, 3  # seg_grad_kernel, seg_grad_stream_kernel, seg_grad_stream3_kernel
LDS_PER_CU = 160 * 1024

# (bn, k, h, w, T), iic_seg_joint_nsplit, iic_seg_grad_workspace_bytes, the joint plan at that split count, the gradient
# plan -- tensors 16-byte aligned, a workspace given, default switches.  Fields in JFIELDS / GFIELDS order.
TABLE = [
    # coco3: head A on the bf16 joint <1, 21, 32>, head B likewise
    ((120, 15, 128, 128, 10), 72, 451584, (J_BF16, 1, 21, 32, 21, 1, 21, 1, 72, 17920),
     (G_STREAM, 1, 32, 16, 336, 21, 15360, 32768, 21, 21)),
    ((120, 3, 128, 128, 10), 72, 112896, (J_BF16, 1, 21, 32, 21, 1, 21, 1, 72, 17920),
     (G_STREAM, 1, 32, 4, 84, 21, 15360, 8192, 21, 6)),
    # potsdam3: head A on seg_joint_stream_kernel<2, 11, 64>, three shift groups of 7
    ((75, 24, 200, 200, 10), 24, 1354752, (J_STREAM, 2, 11, 64, 7, 3, 21, 3, 24, 54272),
     (G_STREAM, 2, 64, 24, 504, 12, 15000, 59904, 21, 63)),
    ((75, 3, 200, 200, 10), 72, 112896, (J_BF16, 1, 21, 64, 21, 1, 21, 1, 72, 30208),
     (G_STREAM, 1, 64, 4, 84, 21, 15000, 9216, 21, 6)),
    # potsdam3 at the bench's --T 1: T < 5, no bf16 joint
    ((75, 24, 200, 200, 1), 512, 27648, (J_STREAM, 2, 11, 64, 3, 1, 3, 1, 512, 51712),
     (G_STREAM, 2, 64, 24, 72, 3, 15000, 32256, 3, 9)),
    ((75, 3, 200, 200, 1), 512, 2304, (J_STREAM, 1, 21, 64, 3, 1, 3, 1, 512, 25856),
     (G_STREAM, 1, 64, 4, 12, 3, 15000, 4608, 3, 1)),
    # overclustering (tools/seg_k48_perf.py): three class tiles
    ((60, 45, 128, 128, 10), 6, 4064256, (J_STREAM, 3, 7, 32, 2, 11, 21, 11, 6, 53760),
     (G_STREAM3, 3, 32, 48, 1008, 4, 7680, 70656, 21, 189)),
    ((60, 36, 200, 200, 5), 32, 836352, (J_STREAM, 3, 7, 64, 3, 4, 11, 4, 32, 79104),
     (G_STREAM3, 3, 64, 36, 396, 5, 12000, 69120, 11, 75)),
    # a width of 64: LW = 16 in the gradient
    ((2, 9, 11, 64, 3), 22, 37632, (J_STREAM, 1, 21, 32, 7, 1, 7, 1, 22, 8704),
     (G_STREAM, 1, 16, 12, 84, 7, 24, 9216, 7, 6)),
    # w % 4 != 0: the generic kernels
    ((2, 5, 8, 9, 6), 16, 86528, (J_GENERIC, 1, 0, 0, 21, 1, 13, 1, 16, 4096),
     (G_GENERIC, 1, 0, 0, 0, 13, 16, 5204, 0, 0)),
]
# the same shapes on the generic kernels: (joint plan with aligned = 0, gradient plan with aligned = 0 or no workspace)
GENERIC = {
    (120, 15, 128, 128, 10): ((1, 1, 0, 0, 21, 1, 21, 1, 72, 17792), (1, 1, 0, 0, 0, 21, 15360, 30428, 0, 0)),
    (120, 3, 128, 128, 10): ((1, 1, 0, 0, 21, 1, 21, 1, 72, 17792), (1, 1, 0, 0, 0, 21, 15360, 6140, 0, 0)),
    (75, 24, 200, 200, 10): ((1, 2, 0, 0, 7, 3, 21, 3, 24, 54016), (1, 2, 0, 0, 0, 12, 15000, 60000, 0, 0)),
    (75, 3, 200, 200, 10): ((1, 1, 0, 0, 21, 1, 21, 1, 72, 27008), (1, 1, 0, 0, 0, 21, 15000, 7100, 0, 0)),
    (75, 24, 200, 200, 1): ((1, 2, 0, 0, 7, 1, 3, 1, 512, 51712), (1, 2, 0, 0, 0, 3, 15000, 29760, 0, 0)),
    (75, 3, 200, 200, 1): ((1, 1, 0, 0, 21, 1, 3, 1, 512, 25856), (1, 1, 0, 0, 0, 3, 15000, 3348, 0, 0)),
    (60, 45, 128, 128, 10): ((1, 3, 0, 0, 3, 7, 21, 7, 6, 53376), (1, 3, 0, 0, 0, 4, 7680, 62100, 0, 0)),
    (60, 36, 200, 200, 5): ((1, 3, 0, 0, 3, 4, 11, 4, 32, 79104), (1, 3, 0, 0, 0, 5, 12000, 66816, 0, 0)),
    (2, 9, 11, 64, 3): ((1, 1, 0, 0, 21, 1, 7, 1, 22, 8704), (1, 1, 0, 0, 0, 7, 22, 6908, 0, 0)),
    (2, 5, 8, 9, 6): ((1, 1, 0, 0, 21, 1, 13, 1, 16, 4096), (1, 1, 0, 0, 0, 13, 16, 5204, 0, 0)),
}
# iic_debug_seg_bf16 (0, 2) -> the joint plan's (kernel, lds) where either differs from the default's
BF16_MODES = {
    (120, 15, 128, 128, 10): ((J_STREAM, 17920), (J_BF16, 17920)),
    (120, 3, 128, 128, 10): ((J_STREAM, 17920), (J_BF16, 17920)),
    (75, 24, 200, 200, 10): ((J_STREAM, 54272), (J_BF16, 60416)),     # the bf16 joint at k = 24 under mode 2 only
    (75, 3, 200, 200, 10): ((J_STREAM, 27136), (J_BF16, 30208)),
    (75, 24, 200, 200, 1): ((J_STREAM, 51712), (J_BF16, 57856)),
    (75, 3, 200, 200, 1): ((J_STREAM, 25856), (J_BF16, 28928)),
    (60, 45, 128, 128, 10): ((J_STREAM, 53760), (J_STREAM, 53760)),   # never at three class tiles (LAB.md S16)
    (60, 36, 200, 200, 5): ((J_STREAM, 79104), (J_STREAM, 79104)),
    (2, 9, 11, 64, 3): ((J_STREAM, 8704), (J_BF16, 8704)),
    (2, 5, 8, 9, 6): ((J_GENERIC, 4096), (J_GENERIC, 4096)),
}


def _load(name):
  from iic_amd import _lib
  path = os.path.join(os.path.dirname(_lib.LIB_PATH), name)
  assert os.path.exists(path), "build it: make -C iic_amd/csrc all dbg"
  h = ctypes.CDLL(path)               # host-side functions only: no device needed
  h.iic_seg_joint_nsplit.restype = ctypes.c_int
  h.iic_seg_grad_workspace_bytes.restype = ctypes.c_long
  return h


@pytest.fixture(scope="module")
def L():
  h = _load("libiic_hip_dbg.so")
  h.iic_debug_seg_joint_plan.restype = None
  h.iic_debug_seg_grad_plan.restype = None
  return h


def _joint(L, shape, ns, aligned=1):
  bn, k, h, w, T = shape
  out = (ctypes.c_int * len(JFIELDS))()
  L.iic_debug_seg_joint_plan(bn, k, h, w, T, ns, aligned, out)
  return tuple(out)


def _grad(L, shape, aligned=1, has_workspace=1):
  bn, k, h, w, T = shape
  out = (ctypes.c_int * len(GFIELDS))()
  L.iic_debug_seg_grad_plan(bn, k, h, w, T, aligned, has_workspace, out)
  return tuple(out)


def _invariants(shape, ns, jt, gt):
  bn, k, h, w, T = shape
  nq = 2 * T + 1
  j, g = dict(zip(JFIELDS, jt)), dict(zip(GFIELDS, gt))
  assert 0 < j["lds"] <= LDS_PER_CU and 0 < g["lds"] <= LDS_PER_CU, (shape, j, g)
  assert (j["gx"], j["gy"], j["gz"]) == (nq, j["groups"], ns), (shape, j)
  assert j["qg"] * j["groups"] >= nq > j["qg"] * (j["groups"] - 1), (shape, j)
  assert j["tk"] == g["tk"] == (k + 15) // 16, (shape, j, g)
  if g["kernel"] == G_GENERIC:
    # one workgroup per output row, no guard in the kernel: exactly bn h
    assert g["grid"] == bn * h and (g["kpad"], g["rowsP"], g["prep_gx"], g["prep_gy"]) == (0, 0, 0, 0), (shape, g)
  else:
    assert g["grid"] == 8 * ((bn * h + 7) // 8), (shape, g)
    assert g["kpad"] == (k + 3) // 4 * 4 and g["prep_gx"] == nq, (shape, g)
    assert g["prep_gy"] == (g["rowsP"] * 16 * g["tk"] + 255) // 256, (shape, g)
  assert g["rowsP"] == nq * g["kpad"] and g["qc"] >= 1, (shape, g)


def test_dispatch_of_the_shapes_the_project_runs(L):
  assert sorted(GENERIC) == sorted(BF16_MODES) == sorted(t[0] for t in TABLE)
  for shape, ns, ws, jwant, gwant in TABLE:
    bn, k, h, w, T = shape
    assert L.iic_seg_joint_nsplit(bn, h, k, T) == ns, shape
    assert L.iic_seg_grad_workspace_bytes(k, T) == ws == (2 * T + 1) ** 2 * gwant[1] * 16 * ((k + 3) // 4 * 4) * 4, shape
    j, g = _joint(L, shape, ns), _grad(L, shape)
    assert j == jwant, (shape, dict(zip(JFIELDS, j)), jwant)
    assert g == gwant, (shape, dict(zip(GFIELDS, g)), gwant)
    _invariants(shape, ns, j, g)
    # the workspace holds exactly what seg_gprep_kernel writes and the gradient kernel reads
    if g[0] != G_GENERIC:
      assert ws == (2 * T + 1) * g[GFIELDS.index("rowsP")] * 16 * g[1] * 4, (shape, g)
    # unaligned tensors, or no workspace for the gradient: the generic kernels
    jgen, ggen = GENERIC[shape]
    j0 = _joint(L, shape, ns, aligned=0)
    assert j0 == jgen, (shape, j0, jgen)
    for al, hw in ((0, 1), (1, 0), (0, 0)):
      g0 = _grad(L, shape, al, hw)
      assert g0 == ggen, (shape, al, hw, g0, ggen)
    _invariants(shape, ns, j0, ggen)
    # another split count moves grid z and nothing else
    assert _joint(L, shape, 5) == j[:8] + (5,) + j[9:], shape


def test_switches_the_gpu_tests_rely_on(L):
  """iic_debug_seg_stream(0): everything generic.  iic_debug_seg_bf16: 0 = no bf16 joint, 2 = the bf16 joint wherever it
  is instantiated (k <= 32); the gradient plan is the fp32 kernel's under every value.  The split count follows none."""
  try:
    for shape, ns, _, jwant, gwant in TABLE:
      bn, k, h, w, T = shape
      L.iic_debug_seg_stream(0)
      assert (_joint(L, shape, ns), _grad(L, shape)) == GENERIC[shape], shape
      assert L.iic_seg_joint_nsplit(bn, h, k, T) == ns, shape
      L.iic_debug_seg_stream(1)
      grads = []
      for mode, (kernel, lds) in zip((0, 2), BF16_MODES[shape]):
        L.iic_debug_seg_bf16(mode)
        j, g = _joint(L, shape, ns), _grad(L, shape)
        assert (j[0], j[9]) == (kernel, lds) and j[1:9] == jwant[1:9], (shape, mode, j)
        assert g == gwant, (shape, mode, g)
        assert L.iic_seg_joint_nsplit(bn, h, k, T) == ns, (shape, mode)
        _invariants(shape, ns, j, g)
        grads.append(g)
      assert grads[0] == grads[1], shape
      L.iic_debug_seg_bf16(1)
  finally:
    L.iic_debug_seg_stream(1)
    L.iic_debug_seg_bf16(1)


def test_unsupported_shapes_give_an_empty_plan(L):
  for shape in ((2, 0, 8, 8, 1), (2, 49, 8, 8, 1), (2, 5, 8, 8, -1), (2, 5, 8, 8, 11), (2, 5, 8, 260, 1), (2, 5, 0, 8, 1),
                (0, 5, 8, 8, 1)):
    assert _joint(L, shape, 4) == (0,) * len(JFIELDS), shape
    assert _grad(L, shape) == (0,) * len(GFIELDS), shape
  assert _joint(L, (2, 5, 8, 8, 1), 0) == (0,) * len(JFIELDS)


def test_abi_queries_outside_the_served_range():
  """iic_seg_joint_nsplit is asked before any launch can reject k: outside 1 <= k <= 48, 0 <= T <= 10 it answers 1 (at
  k = 0 it used to divide by zero); iic_seg_grad_workspace_bytes answers 0.  On the product library."""
  P = _load("libiic_hip.so")
  for k, T in ((0, 10), (-1, 10), (49, 10), (15, -1), (15, 11), (0, -1)):
    assert P.iic_seg_joint_nsplit(120, 128, k, T) == 1, (k, T)
    assert P.iic_seg_grad_workspace_bytes(k, T) == 0, (k, T)
  assert P.iic_seg_joint_nsplit(120, 128, 15, 10) == 72 and P.iic_seg_joint_nsplit(75, 200, 24, 10) == 24
