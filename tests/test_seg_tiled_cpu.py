"""The tiled segmentation-loss kernels (csrc/seg_loss_tiled.hip) without a GPU: the cases of tests/seg_tiled_cases.py
satisfy the preconditions of the exact comparison and have four non-zero gradient references; that comparison rejects a
window without its halo, a window boundary off by one and a class block read at the transposed offset; and the launch
plans, read through iic_debug_seg_tiled_joint_plan / iic_debug_seg_tiled_grad_plan of the instrumented library (host code),
stay inside the LDS, cover every column and every class pair exactly once and split by the shape alone."""
import ctypes
import os

import pytest
import torch

from tests import iid_stage_cases as sc
from tests import seg_tiled_cases as tc
from tests.lattice import exact_mismatch, record

JFIELDS = ("tk", "nb", "qg", "groups", "ws", "nwin", "gx", "gy", "gz", "lds")
GFIELDS = ("tk", "nbo", "ka", "kc", "qc", "ws", "nwin", "gx", "gy", "gz", "lds", "prep_grid")
LDS_PER_CU = 160 * 1024
PATH_NONE, PATH_RESIDENT, PATH_TILED = 0, 1, 2
MAX_K, MAX_T = 255, 10
PART_CAP_BYTES = 64 << 20      # include/iic_hip.h IIC_SEG_TILED_PART_CAP_BYTES


def _load(name):
  from iic_amd import _lib
  path = os.path.join(os.path.dirname(_lib.LIB_PATH), name)
  assert os.path.exists(path), "build it: make -C iic_amd/csrc all dbg"
  h = ctypes.CDLL(path)               # host-side functions only: no device needed
  h.iic_seg_tiled_grad_workspace_bytes.restype = ctypes.c_long
  return h


@pytest.fixture(scope="module")
def L():
  h = _load("libiic_hip_dbg.so")
  h.iic_debug_seg_tiled_joint_plan.restype = None
  h.iic_debug_seg_tiled_grad_plan.restype = None
  return h


def joint_plan(L, shape, ns):
  bn, k, h, w, T = shape
  out = (ctypes.c_int * len(JFIELDS))()
  L.iic_debug_seg_tiled_joint_plan(bn, k, h, w, T, ns, out)
  return dict(zip(JFIELDS, out))


def grad_plan(L, shape, collapsed):
  bn, k, h, w, T = shape
  out = (ctypes.c_int * len(GFIELDS))()
  L.iic_debug_seg_tiled_grad_plan(bn, k, h, w, T, collapsed, out)
  return dict(zip(GFIELDS, out))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CASES)
def test_case_meets_the_exactness_preconditions_and_has_nonzero_gradients(case):
  """seg_exact_reference asserts the lattice preconditions itself (every value a multiple of 2^-6 / 2^-7, every sum of
  magnitudes below 2^24 of that unit); the seed is the lowest at which none of the four gradient references is zero."""
  seed = tc.case_seed(case)
  ref = tc.reference(case)
  for g in tc.GRADS:
    assert float(ref[g].abs().max()) > 0, (case, g)
  assert float(ref["R"].abs().max()) > 0
  for lower in range(seed):      # the lowest: every seed below it has a vacuous gradient
    r = sc.seg_exact_reference(case, lower)
    assert any(float(r[g].abs().max()) == 0 for g in tc.GRADS), (case, lower)
  record(file="test_seg_tiled_cpu", seed=seed, **ref["figures"])


def test_the_seeds_that_seed_zero_leaves_vacuous():
  """With seed 0 both collapsed upstream gradients of these three cases are drawn as 0."""
  for case in ((1, 16, 2, 264, 10), (2, 5, 2, 516, 2), (2, 49, 3, 8, 1)):
    assert tc.case_seed(case) > 0, case
    r = sc.seg_exact_reference(case, 0)
    assert float(r["dc0"].abs().max()) == 0 and float(r["dc1"].abs().max()) == 0, case


# ---- seeded defects -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.WINDOWS_ALIGNED + tc.WINDOWS_UNALIGNED + tc.BOTH)
def test_exact_comparison_rejects_a_broken_window(L, case):
  bn, k, h, w, T = case
  ws = joint_plan(L, case, 1)["ws"]
  assert len(tc.windows(w, ws)) >= 2, (case, ws)
  inp, ref = tc.inputs(case), tc.reference(case)
  x1m, x2m = sc.seg_maps(inp["x1"], inp["x2"], inp["mask"], inp["flips"])
  assert exact_mismatch(tc.windowed_joint(x1m, x2m, T, ws), ref["R"]) is None, case
  for defect in ("no_halo", "off_by_one"):
    assert exact_mismatch(tc.windowed_joint(x1m, x2m, T, ws, defect), ref["R"]) is not None, (case, defect)


@pytest.mark.parametrize("case", tc.CLASS_BLOCKS + tc.BOTH)
def test_exact_comparison_rejects_a_transposed_class_block(L, case):
  bn, k, h, w, T = case
  p = joint_plan(L, case, 1)
  bs = 16 * p["tk"]
  assert p["nb"] >= 2, (case, p)
  inp, ref = tc.inputs(case), tc.reference(case)
  x1m, x2m = sc.seg_maps(inp["x1"], inp["x2"], inp["mask"], inp["flips"])
  assert exact_mismatch(tc.blocked_joint(x1m, x2m, T, bs), ref["R"]) is None, case
  assert exact_mismatch(tc.blocked_joint(x1m, x2m, T, bs, "transposed"), ref["R"]) is not None, case


# ---- plans ----------------------------------------------------------------------------------------------------------------------
def _check_plans(L, shape):
  bn, k, h, w, T = shape
  nq = 2 * T + 1
  ns = L.iic_seg_tiled_joint_nsplit(bn, h, w, k, T)
  assert 1 <= ns <= bn * h, (shape, ns)
  assert ns * nq * nq * k * k * 4 <= max(PART_CAP_BYTES, nq * nq * k * k * 4), (shape, ns)
  j = joint_plan(L, shape, ns)
  assert 0 < j["lds"] <= LDS_PER_CU, (shape, j)
  assert 1 <= j["tk"] <= 3 and j["ws"] <= 256 and j["ws"] % 4 == 0, (shape, j)
  # windows cover [0, w) exactly once
  wins = tc.windows(w, j["ws"])
  assert len(wins) == j["nwin"], (shape, j)
  covered = torch.zeros(w, dtype=torch.int32)
  for x0, n in wins:
    assert 1 <= n <= j["ws"]
    covered[x0:x0 + n] += 1
  assert bool((covered == 1).all()), shape
  # class blocks cover k x k exactly once; the column-shift groups cover the 2T + 1 shifts
  bs = 16 * j["tk"]
  assert (j["nb"] - 1) * bs < k <= j["nb"] * bs, (shape, j)
  pairs = torch.zeros((k, k), dtype=torch.int32)
  for bi in range(j["nb"]):
    for bj in range(j["nb"]):
      pairs[bi * bs:min(k, bi * bs + bs), bj * bs:min(k, bj * bs + bs)] += 1
  assert bool((pairs == 1).all()), shape
  assert j["qg"] * j["groups"] >= nq > j["qg"] * (j["groups"] - 1), (shape, j)
  assert (j["gx"], j["gy"], j["gz"]) == (nq, j["groups"] * j["nb"] ** 2, ns), (shape, j)
  assert j["gy"] <= 65535 and j["gz"] <= 65535
  # staged rows and the cross-wave reduction fit the LDS the plan asks for
  rows = 16 * j["tk"] * (((j["ws"] + 2 * T) | 1) + (j["ws"] | 1)) * 4
  assert j["lds"] == max(rows, 4 * j["tk"] ** 2 * 256 * 4), (shape, j)
  for collapsed in (0, 1):
    g = grad_plan(L, shape, collapsed)
    assert 0 < g["lds"] <= LDS_PER_CU, (shape, g)
    assert (g["tk"], g["nbo"], g["ws"], g["nwin"]) == (j["tk"], j["nb"], j["ws"], j["nwin"]), (shape, g, j)
    assert g["ka"] == g["nbo"] * 16 * g["tk"] >= k, (shape, g)
    assert g["kc"] % 4 == 0 and 1 <= g["kc"] <= 48 and 1 <= g["qc"] <= nq, (shape, g)
    assert g["lds"] == (g["kc"] * ((g["ws"] + 2 * T) | 1) + g["qc"] * g["kc"] * (16 * g["tk"] + 1)) * 4, (shape, g)
    assert (g["gx"], g["gy"], g["gz"]) == (bn * h, g["nwin"], g["nbo"]), (shape, g)
    H = 1 if collapsed else nq * nq
    assert L.iic_seg_tiled_grad_workspace_bytes(k, T, collapsed) == H * k * g["ka"] * 4, (shape, g)
    assert g["prep_grid"] >= 1
  return ns, j


@pytest.mark.parametrize("shape", tc.CASES + tc.WORKLOAD + tc.SHARED + [(1, 255, 4, 1024, 10), (2, 1, 1, 1, 0)])
def test_plans_fit_and_cover(L, shape):
  ns, j = _check_plans(L, shape)
  # another split count moves grid z and nothing else
  other = joint_plan(L, shape, 5)
  assert {**other, "gz": ns} == j, shape


def test_two_workgroups_per_cu_on_the_workload_shapes(L):
  for shape in tc.WORKLOAD:
    assert joint_plan(L, shape, 1)["lds"] <= LDS_PER_CU // 2, shape
    assert grad_plan(L, shape, 1)["lds"] <= LDS_PER_CU // 2, shape


def test_split_count_is_a_function_of_the_shape_alone(L):
  """The same answer from the product library and from the instrumented one under every dispatch switch of the resident
  kernels; bounded by the partial-buffer cap where one partial is large."""
  P = _load("libiic_hip.so")
  try:
    for shape in tc.CASES + tc.WORKLOAD + tc.SHARED:
      bn, k, h, w, T = shape
      want = P.iic_seg_tiled_joint_nsplit(bn, h, w, k, T)
      for stream, bf16 in ((1, 1), (0, 1), (1, 0), (1, 2)):
        L.iic_debug_seg_stream(stream)
        L.iic_debug_seg_bf16(bf16)
        assert L.iic_seg_tiled_joint_nsplit(bn, h, w, k, T) == want, shape
  finally:
    L.iic_debug_seg_stream(1)
    L.iic_debug_seg_bf16(1)
  assert P.iic_seg_tiled_joint_nsplit(8, 320, 320, 255, 10) == 1      # one partial is 115 MB
  for k in (1, 3, 16, 17, 32, 33, 48, 49, 64, 65, 81, 96, 97, 128, 200, 255):
    for T in range(MAX_T + 1):
      one = (2 * T + 1) ** 2 * k * k * 4
      ns = P.iic_seg_tiled_joint_nsplit(64, 512, 512, k, T)
      assert ns >= 1 and ns * one <= max(PART_CAP_BYTES, one), (k, T, ns)
  assert P.iic_seg_tiled_joint_nsplit(1, 1, 8, 49, 1) == 1
  for k, T, w in ((0, 1, 8), (256, 1, 8), (49, 11, 8), (49, -1, 8), (49, 1, 0), (49, 1, 4097)):
    assert P.iic_seg_tiled_joint_nsplit(2, 8, w, k, T) == 1, (k, T, w)
  for k, T in ((0, 1), (256, 1), (49, 11), (49, -1)):
    assert P.iic_seg_tiled_grad_workspace_bytes(k, T, 1) == P.iic_seg_tiled_grad_workspace_bytes(k, T, 0) == 0, (k, T)


def test_unsupported_shapes_give_an_empty_plan(L):
  for shape in ((2, 0, 8, 8, 1), (2, 256, 8, 8, 1), (2, 49, 8, 8, -1), (2, 49, 8, 8, 11), (2, 49, 8, 4097, 1),
                (2, 49, 0, 8, 1), (0, 49, 8, 8, 1), (2, 49, 8, 0, 1)):
    assert set(joint_plan(L, shape, 4).values()) == {0}, shape
    assert set(grad_plan(L, shape, 1).values()) == {0}, shape
  assert set(joint_plan(L, (2, 49, 8, 8, 1), 0).values()) == {0}


# ---- the selector ---------------------------------------------------------------------------------------------------------------
def test_selector_keeps_every_shape_served_today_on_todays_kernels():
  from tests.test_seg_dispatch_cpu import TABLE
  P = _load("libiic_hip.so")
  for (bn, k, h, w, T), *_ in TABLE:
    assert P.iic_seg_loss_path(k, w, T) == PATH_RESIDENT, (k, w, T)
  for bn, k, h, w, T in sc.SEG_CASES + tc.SHARED:
    assert P.iic_seg_loss_path(k, w, T) == PATH_RESIDENT, (k, w, T)
  for k, w, T in ((1, 1, 0), (48, 256, 10)):
    assert P.iic_seg_loss_path(k, w, T) == PATH_RESIDENT
  for bn, k, h, w, T in tc.CASES + tc.WORKLOAD:
    assert P.iic_seg_loss_path(k, w, T) == PATH_TILED, (k, w, T)
  for k, w, T in ((49, 8, 1), (48, 257, 1), (255, 4096, 10)):
    assert P.iic_seg_loss_path(k, w, T) == PATH_TILED
  for k, w, T in ((0, 8, 1), (256, 8, 1), (15, 128, 11), (15, 128, -1), (15, 0, 1), (15, 4097, 1), (49, 8, 11)):
    assert P.iic_seg_loss_path(k, w, T) == PATH_NONE, (k, w, T)
  assert [P.iic_seg_tiled_limit(i) for i in range(4)] == [MAX_K, MAX_T, 4096, 0]
