"""The cases of tests/nonfinite_cases.py, held to their own preconditions on the CPU (the float64 references alone; no
kernel runs here): at least half of every reference's outputs are finite, every class a case is meant to show occurs,
finite operands stay at or below 2^10 and finite reference outputs at or below 2^20.  Then the rule itself: it admits the
correct arithmetic in the kernels' precision and rejects a ReLU and a window fold built on an IEEE maxNum (fmaxf / one
v_max_f32: returns the operand that is not NaN), which is the defect the GPU file exists to catch."""
import pytest
import torch
import torch.nn.functional as F

from tests import nonfinite_cases as nf

REFS = list(nf.all_references())


@pytest.mark.parametrize("name,ref,want,operands", REFS, ids=[r[0] for r in REFS])
def test_reference_meets_the_conditions_of_its_case(name, ref, want, operands):
  c = nf.cls(ref)
  assert float((c == nf.FIN).double().mean()) >= 0.5, "fewer than half of the reference outputs are finite"
  assert nf.ISNAN in want, "every case shows a NaN"
  for k in sorted(want):
    assert bool((c == k).any()), "class %d does not occur in the reference" % k
  fin = ref.double()[c == nf.FIN]
  assert float(fin.abs().max()) <= nf.MAX_OUTPUT
  for t in operands:
    t = t.double()
    assert float(t[torch.isfinite(t)].abs().max()) <= nf.MAX_OPERAND


def test_a_negative_scale_makes_a_negative_infinity_wherever_relu_is_off():
  for C in nf.BN_CS:
    for mode in nf.BN_MODES:
      assert nf.NINF in nf.bn_apply_case(C, 0, mode)["want"]
      c = nf.bn_apply_case(C, 1, mode)
      for i in c["zero"]:
        assert float(c["ref"][i]) == 0.0
      assert int((nf.cls(c["ref"][..., 5]) != nf.ISNAN).sum()) == 0, "NaN coefficients: the whole channel"


def _bn_emulated(c, relu, relu_fn):
  """iic_bn_apply in fp32 with a bf16 store; relu_fn decides what the ReLU does with a NaN."""
  v = c["y"] * c["coef"][0] + c["coef"][1]
  if c["res"] is not None:
    v = v + c["res"]
  if c["y2"] is not None:
    v = v + (c["y2"] * c["coef2"][0] + c["coef2"][1])
  return nf.bf16(relu_fn(v) if relu else v)


@pytest.mark.parametrize("mode", nf.BN_MODES)
@pytest.mark.parametrize("C", nf.BN_CS)
def test_rule_admits_a_propagating_relu_and_rejects_maxnum(C, mode):
  for relu in (0, 1):
    c = nf.bn_apply_case(C, relu, mode)
    tol = 6 * nf.U32 * c["A"] + nf.U16 * c["ref"].abs()
    nf.check(_bn_emulated(c, relu, torch.relu), c["ref"], tol, "fp32 emulation")
    for i in c["zero"]:
      assert float(_bn_emulated(c, relu, torch.relu)[i]) == 0.0
    if relu:
      with pytest.raises(AssertionError):
        nf.check(_bn_emulated(c, relu, lambda v: torch.fmax(v, torch.zeros_like(v))), c["ref"], tol, "maxNum ReLU")


def _fold(x, nan_wins):
  """2 x 2 / 2 fold of [N, H, W, C] from -inf, with torch.maximum (NaN wins) or torch.fmax (maxNum)."""
  N, H, W, C = x.shape
  Ho, Wo = H // 2, W // 2
  m = torch.full((N, Ho, Wo, C), -nf.INF)
  for q in range(4):
    v = x[:, (q >> 1):2 * Ho:2, (q & 1):2 * Wo:2]
    m = torch.maximum(m, v) if nan_wins else torch.fmax(m, v)
  return m


@pytest.mark.parametrize("H,W", nf.POOL_HW)
def test_rule_admits_a_propagating_window_fold_and_rejects_maxnum(H, W):
  c = nf.pool2_case(H, W)
  nf.check(_fold(c["x"], True), c["ref"], 0.0, "propagating fold")
  with pytest.raises(AssertionError):
    nf.check(_fold(c["x"], False), c["ref"], 0.0, "maxNum fold")
  b = nf.bn_pool2_case(H, W)
  a = nf.bf16(torch.relu(b["y"] * b["coef"][0] + b["coef"][1]))
  nf.check(_fold(a, True), b["ref"], b["tol"], "fused pool, propagating")
  with pytest.raises(AssertionError):
    nf.check(_fold(nf.bf16(torch.fmax(b["y"] * b["coef"][0] + b["coef"][1], torch.zeros(()))), False), b["ref"], b["tol"], "maxNum")
  p = nf.pool_s2p1_case(H, W)
  got = F.max_pool2d(p["x"].permute(0, 3, 1, 2), 2, 2, padding=1).permute(0, 2, 3, 1)
  nf.check(got, p["ref"], 0.0, "padded pool in fp32")


def test_softmax_reference_rows():
  for k in nf.SOFTMAX_KS:
    c = nf.softmax_case(k)
    r = c["ref"]
    for row in (5, 9, 30, 66):
      assert bool(torch.isnan(r[row]).all())
    assert float(r[20, 0]) == 0.0 and float(r[20, 2]) == 0.0 and abs(float(r[20].sum()) - 1.0) <= 1e-12
    for row in (4, 6, 8, 10, 19, 21, 29, 31, 65):
      assert bool(torch.isfinite(r[row]).all())


def test_adam_reference_classes_follow_the_kernel_expressions():
  c = nf.adam_case()
  p, m, v = c["ref"][1]
  assert [int(nf.cls(t)[100]) for t in (p, m, v)] == [nf.ISNAN, nf.PINF, nf.PINF]
  assert [int(nf.cls(t)[200]) for t in (p, m, v)] == [nf.ISNAN, nf.NINF, nf.PINF]
  assert [int(nf.cls(t)[0]) for t in (p, m, v)] == [nf.ISNAN] * 3 and [int(nf.cls(t)[256]) for t in (p, m, v)] == [nf.ISNAN] * 3
  assert int(sum((nf.cls(r[0]) != nf.FIN).sum() for r in c["ref"])) == 8


def test_loss_references_are_nan_where_the_defect_is():
  c = nf.iid_case()
  assert [int(k) for k in nf.cls(c["loss"])] == [nf.FIN, nf.ISNAN, nf.FIN]
  assert bool(torch.isnan(c["dz"][1]).all()) and bool(torch.isfinite(c["dz"][[0, 2]]).all())
  assert bool(torch.isnan(c["dzt"][1]).all()) and bool(torch.isfinite(c["dzt"][[0, 2]]).all())
  for collapsed in (False, True):
    assert [int(k) for k in nf.cls(nf.seg_case(collapsed)["ref"])] == [nf.ISNAN, nf.ISNAN, nf.FIN, nf.FIN]
  e = nf.ce_case()
  assert bool(torch.isnan(e["loss"])) and bool(torch.isnan(e["dl"][4]).all())
