"""The stages of the two IID losses, each on its own through the C ABI (csrc/iid_loss.hip, csrc/seg_loss.hip,
csrc/warp.hip): the raw joints and the input gradients EXACTLY on dyadic lattices, the float64 k x k stage inside a bound of
one fp32 rounding plus its counted float64 roundings, the joints on full-mantissa operands inside the accumulation bound
of their kernel family, and the affine warp with its adjoint exactly.  Cases, references and preconditions:
tests/iid_stage_cases.py; their proof without a GPU: tests/test_iid_stages_cpu.py; bounds: tests/parity.py.  pytest -m gpu.

Every output buffer starts as NaN (or parity.SENTINEL where padding must survive): an element never written fails."""
import pytest
import torch

from tests import iid_stage_cases as sc
from tests.conftest import hook
from tests.lattice import assert_exact, record
from tests.parity import (SENTINEL, WORST, assert_bits, assert_within, dev, fma_acc_bound, fma_acc_bound_each, ok,
                          split_joint_bound, stage_bound, stage_n)

pytestmark = pytest.mark.gpu
HOOKS = pytest.mark.hooks
NAN = float("nan")
FAMILIES = ("kxk_loss", "kxk_dR", "seg_joint_f32", "seg_joint_bf16", "iid_joint")


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
  yield
  record(file="test_gpu_iid_stages", worst={f: WORST[f] for f in FAMILIES if f in WORST})


def L():
  from iic_amd import _lib
  return _lib.lib()


def nan_like(shape):
  return torch.full(tuple(shape), NAN, device=dev())


# ---- segmentation joint and gradients, exact ---------------------------------------------------------------------------------
# dispatch modes: the product library's default, and the instrumented library's switches (iic_debug_seg_bf16 chooses the
# JOINT kernel only: the gradient is the fp32 MFMA kernel under every value, so its "bf16" cases run that one again)
MODES = [pytest.param("default", id="default"),
         pytest.param("generic", id="stream0", marks=HOOKS),
         pytest.param("fp32", id="bf16_0", marks=HOOKS),
         pytest.param("bf16", id="bf16_2", marks=HOOKS)]


class dispatch:
  def __init__(self, mode):
    self.mode = mode

  def __enter__(self):
    if self.mode == "generic":
      hook("iic_debug_seg_stream", 0)
    elif self.mode == "fp32":
      hook("iic_debug_seg_bf16", 0)
    elif self.mode == "bf16":
      hook("iic_debug_seg_bf16", 2)

  def __exit__(self, *exc):
    hook("iic_debug_seg_stream", 1)
    hook("iic_debug_seg_bf16", 1)


def seg_joint(inp, ns):
  bn, k, h, w, T = inp["case"]
  nq = 2 * T + 1
  d = dev()
  part = nan_like((ns, nq * nq, k, k))
  ok("iic_seg_joint_raw", inp["x1"].to(d), inp["x2"].to(d), inp["mask"].to(d), inp["flips"].to(d), part, bn, k, h, w, T, ns)
  return part.cpu().double().sum(0).view(nq, nq, k, k)


def seg_grad(inp, which, collapsed, with_ws):
  bn, k, h, w, T = inp["case"]
  d = dev()
  n = "c" if collapsed else "u"
  src = inp["x2" if which == 0 else "x1"].to(d)
  ws = torch.empty(L().iic_seg_grad_workspace_bytes(k, T) // 4, device=d) if with_ws else None
  out = nan_like(src.shape)
  ok("iic_seg_grad", src, inp["mask"].to(d), inp["flips"].to(d), inp["dR1" + n].to(d), inp["dR2" + n].to(d),
     inp["gl" + n].to(d), inp["gnl" + n].to(d), out, bn, k, h, w, T, which, 1 if collapsed else 0, ws)
  return out.cpu()


def split_counts(case):
  bn, k, h, w, T = case
  rows = bn * h
  odd = next(n for n in (3, 4, 5, 7) if rows % n)      # does not divide bn h; beyond bn h: empty splits must write zeros
  return sorted(set([1, L().iic_seg_joint_nsplit(bn, h, k, T), rows, odd]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sc.SEG_CASES)
def test_seg_joint_exact(case, mode):
  inp, ref = sc.seg_inputs(case), sc.seg_exact_reference(case)
  with dispatch(mode):
    for ns in split_counts(case):
      assert_exact(seg_joint(inp, ns), ref["R"], "joint %s nsplit %d %s" % (case, ns, mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", sc.SEG_CASES)
def test_seg_grad_exact(case, mode):
  """Both gradients, collapsed and uncollapsed, with the workspace (streaming kernels where w % 4 == 0) and with
  workspace = NULL (the generic kernel on a streaming shape)."""
  bn, k, h, w, T = case
  inp, ref = sc.seg_inputs(case), sc.seg_exact_reference(case)
  if bn * h > 1 and w > 1:      # the flips move the second gradient: a kernel that stores it unflipped differs from the reference
    assert not torch.equal(ref["du1"], sc.flip_samples(ref["du1"], inp["flips"]))
  with dispatch(mode):
    for collapsed in (False, True):
      for which in (0, 1):
        want = ref["d%s%d" % ("c" if collapsed else "u", which)]
        for with_ws in ((True, False) if w % 4 == 0 else (True,)):
          got = seg_grad(inp, which, collapsed, with_ws)
          assert_exact(got, want, "gradient %s which %d collapsed %d workspace %d %s" % (case, which, collapsed, with_ws, mode))


# ---- clustering joint and gradients, exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sc.IID_LAYOUTS)
@pytest.mark.parametrize("case", sc.IID_CASES)
def test_iid_joint_and_grad_exact(case, layout):
  H, bn, k = case
  inp, ref = sc.iid_inputs(case), sc.iid_exact_reference(case)
  hs, ld, size, idx = sc.iid_layout(case, layout)
  d = dev()
  z, zt = sc.iid_place(inp["z"], case, layout, SENTINEL).to(d), sc.iid_place(inp["zt"], case, layout, SENTINEL).to(d)
  for ns in sorted(set([1, 3, L().iic_iid_nsplit(bn), 16])):
    part = nan_like((ns, H, k, k))
    ok("iic_iid_joint_raw", z, zt, part, H, bn, k, hs, ld, ns)
    assert_exact(part.cpu().double().sum(0), ref["R"], "joint %s %s nsplit %d" % (case, layout, ns))
  dR1, dR2 = inp["dR1"].to(d), inp["dR2"].to(d)
  pad = torch.ones(size, dtype=torch.bool)
  pad[idx.reshape(-1)] = False
  for upstream in (True, False):
    dz, dzt = torch.full((size,), SENTINEL, device=d), torch.full((size,), SENTINEL, device=d)
    ok("iic_iid_grad", z, zt, dR1, dR2, inp["gl"].to(d) if upstream else None, inp["gnl"].to(d) if upstream else None,
       dz, dzt, H, bn, k, hs, ld)
    for got, name in ((dz, "dz"), (dzt, "dzt")):
      got = got.cpu()
      assert_exact(got[idx], ref[name, upstream], "%s %s %s upstream %d" % (name, case, layout, upstream))
      assert bool((got[pad] == SENTINEL).all()), "%s: a pad column was written" % name


# ---- the k x k stage ---------------------------------------------------------------------------------------------------------------
def run_stage(entry, part, lamb, detach):
  nparts, H, k, _ = part.shape
  d = dev()
  ws = torch.full((L().iic_iid_workspace_bytes(H, k) // 8,), NAN, dtype=torch.float64, device=d)
  loss, loss_nl = nan_like((H,)), nan_like((H,))
  dR1, dR2 = nan_like((H, k, k)), nan_like((H, k, k))
  args = (part.to(d), nparts, H, k, float(lamb), sc.EPS, ws, loss, loss_nl, dR1, dR2)
  if entry == "iic_seg_loss_from_joint":
    args = args + (detach,)
  ok(entry, *args)
  return dict(loss1=loss.cpu(), loss2=loss_nl.cpu(), dR1=dR1.cpu(), dR2=dR2.cpu())


@pytest.mark.parametrize("kind", sc.STAGE_DRAWS)
@pytest.mark.parametrize("case", sc.STAGE_CASES)
def test_kxk_stage_within_the_float64_bound(case, kind):
  """iic_iid_loss_from_joint and iic_seg_loss_from_joint (detach_norm 0 and 1) on given partials: all four outputs
  inside parity.stage_bound, two launches bit-identical.  Every head has its own draw: a head reading another head's
  partials leaves the bound."""
  H, k, nparts = case
  part = sc.stage_partials(case, kind)
  for lamb in sc.STAGE_LAMBS:
    for entry, detach in (("iic_iid_loss_from_joint", 0), ("iic_seg_loss_from_joint", 0), ("iic_seg_loss_from_joint", 1)):
      ref = sc.stage_ref(part, lamb, detach)
      got = run_stage(entry, part, lamb, detach)
      again = run_stage(entry, part, lamb, detach)
      what = "%s detach %d %s %s lamb %g" % (entry, detach, case, kind, lamb)
      for name, mag, fam in (("loss1", "M1", "kxk_loss"), ("loss2", "M2", "kxk_loss"), ("dR1", "mag1", "kxk_dR"),
                             ("dR2", "mag2", "kxk_dR")):
        assert_bits(got[name], again[name], what + " " + name + " (two launches)")
        assert_within(got[name], ref[name], stage_bound(ref[name], ref[mag], k, nparts), what + " " + name, fam)
  record(case=list(case), kind=kind, n=stage_n(k, nparts), worst_loss=WORST.get("kxk_loss"), worst_dR=WORST.get("kxk_dR"))


# ---- joints on full-mantissa operands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.SEG_F64_CASES)
def test_seg_joint_full_mantissa_within_its_family_bound(case):
  bn, k, h, w, T = case
  f = sc.seg_f64_inputs(case)
  x1m, x2m = sc.seg_maps(f["x1"], f["x2"], f["mask"], f["flips"])
  ref = sc.seg_joint_ref(x1m, x2m, T)      # operands >= 0: the reference is its own magnitude sum A
  terms = sc.seg_terms(case)[:, :, None, None]
  bf16 = case in sc.SEG_BF16      # (default dispatch: w % 4 == 0, k <= 16, T >= 5)
  bound = split_joint_bound(terms, ref) if bf16 else fma_acc_bound_each(terms, ref)
  got = seg_joint(f, L().iic_seg_joint_nsplit(bn, h, k, T))
  assert_within(got, ref, bound, "joint %s" % (case,), "seg_joint_bf16" if bf16 else "seg_joint_f32")


@pytest.mark.parametrize("case", sc.IID_F64_CASES)
def test_iid_joint_full_mantissa_within_the_fma_bound(case):
  H, bn, k = case
  f = sc.iid_f64_inputs(case)
  ref = sc.iid_joint_ref(f["z"], f["zt"])
  hs, ld, size, idx = sc.iid_layout(case, "packed")
  d = dev()
  ns = L().iic_iid_nsplit(bn)
  part = nan_like((ns, H, k, k))
  ok("iic_iid_joint_raw", sc.iid_place(f["z"], case, "packed", SENTINEL).to(d),
     sc.iid_place(f["zt"], case, "packed", SENTINEL).to(d), part, H, bn, k, hs, ld, ns)
  assert_within(part.cpu().double().sum(0), ref, fma_acc_bound(bn, ref), "joint %s" % (case,), "iid_joint")


# ---- affine warp, exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.WARP_SHAPES)
def test_affine_warp_forward_and_adjoint_exact(shape):
  """iic_affine_warp_fwd / iic_affine_warp_bwd with pixel-space matrices passed directly: every contribution is exact, so
  the float atomics of the backward are order-independent here; dx must be rewritten completely."""
  N, K, H, W = shape
  inp = sc.warp_inputs(shape)
  d = dev()
  x, dout = inp["x"].to(d), inp["dout"].to(d)
  for name, M, sx, sy in sc.warp_matrices(shape):
    out, dx = nan_like(shape), nan_like(shape)
    ok("iic_affine_warp_fwd", x, M.to(d), out, N, K, H, W, sx, sy)
    assert_exact(out.cpu(), sc.warp_fwd_ref(inp["x"], M, sx, sy), "warp forward %s %s" % (shape, name))
    ok("iic_affine_warp_bwd", dout, M.to(d), dx, N, K, H, W, sx, sy)
    assert_exact(dx.cpu(), sc.warp_bwd_ref(inp["dout"], M, sx, sy), "warp backward %s %s" % (shape, name))
