"""BatchNorm backward on running statistics: gradients through eval() and through frozen BatchNorm layers.

Kernel level: iic_bn_bwd_frozen and iic_bn_bwd_finalize_frozen through the C ABI, against the float64 references and
bounds of tests/bn_frozen_cases.py (tests/test_bn_frozen_cpu.py proves on a numpy emulation that those bounds admit the
correct arithmetic and reject seeded defects): dy exact, borders untouched, sums / dgamma / dbeta within the bounds of
the batch-statistics kernels, argument errors.

Module level: ClusterNet5g, ClusterNet6c and SegmentationNet10a differentiated in eval() -- and, for ClusterNet5g, under
the fine-tuning recipe net.train() + .eval() on every BatchNorm2d -- against the CPU oracle with training=False, on the
exact-fp32 kernels (ops.fp32_mode()) with the gates of test_net5g_five_input_channels_fp32_mode_vs_oracle, then on the bf16
path; single blocks and stages against the bf16-emulating oracle; one block with mixed modes against float64; the
pre-masked gradient chain; and the graph-replay wrapper, which leaves such a module to eager launches."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import bn_bf16_cases as cases
from tests import bn_frozen_cases as fcases
from tests.parity import SENTINEL, assert_border, call, dev, interior, ok, pt_of

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
IIC_ERR_ARG, IIC_ERR_UNSUPPORTED = -1, -3


def _cos(a, b):
  a, b = a.double().flatten(), b.double().flatten()
  return float((a @ b) / (a.norm() * b.norm() + 1e-30))


# --------------------------------------------------------------------------------------
# kernel level
# --------------------------------------------------------------------------------------
def _pt(x, P):
  return None if x is None else pt_of(x, P, BF16)


def _sentinel(shape):
  N, H, W, P, C = shape
  return torch.full((N, H + 2 * P, W + 2 * P, C), SENTINEL, dtype=BF16, device=dev())


def _d(c):
  return None if c is None else c.to(dev()).contiguous()


class Gpu:
  """iic_bn_bwd_frozen / iic_bn_bwd_finalize_frozen as a backend of tests/bn_frozen_cases.py."""

  def frozen(self, dout, act, y, coef, y2, coef2, mcoef, shape):
    from iic_amd import ops
    N, H, W, P, C = shape
    dy, dy2 = _sentinel(shape), _sentinel(shape)
    s1, s2 = ops.new_stats(C, dev()), ops.new_stats(C, dev())
    two = y2 is not None
    ok("iic_bn_bwd_frozen", _pt(dout, P), _pt(act, P), _pt(y, P), _d(coef), dy, _pt(y2, P), _d(coef2), dy2 if two else None,
       s1, s2 if two else None, _d(mcoef), N, H, W, P, C)
    assert_border(dy, P, SENTINEL, "bn_bwd_frozen dy")
    assert_border(dy2, P, SENTINEL, "bn_bwd_frozen dy2")
    if not two:
      assert bool((dy2.float() == SENTINEL).all()), "dy2 written without y2"
      assert int(s2.abs().max()) == 0, "sums2 written without y2"
    return (interior(dy, P).float(), interior(dy2, P).float() if two else None, ops.stats_decode(s1, C).cpu(),
            ops.stats_decode(s2, C).cpu() if two else None)

  def finalize_frozen(self, sums, coef):
    from iic_amd import ops
    C = coef.shape[1]
    st = ops.new_stats(C, dev())
    ops.stats_encode(st, C, sums)
    out = []
    for _ in range(2):
      bcoef, dg, db = (torch.full(s, SENTINEL, device=dev()) for s in ((3, C), (C,), (C,)))
      ok("iic_bn_bwd_finalize_frozen", st, _d(coef), bcoef, dg, db, C)
      assert int(st.abs().max()) == 0, "the accumulator is not zero after iic_bn_bwd_finalize_frozen"
      out.append((bcoef.cpu(), dg.cpu(), db.cpu()))
    return out[0] + out[1][1:]


GPU = Gpu()


@pytest.mark.parametrize("shape", fcases.SHAPES, ids=str)
def test_bn_bwd_frozen_vs_float64(shape):
  """iic_bn_bwd_frozen, three mask modes x with / without the second BatchNorm: dy = bf16(fp32(scale) * g) exactly,
  borders untouched, sums within n_block * U32 * sum |terms|, sums2[0] == sums[0]."""
  fcases.check_frozen(GPU, shape)


@pytest.mark.parametrize("shape", [(5, 49, 49, 1, 64),       # pair loop plus a ragged tail
                                   (3, 3, 5, 2, 64),         # one advance crosses two image borders
                                   (11, 7, 7, 1, 512)],      # 4 pixel lanes, a last chunk shorter than that
                         ids=str)
def test_bn_bwd_frozen_leaves_the_statistic_cells_of_bn_bwd_reduce(shape):
  """iic_bn_bwd_frozen and iic_bn_bwd_reduce walk the pixels in the same order, mask and accumulate alike and end in the
  same block sums (one walk, one mask, one block-sum routine in csrc/bn.hip): on the same inputs the raw accumulator
  cells of sums and sums2 are equal bit for bit, in every mask mode, with and without the second BatchNorm."""
  from iic_amd import ops
  N, H, W, P, C = shape
  i = cases.inputs(*shape)
  dout, act, y, y2 = (_pt(i[k], P) for k in ("dout", "act", "y", "y2"))
  coef, coef2, mcoef = _d(i["coef"]), _d(i["coef2"]), _d(i["mcoef"])
  dy, dy2 = _sentinel(shape), _sentinel(shape)
  for mode in cases.MASK_MODES:
    a, m = (act if mode == "act" else None), (mcoef if mode == "mask_coef" else None)
    for two in (False, True):
      cells = {}
      for entry in ("reduce", "frozen"):
        s1, s2 = ops.new_stats(C, dev()), (ops.new_stats(C, dev()) if two else None)
        if entry == "reduce":
          ok("iic_bn_bwd_reduce", dout, a, y, y2 if two else None, s1, s2, m, N, H, W, P, C)
        else:
          ok("iic_bn_bwd_frozen", dout, a, y, coef, dy, y2 if two else None, coef2 if two else None, dy2 if two else None,
             s1, s2, m, N, H, W, P, C)
        assert int(s1.abs().max()) > 0
        cells[entry] = (s1, s2)
      what = "%s mask=%s y2=%d" % (shape, mode, two)
      assert torch.equal(cells["frozen"][0], cells["reduce"][0]), what + ": sums"
      if two:
        assert torch.equal(cells["frozen"][1], cells["reduce"][1]), what + ": sums2"


def test_bn_bwd_finalize_frozen_vs_float64():
  """iic_bn_bwd_finalize_frozen: dgamma, dbeta within (U32 + 8 EPS64) |ref| (sums with sy within a few ulps of
  mean * s), bcoef = (scale, 0, 0), sums re-zeroed -- a second finalise returns zeros."""
  fcases.check_finalize_frozen(GPU)


def test_bn_bwd_finalize_frozen_without_bcoef():
  """bcoef is nullable: the same dgamma / dbeta bit for bit."""
  from iic_amd import ops
  sums, coef = fcases.finalize_inputs()
  C = coef.shape[1]
  res = []
  for with_bcoef in (True, False):
    st = ops.new_stats(C, dev())
    ops.stats_encode(st, C, sums)
    dg, db = torch.empty(C, device=dev()), torch.empty(C, device=dev())
    ok("iic_bn_bwd_finalize_frozen", st, _d(coef), torch.empty((3, C), device=dev()) if with_bcoef else None, dg, db, C)
    res.append((dg.cpu(), db.cpu()))
  assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("C", fcases.UNSUPPORTED_C)
def test_bn_bwd_frozen_refuses_other_channel_counts(C):
  """check_c fails: IIC_ERR_UNSUPPORTED before a launch -- dy and the accumulator untouched."""
  from iic_amd import ops
  shape = (2, 5, 7, 1, C)
  N, H, W, P, _ = shape
  i = cases.inputs(*shape)
  dy, st = _sentinel(shape), ops.new_stats(C, dev())
  rc = call("iic_bn_bwd_frozen", _pt(i["dout"], P), None, _pt(i["y"], P), _d(i["coef"]), dy, None, None, None, st, None,
            None, N, H, W, P, C)
  assert rc == IIC_ERR_UNSUPPORTED
  assert bool((dy.float() == SENTINEL).all()) and int(st.abs().max()) == 0


def test_bn_bwd_frozen_argument_errors():
  """A half-given (y2, coef2, dy2, sums2) group, and act together with mask_coef: IIC_ERR_ARG, nothing written."""
  from iic_amd import ops
  shape = (2, 5, 7, 1, 128)
  N, H, W, P, C = shape
  i = cases.inputs(*shape)
  dout, act, y, y2 = (_pt(i[k], P) for k in ("dout", "act", "y", "y2"))
  coef, coef2, mcoef = _d(i["coef"]), _d(i["coef2"]), _d(i["mcoef"])
  dy, dy2 = _sentinel(shape), _sentinel(shape)
  s1, s2 = ops.new_stats(C, dev()), ops.new_stats(C, dev())
  full = (y2, coef2, dy2, s2)
  for drop in range(4):
    for keep_only in (False, True):      # one of the four missing / only one of the four given
      g = [(a if (k == drop) == keep_only else None) for k, a in enumerate(full)]
      rc = call("iic_bn_bwd_frozen", dout, None, y, coef, dy, g[0], g[1], g[2], s1, g[3], None, N, H, W, P, C)
      assert rc == IIC_ERR_ARG, (drop, keep_only, rc)
  assert call("iic_bn_bwd_frozen", dout, act, y, coef, dy, None, None, None, s1, None, mcoef, N, H, W, P, C) == IIC_ERR_ARG
  assert call("iic_bn_bwd_frozen", dout, None, y, None, dy, None, None, None, s1, None, None, N, H, W, P, C) == IIC_ERR_ARG
  assert call("iic_bn_bwd_frozen", dout, None, y, coef, dy, None, None, None, None, None, None, N, H, W, P, C) == IIC_ERR_ARG
  assert bool((dy.float() == SENTINEL).all()) and bool((dy2.float() == SENTINEL).all())
  assert int(s1.abs().max()) == 0 and int(s2.abs().max()) == 0


# --------------------------------------------------------------------------------------
# module level: shared helpers
# --------------------------------------------------------------------------------------
def _grad_leaves(params, dtype=None):
  """A copy of an oracle parameter dictionary whose floating-point non-buffer entries require gradients."""
  out = {}
  for k, v in params.items():
    v = v.clone()
    if v.dtype.is_floating_point:
      if dtype is not None:
        v = v.to(dtype)
      if "running" not in k:
        v.requires_grad_(True)
    out[k] = v
  return out


def _warm(params, forward, n=10):
  """Running statistics warmed by n train-mode forwards of the oracle (in place, like nn.BatchNorm2d)."""
  with torch.no_grad():
    for _ in range(n):
      forward(params)
  for k, v in params.items():
    if k.endswith("running_mean"):
      assert bool((v != 0).all()), k


def _relu_keep_fractions(fn):
  """Share of positive inputs of every F.relu the oracle calls inside fn()."""
  import torch.nn.functional as F
  orig, seen = F.relu, []

  def spy(x, *a, **k):
    seen.append(float((x > 0).float().mean()))
    return orig(x, *a, **k)
  F.relu = spy
  try:
    fn()
  finally:
    F.relu = orig
  return seen


def _buffers(net):
  return {k: v.detach().clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}


def _assert_buffers_untouched(net, before):
  after = _buffers(net)
  for k in before:
    assert torch.equal(before[k], after[k]), "%s changed in a backward on running statistics" % k


def _freeze_recipe(net):
  net.train()
  for m in net.modules():
    if isinstance(m, torch.nn.BatchNorm2d):
      m.eval()
  return net


def _fp32_gates(outs, refs, named_grads, ref_grads):
  """The gates of test_net5g_five_input_channels_fp32_mode_vs_oracle: outputs within 2e-4, every gradient norm within 1e-2."""
  for o, r in zip(outs, refs):
    assert (o.detach().cpu() - r.detach()).abs().max().item() <= 2e-4, (o.detach().cpu() - r.detach()).abs().max().item()
  for n, gr in named_grads:
    gn = float(ref_grads[n].double().norm())
    assert abs(float(gr.double().norm()) - gn) <= 1e-2 * max(gn, 1e-6) + 1e-9, (n, float(gr.double().norm()), gn)


# --------------------------------------------------------------------------------------
# ClusterNet5g in eval() and under the freeze recipe
# --------------------------------------------------------------------------------------
N5G = 12


@functools.lru_cache(maxsize=None)
def _net5g_case():
  """Parameters with warmed running statistics, the batch, the upstream gradients and the oracle's eval-mode step."""
  from oracle import net_oracle
  params = net_oracle.make_net5g_params(2, 10, 2, True, randomize_bn=True, head_std=0.3)
  imgs, _ = net_oracle.make_paired_batch(N5G, 32, 3, seed=9)
  x = net_oracle.sobel_process(imgs, False)
  assert tuple(x.shape) == (N5G, 2, 32, 32)
  _warm(params, lambda p: net_oracle.net5g_forward(p, x, True, 32, "head", 2))
  rng = np.random.default_rng(31)
  gsel = [torch.from_numpy(rng.standard_normal((N5G, 10)).astype(np.float32)) for _ in range(2)]
  rp = _grad_leaves(params)
  keep = _relu_keep_fractions(lambda: sum((o * g).sum() for o, g in zip(
    net_oracle.net5g_forward(rp, x, False, 32, "head", 2), gsel)).backward())
  assert len(keep) == 33 and 0.25 <= min(keep) and max(keep) <= 0.9, keep
  with torch.no_grad():
    ro = net_oracle.net5g_forward(params, x, False, 32, "head", 2)
  return params, x, gsel, ro, {k: v.grad for k, v in rp.items() if v.requires_grad}


@functools.lru_cache(maxsize=None)
def _net5g_runs():
  """{(recipe, path): (outputs, {name: grad})} for recipe in eval / freeze and path in fp32 / bf16, one net each."""
  from iic_amd import archs, ops
  params, x, gsel, _, _ = _net5g_case()
  cfg = types.SimpleNamespace(in_channels=2, input_sz=32, batchnorm_track=True, num_sub_heads=2, output_k=10)
  res = {}
  for recipe in ("eval", "freeze"):
    net = archs.ClusterNet5g(cfg)
    net.load_state_dict(params, strict=True)
    net.to(dev())
    if recipe == "eval":
      net.eval()
    else:
      _freeze_recipe(net)
    before = _buffers(net)
    for path in ("fp32", "bf16"):
      net.zero_grad()
      if path == "fp32":
        with ops.fp32_mode():
          outs = net(x.to(dev()))
      else:
        outs = net(x.to(dev()))
      sum((o * g.to(dev())).sum() for o, g in zip(outs, gsel)).backward()
      torch.cuda.synchronize()
      _assert_buffers_untouched(net, before)
      res[(recipe, path)] = ([o.detach().cpu() for o in outs], {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()})
  return res


def test_net5g_eval_mode_step_fp32_mode_vs_oracle():
  """net.eval(); loss.backward() on the exact-fp32 kernels against net_oracle.net5g_forward(training=False): outputs within
  2e-4, every parameter's gradient norm within 1e-2; running statistics and num_batches_tracked bit-identical before and
  after (asserted in _net5g_runs)."""
  _, _, _, ro, rgrads = _net5g_case()
  outs, grads = _net5g_runs()[("eval", "fp32")]
  assert set(grads) == set(rgrads)
  _fp32_gates(outs, ro, sorted(grads.items()), rgrads)


def test_net5g_eval_mode_step_bf16():
  """The same step on the bf16 path: finite gradients, outputs inside the bf16 aggregates of the training-mode test."""
  _, _, _, ro, rgrads = _net5g_case()
  outs, grads = _net5g_runs()[("eval", "bf16")]
  for o, r in zip(outs, ro):
    d = (o - r).abs()
    assert d.mean().item() <= 3e-2, d.mean().item()
    assert (o.argmax(1) == r.argmax(1)).float().mean().item() >= 0.75
  assert all(bool(torch.isfinite(g).all()) for g in grads.values())
  assert all(float(g.norm()) > 0 for n, g in grads.items() if float(rgrads[n].norm()) > 0)


@pytest.mark.parametrize("path", ["fp32", "bf16"])
def test_net5g_freeze_recipe_equals_eval_mode_bit_for_bit(path):
  """net.train() followed by .eval() on every BatchNorm2d: outputs and gradients bit-identical to the net.eval() run."""
  runs = _net5g_runs()
  (oe, ge), (of, gf) = runs[("eval", path)], runs[("freeze", path)]
  assert all(torch.equal(a, b) for a, b in zip(oe, of))
  for n in ge:
    assert torch.equal(ge[n], gf[n]), n


# --------------------------------------------------------------------------------------
# single blocks
# --------------------------------------------------------------------------------------
def _randomize_running(params, rng):
  for k in params:
    if k.endswith("running_mean"):
      params[k] = torch.from_numpy((0.3 * rng.standard_normal(tuple(params[k].shape))).astype(np.float32))
    elif k.endswith("running_var"):
      params[k] = torch.from_numpy(rng.uniform(0.5, 1.5, tuple(params[k].shape)).astype(np.float32))


def _block(pre, full, cin, planes, stride):
  import torch.nn as nn
  from iic_amd.archs.cluster import BasicBlock
  params = {k: v.clone() for k, v in full.items() if k.startswith(pre + ".")}
  ds = None
  if (pre + ".downsample.0.weight") in params:
    ds = nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
  blk = BasicBlock(cin, planes, stride, ds, track_running_stats=True)
  blk.load_state_dict({k[len(pre) + 1:]: v for k, v in params.items()}, strict=True)
  return blk.to(dev()), params


@pytest.mark.parametrize("layer,bidx,cin,planes,stride,H", [(1, 0, 64, 64, 1, 17), (2, 0, 64, 128, 2, 17)])
def test_basic_block_teacher_forced_on_running_statistics(layer, bidx, cin, planes, stride, H):
  """One BasicBlock in eval() (forward + backward) against net_oracle.block_bf16emu(training=False) on the same input and
  upstream gradient, with the tolerances of test_basic_block_teacher_forced: a stride-1 block and a stride-2 block whose
  bn2 and downsample BatchNorm share one launch."""
  from iic_amd import ops
  from oracle import net_oracle
  N = 8
  rng = np.random.default_rng(layer * 10 + bidx)
  pre = "trunk.layer%d.%d" % (layer, bidx)
  full = net_oracle.make_net5g_params(2, 10, 2, True, seed=3, randomize_bn=True)
  _randomize_running(full, rng)
  blk, params = _block(pre, full, cin, planes, stride)
  blk.eval()
  before = _buffers(blk)
  x = torch.from_numpy(rng.standard_normal((N, cin, H, H)).astype(np.float32)).relu().to(BF16).float()
  Ho = (H + 2 - 3) // stride + 1
  dout = torch.from_numpy(rng.standard_normal((N, planes, Ho, Ho)).astype(np.float32)).to(BF16).float()
  params = _grad_leaves(params)
  xe = x.clone().requires_grad_(True)
  oe = net_oracle.block_bf16emu(params, pre, xe, stride, False)
  oe.backward(dout)
  xp = ops.pt_from_nchw(x.to(dev()), 1).requires_grad_(True)
  o = blk(xp)
  o.backward(ops.pt_from_nchw(dout.to(dev()), 1))
  torch.cuda.synchronize()
  _assert_buffers_untouched(blk, before)
  got = ops.pt_to_nchw(o.detach(), 1).cpu()
  scale = float(oe.detach().abs().max())
  assert float((got - oe.detach()).abs().max()) <= 2e-2 * scale
  assert float((got - oe.detach()).abs().mean()) <= 2e-3 * scale
  gx = ops.pt_to_nchw(xp.grad, 1).cpu()
  assert _cos(gx, xe.grad) >= 0.999 and abs(float(gx.norm() / xe.grad.norm()) - 1) < 2e-2
  for n, p in blk.named_parameters():
    ref = params[pre + "." + n].grad
    c = _cos(p.grad.cpu(), ref)
    r = float(p.grad.norm().cpu() / ref.norm())
    assert c >= 0.998 and abs(r - 1) < 2e-2, (n, c, r)


def test_block_with_mixed_batchnorm_modes_fp32_mode_vs_float64():
  """bn1 frozen, bn2 on batch statistics, downsample BatchNorm frozen: every BatchNorm goes its own way (bn2 and the
  downsample BatchNorm are served separately).  Exact-fp32 kernels against a float64 composition of F.conv2d /
  F.batch_norm; outputs within 2e-4, every gradient norm (the input's included) within 1e-2; the batch-statistics layer
  updates its running statistics, the frozen ones do not."""
  import torch.nn.functional as F
  from iic_amd import ops
  from oracle import net_oracle
  N, cin, planes, stride, H = 6, 64, 128, 2, 9
  rng = np.random.default_rng(77)
  pre = "trunk.layer2.0"
  full = net_oracle.make_net5g_params(2, 10, 2, True, seed=3, randomize_bn=True)
  _randomize_running(full, rng)
  blk, params = _block(pre, full, cin, planes, stride)
  blk.train()
  blk.bn1.eval()
  blk.downsample[1].eval()
  before = _buffers(blk)
  x = torch.from_numpy(rng.standard_normal((N, cin, H, H)).astype(np.float32)).relu()
  Ho = (H + 2 - 3) // stride + 1
  dout = torch.from_numpy(rng.standard_normal((N, planes, Ho, Ho)).astype(np.float32))
  p64 = _grad_leaves(params, torch.float64)

  def bn(t, name, training):
    return F.batch_norm(t, p64[pre + name + ".running_mean"].clone(), p64[pre + name + ".running_var"].clone(),
                        p64[pre + name + ".weight"], p64[pre + name + ".bias"], training, 0.1, 1e-5)
  xe = x.double().requires_grad_(True)
  a1 = F.relu(bn(F.conv2d(xe, p64[pre + ".conv1.weight"], stride=stride, padding=1), ".bn1", False))
  o2 = bn(F.conv2d(a1, p64[pre + ".conv2.weight"], stride=1, padding=1), ".bn2", True)
  od = bn(F.conv2d(xe, p64[pre + ".downsample.0.weight"], stride=stride), ".downsample.1", False)
  oe = F.relu(o2 + od)
  keep = float((oe > 0).double().mean())
  assert 0.25 <= keep <= 0.9, keep
  oe.backward(dout.double())
  with ops.fp32_mode():
    xp = ops.pt_from_nchw(x.to(dev()), 1).requires_grad_(True)
    o = blk(xp)
    o.backward(ops.pt_from_nchw(dout.to(dev()), 1))
  torch.cuda.synchronize()
  assert xp.dtype == torch.float32 and o.dtype == torch.float32
  grads = [("input", ops.pt_to_nchw(xp.grad, 1).cpu())] + [(pre + "." + n, p.grad.cpu()) for n, p in blk.named_parameters()]
  refs = {k: v.grad for k, v in p64.items() if v.requires_grad}
  refs["input"] = xe.grad
  _fp32_gates([ops.pt_to_nchw(o.detach(), 1)], [oe.float()], grads, refs)
  after = _buffers(blk)
  for k in before:
    changed = not torch.equal(before[k], after[k])
    assert changed == k.startswith("bn2."), (k, changed)


def test_premasked_gradient_chain_matches_self_masking_blocks_on_running_statistics():
  """Frozen-mode twin of test_premasked_gradient_chain_matches_self_masking_blocks: who applies the ReLU mask of `out`
  (PREMASK) is independent of the BatchNorm mode -- the same three blocks under the freeze recipe, with and without the
  pre-masked chain, give the same features and gradients (fp32 accumulation order apart, that test's tolerances)."""
  from iic_amd import ops
  from iic_amd.archs import cluster as cl
  torch.manual_seed(3)
  d = dev()
  N, H = 6, 14
  ds = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 1, 2, bias=False),
                           torch.nn.BatchNorm2d(128, track_running_stats=True))
  blocks = [cl.BasicBlock(64, 64, track_running_stats=True),
            cl.BasicBlock(64, 128, 2, ds, track_running_stats=True),
            cl.BasicBlock(128, 128, track_running_stats=True)]
  for b in blocks:
    for m in b.modules():
      if isinstance(m, torch.nn.BatchNorm2d):
        m.weight.data.uniform_(0.5, 1.5)
        m.bias.data.normal_(0, 0.3)
        m.running_mean.normal_(0, 0.3)
        m.running_var.uniform_(0.5, 1.5)
    _freeze_recipe(b.to(d))
  x0 = torch.relu(torch.randn(N, 64, H, H))
  dfe = torch.randn(N, 128)
  res = {}
  for chain in (False, True):
    for b in blocks:
      b.zero_grad()
    x = ops.pt_from_nchw(x0.to(d), 1).requires_grad_(True)
    for i, b in enumerate(blocks):
      b._dout_premasked, b._mask_dx = chain, chain and i > 0
    try:
      h = x
      link = cl._Chain() if chain else None      # as the trunk's forward: no frozen BatchNorm may enter the fused chain
      for b in blocks:
        h = b(h, link)
      f = cl._AvgPoolFn.apply(h, chain)
    finally:
      for b in blocks:
        b._dout_premasked = b._mask_dx = False
    f.backward(dfe.to(d))
    torch.cuda.synchronize()
    res[chain] = (f.detach().clone(), x.grad.detach().float().clone(),
                  {n: p.grad.clone() for bi, b in enumerate(blocks) for n, p in
                   ((("%d.%s" % (bi, k)), v) for k, v in b.named_parameters())})
  f0, dx0, g0 = res[False]
  f1, dx1, g1 = res[True]
  assert torch.equal(f0, f1)
  assert (dx0 - dx1).abs().max().item() <= 2e-2 * dx0.abs().max().item()
  assert _cos(dx0, dx1) > 0.9999
  for n in g0:
    assert _cos(g0[n], g1[n]) > 0.9999, n
    assert abs(float(g1[n].norm() / g0[n].norm()) - 1) < 2e-3, n


# --------------------------------------------------------------------------------------
# VGG trunks: ClusterNet6c, SegmentationNet10a, single stages
# --------------------------------------------------------------------------------------
def _vgg_eval_step(make_net, params, x, oracle_forward):
  """fp32-mode eval() step against the oracle (gates of the fp32-mode step), then one finite bf16 step."""
  from iic_amd import ops
  _warm(params, lambda p: oracle_forward(p, x, True))
  rp = _grad_leaves(params)
  keep = []
  ro = None

  def ref_step():
    nonlocal ro
    ro = oracle_forward(rp, x, False)
    rng = np.random.default_rng(41)
    gs = [torch.from_numpy(rng.standard_normal(tuple(o.shape)).astype(np.float32)) for o in ro]
    sum((o * g).sum() for o, g in zip(ro, gs)).backward()
    return gs
  gsel = []
  keep = _relu_keep_fractions(lambda: gsel.extend(ref_step()))
  assert 0.25 <= min(keep) and max(keep) <= 0.9, keep
  net = make_net()
  net.load_state_dict(params, strict=True)
  net.to(dev()).eval()
  before = _buffers(net)
  with ops.fp32_mode():
    outs = net(x.to(dev()))
  sum((o * g.to(dev())).sum() for o, g in zip(outs, gsel)).backward()
  torch.cuda.synchronize()
  _fp32_gates(outs, ro, [(n, p.grad.cpu()) for n, p in net.named_parameters()],
              {k: v.grad for k, v in rp.items() if v.requires_grad})
  net.zero_grad()
  outs = net(x.to(dev()))              # bf16: the fused-pool stages are on this path
  sum((o * g.to(dev())).sum() for o, g in zip(outs, gsel)).backward()
  torch.cuda.synchronize()
  assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.norm()) > 0 for p in net.parameters())
  _assert_buffers_untouched(net, before)


def test_net6c_eval_mode_step_vs_oracle():
  """ClusterNet6c (24 x 24, 1 channel, 8 images) in eval(): _StageFn through VGGTrunkHIP, three pooled stages."""
  from iic_amd import archs
  from oracle import net_oracle
  cfg = types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, num_sub_heads=2, output_k=10)
  params = net_oracle.make_net6c_params(1, 24, 10, 2, True, seed=4, randomize_bn=True, head_std=0.05)
  x, _ = net_oracle.make_paired_batch(9, 24, 3, seed=6)
  _vgg_eval_step(lambda: archs.ClusterNet6c(cfg), params, x[:8].contiguous(),
                 lambda p, xx, tr: net_oracle.net6c_forward(p, xx, tr, "head", 2))


def test_net10a_eval_mode_step_vs_oracle():
  """SegmentationNet10a in eval() on the input of its existing GPU tests (2 x 4 x 24 x 24)."""
  import os
  from iic_amd import archs
  from oracle import net_oracle
  g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nets.npz"))
  cfg = types.SimpleNamespace(in_channels=4, input_sz=24, batchnorm_track=True, num_sub_heads=1, output_k=3)
  params = net_oracle.make_net10a_params(4, 3, 1, True, seed=5, randomize_bn=True)
  x = torch.from_numpy(g["net10a_in"])
  _vgg_eval_step(lambda: archs.SegmentationNet10a(cfg), params, x,
                 lambda p, xx, tr: net_oracle.net10a_forward(p, xx, 24, tr, "head", 1))


@pytest.mark.parametrize("idx,pool,cin,S", [(4, True, 64, 12), (12, False, 256, 3)])
def test_vgg_stage_teacher_forced_on_running_statistics(idx, pool, cin, S):
  """One conv-BN-ReLU(-pool) stage Function in eval() against net_oracle.vgg_stage_bf16emu(training=False), with the
  tolerances of test_vgg_stage_teacher_forced: a pooled stage (the fused pool backward feeds the one-pass kernel) and an
  unpooled one."""
  from iic_amd import archs, ops
  from iic_amd.archs.vgg import _StageFn
  from oracle import net_oracle
  N = 16
  cfg = types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, num_sub_heads=2, output_k=10)
  full = net_oracle.make_net6c_params(1, 24, 10, 2, True, seed=4, randomize_bn=True)
  rng = np.random.default_rng(idx)
  _randomize_running(full, rng)
  net = archs.ClusterNet6c(cfg)
  net.load_state_dict(full, strict=True)
  net.to(dev()).eval()
  before = _buffers(net)
  st = [s for s in net.trunk._stages if s.conv is net.trunk.features[idx]][0]
  x = torch.from_numpy(rng.standard_normal((N, cin, S, S)).astype(np.float32)).relu().to(BF16).float()
  keys = ("trunk.features.%d.weight" % idx, "trunk.features.%d.weight" % (idx + 1), "trunk.features.%d.bias" % (idx + 1))
  params = {k: v.clone() for k, v in full.items()}
  for k in keys:
    params[k].requires_grad_(True)
  xe = x.clone().requires_grad_(True)
  oe = net_oracle.vgg_stage_bf16emu(params, idx, xe, 2, 1, pool, False, False)
  dout = torch.from_numpy(rng.standard_normal(tuple(oe.shape)).astype(np.float32)).to(BF16).float()
  oe.backward(dout)
  xin = ops.pt_from_nchw(x.to(dev()), 2).requires_grad_(True)
  o = _StageFn.apply(xin, st.conv.weight, st.bn.weight, st.bn.bias, st)
  o.backward(ops.pt_from_nchw(dout.to(dev()), 2))
  torch.cuda.synchronize()
  _assert_buffers_untouched(net, before)
  got = ops.pt_to_nchw(o.detach(), 2).cpu()
  scale = float(oe.detach().abs().max())
  assert float((got - oe.detach()).abs().max()) <= 2e-2 * scale
  assert float((got - oe.detach()).abs().mean()) <= 2e-3 * scale
  assert _cos(ops.pt_to_nchw(xin.grad, 2).cpu(), xe.grad) >= 0.999
  for p_, key in zip((st.conv.weight, st.bn.weight, st.bn.bias), keys):
    c = _cos(p_.grad.cpu(), params[key].grad)
    r = float(p_.grad.norm().cpu() / params[key].grad.norm())
    assert c >= 0.998 and abs(r - 1) < 2e-2, (key, c, r)


# --------------------------------------------------------------------------------------
# graph replay
# --------------------------------------------------------------------------------------
def test_graphed_wrapper_runs_a_net_with_frozen_batchnorm_eagerly():
  """iic_amd.graphed: a module with a frozen BatchNorm is not eligible for graph replay.  Six optimiser steps under the
  freeze recipe, past the wrapper's warm-up count, with and without GRAPH_FORWARD: nothing is captured, and losses, final
  gradients and parameters are bit-identical."""
  from iic_amd import archs, graphed, ops
  from iic_amd.losses import IID_loss
  from iic_amd.optim import Adam
  from iic_amd.transforms import sobel_process
  steps = 6
  assert steps > graphed.WARMUP + 1
  cfg = types.SimpleNamespace(in_channels=2, input_sz=32, batchnorm_track=True, num_sub_heads=2, output_k=10)
  g = torch.Generator().manual_seed(1)
  base = torch.rand(4, 1, 32, 32, generator=g)
  imgs = base.repeat(3, 1, 1, 1).to(dev())
  imgs_tf = (torch.flip(imgs, dims=[3]) * 0.9 + 0.03).clamp(0, 1)
  res = []
  prev = ops.GRAPH_FORWARD[0]
  try:
    for graph in (False, True):
      torch.manual_seed(0)
      net = archs.ClusterNet5g(cfg).to(dev())
      with torch.no_grad():
        for m in net.modules():
          if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
      _freeze_recipe(net)
      assert graphed._any_frozen_bn(net)
      opt = Adam(net.parameters(), lr=1e-3)
      ops.GRAPH_FORWARD[0] = graph
      losses = []
      for _ in range(steps):
        net.zero_grad()
        xo, xt = net(sobel_process(imgs, False)), net(sobel_process(imgs_tf, False))
        avg = sum(IID_loss(xo[i], xt[i], lamb=1.0)[0] for i in range(2)) / 2
        losses.append(avg.item())
        avg.backward()
        opt.step()
      torch.cuda.synchronize()
      assert len(net.__dict__.get("_iic_graphed", {"graphs": {}})["graphs"]) == 0, "a forward was captured"
      res.append((losses, [p.grad.detach().clone() for p in net.parameters()], [p.detach().clone() for p in net.parameters()]))
      # the same net back on batch statistics is eligible again
      net.train()
      assert not graphed._any_frozen_bn(net)
  finally:
    ops.GRAPH_FORWARD[0] = prev
    ops.join()
  assert res[0][0] == res[1][0], (res[0][0], res[1][0])
  for a, b in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
    assert torch.equal(a, b)
