"""The triplets baseline on the device (csrc/triplets.hip, iic_amd/triplets.py, iic_amd/archs/triplets.py) against the
float64 closed form and the derived bounds of tests/triplets_cases.py, and the nets against the CPU restatement of the
reference (oracle/net_oracle.py).

Entry points: iic_triplets_loss (loss_and_grads, triplets_loss) and the host-side queries iic_triplets_supported /
iic_triplets_workspace_bytes (supported, workspace_bytes).  tests/test_triplets_cpu.py proves the bounds without a GPU."""
import types

import numpy as np
import pytest
import torch

from tests import triplets_cases as tc
from tests.parity import assert_bits

pytestmark = pytest.mark.gpu
KEYS = ("loss", "d_a", "d_b", "d_c")


def dev():
  return torch.device("cuda:0")


def _run(a, b, c, grads="all"):
  from iic_amd import triplets
  out = triplets.loss_and_grads(a, b, c, grads)
  torch.cuda.synchronize()
  return dict(zip(KEYS, out))


def _device_inputs(case):
  """The case's logits on the device; the strided case as [N, k] views of [N, STRIDED_LD] buffers whose padding holds
  a value that must never reach a result."""
  ts = tc.inputs(case)
  if case.name != "strided":
    return [t.to(dev()) for t in ts]
  views = []
  for t in ts:
    wide = torch.full((case.N, tc.STRIDED_LD), 1e30, device=dev())
    wide[:, :case.k] = t.to(dev())
    views.append(wide[:, :case.k])
    assert views[-1].stride(0) == tc.STRIDED_LD
  return views


def _assert_inside(got, r, tol, what):
  for key in KEYS:
    w = tc.worst(got[key].cpu(), r[key], tol[key])
    print("%s %s: worst |err| / bound = %.3f" % (what, key, w))
  for key in KEYS:
    assert tc.outside(got[key].cpu(), r[key], tol[key]) == 0, (what, key, tc.worst(got[key].cpu(), r[key], tol[key]))


# ---- the kernel on every case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_loss_and_gradients_inside_the_derived_bounds(case):
  from iic_amd import triplets
  assert triplets.supported(case.N, case.k) and triplets.workspace_bytes(case.N, case.k) > 0
  a, b, c = _device_inputs(case)
  got = _run(a, b, c)
  assert all(got[key].dtype == torch.float32 for key in KEYS) and got["loss"].dim() == 0
  assert all(got[key].shape == (case.N, case.k) and got[key].is_contiguous() for key in KEYS[1:])
  _assert_inside(got, tc.refs(case), tc.case_bounds(case), case.name)
  # targets as constants: the same loss and d_a, bit for bit; loss only: the same loss
  orig = _run(a, b, c, "orig")
  assert orig["d_b"] is None and orig["d_c"] is None
  assert_bits(orig["loss"], got["loss"], "loss (detached targets)")
  assert_bits(orig["d_a"], got["d_a"], "d_a (detached targets)")
  none = _run(a, b, c, "none")
  assert none["d_a"] is None
  assert_bits(none["loss"], got["loss"], "loss (loss only)")
  if case.name == "strided":
    dense = _run(a.contiguous(), b.contiguous(), c.contiguous())
    for key in KEYS:
      assert_bits(dense[key], got[key], key + " (strided view against its contiguous copy)")


def test_same_routine_properties_and_repeatability():
  case = tc.CASES[5]      # 5 x 65: two values in some lanes
  a, b, c = _device_inputs(case)
  got = _run(a, b, b.clone())
  assert float(got["loss"]) == 0.0
  assert torch.equal(got["d_a"], torch.zeros_like(got["d_a"]))
  assert torch.equal(got["d_b"], -got["d_c"])
  assert bool((got["d_b"] != 0).any())
  again, first = _run(a, b, c), _run(a, b, c)
  for key in KEYS:
    assert_bits(again[key], first[key], key + " (second call)")


def test_spread_1600_row_is_finite_and_inside_the_closed_forms_bound():
  a, b, c = tc.inputs(tc.HUGE_CASE)
  r = tc.closed64(a, b, c)
  got = _run(a.to(dev()), b.to(dev()), c.to(dev()))
  assert all(bool(torch.isfinite(got[key]).all()) for key in KEYS)
  _assert_inside(got, r, tc.bounds(a, b, c, r), tc.HUGE_CASE.name)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["orig", "pos", "neg"])
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["+inf", "-inf", "nan"])
def test_non_finite_inputs_against_float64_torch(which, value):
  case = tc.CASES[2]      # 3 x 10; row 1 carries the wide linspace, row 0 takes the bad value
  clean = [t.to(dev()) for t in tc.inputs(case)]
  base = _run(*clean)
  x = [t.clone() for t in tc.inputs(case)]
  x[which][0, 4] = value
  t_loss, t_da, t_db, t_dc = tc.autograd64(*x)
  got = _run(*[t.to(dev()) for t in x])
  assert bool(torch.isfinite(got["loss"])) == bool(torch.isfinite(t_loss)), (float(got["loss"]), float(t_loss))
  for key, ref in zip(KEYS[1:], (t_da, t_db, t_dc)):
    assert torch.equal(got[key][1:], base[key][1:]), key      # rows with finite inputs: untouched by the bad row
    bad = ~torch.isfinite(ref[0])
    assert not bool(torch.isfinite(got[key][0].cpu()[bad]).any()), key


def test_unsupported_shapes_and_cpu_tensors_raise_before_a_launch():
  from iic_amd import _lib, triplets
  assert not triplets.supported(2, 1025) and triplets.workspace_bytes(2, 1025) == 0
  x = torch.zeros((2, 1025), device=dev())
  with pytest.raises(ValueError, match="served range"):
    triplets.triplets_loss(x, x, x)
  # the entry point itself answers IIC_ERR_UNSUPPORTED (-3) with nothing enqueued
  out = torch.full((1,), 7.0, device=dev())
  ws = torch.zeros(4096, dtype=torch.uint8, device=dev())
  rc = _lib.lib().iic_triplets_loss(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1025, 2, 1025, out.data_ptr(), None, None,
                                    None, ws.data_ptr(), _lib.stream_ptr())
  torch.cuda.synchronize()
  assert rc == -3 and float(out) == 7.0
  # d_b without d_c, gradients of the targets without d_a, ld < k: IIC_ERR_ARG (-1)
  y = torch.zeros((2, 8), device=dev())
  g = torch.zeros((2, 8), device=dev())
  L = _lib.lib()
  args = (y.data_ptr(), y.data_ptr(), y.data_ptr())
  assert L.iic_triplets_loss(*args, 8, 2, 8, out.data_ptr(), g.data_ptr(), g.data_ptr(), None, ws.data_ptr(), _lib.stream_ptr()) == -1
  assert L.iic_triplets_loss(*args, 8, 2, 8, out.data_ptr(), None, g.data_ptr(), g.data_ptr(), ws.data_ptr(), _lib.stream_ptr()) == -1
  assert L.iic_triplets_loss(*args, 7, 2, 8, out.data_ptr(), None, None, None, ws.data_ptr(), _lib.stream_ptr()) == -1
  with pytest.raises(ValueError, match="no CPU fallback"):
    triplets.triplets_loss(torch.zeros((2, 8)), torch.zeros((2, 8)), torch.zeros((2, 8)))


def test_triplets_loss_autograd_scales_by_the_upstream_factor():
  from iic_amd import triplets
  case = tc.CASES[3]
  a, b, c = [t.to(dev()).requires_grad_(True) for t in tc.inputs(case)]
  kernel = _run(a, b, c)
  loss = triplets.triplets_loss(a, b, c)
  assert_bits(loss.detach(), kernel["loss"], "loss")
  (loss * 0.5).backward()
  torch.cuda.synchronize()
  # the product with 0.5 is exact in fp32 except on a subnormal gradient (the wide row has some: p near exp(-160)),
  # where it rounds to the subnormal spacing
  for t, key in ((a, "d_a"), (b, "d_b"), (c, "d_c")):
    want = 0.5 * kernel[key].double()
    err = (t.grad.double() - want).abs()
    print("%s: max |grad - kernel / 2| = %.3g" % (key, float(err.max())))
    assert bool((err <= tc.U32 * want.abs() + tc.subnormal_term()).all()), key
  # targets detached: no gradient reaches pos / neg, orig's is the same; no_grad: the loss alone
  a2, b2, c2 = [t.detach().clone().requires_grad_(True) for t in (a, b, c)]
  triplets.triplets_loss(a2, b2, c2, detach_targets=True).backward()
  assert b2.grad is None and c2.grad is None
  assert_bits(a2.grad, kernel["d_a"], "d_a (detach_targets)")
  with torch.no_grad():
    assert_bits(triplets.triplets_loss(a, b, c), kernel["loss"], "loss under no_grad")


# ---- the nets: one whole triplet step against the CPU restatement of the reference -------------------------------------
def _renamed(params):
  out = {}
  for key, v in params.items():
    out[key.replace("head.heads.0.0.", "head.head.")] = v
  return out


def _oracle_step(params, trunk, batches):
  """CPU fp32 autograd: trunk -> flatten -> linear three times (orig, pos, neg, in this order: the running statistics
  are updated in it), then the closed-form loss."""
  rp = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
        for k, v in params.items()}
  logits = []
  for x in batches:
    f = trunk(rp, x)
    logits.append(torch.nn.functional.linear(f.reshape(f.size(0), -1), rp["head.head.weight"], rp["head.head.bias"]))
  loss = tc.closed64(*logits)["loss"]
  loss.backward()
  return rp, [l.detach() for l in logits], float(loss.detach())


def _check_step(net, rp, ref_logits, ref_loss, batches):
  """The whole step on the exact-fp32 kernels at the tolerances of test_net6c_input_sz_64_fp32_mode_vs_oracle (2e-4 on
  the outputs, here logits: scaled by max(1, max |logit_ref|); 5e-4 relative on the loss; 1e-2 of each gradient norm),
  then the bf16 path on the same batch: finite gradients, arg-max agreement >= 0.9."""
  from iic_amd import ops
  from iic_amd.triplets import triplets_loss
  with ops.fp32_mode():
    outs = [net(x.to(dev())) for x in batches]
    loss = triplets_loss(*outs)
    loss.backward()
  torch.cuda.synchronize()
  assert all(torch.is_tensor(o) and o.dim() == 2 for o in outs)
  for o, r in zip(outs, ref_logits):
    d = (o.detach().cpu() - r).abs().max().item()
    scale = max(1.0, r.abs().max().item())
    print("max |logit - ref| = %.3e (scale %.3f)" % (d, scale))
    assert d <= 2e-4 * scale, (d, scale)
  print("loss %.8e, reference %.8e" % (float(loss.detach()), ref_loss))
  assert abs(float(loss.detach()) - ref_loss) <= 5e-4 * abs(ref_loss) + 1e-7, (float(loss.detach()), ref_loss)
  for n, p in net.named_parameters():
    gn = float(rp[n].grad.double().norm())
    assert abs(float(p.grad.double().norm()) - gn) <= 1e-2 * max(gn, 1e-6) + 1e-9, (n, float(p.grad.double().norm()), gn)
  net.zero_grad()
  outs = [net(x.to(dev())) for x in batches]
  triplets_loss(*outs).backward()
  torch.cuda.synchronize()
  assert all(torch.isfinite(p.grad).all() for p in net.parameters())
  for o, r in zip(outs, ref_logits):
    assert (o.detach().cpu().argmax(1) == r.argmax(1)).float().mean().item() >= 0.9


def test_triplets_net6c_step_vs_oracle():
  from iic_amd import archs
  from oracle import net_oracle
  cfg = types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, output_k=10)
  params = _renamed(net_oracle.make_net6c_params(1, 24, 10, num_sub_heads=1, batchnorm_track=True, seed=9,
                                                 randomize_bn=True, head_std=0.05))
  x, xt = net_oracle.make_paired_batch(12, 24, 3, seed=10)
  batches = [x, xt, x.roll(1, 0).contiguous()]      # orig, pos, neg: other images in the negative's rows
  rp, ref_logits, ref_loss = _oracle_step(
    params, lambda p, im: net_oracle.vgg_trunk(p, im, net_oracle.NET6C_CFG, 5, 2, True), batches)
  net = archs.TripletsNet6c(cfg)
  net.load_state_dict(params, strict=True)
  net.to(dev()).train()
  _check_step(net, rp, ref_logits, ref_loss, batches)


def test_triplets_net5g_step_vs_oracle():
  from iic_amd import archs
  from oracle import net_oracle
  cfg = types.SimpleNamespace(in_channels=2, input_sz=32, batchnorm_track=True, output_k=10)
  params = _renamed(net_oracle.make_net5g_params(2, 10, num_sub_heads=1, batchnorm_track=True, seed=11,
                                                 randomize_bn=True, head_std=0.05))
  x, xt = net_oracle.make_paired_batch(6, 32, 3, seed=12)
  batches = [net_oracle.sobel_process(t, False) for t in (x, xt, x.roll(1, 0).contiguous())]
  rp, ref_logits, ref_loss = _oracle_step(params, lambda p, im: net_oracle.net5g_trunk(p, im, True, 32), batches)
  net = archs.TripletsNet5g(cfg)
  net.load_state_dict(params, strict=True)
  net.to(dev()).train()
  _check_step(net, rp, ref_logits, ref_loss, batches)


def _small_net6c(output_k=4, seed=3):
  from iic_amd import archs
  torch.manual_seed(seed)
  net = archs.TripletsNet6c(types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, output_k=output_k))
  with torch.no_grad():
    net.head.head.weight.normal_(0, 0.05)
  return net


def test_three_forwards_never_fork_or_postpone_under_auto_branch():
  from iic_amd import branches
  from iic_amd.triplets import triplets_loss
  from oracle import net_oracle
  x, xt = net_oracle.make_paired_batch(6, 24, 3, seed=14)
  batches = [t.to(dev()) for t in (x, xt, x.roll(1, 0).contiguous())]
  state = _small_net6c(10).state_dict()

  def step(switch):
    from iic_amd import archs
    net = archs.TripletsNet6c(types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, output_k=10))
    net.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    net.to(dev()).train()
    prev = branches.AUTO_BRANCH[0]
    branches.AUTO_BRANCH[0] = switch
    try:
      outs = []
      for b in batches:
        outs.append(net(b))
        c = branches.context()
        assert c.solo_first == 0 and not c.pending_join and not c.deferred_running and c.branch == 0
      triplets_loss(*outs).backward()
      c = branches.context()
      assert c.solo_first == 0 and not c.pending_join and not c.deferred_running
    finally:
      branches.AUTO_BRANCH[0] = prev
    torch.cuda.synchronize()
    return net
  off, on = step(False), step(True)
  bufs = dict(off.named_buffers())
  assert any(k.endswith("running_mean") for k in bufs)
  for k, v in on.named_buffers():
    assert torch.equal(v, bufs[k]), k
  assert int(on.trunk.features[1].num_batches_tracked) == 3


# ---- evaluation twins --------------------------------------------------------------------------------------------------
class _GivenLogits(torch.nn.Module):
  """A net that answers the i-th call with the i-th given logits (on the device)."""

  def __init__(self, logits):
    super(_GivenLogits, self).__init__()
    self.logits, self.i = [torch.from_numpy(l).to(dev()) for l in logits], 0

  def forward(self, x, kmeans_use_features=False):
    assert not kmeans_use_features      # the reference's triplets evaluation calls net(imgs)
    out = self.logits[self.i % len(self.logits)]
    self.i += 1
    return out


def _config(output_k, gt_k, kmeans_on_features):
  return types.SimpleNamespace(output_k=output_k, gt_k=gt_k, batch_sz=8, include_rgb=False,
                               kmeans_on_features=kmeans_on_features, epoch_acc=[], masses=None, per_class_acc=None)


def test_triplets_get_data_breaks_ties_to_the_lowest_index():
  from iic_amd import triplets
  logits, targets = tc.eval_batches(gt_k=4, sizes=(8, 8, 5))
  loader = [(torch.zeros((len(t), 1, 24, 24)), torch.from_numpy(t)) for t in targets]
  preds, tg = triplets.triplets_get_data(_config(4, 4, False), _GivenLogits(logits), loader, sobel=False)
  assert preds.is_cuda and preds.dtype == torch.int32 and tg.dtype == torch.int32 and preds.shape == (21,)
  want = np.argmax(np.concatenate(logits, 0), axis=1)
  assert want[3] == 1 and logits[0][3, 1] == logits[0][3, 3]
  assert np.array_equal(preds.cpu().numpy(), want)
  assert np.array_equal(tg.cpu().numpy(), np.concatenate(targets))


def _image_batches(sizes=(8, 8, 5), gt_k=4, seed=6):
  rng = np.random.default_rng([33, seed])
  return [(torch.from_numpy(rng.random((n, 1, 24, 24)).astype(np.float32)),
           torch.from_numpy(rng.integers(0, gt_k, n).astype(np.int64))) for n in sizes]


def test_eval_twins_on_a_real_net_argmax_branch():
  from iic_amd import triplets
  gt_k = 4
  net = _small_net6c(gt_k).to(dev()).train()
  loader = _image_batches(gt_k=gt_k)
  targets = np.concatenate([b[1].numpy() for b in loader])
  net.eval()
  with torch.no_grad():
    logits = torch.cat([net(b[0].to(dev())).clone() for b in loader], 0)
  net.train()
  assert logits.shape == (21, gt_k)
  want = np.argmax(logits.cpu().numpy(), axis=1)
  config = _config(gt_k, gt_k, False)
  net.eval()
  preds, tg = triplets.triplets_get_data(config, net, loader, sobel=False)
  net.train()
  assert np.array_equal(preds.cpu().numpy(), want) and np.array_equal(tg.cpu().numpy(), targets)
  assert triplets.triplets_eval(config, net, loader, sobel=False) is False
  assert net.training
  acc, mass, pca = tc.eval_np(want, targets, gt_k)
  assert config.epoch_acc == [acc]
  assert np.array_equal(config.masses, mass) and np.array_equal(config.per_class_acc, pca)
  # the same pass again is no better than itself
  assert triplets.triplets_eval(config, net, loader, sobel=False) is False
  assert config.masses.shape == (2, gt_k) and config.epoch_acc == [acc, acc]


def test_eval_twins_on_a_real_net_kmeans_branch():
  from iic_amd import kmeans, triplets
  gt_k, output_k = 4, 10
  net = _small_net6c(output_k).to(dev()).train()
  loader = _image_batches(gt_k=gt_k, seed=7)
  targets = np.concatenate([b[1].numpy() for b in loader])
  net.eval()
  with torch.no_grad():
    logits = torch.cat([net(b[0].to(dev())).clone() for b in loader], 0)
  net.train()
  assert logits.shape == (21, output_k)
  want = kmeans.KMeans(n_clusters=gt_k).fit(logits.contiguous()).labels_.cpu().numpy()
  config = _config(output_k, gt_k, True)
  net.eval()
  preds, tg = triplets.triplets_get_data_kmeans_on_features(config, net, loader, sobel=False)
  net.train()
  assert preds.shape == (21,) and int(preds.max()) < gt_k
  assert np.array_equal(preds.cpu().numpy(), want) and np.array_equal(tg.cpu().numpy(), targets)
  assert triplets.triplets_eval(config, net, loader, sobel=False) is False
  assert net.training
  acc, mass, pca = tc.eval_np(want, targets, gt_k)
  assert config.epoch_acc == [acc]
  assert np.array_equal(config.masses, mass) and np.array_equal(config.per_class_acc, pca)


# ---- training batches --------------------------------------------------------------------------------------------------
def test_triplet_batches():
  from iic_amd import augment, triplets
  rng = np.random.default_rng(35)
  imgs = torch.from_numpy(rng.integers(0, 256, (11, 32, 32, 3)).astype(np.uint8)).to(dev())

  def epoch(seed):
    aug = augment.PairedAugmenter(imgs, 20, 24, False, seed=5)
    calls = []
    plain, jittered = aug.plain, aug.jittered
    aug.plain = lambda idx: (calls.append(("plain", np.asarray(idx).copy())), plain(idx))[1]
    aug.jittered = lambda idx: (calls.append(("jittered", np.asarray(idx).copy())), jittered(idx))[1]
    return list(triplets.triplet_batches(aug, 4, seed)), calls
  batches, calls = epoch(3)
  assert [b[0].shape[0] for b in batches] == [4, 4, 3]      # the ragged tail
  for orig, pos, neg in batches:
    assert orig.shape == pos.shape == neg.shape and orig.shape[1:] == (1, 24, 24) and orig.is_cuda
  assert [c[0] for c in calls] == ["plain", "jittered", "plain"] * 3
  for i in range(3):
    o, p, n = calls[3 * i:3 * i + 3]
    assert np.array_equal(o[1], p[1])                          # pos: the same samples as orig
    assert np.array_equal(o[1], np.arange(4 * i, min(11, 4 * i + 4)))      # in dataset order
  neg_idx = np.concatenate([calls[3 * i + 2][1] for i in range(3)])
  assert np.array_equal(np.sort(neg_idx), np.arange(11)) and not np.array_equal(neg_idx, np.arange(11))
  again, _ = epoch(3)
  for b0, b1 in zip(batches, again):
    assert all(torch.equal(u, v) for u, v in zip(b0, b1))
  other, calls2 = epoch(4)
  assert not np.array_equal(np.concatenate([calls2[3 * i + 2][1] for i in range(3)]), neg_idx)
