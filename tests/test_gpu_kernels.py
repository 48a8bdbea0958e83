"""Per-kernel parity of the HIP path (through the C ABI) against the CPU oracle / plain
fp32 torch-CPU references on seeded inputs.  Needs a real MI355X:  pytest -m gpu.

Tolerances
  * fp32 kernels (IID loss, heads, stem statistics, Adam, sobel): the north-star clause
    |ours - ref| <= 1e-5*|ref64| + 2e-7 for the loss, ||dg||/||g|| <= 1e-5 for its grads.
  * bf16-operand MFMA convs: compared with an fp32 reference fed the SAME bf16-rounded
    operands; what remains is fp32 accumulation order + the bf16 rounding of the stored
    output (rel 2^-9), so |d| <= 1e-2*max|ref| is generous and catches any indexing bug.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


def bf16_round(t):
  return t.to(torch.bfloat16).float()


# --------------------------------------------------------------------------------------
def test_library_loaded_and_probe_tr16():
  from iic_amd import _lib
  L = _lib.lib()
  assert L.iic_version() >= 1
  out = torch.zeros(256, dtype=torch.int16, device=dev())
  _lib.check(L.iic_probe_tr16(out.data_ptr(), _lib.stream_ptr()))
  torch.cuda.synchronize()
  got = out.cpu().numpy().astype(np.int64).reshape(64, 4)
  l = np.arange(64)[:, None]
  j = np.arange(4)[None, :]
  want = (l & 15) + j * 16 + (l >> 4) * 64
  os.makedirs("gpurun_out", exist_ok=True)
  np.savetxt("gpurun_out/probe_tr16.txt", got, fmt="%d")
  assert np.array_equal(got, want), "ds_read_b64_tr_b16 mapping differs from the model:\n%s" % got


# --------------------------------------------------------------------------------------
# IID loss
# --------------------------------------------------------------------------------------
def _iid_tol(ref64):
  return 1e-5 * abs(ref64) + 2e-7


def test_iid_loss_golden_cases():
  from iic_amd.losses import IID_loss
  from oracle import iid_oracle
  from oracle.gen_golden import IID_CASES
  g = np.load(os.path.join(G, "iid_loss.npz"), allow_pickle=True)
  for ci, (bn, k, kind, lamb, seed) in enumerate(IID_CASES):
    z, zt = iid_oracle.make_softmax_pair(bn, k, kind, seed)
    a = torch.from_numpy(z).to(dev()).requires_grad_(True)
    b = torch.from_numpy(zt).to(dev()).requires_grad_(True)
    loss, loss_nl = IID_loss(a, b, lamb=lamb)
    loss.backward()
    ref64 = g["c%d_loss_f64" % ci]
    assert abs(loss.item() - ref64[0]) <= _iid_tol(ref64[0]), (ci, loss.item(), ref64[0])
    assert abs(loss_nl.item() - ref64[1]) <= _iid_tol(ref64[1]), (ci, loss_nl.item(), ref64[1])
    for t, key in ((a, "dz"), (b, "dzt")):
      gref = g["c%d_%s_f64" % (ci, key)]
      nrm = max(np.linalg.norm(gref), 1e-30)
      err = np.linalg.norm(t.grad.cpu().numpy().astype(np.float64) - gref) / nrm
      # 1e-5 relative, or -- when MI ~ 0 and the gradient itself is cancellation noise --
      # at least as accurate as the reference's own fp32 autograd is w.r.t. float64
      ref32_err = np.linalg.norm(g["c%d_%s_f32" % (ci, key)].astype(np.float64) - gref) / nrm
      assert err <= max(1e-5, ref32_err), (ci, key, err, ref32_err)


def test_iid_loss_packed_heads_full_size_and_no_lamb_grad():
  """5 sub-heads x 660 x 70 in 3 launches; gradient through BOTH outputs."""
  from iic_amd.losses import IID_loss_heads
  from oracle import iid_oracle
  H, bn, k = 5, 660, 70
  zs, zts = [], []
  for h in range(H):
    z, zt = iid_oracle.make_softmax_pair(bn, k, "trained" if h % 2 == 0 else "init", 100 + h)
    zs.append(z)
    zts.append(zt)
  Z = torch.from_numpy(np.stack(zs, 1)).to(dev()).requires_grad_(True)      # [bn, H, k]
  ZT = torch.from_numpy(np.stack(zts, 1)).to(dev()).requires_grad_(True)
  loss, loss_nl = IID_loss_heads(Z, ZT, lamb=1.5)
  w1 = torch.tensor([1.0, 0.5, -2.0, 0.0, 3.0], device=dev())
  w2 = torch.tensor([0.0, 1.0, 0.25, -1.0, 0.0], device=dev())
  ((loss * w1).sum() + (loss_nl * w2).sum()).backward()
  for h in range(H):
    l, lnl, dz, dzt = iid_oracle.iid_loss_np(zs[h], zts[h], 1.5, float(w1[h]), float(w2[h]))
    assert abs(loss[h].item() - l) <= _iid_tol(l)
    assert abs(loss_nl[h].item() - lnl) <= _iid_tol(lnl)
    # the fp32 reference restatement (torch autograd) on the same inputs: our error w.r.t.
    # float64 must be <= 1e-5 or no worse than the fp32 reference's own error (MI ~ 0 heads)
    a32 = torch.from_numpy(zs[h]).requires_grad_(True)
    b32 = torch.from_numpy(zts[h]).requires_grad_(True)
    l32, lnl32 = iid_oracle.IID_loss(a32, b32, lamb=1.5)
    (float(w1[h]) * l32 + float(w2[h]) * lnl32).backward()
    for mine, ref, r32 in ((Z.grad[:, h].cpu().numpy(), dz, a32.grad.numpy()),
                           (ZT.grad[:, h].cpu().numpy(), dzt, b32.grad.numpy())):
      nrm = np.linalg.norm(ref)
      if nrm > 0:
        assert np.linalg.norm(mine - ref) / nrm <= max(1e-5, np.linalg.norm(r32 - ref) / nrm)


@pytest.mark.parametrize("k,bn", [(96, 300), (140, 700), (280, 700)])
def test_iid_loss_large_k_multi_block_path(k, bn):
  """Over-clustering heads (k = 280 at CIFAR-20, examples/commands.txt): k >= 96 takes the four-launch
  multi-block k x k stage (iid_loss.hip 2b) -- same float64 arithmetic as the one-block kernel, checked
  against the float64 oracle; at bn = 700 most of the k*k joint entries sit below EPS, so the clamp
  branches (IID_losses.py:17-19) are exercised too.  Two runs agree bit for bit."""
  from iic_amd.losses import IID_loss_heads
  from oracle import iid_oracle
  H = 3
  zs, zts = [], []
  for h in range(H):
    z, zt = iid_oracle.make_softmax_pair(bn, k, "trained" if h != 1 else "init", 300 + h)
    zs.append(z)
    zts.append(zt)
  w1 = [1.0, -0.5, 2.0]
  w2 = [0.25, 1.0, 0.0]

  def run():
    Z = torch.from_numpy(np.stack(zs, 1)).to(dev()).requires_grad_(True)
    ZT = torch.from_numpy(np.stack(zts, 1)).to(dev()).requires_grad_(True)
    loss, loss_nl = IID_loss_heads(Z, ZT, lamb=1.2)
    ((loss * torch.tensor(w1, device=dev())).sum() + (loss_nl * torch.tensor(w2, device=dev())).sum()).backward()
    return loss, loss_nl, Z.grad, ZT.grad
  loss, loss_nl, gz, gzt = run()
  loss_b, loss_nl_b, gz_b, gzt_b = run()
  assert torch.equal(loss, loss_b) and torch.equal(loss_nl, loss_nl_b)
  assert torch.equal(gz, gz_b) and torch.equal(gzt, gzt_b)
  for h in range(H):
    l, lnl, dz, dzt = iid_oracle.iid_loss_np(zs[h], zts[h], 1.2, w1[h], w2[h])
    assert abs(loss[h].item() - l) <= _iid_tol(l), (h, loss[h].item(), l)
    assert abs(loss_nl[h].item() - lnl) <= _iid_tol(lnl)
    a32 = torch.from_numpy(zs[h]).requires_grad_(True)
    b32 = torch.from_numpy(zts[h]).requires_grad_(True)
    l32, lnl32 = iid_oracle.IID_loss(a32, b32, lamb=1.2)
    (w1[h] * l32 + w2[h] * lnl32).backward()
    for mine, ref, r32 in ((gz[:, h].cpu().numpy(), dz, a32.grad.numpy()),
                           (gzt[:, h].cpu().numpy(), dzt, b32.grad.numpy())):
      nrm = np.linalg.norm(ref)
      assert nrm > 0
      assert np.linalg.norm(mine - ref) / nrm <= max(1e-5, np.linalg.norm(r32 - ref) / nrm)


def test_iid_loss_full_size_invariances():
  """Size-independent properties at the north-star size (660 x 70): the loss is symmetric in the two
  views (the joint is symmetrised, IID_losses.py:44), invariant to a permutation of the batch rows
  and to a common relabelling of the classes; the gradients transform accordingly."""
  from iic_amd.losses import IID_loss
  from oracle import iid_oracle
  bn, k = 660, 70
  z, zt = iid_oracle.make_softmax_pair(bn, k, "trained", 7)
  Z, ZT = torch.from_numpy(z).to(dev()), torch.from_numpy(zt).to(dev())

  def run(a, b):
    a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    l, ln = IID_loss(a, b, lamb=1.3)
    (l + 0.5 * ln).backward()
    return l.item(), ln.item(), a.grad, b.grad

  l0, n0, ga, gb = run(Z, ZT)
  tol = 1e-5 * abs(l0) + 2e-7
  # swap the views
  l1, n1, gb1, ga1 = run(ZT, Z)
  assert abs(l1 - l0) <= tol and abs(n1 - n0) <= tol
  assert float((ga1 - ga).norm() / ga.norm()) <= 1e-5 and float((gb1 - gb).norm() / gb.norm()) <= 1e-5
  # permute the batch rows
  perm = torch.randperm(bn, generator=torch.Generator().manual_seed(1)).to(dev())
  l2, n2, ga2, gb2 = run(Z[perm], ZT[perm])
  assert abs(l2 - l0) <= tol and abs(n2 - n0) <= tol
  assert float((ga2 - ga[perm]).norm() / ga.norm()) <= 1e-5
  # relabel the classes (same permutation in both views)
  cp = torch.randperm(k, generator=torch.Generator().manual_seed(2)).to(dev())
  l3, n3, ga3, gb3 = run(Z[:, cp].contiguous(), ZT[:, cp].contiguous())
  assert abs(l3 - l0) <= tol and abs(n3 - n0) <= tol
  assert float((gb3 - gb[:, cp]).norm() / gb.norm()) <= 1e-5


def test_iid_loss_analytic_pins_and_no_grad():
  from iic_amd.losses import IID_loss
  from oracle import iid_oracle
  for k in (5, 10):
    z, zt = iid_oracle.make_softmax_pair(10 * k, k, "onehot", 0)
    with torch.no_grad():
      l, lnl = IID_loss(torch.from_numpy(z).to(dev()), torch.from_numpy(zt).to(dev()))
    assert abs(l.item() + math.log(k)) < 1e-5 and abs(l.item() - lnl.item()) < 1e-7
    u = torch.full((30, k), 1.0 / k, device=dev())
    l, _ = IID_loss(u, u)
    assert abs(l.item()) < 2e-7
  # ragged last batch / odd sizes
  z, zt = iid_oracle.make_softmax_pair(333, 37, "trained", 9)
  l, _ = IID_loss(torch.from_numpy(z).to(dev()), torch.from_numpy(zt).to(dev()), lamb=1.0)
  ref, _, _, _ = iid_oracle.iid_loss_np(z, zt, 1.0)
  assert abs(l.item() - ref) <= _iid_tol(ref)


@pytest.mark.parametrize("bn,k,lamb", [(1, 2, 1.0), (2, 3, 1.0), (3, 2, 1.5), (5, 7, 0.5), (17, 4, 1.0), (64, 10, 1.5),
                                       (129, 33, 1.0), (700, 50, 1.0), (41, 280, 1.0)])
def test_iid_loss_small_ragged_and_strided_inputs_vs_oracle(bn, k, lamb):
  """Edge shapes of the drop-in boundary (IID_losses.py:6-47): a last batch of one or two rows, k = 2, lamb != 1, and
  NON-CONTIGUOUS inputs (row slices and the column-sliced views a packed head output hands to the per-sub-head calls) --
  loss, loss_no_lamb and both input gradients against the float64 oracle at the north-star tolerance."""
  from iic_amd.losses import IID_loss
  from oracle import iid_oracle
  z, zt = iid_oracle.make_softmax_pair(bn, k, "trained", 100 + bn + k)
  # strided views of larger buffers: every other row of a [2*bn, k] tensor, and a [bn, 3, k] pack's middle slice
  big = torch.zeros(2 * bn, k, device=dev())
  big[::2] = torch.from_numpy(z).to(dev())
  a = big[::2].detach().requires_grad_(True)
  pack = torch.zeros(bn, 3, k, device=dev())
  pack[:, 1, :] = torch.from_numpy(zt).to(dev())
  pack.requires_grad_(True)
  b = pack[:, 1, :]
  assert not b.is_contiguous() or bn == 1
  loss, loss_nl = IID_loss(a, b, lamb=lamb)
  (loss + 0.25 * loss_nl).backward()
  ref, ref_nl, dz, dzt = iid_oracle.iid_loss_np(z, zt, lamb, 1.0, 0.25)
  assert abs(loss.item() - ref) <= _iid_tol(ref), (loss.item(), ref)
  assert abs(loss_nl.item() - ref_nl) <= _iid_tol(ref_nl), (loss_nl.item(), ref_nl)
  ga = a.grad.cpu().numpy().astype(np.float64)
  gb = pack.grad[:, 1, :].cpu().numpy().astype(np.float64)
  for got, want in ((ga, dz), (gb, dzt)):
    nrm = max(np.linalg.norm(want), 1e-30)
    assert np.linalg.norm(got - want) / nrm <= 2e-5, np.linalg.norm(got - want) / nrm
  assert float(pack.grad[:, 0, :].abs().max()) == 0.0 and float(pack.grad[:, 2, :].abs().max()) == 0.0


# --------------------------------------------------------------------------------------
# conv: implicit GEMM forward / backward-data / backward-weight
# --------------------------------------------------------------------------------------
CONV_CASES = [  # cin, cout, K, stride, pad, N, H
  (64, 64, 3, 1, 1, 5, 13),     # M = 845: tail tile, BN = 64
  (64, 128, 3, 2, 1, 3, 25),    # stride 2, BN = 128
  (128, 128, 3, 1, 1, 4, 7),    # two channel chunks
  (64, 128, 1, 2, 0, 3, 13),    # 1x1 stride-2 downsample
  (256, 512, 3, 2, 1, 2, 13),   # 4 chunks
  (64, 64, 3, 1, 1, 2, 49),     # wide rows (layer1 geometry)
  (512, 512, 3, 1, 1, 6, 7),    # 8 chunks, 256-row tail tile (layer4 geometry)
  (128, 128, 3, 1, 1, 20, 25),  # many tiles (layer2 geometry)
  (64, 128, 3, 1, 1, 3, 30),    # SegmentationNet10a c2-like: the backward-data conv has 64 couts (64-cout tiles)
  (128, 64, 3, 1, 1, 2, 21),    # ... and a forward with 64 couts, two channel chunks, tail tile
]


def _conv_inputs(cin, cout, K, N, H, seed=0):
  rng = np.random.default_rng(seed)
  x = torch.from_numpy(rng.standard_normal((N, cin, H, H)).astype(np.float32))
  w = torch.from_numpy((rng.standard_normal((cout, cin, K, K)) / math.sqrt(cin * K * K)).astype(np.float32))
  return bf16_round(x), w


# Measurement switches (iic_debug_*) exist in the instrumented library only (make dbg; IIC_HIP_LIB=dbg): parameters that
# set one to a non-default value carry the `hooks` marker (tests/conftest.py deselects them in the product library and
# test_switch_dependent_tests_pass_in_the_instrumented_library runs them in a sub-process); hook() is a no-op otherwise.
from tests.conftest import hook      # noqa: E402

HOOKS = pytest.mark.hooks


def _force_bm(bm):
  hook("iic_debug_force_bm", bm)


def _p64_grid(n):
  hook("iic_debug_p64_grid", n)


@pytest.mark.parametrize("grid", [pytest.param(1, marks=HOOKS), pytest.param(3, marks=HOOKS), 0])
def test_conv_p64_persistent_tiles(grid):
  """64 -> 64 3x3 layers run on the persistent DMA-fed kernel (conv_igemm_p64.hip); a forced
  small grid makes every workgroup walk many tiles (double-buffered patches, deferred stores,
  statistics carried in registers), grid 0 = one workgroup per CU."""
  case = (64, 64, 3, 1, 1, 6, 49) if grid else (64, 64, 3, 1, 1, 40, 49)
  _p64_grid(grid)
  try:
    _conv_forward_and_stats(case, frag=True)
    _conv_backward_data(case, frag=True)
  finally:
    _p64_grid(0)


@pytest.mark.parametrize("bm", [0, pytest.param(256, marks=HOOKS), "frag"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_forward_and_stats(case, bm):
  """bm: 0 / 256 = first-generation kernel with 128- / 256-row tiles (row-major weights);
  "frag" = second-generation weights-direct kernel (conv_igemm_bd.hip)."""
  from iic_amd import geom, ops
  cin, cout, K, s, p, N, H = case
  if bm == "frag":
    return _conv_forward_and_stats(case, frag=True)
  if bm == 256 and s != 1:
    pytest.skip("256-row tiles are used for stride-1 convs only (LDS footprint)")
  _force_bm(bm)
  try:
    _conv_forward_and_stats(case)
  finally:
    _force_bm(0)


def _conv_forward_and_stats(case, frag=False):
  from iic_amd import geom, ops
  cin, cout, K, s, p, N, H = case
  x, w = _conv_inputs(cin, cout, K, N, H)
  ref = F.conv2d(x, bf16_round(w), stride=s, padding=p)
  spec = geom.ConvSpec(cin, cout, K, s, p)
  Ho = spec.out_size(H)
  g = geom.fwd_geom(spec, N, H, H, 1, 1)
  wf, wb = ops.weight_prep(w.to(dev()))
  wop = wf
  if frag:
    if not ops.frag_supported(g):
      assert not (cin == 64 and cout == 64 and K == 3), "64->64 3x3 must run on the persistent kernel"
      pytest.skip("geometry not served by the weights-direct kernel (Cout % 128 != 0)")
    wop = ops.PreppedWeights(w.to(dev()))[0]
  xp = ops.pt_from_nchw(x.to(dev()), 1)
  out = torch.zeros((N, Ho + 2, Ho + 2, cout), dtype=torch.bfloat16, device=dev())
  stats = ops.new_stats(cout, dev())
  ops.conv_igemm(g, xp, wop, out, stats=stats)
  torch.cuda.synchronize()
  got = ops.pt_to_nchw(out, 1).cpu()
  scale = ref.abs().max().item()
  assert (got - ref).abs().max().item() <= 1e-2 * scale, (got - ref).abs().max().item() / scale
  o = out.float().cpu()
  assert o[:, 0].abs().max() == 0 and o[:, :, 0].abs().max() == 0 and o[:, -1].abs().max() == 0
  st = ops.stats_decode(stats, cout).float().cpu()
  cnt = N * Ho * Ho
  assert torch.allclose(st[0] / cnt, ref.mean((0, 2, 3)), atol=2e-3 * scale)
  assert torch.allclose(st[1] / cnt, (ref * ref).mean((0, 2, 3)), rtol=2e-3, atol=1e-4 * scale * scale)
  # weight prep layouts
  assert torch.equal(wf.float().cpu(), bf16_round(w).permute(2, 3, 0, 1).reshape(K * K, cout, cin))
  assert torch.equal(wb.float().cpu(), bf16_round(w).permute(2, 3, 1, 0).reshape(K * K, cin, cout))


@pytest.mark.parametrize("cin,cout,d,frag", [(64, 128, 1, False), (128, 128, 1, True), (64, 64, 2, False)])
def test_conv_large_images_padded_row_numbering(cin, cout, d, frag):
  """Large images with a wide PT border (segmentation trunk: 100x100, border 3): the geometry pads
  the per-image GEMM row count (iic_conv_geom.MP) so that no tile straddles two images; rows in
  the padding are invalid (not stored, no statistics, no weight gradient).  Forward + statistics,
  backward-data and backward-weight against torch on the same bf16 operands."""
  from iic_amd import geom, ops
  N, H, P, K = 2, 100, 3, 3
  x, w = _conv_inputs(cin, cout, K, N, H, 7)
  wr = bf16_round(w)
  spec = geom.ConvSpec(cin, cout, K, 1, 1, d)
  Ho = spec.out_size(H)
  xt = x.clone().requires_grad_(True)
  wt = wr.clone().requires_grad_(True)
  ref = F.conv2d(xt, wt, stride=1, padding=1, dilation=d)
  dy = bf16_round(torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(ref.shape)).astype(np.float32)))
  ref.backward(dy)
  g = geom.fwd_geom(spec, N, H, H, P, P)
  assert g.MP > 0 and g.MP % 256 == 0, "this case must exercise the padded row numbering"
  pw = ops.PreppedWeights(w.to(dev()))
  if frag:
    assert ops.frag_supported(g)
  wop = pw[0] if frag else pw.rows(False)
  xp = ops.pt_from_nchw(x.to(dev()), P)
  out = torch.zeros((N, Ho + 2 * P, Ho + 2 * P, cout), dtype=torch.bfloat16, device=dev())
  stats = ops.new_stats(cout, dev())
  ops.conv_igemm(g, xp, wop, out, stats=stats)
  torch.cuda.synchronize()
  got = ops.pt_to_nchw(out, P).cpu()
  scale = ref.abs().max().item()
  assert (got - ref.detach()).abs().max().item() <= 1e-2 * scale
  o = out.float()
  assert float(o[:, :P].abs().max()) == 0 and float(o[:, :, -P:].abs().max()) == 0
  st = ops.stats_decode(stats, cout).float().cpu()
  cnt = N * Ho * Ho
  assert torch.allclose(st[0] / cnt, ref.detach().mean((0, 2, 3)), atol=2e-3 * scale)
  assert torch.allclose(st[1] / cnt, (ref.detach() ** 2).mean((0, 2, 3)), rtol=2e-3, atol=1e-4 * scale * scale)
  # backward-data (dy lives in a PT tensor with the same border) and backward-weight
  geoms = geom.bwd_data_geoms(spec, N, H, H, P, P)
  dyp = ops.pt_from_nchw(dy.to(dev()), P)
  dx = torch.zeros((N, H + 2 * P, H + 2 * P, cin), dtype=torch.bfloat16, device=dev())
  for gb in geoms:
    ops.conv_igemm(gb, dyp, pw[1] if (frag and ops.frag_supported(gb)) else pw.rows(True), dx)
  dW = ops.conv_wgrad(g, xp, dyp, K * K, use_tr=True)
  torch.cuda.synchronize()
  gx = ops.pt_to_nchw(dx, P).cpu()
  assert (gx - xt.grad).abs().max().item() <= 1e-2 * xt.grad.abs().max().item()
  gw = dW.view(cout, cin, K, K).cpu()
  assert (gw - wt.grad).abs().max().item() <= 3e-3 * wt.grad.abs().max().item()


@pytest.mark.parametrize("bm", [0, pytest.param(256, marks=HOOKS), "frag"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_backward_data(case, bm):
  if bm == "frag":
    return _conv_backward_data(case, frag=True)
  if bm == 256 and case[3] != 1:
    pytest.skip("256-row tiles are used for stride-1 convs only (LDS footprint)")
  _force_bm(bm)
  try:
    _conv_backward_data(case)
  finally:
    _force_bm(0)


def _conv_backward_data(case, frag=False):
  from iic_amd import geom, ops
  cin, cout, K, s, p, N, H = case
  x, w = _conv_inputs(cin, cout, K, N, H, 1)
  wr = bf16_round(w)
  xt = x.clone().requires_grad_(True)
  y = F.conv2d(xt, wr, stride=s, padding=p)
  dy = bf16_round(torch.from_numpy(np.random.default_rng(2).standard_normal(tuple(y.shape)).astype(np.float32)))
  y.backward(dy)
  ref = xt.grad
  spec = geom.ConvSpec(cin, cout, K, s, p)
  geoms = geom.bwd_data_geoms(spec, N, H, H, 1, 1)
  _, wb = ops.weight_prep(w.to(dev()))
  if frag:
    if not all(ops.frag_supported(g) for g in geoms):
      pytest.skip("geometry not served by the weights-direct kernel (Cin % 128 != 0)")
    wb = ops.PreppedWeights(w.to(dev()))[1]
  dyp = ops.pt_from_nchw(dy.to(dev()), 1)
  dx = torch.zeros((N, H + 2, H + 2, cin), dtype=torch.bfloat16, device=dev())
  for g in geoms:
    ops.conv_igemm(g, dyp, wb, dx)
  torch.cuda.synchronize()
  got = ops.pt_to_nchw(dx, 1).cpu()
  scale = ref.abs().max().item()
  assert (got - ref).abs().max().item() <= 1e-2 * scale
  if geom.bwd_data_covers_all(spec):
    # epilogue variants: accumulate, fused ReLU-masked residual gradient
    rng = np.random.default_rng(3)
    rg = bf16_round(torch.from_numpy(rng.standard_normal((N, cin, H, H)).astype(np.float32)))
    ra = bf16_round(torch.from_numpy(rng.standard_normal((N, cin, H, H)).astype(np.float32)))
    dx2 = torch.zeros_like(dx)
    for g in geoms:
      ops.conv_igemm(g, dyp, wb, dx2, res_grad=ops.pt_from_nchw(rg.to(dev()), 1),
                     res_act=ops.pt_from_nchw(ra.to(dev()), 1))
    for g in geoms:
      ops.conv_igemm(g, dyp, wb, dx2, accumulate=True)
    torch.cuda.synchronize()
    want = 2 * ref + rg * (ra > 0).float()
    got2 = ops.pt_to_nchw(dx2, 1).cpu()
    assert (got2 - want).abs().max().item() <= 2e-2 * want.abs().max().item()
    # IIC_ACC_PREMASK: out = (value [+ previous] [+ res_grad]) where res_act > 0 else 0 -- exact
    # against the plain launch's own bf16 output (the epilogue works on the bf16-rounded tile)
    rgp, rap = ops.pt_from_nchw(rg.to(dev()), 1), ops.pt_from_nchw(ra.to(dev()), 1)
    plain = dx.float()
    m = (rap.float() > 0).float()
    interior = torch.zeros_like(m)
    interior[:, 1:-1, 1:-1] = 1
    for name, kw, expect in (
        ("mask", dict(res_act=rap), plain * m),
        ("grad", dict(res_grad=rgp), plain + rgp.float() * interior),
        ("grad+mask", dict(res_grad=rgp, res_act=rap), (plain + rgp.float()) * m)):
      dx3 = torch.zeros_like(dx)
      for g in geoms:
        ops.conv_igemm(g, dyp, wb, dx3, premask=True, **kw)
      torch.cuda.synchronize()
      assert torch.equal(dx3, expect.to(torch.bfloat16)), name
    dx4 = dx.clone()                      # accumulate onto the plain result, then mask
    for g in geoms:
      ops.conv_igemm(g, dyp, wb, dx4, accumulate=True, premask=True, res_act=rap)
    torch.cuda.synchronize()
    assert torch.equal(dx4, ((plain + plain).to(torch.bfloat16).float() * m).to(torch.bfloat16))


@pytest.mark.parametrize("use_tr", [False, True])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_backward_weight(case, use_tr):
  _conv_backward_weight(case, use_tr)


def _wgrad_dma(mode):
  """mode 1 / 3 / 0 as iic_debug_enable_wgrad_dma."""
  hook("iic_debug_enable_wgrad_dma", int(mode))


@pytest.mark.parametrize("dma", [1, pytest.param(3, marks=HOOKS), pytest.param(0, marks=HOOKS)])
@pytest.mark.parametrize("case,nsplit", [((64, 64, 3, 1, 1, 2, 49), 2), ((128, 128, 3, 1, 1, 20, 25), 3),
                                         ((512, 512, 3, 1, 1, 6, 7), 1), ((64, 64, 3, 1, 1, 5, 13), 1)])
def test_conv_backward_weight_long_k_ranges(case, nsplit, dma):
  """Few splits => every workgroup walks many K-tiles: the LDS-DMA ring of conv_wgrad_dma.hip
  (dma=1: 128-pixel tiles, 2 buffers; dma=3: 64-pixel tiles, 3-4 buffers) and the register-staged
  pipeline of conv_wgrad.hip (dma=0)."""
  _wgrad_dma(dma)
  try:
    _conv_backward_weight(case, True, nsplit=nsplit)
  finally:
    _wgrad_dma(1)


@pytest.mark.parametrize("dma", [pytest.param(3, marks=HOOKS), pytest.param(0, marks=HOOKS), 1])
@pytest.mark.parametrize("cin,cout,H,dil", [(64, 128, 200, 1), (128, 128, 100, 2)])
def test_conv_backward_weight_padded_row_numbering(cin, cout, H, dil, dma):
  """Large images (SegmentationNet10a at 200 x 200, PT border 3): iic_amd.geom pads the per-image GEMM row
  count to a multiple of 256 (g.MP) so that no tile straddles two images; rows past the image are invalid
  (zero dY).  The DMA weight-gradient kernel walks that numbering too (dma = 3 forces its 64-pixel ring: by
  default the dispatcher keeps these layers on the register-staged kernel, which is 4-5 % faster there);
  both against F.conv2d's weight gradient."""
  from iic_amd import geom, ops
  N, K, P = 2, 3, 3
  x, w = _conv_inputs(cin, cout, K, N, H, 11)
  wt = w.clone().requires_grad_(True)
  y = F.conv2d(x, wt, stride=1, padding=1, dilation=dil)
  dy = bf16_round(torch.from_numpy(np.random.default_rng(6).standard_normal(tuple(y.shape)).astype(np.float32)))
  y.backward(dy)
  ref = wt.grad
  spec = geom.ConvSpec(cin, cout, K, 1, 1, dil)
  g = geom.fwd_geom(spec, N, H, H, P, P)
  assert g.MP > g.MY * g.MX and g.MP % 256 == 0, "this case is meant to exercise the padded numbering"
  _wgrad_dma(dma)
  try:
    dW = ops.conv_wgrad(g, ops.pt_from_nchw(x.to(dev()), P), ops.pt_from_nchw(dy.to(dev()), P), K * K, use_tr=True)
    torch.cuda.synchronize()
  finally:
    _wgrad_dma(1)
  got = dW.view(cout, cin, K, K).cpu()
  scale = ref.abs().max().item()
  assert (got - ref).abs().max().item() <= 2e-3 * scale, (got - ref).abs().max().item() / scale


@HOOKS
@pytest.mark.parametrize("cin,cout,H,dil,N,nsplit,dma", [
    (64, 64, 49, 1, 3, 2, 1),        # 64-cout tiles: pipelined + software-pipelined form by default
    (128, 128, 25, 1, 20, 3, 1),     # 128-cout tiles: planar asm form by default
    (256, 256, 13, 1, 10, 1, 1),     # one split: a workgroup walks every K-tile (images straddle tiles)
    (512, 512, 7, 1, 6, 2, 1),
    (128, 128, 20, 2, 4, 1, 1),      # dilation 2: a wave's taps are 2 pixels apart (template TXS = 2)
    (64, 128, 12, 1, 9, 1, 1),       # ClusterNet6c 12 x 12: short image rows, many row / image wraps per tile
    (64, 64, 200, 1, 2, 2, 3),       # 64-pixel ring, padded row numbering, 64-cout tiles
    (64, 128, 200, 1, 2, 2, 3)])     # 64-pixel ring, padded row numbering, 128-cout tiles
def test_weight_gradient_k_loop_forms_are_bit_identical(cin, cout, H, dil, N, nsplit, dma):
  """conv_wgrad_dma.hip holds four forms of the K loop behind iic_debug_wgrad_planar (0 = first generation, 1 / 2 =
  planar patch with builtin / inline-asm reads, 4 = pipelined, 5 = the default choice): same work split, same k
  order, same MFMA sequence => the same bits; and the result against F.conv2d's weight gradient."""
  from iic_amd import geom, ops
  K, P = 3, max(dil, 1) if H < 200 else 3
  x, w = _conv_inputs(cin, cout, K, N, H, 21)
  wt = w.clone().requires_grad_(True)
  y = F.conv2d(x, wt, stride=1, padding=dil, dilation=dil)
  dy = bf16_round(torch.from_numpy(np.random.default_rng(8).standard_normal(tuple(y.shape)).astype(np.float32)))
  y.backward(dy)
  ref = wt.grad
  spec = geom.ConvSpec(cin, cout, K, 1, dil, dil)
  g = geom.fwd_geom(spec, N, H, H, P, P)
  xp, dyp = ops.pt_from_nchw(x.to(dev()), P), ops.pt_from_nchw(dy.to(dev()), P)
  out = {}
  _wgrad_dma(dma)
  try:
    for form in (0, 1, 2, 4, 5):
      hook("iic_debug_wgrad_planar", form)
      out[form] = ops.conv_wgrad(g, xp, dyp, K * K, use_tr=True, nsplit=nsplit).clone()
    torch.cuda.synchronize()
  finally:
    hook("iic_debug_wgrad_planar", 5)
    _wgrad_dma(1)
  for form in (1, 2, 4, 5):
    assert torch.equal(out[form], out[0]), form
  got = out[5].view(cout, cin, K, K).cpu()
  scale = ref.abs().max().item()
  assert (got - ref).abs().max().item() <= 2e-3 * scale, (got - ref).abs().max().item() / scale


@HOOKS
@pytest.mark.parametrize("cin,cout,H,W,pad,dil,N", [(64, 128, 200, 200, 1, 1, 1), (256, 512, 100, 100, 1, 2, 2), (512, 512, 98, 98, 1, 2, 1),
                                                    (128, 256, 64, 64, 1, 1, 3), (256, 512, 64, 64, 1, 2, 2), (64, 128, 49, 49, 1, 1, 5),
                                                    (128, 128, 40, 75, 1, 1, 2), (64, 128, 67, 33, 1, 2, 3)])
def test_block_tiled_conv_is_bit_identical_to_row_major_tiles(cin, cout, H, W, pad, dil, N):
  """conv_igemm_bd.hip block tiling (a 256-row tile = a 2-D block of output pixels, the patch = the sub-image under it;
  iic_debug_bd_blk 2 = wherever it applies, 0 = off): which tile computes an output row changes, the row's accumulation
  order does not -- forward and backward-data outputs must carry the same bits, with and without the epilogue's residual
  add / ReLU mask / fused BatchNorm-backward reduction (the BatchNorm statistics and the fused sums agree to fp32
  rounding: their per-tile partials group other rows); the forward also against F.conv2d.  SegmentationNet10a shapes (PT
  border 3, dilated convs with padding 1, both kernel widths: the backward-data of 64 -> 128 has 64-cout tiles), a ragged
  49 x 49 and two non-square images."""
  from iic_amd import geom, ops
  K, P = 3, 3
  rng = np.random.default_rng(41)
  x = bf16_round(torch.from_numpy(rng.standard_normal((N, cin, H, W)).astype(np.float32)))
  w = torch.from_numpy((rng.standard_normal((cout, cin, K, K)) / math.sqrt(cin * K * K)).astype(np.float32))
  y_ref = F.conv2d(x, bf16_round(w), stride=1, padding=pad, dilation=dil)
  dy = bf16_round(torch.from_numpy(rng.standard_normal(tuple(y_ref.shape)).astype(np.float32)))
  spec = geom.ConvSpec(cin, cout, K, 1, pad, dil)
  gf = geom.fwd_geom(spec, N, H, W, P, P)
  gb = geom.bwd_data_geoms(spec, N, H, W, P, P)
  Ho, Wo = y_ref.shape[2], y_ref.shape[3]
  xp, dyp = ops.pt_from_nchw(x.to(dev()), P), ops.pt_from_nchw(dy.to(dev()), P)
  res = ops.pt_from_nchw(bf16_round(torch.from_numpy(rng.standard_normal((N, cin, H, W)).astype(np.float32))).to(dev()), P)
  act = ops.pt_from_nchw(bf16_round(torch.from_numpy(rng.standard_normal((N, cin, H, W)).astype(np.float32))).to(dev()), P)
  coef = torch.stack([torch.rand(cin) + 0.5, torch.randn(cin) * 0.3, torch.zeros(cin), torch.ones(cin), torch.zeros(cin)]).to(dev())
  pw = ops.PreppedWeights(w.to(dev()))
  hook("iic_debug_enable_pw", 0)          # every launch on conv_igemm_bd_kernel
  out = {}
  try:
    for mode in (0, 2):
      hook("iic_debug_bd_blk", mode)
      for g in gb:
        g._red_ok = None
      yo = torch.zeros(N, Ho + 2 * P, Wo + 2 * P, cout, dtype=torch.bfloat16, device=dev())
      dx = torch.zeros(N, H + 2 * P, W + 2 * P, cin, dtype=torch.bfloat16, device=dev())
      dx2 = torch.zeros_like(dx)
      st, s1 = ops.new_stats(cout, dev()), ops.new_stats(cin, dev())
      ops.conv_igemm(gf, xp, pw[0], yo, stats=st)
      for g in gb:
        ops.conv_igemm(g, dyp, pw[1], dx)
      assert len(gb) == 1 and ops.red_supported(gb[0], pw[1])
      ops.conv_igemm(gb[0], dyp, pw[1], dx2, res_grad=res, res_act=act, premask=True, red=(xp, coef, s1, None, None))
      torch.cuda.synchronize()
      out[mode] = (yo.clone(), dx.clone(), dx2.clone(), ops.stats_decode(st, cout).clone(), ops.stats_decode(s1, cin).clone())
  finally:
    hook("iic_debug_bd_blk", 1)
    hook("iic_debug_enable_pw", 1)
  for i in range(3):
    assert torch.equal(out[0][i], out[2][i]), i
  for i in (3, 4):      # sums of per-tile fp32 partials: the grouping of rows into tiles differs, the last bits may
    scale = float(out[0][i].abs().max())
    assert float((out[0][i] - out[2][i]).abs().max()) <= 2e-5 * scale + 1e-6, i
  got = ops.pt_to_nchw(out[2][0], P).float().cpu()
  assert (got - y_ref).abs().max().item() <= 2e-2 * y_ref.abs().max().item()
  assert float(out[2][0][:, :P].abs().max()) == 0.0 and float(out[2][0][:, :, -P:].abs().max()) == 0.0   # borders untouched
  assert float(out[2][1][:, :P].abs().max()) == 0.0 and float(out[2][1][:, :, -P:].abs().max()) == 0.0


@pytest.mark.parametrize("cin,cout,H,W,dil", [(64, 128, 320, 320, 2), (64, 128, 40, 640, 1)])
def test_wide_images_run_on_block_tiles(cin, cout, H, W, dil):
  """Images too wide for any row-major LDS patch of the weights-direct kernel (> ~290 pixels at dilation 2, > ~580 at
  dilation 1: the span of 128 output rows + the tap halo exceeds 160 KB) used to fall back to the first-generation
  kernel; with block tiles (conv_igemm_bd.hip bd_block_config) the patch is the sub-image under a 2-D block and they stay on
  the weights-direct kernel, both widths (backward-data of 64 -> 128 has 64-cout tiles).  Forward and backward-data
  against F.conv2d and its autograd."""
  from iic_amd import geom, ops
  P = 3
  rng = np.random.default_rng(7)
  x = bf16_round(torch.from_numpy(rng.standard_normal((1, cin, H, W)).astype(np.float32))).requires_grad_(True)
  w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32))
  y_ref = F.conv2d(x, bf16_round(w), stride=1, padding=1, dilation=dil)
  dy = bf16_round(torch.from_numpy(rng.standard_normal(tuple(y_ref.shape)).astype(np.float32)))
  y_ref.backward(dy)
  spec = geom.ConvSpec(cin, cout, 3, 1, 1, dil)
  gf = geom.fwd_geom(spec, 1, H, W, P, P)
  (gb,) = geom.bwd_data_geoms(spec, 1, H, W, P, P)
  assert ops.frag_supported(gf) and ops.frag_supported(gb)
  Ho, Wo = y_ref.shape[2], y_ref.shape[3]
  xp, dyp = ops.pt_from_nchw(x.detach().to(dev()), P), ops.pt_from_nchw(dy.to(dev()), P)
  pw = ops.PreppedWeights(w.to(dev()))
  yo = torch.zeros(1, Ho + 2 * P, Wo + 2 * P, cout, dtype=torch.bfloat16, device=dev())
  dx = torch.zeros(1, H + 2 * P, W + 2 * P, cin, dtype=torch.bfloat16, device=dev())
  st = ops.new_stats(cout, dev())
  ops.conv_igemm(gf, xp, pw[0], yo, stats=st)
  ops.conv_igemm(gb, dyp, pw[1], dx)
  torch.cuda.synchronize()
  got = ops.pt_to_nchw(yo, P).cpu()
  assert (got - y_ref.detach()).abs().max().item() <= 2e-2 * y_ref.abs().max().item()
  gdx = ops.pt_to_nchw(dx, P).cpu()
  assert (gdx - x.grad).abs().max().item() <= 2e-2 * x.grad.abs().max().item()
  sums = ops.stats_decode(st, cout).cpu()
  ref_s = torch.stack([got.double().sum((0, 2, 3)), (got.double() ** 2).sum((0, 2, 3))])
  assert float((sums - ref_s).abs().max()) <= 2e-3 * float(ref_s.abs().max())     # (statistics from the fp32 accumulators, got is bf16)
  assert float(yo[:, :P].abs().max()) == 0.0 and float(dx[:, :, -P:].abs().max()) == 0.0


@pytest.mark.parametrize("cin,cout,H,pad,dil,N", [
    (128, 256, 100, 1, 1, 3),     # Potsdam c3: padded numbering, 128-pixel tiles that fit 160 KB only with the 4-tile table ring
    (64, 128, 128, 1, 1, 2),      # COCO-Stuff c2: 64-pixel tiles, two buffers
    (256, 512, 64, 1, 2, 2),      # COCO-Stuff c5: dilation 2 with padding 1 (62 x 62 outputs), padded numbering, 64-pixel tiles
    (512, 512, 62, 1, 2, 2),      # COCO-Stuff c6
    (64, 128, 200, 1, 1, 1),      # Potsdam c2: banded patch (3 x 80 rows instead of 484 per 64-pixel tile)
    (256, 512, 100, 1, 2, 1),     # Potsdam c5: dilation 2, padded numbering, banded patch
    (512, 512, 98, 1, 2, 1)])     # Potsdam c6: dilation 2, dense numbering, banded patch
def test_conv_backward_weight_segmentation_net_shapes(cin, cout, H, pad, dil, N):
  """The 3 x 3 layers of SegmentationNet10a as archs/seg.py builds them (PT border 3, the dilated convs with padding 1:
  /root/reference/code/archs/segmentation/net10a.py:16-22) -- the shapes for which conv_wgrad_dma.hip's planar kernels
  choose the 4-tile table ring, the 64-pixel ring and the padded row numbering; against F.conv2d's weight gradient, and
  the result must not depend on the split count beyond rounding."""
  from iic_amd import geom, ops
  K, P = 3, 3
  x, w = _conv_inputs(cin, cout, K, N, H, 31)
  wt = w.clone().requires_grad_(True)
  y = F.conv2d(x, wt, stride=1, padding=pad, dilation=dil)
  dy = bf16_round(torch.from_numpy(np.random.default_rng(10).standard_normal(tuple(y.shape)).astype(np.float32)))
  y.backward(dy)
  ref = wt.grad
  g = geom.fwd_geom(geom.ConvSpec(cin, cout, K, 1, pad, dil), N, H, H, P, P)
  xp, dyp = ops.pt_from_nchw(x.to(dev()), P), ops.pt_from_nchw(dy.to(dev()), P)
  scale = ref.abs().max().item()
  for nsplit in (None, 2):
    dW = ops.conv_wgrad(g, xp, dyp, K * K, use_tr=True, nsplit=nsplit)
    torch.cuda.synchronize()
    got = dW.view(cout, cin, K, K).cpu()
    assert (got - ref).abs().max().item() <= 2e-3 * scale, (nsplit, (got - ref).abs().max().item() / scale)


@pytest.mark.parametrize("cin,cout,H,dil,N", [(128, 128, 20, 2, 4), (64, 128, 12, 1, 9), (64, 64, 30, 2, 3)])
def test_conv_backward_weight_planar_kernel_shapes(cin, cout, H, dil, N):
  """Shapes the planar-patch weight-gradient kernels take in the product library that the ClusterNet5g cases above do
  not reach: dilation 2 (a wave's three taps two pixels apart) and short image rows; against F.conv2d."""
  from iic_amd import geom, ops
  K, P = 3, dil
  x, w = _conv_inputs(cin, cout, K, N, H, 22)
  wt = w.clone().requires_grad_(True)
  y = F.conv2d(x, wt, stride=1, padding=dil, dilation=dil)
  dy = bf16_round(torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(y.shape)).astype(np.float32)))
  y.backward(dy)
  ref = wt.grad
  g = geom.fwd_geom(geom.ConvSpec(cin, cout, K, 1, dil, dil), N, H, H, P, P)
  for nsplit in (1, 3):
    dW = ops.conv_wgrad(g, ops.pt_from_nchw(x.to(dev()), P), ops.pt_from_nchw(dy.to(dev()), P), K * K, use_tr=True,
                        nsplit=nsplit)
    torch.cuda.synchronize()
    got = dW.view(cout, cin, K, K).cpu()
    scale = ref.abs().max().item()
    assert (got - ref).abs().max().item() <= 2e-3 * scale, (nsplit, (got - ref).abs().max().item() / scale)


def _conv_backward_weight(case, use_tr, nsplit=None):
  from iic_amd import geom, ops
  cin, cout, K, s, p, N, H = case
  x, w = _conv_inputs(cin, cout, K, N, H, 4)
  wt = w.clone().requires_grad_(True)
  y = F.conv2d(x, wt, stride=s, padding=p)
  dy = bf16_round(torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(y.shape)).astype(np.float32)))
  y.backward(dy)
  ref = wt.grad
  spec = geom.ConvSpec(cin, cout, K, s, p)
  g = geom.fwd_geom(spec, N, H, H, 1, 1)
  dW = ops.conv_wgrad(g, ops.pt_from_nchw(x.to(dev()), 1), ops.pt_from_nchw(dy.to(dev()), 1), K * K,
                      use_tr=use_tr, nsplit=nsplit)
  torch.cuda.synchronize()
  got = dW.view(cout, cin, K, K).cpu()
  scale = ref.abs().max().item()
  assert (got - ref).abs().max().item() <= 2e-3 * scale, (got - ref).abs().max().item() / scale


# --------------------------------------------------------------------------------------
# batch norm streaming kernels
# --------------------------------------------------------------------------------------
def test_bn_forward_backward_kernels():
  from iic_amd import ops
  N, H, C = 6, 13, 128
  rng = np.random.default_rng(7)
  y = bf16_round(torch.from_numpy(rng.standard_normal((N, C, H, H)).astype(np.float32)) * 1.5 + 0.3)
  y2 = bf16_round(torch.from_numpy(rng.standard_normal((N, C, H, H)).astype(np.float32)))
  res = bf16_round(torch.from_numpy(rng.standard_normal((N, C, H, H)).astype(np.float32)))
  gamma = torch.from_numpy((1 + 0.2 * rng.standard_normal(C)).astype(np.float32))
  beta = torch.from_numpy((0.1 * rng.standard_normal(C)).astype(np.float32))
  cnt = N * H * H
  d = dev()

  def stats_of(t):
    st = ops.new_stats(C, d)
    ops.stats_encode(st, C, torch.stack([t.sum((0, 2, 3)), (t * t).sum((0, 2, 3))]))
    return st
  rm, rv = torch.zeros(C, device=d), torch.ones(C, device=d)
  nbt = torch.zeros((), dtype=torch.long, device=d)
  st = stats_of(y)
  coef = ops.bn_finalize(st, gamma.to(d), beta.to(d), rm, rv, nbt, C, cnt, True)
  torch.cuda.synchronize()
  assert st.abs().max().item() == 0 and nbt.item() == 1
  mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
  assert torch.allclose(coef[2].cpu(), mean, atol=1e-5) and torch.allclose(coef[3].cpu(), (var + 1e-5).rsqrt(), rtol=1e-4)
  assert torch.allclose(rm.cpu(), 0.1 * mean, atol=1e-6)
  assert torch.allclose(rv.cpu(), 0.9 + 0.1 * y.var((0, 2, 3), unbiased=True), rtol=1e-5)
  yp, y2p, rp = (ops.pt_from_nchw(t.to(d), 1) for t in (y, y2, res))
  # relu(bn(y) + res)
  out = torch.zeros_like(yp)
  ops.bn_apply(yp, coef, out, N, H, H, 1, C, res=rp, relu=True)
  ref = F.relu(F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5) + res)
  assert (ops.pt_to_nchw(out, 1).cpu() - ref).abs().max() <= 2e-2
  assert out[:, 0].abs().max() == 0 and out[:, :, -1].abs().max() == 0
  # relu(bn(y) + bn2(y2))
  coef2 = ops.bn_finalize(stats_of(y2), beta.to(d) + 1.0, gamma.to(d) * 0.1, None, None, None, C, cnt, True)
  out2 = torch.zeros_like(yp)
  ops.bn_apply(yp, coef, out2, N, H, H, 1, C, y2=y2p, coef2=coef2, relu=True)
  ref2 = F.relu(F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5) +
                F.batch_norm(y2, None, None, beta + 1.0, gamma * 0.1, True, 0.1, 1e-5))
  assert (ops.pt_to_nchw(out2, 1).cpu() - ref2).abs().max() <= 2e-2
  # eval mode with running stats
  coef_e = ops.bn_finalize(None, gamma.to(d), beta.to(d), rm, rv, None, C, cnt, False)
  oute = torch.zeros_like(yp)
  ops.bn_apply(yp, coef_e, oute, N, H, H, 1, C, relu=False)
  refe = F.batch_norm(y, rm.cpu(), rv.cpu(), gamma, beta, False, 0.1, 1e-5)
  assert (ops.pt_to_nchw(oute, 1).cpu() - refe).abs().max() <= 2e-2
  # backward of out = relu(bn(y) + res) w.r.t. y, gamma, beta
  dout = bf16_round(torch.from_numpy(rng.standard_normal((N, C, H, H)).astype(np.float32)))
  yt = y.clone().requires_grad_(True)
  gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
  o = F.relu(F.batch_norm(yt, None, None, gt, bt, True, 0.1, 1e-5) + res)
  o.backward(dout)
  act = ops.pt_from_nchw(bf16_round(o.detach()).to(d), 1)
  dp = ops.pt_from_nchw(dout.to(d), 1)
  sums = ops.new_stats(C, d)
  ops.bn_bwd_reduce(dp, act, yp, sums, N, H, H, 1, C)
  bcoef, dg, db = ops.bn_bwd_finalize(sums, gamma.to(d), coef, C, cnt)
  dy = torch.zeros_like(yp)
  ops.bn_bwd_apply(dp, act, yp, bcoef, dy, N, H, H, 1, C)
  torch.cuda.synchronize()
  assert sums.abs().max().item() == 0
  assert torch.allclose(dg.cpu(), gt.grad, rtol=2e-3, atol=2e-3 * gt.grad.abs().max().item())
  assert torch.allclose(db.cpu(), bt.grad, rtol=2e-3, atol=2e-3 * bt.grad.abs().max().item())
  assert (ops.pt_to_nchw(dy, 1).cpu() - yt.grad).abs().max() <= 1e-2 * yt.grad.abs().max()
  # mask recomputed from y (act = relu(bn(y)) with nothing added): identical to reading act
  a_plain = torch.zeros_like(yp)
  ops.bn_apply(yp, coef, a_plain, N, H, H, 1, C, relu=True)
  s_a, s_m = ops.new_stats(C, d), ops.new_stats(C, d)
  ops.bn_bwd_reduce(dp, a_plain, yp, s_a, N, H, H, 1, C)
  ops.bn_bwd_reduce(dp, None, yp, s_m, N, H, H, 1, C, mask_coef=coef)
  torch.cuda.synchronize()
  assert torch.allclose(ops.stats_decode(s_a, C), ops.stats_decode(s_m, C), rtol=1e-5, atol=1e-4)
  bc_a, _, _ = ops.bn_bwd_finalize(s_a, gamma.to(d), coef, C, cnt)
  dy_a, dy_m = torch.zeros_like(yp), torch.zeros_like(yp)
  ops.bn_bwd_apply(dp, a_plain, yp, bc_a, dy_a, N, H, H, 1, C)
  ops.bn_bwd_apply(dp, None, yp, bc_a, dy_m, N, H, H, 1, C, mask_coef=coef)
  torch.cuda.synchronize()
  assert torch.equal(dy_a, dy_m)


@pytest.mark.parametrize("N,H,W,P,C", [(5, 49, 49, 1, 64), (7, 25, 25, 1, 128), (9, 13, 13, 1, 256),
                                       (11, 7, 7, 1, 512), (3, 3, 5, 2, 512), (2, 20, 36, 2, 64),
                                       (1, 1, 1, 1, 64)])
@pytest.mark.hooks
def test_bn_backward_kernel_generations_agree(N, H, W, P, C):
  """Second-generation backward passes (pixel walkers, coefficients in registers) against the first:
  bn_bwd_apply is the same expression per element => bit-identical; bn_bwd_reduce sums in another
  order => fp32 summation noise only.  All mask modes, with and without the shared downsample BN;
  borders must stay untouched."""
  import ctypes
  from iic_amd import ops, _lib
  L = ctypes.CDLL(_lib.LIB_PATH)
  d = dev()
  g = torch.Generator().manual_seed(N * 1000 + C)
  shape = (N, H + 2 * P, W + 2 * P, C)

  def pt(scale=1.0):
    t = torch.zeros(shape, dtype=torch.bfloat16)
    t[:, P:P + H, P:P + W] = (torch.randn(N, H, W, C, generator=g) * scale).to(torch.bfloat16)
    return t.to(d)
  dout, y, y2 = pt(), pt(1.5), pt()
  act = torch.relu(pt())
  coef = (torch.randn(4, C, generator=g) * 0.5).to(d)
  bcoef = torch.randn(3, C, generator=g).to(d)
  bcoef2 = torch.randn(3, C, generator=g).to(d)
  try:
    for mode in ("none", "act", "from_y"):
      for has2 in (False, True):
        a = act if mode == "act" else None
        mc = coef if mode == "from_y" else None
        res = {}
        for gen in (0, 2):                       # 2 = second generation for every mask mode
          L.iic_debug_bn_v2(gen, 0)
          s1, s2 = ops.new_stats(C, d), ops.new_stats(C, d)
          ops.bn_bwd_reduce(dout, a, y, s1, N, H, W, P, C, y2=y2 if has2 else None,
                            sums2=s2 if has2 else None, mask_coef=mc)
          dy = torch.full(shape, 7.0, dtype=torch.bfloat16, device=d)
          dy2 = torch.full(shape, 7.0, dtype=torch.bfloat16, device=d)
          ops.bn_bwd_apply(dout, a, y, bcoef, dy, N, H, W, P, C, y2=y2 if has2 else None,
                           bcoef2=bcoef2 if has2 else None, dy2=dy2 if has2 else None, mask_coef=mc)
          torch.cuda.synchronize()
          res[gen] = (ops.stats_decode(s1, C), ops.stats_decode(s2, C), dy, dy2)
        for k in (0, 1):
          ref, got = res[0][k], res[2][k]
          assert (ref - got).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item()) , (mode, has2, k)
        assert torch.equal(res[0][2], res[2][2]) and torch.equal(res[0][3], res[2][3]), (mode, has2)
        border = res[2][2].clone()
        border[:, P:P + H, P:P + W] = 7.0
        assert (border == 7.0).all()              # only interior pixels are written
  finally:
    L.iic_debug_bn_v2(1, 0)


@pytest.mark.parametrize("N,H,W,P,C", [(5, 49, 49, 1, 64), (9, 13, 13, 1, 256), (3, 3, 5, 2, 512)])
@pytest.mark.hooks
def test_bn_passes_with_and_without_the_non_temporal_hint_are_bit_identical(N, H, W, P, C):
  """The BatchNorm passes read their streams with `global_load ... nt` (cache policy only, LAB.md section R5.6):
  forward apply (plain, residual, downsample branch), both backward passes in every mask mode -- the
  hinted kernels (the product's default) against the plain loads, bit for bit, borders untouched."""
  import ctypes
  from iic_amd import ops, _lib
  L = ctypes.CDLL(_lib.LIB_PATH)
  d = dev()
  g = torch.Generator().manual_seed(N * 77 + C)
  shape = (N, H + 2 * P, W + 2 * P, C)

  def pt(scale=1.0):
    t = torch.zeros(shape, dtype=torch.bfloat16)
    t[:, P:P + H, P:P + W] = (torch.randn(N, H, W, C, generator=g) * scale).to(torch.bfloat16)
    return t.to(d)
  dout, y, y2, res = pt(), pt(1.5), pt(), pt()
  coef = (torch.randn(5, C, generator=g) * 0.5).to(d)
  coef2 = (torch.randn(5, C, generator=g) * 0.5).to(d)
  bcoef = torch.randn(3, C, generator=g).to(d)
  bcoef2 = torch.randn(3, C, generator=g).to(d)
  out = {}
  try:
    for nt in (0, 1):
      L.iic_debug_bn_nt(nt)
      r = []
      for kw in ({}, {"res": res}, {"y2": y2, "coef2": coef2}):
        o = torch.full(shape, 7.0, dtype=torch.bfloat16, device=d)
        ops.bn_apply(y, coef, o, N, H, W, P, C, relu=True, **kw)
        r.append(o)
      for mc in (None, coef):
        for has2 in (False, True):
          s1, s2 = ops.new_stats(C, d), ops.new_stats(C, d)
          ops.bn_bwd_reduce(dout, None, y, s1, N, H, W, P, C, y2=y2 if has2 else None,
                            sums2=s2 if has2 else None, mask_coef=mc)
          dy = torch.full(shape, 7.0, dtype=torch.bfloat16, device=d)
          dy2 = torch.full(shape, 7.0, dtype=torch.bfloat16, device=d)
          ops.bn_bwd_apply(dout, None, y, bcoef, dy, N, H, W, P, C, y2=y2 if has2 else None,
                           bcoef2=bcoef2 if has2 else None, dy2=dy2 if has2 else None, mask_coef=mc)
          r += [s1.clone(), s2.clone(), dy, dy2]
      torch.cuda.synchronize()
      out[nt] = r
  finally:
    L.iic_debug_bn_nt(1)
  assert len(out[0]) == len(out[1])
  for a, b in zip(out[0], out[1]):
    assert torch.equal(a, b)
  border = out[1][0].clone()
  border[:, P:P + H, P:P + W] = 7.0
  assert (border == 7.0).all()


# --------------------------------------------------------------------------------------
# sobel + stem
# --------------------------------------------------------------------------------------
def test_sobel_matches_reference_golden():
  from iic_amd.transforms import sobel_process
  g = np.load(os.path.join(G, "nets.npz"))
  o = sobel_process(torch.from_numpy(g["sobel_in1"]).to(dev()), False)
  assert np.abs(o.cpu().numpy() - g["sobel_out1"]).max() <= 1e-6
  o = sobel_process(torch.from_numpy(g["sobel_in4"]).to(dev()), True)
  assert np.abs(o.cpu().numpy() - g["sobel_out4"]).max() <= 1e-6


def _stem_forward_backward(cin, S):
  from iic_amd import ops
  N = 3
  rng = np.random.default_rng(11)
  x = torch.from_numpy(rng.standard_normal((N, cin, S, S)).astype(np.float32))
  w = torch.from_numpy((rng.standard_normal((64, cin, 3, 3)) * 0.3).astype(np.float32))
  gamma = torch.from_numpy((1 + 0.2 * rng.standard_normal(64)).astype(np.float32))
  beta = torch.from_numpy((0.1 * rng.standard_normal(64)).astype(np.float32))
  wt, gt, bt = (t.clone().requires_grad_(True) for t in (w, gamma, beta))
  y = F.conv2d(x, wt, padding=1)
  a = F.relu(F.batch_norm(y, None, None, gt, bt, True, 0.1, 1e-5))
  pool = F.max_pool2d(a, 2, 2, padding=1)
  d = dev()
  xd, wd = x.to(d), w.to(d)
  st = ops.new_stats(64, d)
  ops.stem_stats(xd, wd, st)
  torch.cuda.synchronize()
  cnt = N * S * S
  ssum = ops.stats_decode(st, 64).float().cpu()
  assert torch.allclose(ssum[0] / cnt, y.detach().mean((0, 2, 3)), atol=1e-4)
  assert torch.allclose(ssum[1] / cnt, (y.detach() ** 2).mean((0, 2, 3)), rtol=1e-4, atol=1e-4)
  coef = ops.bn_finalize(st, gamma.to(d), beta.to(d), None, None, None, 64, cnt, True)
  So = S // 2 + 1
  out = torch.zeros((N, So + 2, So + 2, 64), dtype=torch.bfloat16, device=d)
  ops.stem_apply_pool(xd, wd, coef, out)
  torch.cuda.synchronize()
  got = ops.pt_to_nchw(out, 1).cpu()
  assert got.shape == pool.shape
  assert (got - pool.detach()).abs().max() <= 1e-2 * pool.abs().max().item()
  # backward
  dpool = bf16_round(torch.from_numpy(rng.standard_normal(tuple(pool.shape)).astype(np.float32)))
  pool.backward(dpool)
  dpp = ops.pt_from_nchw(dpool.to(d), 1)
  sums = ops.new_stats(64, d)
  ops.stem_bwd_reduce(xd, wd, coef, dpp, sums)
  bcoef, dg, db = ops.bn_bwd_finalize(sums, gamma.to(d), coef, 64, cnt)
  dW = ops.stem_bwd_wgrad(xd, wd, coef, bcoef, dpp)
  torch.cuda.synchronize()
  assert torch.allclose(db.cpu(), bt.grad, rtol=1e-3, atol=1e-3 * bt.grad.abs().max().item())
  assert torch.allclose(dg.cpu(), gt.grad, rtol=1e-3, atol=1e-3 * gt.grad.abs().max().item())
  # dy and the input patch enter the dW GEMM as bf16 MFMA operands (fp32 accumulate)
  assert (dW.cpu() - wt.grad).abs().max() <= 4e-3 * wt.grad.abs().max().item()
  # one-pass backward (the product path when 9*Cin <= 32): sums identical, dW from the
  # coefficient-free GEMMs G1 (g), G2 (y), G3 (valid patch sums)
  if ops.stem_bwd_fused_ok(cin):
    sums2 = ops.new_stats(64, d)
    h = ops.stem_bwd_fused(xd, wd, coef, dpp, sums2)
    bcoef2, dg2, db2 = ops.bn_bwd_finalize(sums2, gamma.to(d), coef, 64, cnt)
    dW2 = ops.stem_wgrad_combine(h, bcoef2, wd)
    torch.cuda.synchronize()
    assert torch.allclose(db2.cpu(), bt.grad, rtol=1e-3, atol=1e-3 * bt.grad.abs().max().item())
    assert torch.allclose(dg2.cpu(), gt.grad, rtol=1e-3, atol=1e-3 * gt.grad.abs().max().item())
    assert (dW2.cpu() - wt.grad).abs().max() <= 4e-3 * wt.grad.abs().max().item(), \
        (dW2.cpu() - wt.grad).abs().max().item() / wt.grad.abs().max().item()


# (5, 104): iic_stem_bwd_reduce keeps two conv rows of W * 64 floats in LDS -- 512 * 104 = 53 248 bytes, above the 48 KB a
# kernel may use without its limit raised (49 152 exactly at W = 96); a ragged last 32-pixel segment as well
@pytest.mark.parametrize("cin,S", [(2, 32), (2, 96), (1, 24), (3, 64), (5, 32), (5, 104)])
def test_stem_forward_backward(cin, S):
  _stem_forward_backward(cin, S)


@pytest.mark.hooks
def test_stem_fused_backward_without_the_register_resident_routing():
  """iic_debug_enable_stem_bwd2(0): iic_stem_bwd_fused runs stem_bwd_kernel<CIN, 2> (the one-pass backward before
  stem_bwd2.hip, still what the entry point falls back to) -- 78 144 bytes of dynamic LDS at Cin = 2, W = 96.  Same
  references and bounds as test_stem_forward_backward."""
  hook("iic_debug_enable_stem_bwd2", 0)
  try:
    _stem_forward_backward(2, 96)
  finally:
    hook("iic_debug_enable_stem_bwd2", 1)


# --------------------------------------------------------------------------------------
# heads, adam
# --------------------------------------------------------------------------------------
def test_heads_forward_backward():
  from iic_amd import ops
  from iic_amd.archs.cluster import _AvgPoolFn, _HeadsFn
  N, F_, H, k = 37, 512, 5, 70
  rng = np.random.default_rng(13)
  xin = bf16_round(torch.from_numpy(rng.standard_normal((N, F_, 7, 7)).astype(np.float32)))
  W = torch.from_numpy((rng.standard_normal((H * k, F_)) * 0.05).astype(np.float32))
  b = torch.from_numpy((rng.standard_normal(H * k) * 0.1).astype(np.float32))
  xt, Wt, bt = (t.clone().requires_grad_(True) for t in (xin, W, b))
  feats = xt.mean((2, 3))
  probs = F.softmax((feats @ Wt.t() + bt).view(N, H, k), dim=2)
  gout = torch.from_numpy(rng.standard_normal((N, H, k)).astype(np.float32))
  (probs * gout).sum().backward()
  d = dev()
  xp = ops.pt_from_nchw(xin.to(d), 1).requires_grad_(True)
  Wd, bd = W.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
  f = _AvgPoolFn.apply(xp, False)
  p = _HeadsFn.apply(f, Wd, bd, H, k)
  (p * gout.to(d)).sum().backward()
  torch.cuda.synchronize()
  assert (p.detach().cpu() - probs.detach()).abs().max() <= 2e-6
  assert torch.allclose(Wd.grad.cpu(), Wt.grad, rtol=1e-4, atol=1e-6)
  assert torch.allclose(bd.grad.cpu(), bt.grad, rtol=1e-4, atol=1e-6)
  gx = ops.pt_to_nchw(xp.grad, 1).cpu()
  assert (gx - xt.grad).abs().max() <= 1e-2 * xt.grad.abs().max().item()
  # pre-masked variant (archs.cluster.PREMASK): the same gradient, zero where the activation <= 0
  xp2 = ops.pt_from_nchw(xin.to(d), 1).requires_grad_(True)
  f2 = _AvgPoolFn.apply(xp2, True)
  (_HeadsFn.apply(f2, Wd.detach(), bd.detach(), H, k) * gout.to(d)).sum().backward()
  torch.cuda.synchronize()
  assert torch.equal(f2, f)
  assert torch.equal(xp2.grad, torch.where(xp.detach() > 0, xp.grad, torch.zeros_like(xp.grad)))


@pytest.mark.parametrize("k", [1, 3, 4, 7, 15, 16, 24, 32, 33, 70])
def test_softmax_rows_forward_backward(k):
  """Row softmax of the heads (net5g.py:69-71, net10a.py Softmax2d as rows of k): grouped kernels for
  k <= 32 (several rows per wave), one wave per row above; against torch in float64."""
  from iic_amd import ops
  rows = 1000 + k
  g = torch.Generator().manual_seed(k)
  x = (torch.randn(rows, k, generator=g) * 3).to(dev())
  dp = torch.randn(rows, k, generator=g).to(dev())
  p = ops.softmax_fwd(x, rows, k)
  dx = ops.softmax_bwd(p, dp, rows, k)
  x64 = x.double().cpu().requires_grad_(True)
  p64 = torch.softmax(x64, 1)
  p64.backward(dp.double().cpu())
  assert float((p.cpu().double() - p64.detach()).abs().max()) <= 2e-7
  assert float((p.sum(1) - 1).abs().max()) <= 1e-6
  assert float((dx.cpu().double() - x64.grad).abs().max()) <= 1e-6 * float(x64.grad.abs().max() + 1)


def test_adam_matches_torch():
  from iic_amd.optim import Adam
  d = dev()
  rng = np.random.default_rng(17)
  shapes = [(64, 2, 3, 3), (64,), (128, 64, 3, 3), (70, 512), (1,)] + [(33,)] * 60
  ps = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in shapes]
  mine = [p.clone().to(d).requires_grad_(True) for p in ps]
  theirs = [p.clone().to(d).requires_grad_(True) for p in ps]
  o1, o2 = Adam(mine, lr=1e-2), torch.optim.Adam(theirs, lr=1e-2)
  for step in range(3):
    for a, b in zip(mine, theirs):
      gr = torch.from_numpy(rng.standard_normal(tuple(a.shape)).astype(np.float32)).to(d)
      a.grad, b.grad = gr.clone(), gr.clone()
    o1.step()
    o2.step()
  torch.cuda.synchronize()
  for a, b in zip(mine, theirs):
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_adam_per_parameter_step_counts():
  """Two-head training: parameters that get no gradient in a step are skipped and keep their own
  step count (bias correction), exactly like torch.optim.Adam."""
  from iic_amd.optim import Adam
  torch.manual_seed(3)
  shapes = [(7, 5), (33,), (4, 3, 3, 3)]
  ps = [torch.nn.Parameter(torch.randn(s, device=dev())) for s in shapes]
  rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  ours, ref = Adam(ps, lr=1e-2), torch.optim.Adam(rs, lr=1e-2)
  for it in range(6):
    active = [0, 1] if it % 2 == 0 else [0, 2]       # parameter 0 always, 1 and 2 alternate
    for o in (ours, ref):
      o.zero_grad(set_to_none=True)
    for i in active:
      g = torch.randn(shapes[i], device=dev())
      ps[i].grad = g.clone()
      rs[i].grad = g.clone()
    ours.step()
    ref.step()
  for p, r in zip(ps, rs):
    assert torch.allclose(p, r, rtol=1e-5, atol=1e-6), (p - r).abs().max()
  assert [ours.state[p]["step"] for p in ps] == [6, 3, 3]


@pytest.mark.parametrize("cin,cout,H", [(64, 64, 49), (128, 128, 25), (256, 256, 13), (512, 512, 7)])
@pytest.mark.hooks
def test_full_size_kernel_generations_agree(cin, cout, H):
  """North-star shapes at the FULL batch (660 images): the second-generation kernels
  (weights-direct / persistent DMA conv, DMA weight gradient) against the first-generation ones,
  which are checked against torch at small sizes above.  Same bf16 operands, fp32 accumulation in
  a different order => outputs agree to a bf16 ulp, statistics and weight gradients to fp32
  reduction noise."""
  import ctypes
  from iic_amd import _lib, geom, ops
  L = ctypes.CDLL(_lib.LIB_PATH)
  N = 660
  g0 = torch.Generator(device="cpu").manual_seed(cin + H)
  x = torch.randn(N, H + 2, H + 2, cin, generator=g0).to(torch.bfloat16)
  x[:, 0] = 0; x[:, -1] = 0; x[:, :, 0] = 0; x[:, :, -1] = 0
  dy = torch.randn(N, H + 2, H + 2, cout, generator=g0).to(torch.bfloat16)
  dy[:, 0] = 0; dy[:, -1] = 0; dy[:, :, 0] = 0; dy[:, :, -1] = 0
  w = torch.randn(cout, cin, 3, 3, generator=g0) / math.sqrt(cin * 9)
  x, dy, w = x.to(dev()), dy.to(dev()), w.to(dev())
  spec = geom.ConvSpec(cin, cout, 3, 1, 1)
  gf = geom.fwd_geom(spec, N, H, H, 1, 1)
  gb = geom.bwd_data_geoms(spec, N, H, H, 1, 1)
  pw = ops.PreppedWeights(w)
  assert ops.frag_supported(gf) and all(ops.frag_supported(g) for g in gb)

  def run(new):
    y = torch.zeros(N, H + 2, H + 2, cout, dtype=torch.bfloat16, device=dev())
    dx = torch.zeros(N, H + 2, H + 2, cin, dtype=torch.bfloat16, device=dev())
    st = ops.new_stats(cout, dev())
    ops.conv_igemm(gf, x, pw[0] if new else pw.rows(False), y, stats=st)
    for g in gb:
      ops.conv_igemm(g, dy, pw[1] if new else pw.rows(True), dx)
    L.iic_debug_enable_wgrad_dma(1 if new else 0)
    try:
      dW = ops.conv_wgrad(gf, x, dy, 9, use_tr=True).clone()
    finally:
      L.iic_debug_enable_wgrad_dma(1)
    torch.cuda.synchronize()
    return y.float(), dx.float(), ops.stats_decode(st, cout), dW

  y1, dx1, st1, dW1 = run(True)
  y0, dx0, st0, dW0 = run(False)
  for a, b in ((y1, y0), (dx1, dx0)):
    d = (a - b).abs()
    assert float(d.max()) <= 2 ** -7 * float(b.abs().max()), float(d.max())    # <= 1 bf16 ulp of the largest
    assert float((d > 0).float().mean()) < 0.02                                 # and only rarely
  assert torch.allclose(st1, st0, rtol=1e-4, atol=1e-2)
  assert float((dW1 - dW0).abs().max()) <= 1e-4 * float(dW0.abs().max())


@pytest.mark.parametrize("cin,cout,H", [(64, 64, 49), (128, 128, 25), (256, 256, 13), (512, 512, 7)])
def test_full_size_kernels_vs_independent_reference(cin, cout, H):
  """The full-batch (660 images) launches of the second-generation kernels -- 256-row tiles,
  XCD-remapped order, persistent 64->64 kernel, DMA weight gradient -- against an INDEPENDENT
  reference, not against the first kernel generation:
    * forward / backward-data: F.conv2d / conv_transpose2d in fp64 on the CPU, same bf16-rounded
      operands, on a strided sample of images that includes the first and last image, the images
      around a 256-row tile boundary and the last (partial) tile;
    * BatchNorm statistics: sum / sum of squares of the kernel's own full output tensor;
    * weight gradient: the FULL 660-image contraction by torch on the device in fp32
      (an einsum over the unfolded input: independent of libiic_hip)."""
  import torch.nn.functional as F
  from iic_amd import geom, ops
  N = 660
  g0 = torch.Generator(device="cpu").manual_seed(3 * cin + H)
  x = torch.randn(N, H + 2, H + 2, cin, generator=g0).to(torch.bfloat16)
  x[:, 0] = 0; x[:, -1] = 0; x[:, :, 0] = 0; x[:, :, -1] = 0
  dy = torch.randn(N, H + 2, H + 2, cout, generator=g0).to(torch.bfloat16)
  dy[:, 0] = 0; dy[:, -1] = 0; dy[:, :, 0] = 0; dy[:, :, -1] = 0
  w = torch.randn(cout, cin, 3, 3, generator=g0) / math.sqrt(cin * 9)
  xd, dyd, wd = x.to(dev()), dy.to(dev()), w.to(dev())
  spec = geom.ConvSpec(cin, cout, 3, 1, 1)
  gf = geom.fwd_geom(spec, N, H, H, 1, 1)
  gb = geom.bwd_data_geoms(spec, N, H, H, 1, 1)
  pw = ops.PreppedWeights(wd)
  assert ops.frag_supported(gf) and all(ops.frag_supported(g) for g in gb)
  y = torch.zeros(N, H + 2, H + 2, cout, dtype=torch.bfloat16, device=dev())
  dx = torch.zeros(N, H + 2, H + 2, cin, dtype=torch.bfloat16, device=dev())
  st = ops.new_stats(cout, dev())
  ops.conv_igemm(gf, xd, pw[0], y, stats=st)
  for g in gb:
    ops.conv_igemm(g, dyd, pw[1], dx)
  dW = ops.conv_wgrad(gf, xd, dyd, 9, use_tr=True).view(cout, cin, 3, 3).clone()
  torch.cuda.synchronize()
  # ---- sampled images: ends, a stride through the batch, both sides of 256-row tile boundaries
  per = H * H
  edge = sorted(set(t * 256 // per for t in (1, 2, 97, 1000, (N * per) // 256)) |
                set(t * 256 // per - 1 for t in (1, 97, 1000)))
  sample = sorted(set([0, 1, N - 2, N - 1] + list(range(5, N, 83)) + [i for i in edge if 0 <= i < N]))
  wq = w.to(torch.bfloat16).double()
  xs = x[sample, 1:-1, 1:-1, :].double().permute(0, 3, 1, 2)
  ds = dy[sample, 1:-1, 1:-1, :].double().permute(0, 3, 1, 2)
  y_ref = F.conv2d(xs, wq, padding=1)
  dx_ref = F.conv_transpose2d(ds, wq, padding=1)
  y_k = y[sample, 1:-1, 1:-1, :].double().cpu().permute(0, 3, 1, 2)
  dx_k = dx[sample, 1:-1, 1:-1, :].double().cpu().permute(0, 3, 1, 2)
  for k_, r_ in ((y_k, y_ref), (dx_k, dx_ref)):
    # fp32 accumulation + one bf16 rounding of the stored value
    assert float((k_ - r_).abs().max()) <= 2 ** -7 * float(r_.abs().max()), float((k_ - r_).abs().max())
    assert float((k_ - r_).abs().mean()) <= 2 ** -9 * float(r_.abs().mean())
  # borders stay zero (kernels write interiors only)
  assert float(y[:, 0].abs().max()) == 0 and float(y[:, :, -1].abs().max()) == 0
  # ---- statistics of the stored tensor (the kernel sums its fp32 accumulators before rounding)
  yi = y[:, 1:-1, 1:-1, :].double()
  s_ref = torch.stack([yi.sum((0, 1, 2)), (yi * yi).sum((0, 1, 2))])
  s_k = ops.stats_decode(st, cout)
  cnt = N * per
  assert float(((s_k[0] - s_ref[0]) / cnt).abs().max()) <= 2e-4 * float(yi.abs().mean())
  assert torch.allclose(s_k[1], s_ref[1], rtol=2e-4)
  # ---- full weight gradient by torch on the device (fp32 accumulate of bf16 operands)
  xi = xd[:, :, :, :].float()
  dyi = dyd[:, 1:-1, 1:-1, :].float()
  dW_ref = torch.empty(cout, cin, 3, 3, device=dev())
  for kh in range(3):
    for kw in range(3):
      patch = xi[:, kh:kh + H, kw:kw + H, :]
      dW_ref[:, :, kh, kw] = torch.einsum("nyxo,nyxi->oi", dyi, patch)
  err = float((dW - dW_ref).abs().max()) / float(dW_ref.abs().max())
  assert err <= 2e-4, err


@pytest.mark.parametrize("cin,cout,H", [(64, 128, 49), (256, 512, 13)])
def test_full_size_stride2_weight_gradient_vs_torch(cin, cout, H):
  """Stride-2 3x3 weight gradient at the full batch (DMA kernel, 64-pixel K-tiles, 2 buffers: its
  128-pixel patch does not fit LDS twice) against a torch einsum on the device."""
  from iic_amd import geom, ops
  N = 660
  Ho = (H + 2 - 3) // 2 + 1
  g0 = torch.Generator(device="cpu").manual_seed(cin + H)
  x = torch.randn(N, H + 2, H + 2, cin, generator=g0).to(torch.bfloat16)
  x[:, 0] = 0; x[:, -1] = 0; x[:, :, 0] = 0; x[:, :, -1] = 0
  dy = torch.randn(N, Ho + 2, Ho + 2, cout, generator=g0).to(torch.bfloat16)
  dy[:, 0] = 0; dy[:, -1] = 0; dy[:, :, 0] = 0; dy[:, :, -1] = 0
  xd, dyd = x.to(dev()), dy.to(dev())
  gf = geom.fwd_geom(geom.ConvSpec(cin, cout, 3, 2, 1), N, H, H, 1, 1)
  dW = ops.conv_wgrad(gf, xd, dyd, 9, use_tr=True).view(cout, cin, 3, 3).clone()
  torch.cuda.synchronize()
  xi, dyi = xd.float(), dyd[:, 1:-1, 1:-1, :].float()
  ref = torch.empty(cout, cin, 3, 3, device=dev())
  for kh in range(3):
    for kw in range(3):
      patch = xi[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Ho:2, :]
      ref[:, :, kh, kw] = torch.einsum("nyxo,nyxi->oi", dyi, patch)
  err = float((dW - ref).abs().max()) / float(ref.abs().max())
  assert err <= 2e-4, err


def test_eval_matching_against_reference_golden():
  """iic_amd.eval_metrics (one contingency kernel) vs the reference's own matching functions
  (tests/golden/eval.npz) -- integer work, exact; plus a large random case vs the oracle."""
  from iic_amd import eval_metrics as em
  from oracle import eval_oracle
  g = np.load(os.path.join(G, "eval.npz"))
  n_cases = len([k for k in g.files if k.endswith("/k")])
  for i in range(n_cases):
    p, t = g["c%d/preds" % i], g["c%d/targets" % i]
    kp, kt = (int(v) for v in g["c%d/k" % i])
    pd, td = torch.from_numpy(p).to(dev()), torch.from_numpy(t).to(dev())
    assert em._original_match(pd, td, kp, kt) == [tuple(int(v) for v in r) for r in g["c%d/original_match" % i]]
    if kp == kt:
      c = g["c%d/num_correct" % i]
      assert np.array_equal(em._counts(pd, td, kp, kt), c)
      hm = em._hungarian_match(pd, td, kp, kt)
      ref = [tuple(int(v) for v in r) for r in g["c%d/hungarian_match" % i]]
      assert sum(c[a, b] for a, b in hm) == sum(c[a, b] for a, b in ref)
      re = torch.zeros_like(pd)
      for a, b in hm:
        re[pd == a] = b
      assert abs(em._acc(re, td, kt) - float(g["c%d/acc" % i][0])) < 1e-12
  # segmentation-sized input with labels outside [0, k) (masked pixels = -1): they match nothing
  rng = np.random.default_rng(0)
  n = 3_000_000
  p = rng.integers(0, 24, n)
  t = rng.integers(-1, 3, n)
  pd, td = torch.from_numpy(p).to(dev()), torch.from_numpy(t).to(dev())
  assert np.array_equal(em._counts(pd, td, 24, 3), eval_oracle.contingency(p, t, 24, 3))
  assert em._original_match(pd, td, 24, 3) == eval_oracle.original_match(p, t, 24, 3)
  with pytest.raises(AssertionError):
    em._original_match(torch.from_numpy(p), td, 24, 3)        # the reference's is_cuda assert is kept


@pytest.mark.parametrize("cin,cout,H,N,has2,masked", [
  pytest.param(64, 64, 19, 24, False, True, marks=HOOKS),      # persistent 64->64 kernel (fuses only behind iic_debug_p64_red), mask from y
  pytest.param(64, 64, 19, 24, True, False, marks=HOOKS),      # ... with the downsample branch's second sum
  (128, 128, 13, 40, False, True), (256, 128, 9, 33, True, False), (512, 512, 7, 16, False, False)])
def test_fused_bn_backward_reduction_in_conv_epilogue(cin, cout, H, N, has2, masked, request):
  """iic_conv_igemm_frag_red: the sums a BatchNorm backward needs (sum g, sum g*y [, sum g*y2]),
  taken in the backward-data conv's epilogue, against (a) the separate iic_bn_bwd_reduce pass over
  the tensor the same conv stored and (b) float64 sums of that tensor on the host; the stored
  tensor itself must be bit-identical to the launch without the fused reduction."""
  from iic_amd import geom, ops
  g0 = torch.Generator(device="cpu").manual_seed(cin + cout + H)
  def pt(c):
    t = torch.randn(N, H + 2, H + 2, c, generator=g0).to(torch.bfloat16)
    t[:, 0] = 0; t[:, -1] = 0; t[:, :, 0] = 0; t[:, :, -1] = 0
    return t.to(dev())
  # backward-data of a conv cin -> cout: the gradient dy has cout channels, the result dx cin
  dy, y, y2, res, act = pt(cout), pt(cin), pt(cin), pt(cin), pt(cin)
  w = (torch.randn(cout, cin, 3, 3, generator=g0) / math.sqrt(cout * 9)).to(dev())
  coef = torch.stack([torch.rand(cin, generator=g0) + 0.5, torch.randn(cin, generator=g0) * 0.3,
                      torch.zeros(cin), torch.ones(cin), torch.zeros(cin)]).to(dev())
  spec = geom.ConvSpec(cin, cout, 3, 1, 1)
  (gb,) = geom.bwd_data_geoms(spec, N, H, H, 1, 1)
  pw = ops.PreppedWeights(w)
  hook("iic_debug_p64_red", 1)    # (the persistent 64->64 kernel does not fuse by default: slower)
  request.addfinalizer(lambda: hook("iic_debug_p64_red", 0))
  gb._red_ok = None
  assert ops.red_supported(gb, pw[1])
  dx0 = torch.zeros(N, H + 2, H + 2, cin, dtype=torch.bfloat16, device=dev())
  dx1 = torch.zeros_like(dx0)
  ops.conv_igemm(gb, dy, pw[1], dx0, res_grad=res, res_act=act, premask=True)
  s1, s2 = ops.new_stats(cin, dev()), ops.new_stats(cin, dev())
  ops.conv_igemm(gb, dy, pw[1], dx1, res_grad=res, res_act=act, premask=True,
                 red=(y, coef if masked else None, s1, y2 if has2 else None, s2 if has2 else None))
  torch.cuda.synchronize()
  assert torch.equal(dx0, dx1)
  r1, r2 = ops.new_stats(cin, dev()), ops.new_stats(cin, dev())
  ops.bn_bwd_reduce(dx0, None, y, r1, N, H, H, 1, cin, y2=y2 if has2 else None, sums2=r2 if has2 else None,
                    mask_coef=coef if masked else None)
  torch.cuda.synchronize()
  gi = dx0[:, 1:-1, 1:-1, :].double()
  yi = y[:, 1:-1, 1:-1, :].double()
  if masked:
    keep = (y[:, 1:-1, 1:-1, :].float() * coef[0] + coef[1]) > 0
    gi = gi * keep
  host = torch.stack([gi.sum((0, 1, 2)), (gi * yi).sum((0, 1, 2))])
  for fused, sep, ref in ((s1, r1, host),) + (((s2, r2, torch.stack([gi.sum((0, 1, 2)), (gi * y2[:, 1:-1, 1:-1, :].double()).sum((0, 1, 2))])),) if has2 else ()):
    f, s_ = ops.stats_decode(fused, cin), ops.stats_decode(sep, cin)
    scale = float(ref.abs().max())
    assert float((f - ref).abs().max()) <= 2e-5 * scale + 1e-6, float((f - ref).abs().max()) / scale
    assert float((f - s_).abs().max()) <= 2e-5 * scale + 1e-6


def test_switch_dependent_tests_pass_in_the_instrumented_library():
  """The kernel-generation cross-checks and forced-variant parametrisations toggle iic_debug_* switches, which the product
  library does not have (include/iic_hip.h is its whole surface; csrc/common.h IIC_SWITCH).  They run here, in a
  sub-process that loads libiic_hip_dbg.so -- the same sources built with the switches compiled in."""
  import subprocess
  import sys
  from iic_amd import _lib
  if _lib.HAS_HOOKS:
    pytest.skip("this process already runs the instrumented library")
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  dbg = os.path.join(root, "iic_amd", "libiic_hip_dbg.so")
  if not os.path.exists(dbg):      # (build() treats the measurement libraries as best effort: the product does not need them)
    pytest.skip("libiic_hip_dbg.so not built: make -C iic_amd/csrc dbg")
  env = dict(os.environ, IIC_HIP_LIB="dbg")
  r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests"), "-m", "gpu and hooks", "-x", "-q",
                      "-p", "no:cacheprovider"], cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                     universal_newlines=True, timeout=1500)
  tail = "\n".join(r.stdout.splitlines()[-15:])
  assert r.returncode == 0, tail
  import re as _re
  m = _re.search(r"(\d+) passed", r.stdout)
  assert m and int(m.group(1)) >= 40, tail
