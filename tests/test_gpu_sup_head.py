"""The supervised head of the semi-supervised step on the GPU (csrc/sup_head.hip, iic_amd/semisup.py): exact lattice,
float64 bounds on full-mantissa operands, BatchNorm1d + ReLU, cross-entropy, reproducibility, ten-crop pixels and counts,
the whole SupHead5 module against the oracle, and the unsupported shapes.  Cases, references and bounds:
tests/sup_head_cases.py (proved on the CPU by tests/test_sup_head_cpu.py)."""
import types

import numpy as np
import pytest
import torch

from tests import parity
from tests import sup_head_cases as sc
from tests.parity import assert_bits, assert_border, assert_in_bracket, assert_within, dev

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _nsplit(case):
  from iic_amd import _lib
  return _lib.lib().iic_sup_fwd_nsplit(case.N, case.F, case.C, case.H, case.W)


def _prep(case, w):
  K = sc.K_of(case)
  wb = torch.empty((case.F, K), dtype=BF16, device=dev())
  wt = torch.empty((K, case.F), dtype=BF16, device=dev())
  parity.ok("iic_sup_weight_prep", w.to(dev()), wb, wt, case.F, case.C, case.H, case.W)
  return wb, wt


def _products(case, t, border=0.0):
  """y, dW, dx_pt of the three kernels for host operands t (x bf16-valued, w / b / dy fp32); the PT border of x holds
  `border` (read by nothing) and dx_pt starts from a zero tensor."""
  K, S = sc.K_of(case), _nsplit(case)
  assert S >= 1
  x_pt = sc.to_pt(t["x"], fill=border).to(dev())
  wb, wt = _prep(case, t["w"])
  y = torch.empty((case.N, case.F), dtype=F32, device=dev())
  ws = torch.empty(max(1, S * case.N * case.F), dtype=F32, device=dev())
  parity.ok("iic_sup_linear_fwd", x_pt, wb, t["b"].to(dev()), y, ws, case.N, case.F, case.C, case.H, case.W)
  Np = (case.N + 63) // 64 * 64
  dyb = torch.empty((case.N, case.F), dtype=BF16, device=dev())
  dyt = torch.empty((case.F, Np), dtype=BF16, device=dev())
  parity.ok("iic_sup_dy_cast", t["dy"].to(dev()), dyb, dyt, case.N, case.F)
  dx_pt = torch.zeros_like(x_pt)
  parity.ok("iic_sup_linear_bwd_dx", dyb, wt, dx_pt, case.N, case.F, case.C, case.H, case.W)
  dW = torch.empty((case.F, K), dtype=F32, device=dev())
  parity.ok("iic_sup_linear_wgrad", dyt, x_pt, dW, case.N, case.F, case.C, case.H, case.W)
  return y, dW, dx_pt, (wb, wt, dyb, dyt)


# ---- 1. exact lattice ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.LATTICE_CASES, ids=lambda c: c.name)
def test_exact_lattice(case):
  t = sc.lattice_inputs(case)
  assert sc.columns_distinct(t["w"])
  y64, Ay, dW64, AdW, dx64, Adx = sc.products64(t["x"], t["w"], t["b"], t["dy"])
  assert float(max(Ay.max(), AdW.max(), Adx.max())) < 2 ** 24      # every partial sum exact in fp32
  y, dW, dx_pt, (wb, wt, dyb, dyt) = _products(case, t, border=parity.SENTINEL)
  # the operands themselves: the permutation (h, w, c) <- (c, h, w), its transpose, the padded transpose of dy
  from iic_amd.semisup import permute_columns
  perm = torch.from_numpy(permute_columns(case.C, case.H, case.W))
  assert_bits(wb, t["w"][:, perm].to(BF16), "wb")
  assert_bits(wt, t["w"][:, perm].t().contiguous().to(BF16), "wt")
  assert_bits(dyb, t["dy"].to(BF16), "dyb")
  assert_bits(dyt[:, :case.N], t["dy"].t().contiguous().to(BF16), "dyt")
  assert float(dyt[:, case.N:].float().abs().sum()) == 0.0
  assert_bits(y, y64.float(), "forward %s" % case.name)
  assert_bits(dW, dW64.float(), "dW %s" % case.name)
  assert_bits(sc.from_pt(dx_pt).to(BF16), parity.bf16_rne(dx64).to(BF16), "dx %s" % case.name)
  assert_border(dx_pt, 1, 0.0, "dx %s" % case.name)


# ---- 2. float64 bounds on full-mantissa operands ------------------------------------------------------------------
@pytest.mark.parametrize("draw", sc.DRAWS)
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_products_within_f64_bounds(case, draw):
  t = sc.inputs(case, draw)
  y64, Ay, dW64, AdW, dx64, Adx = sc.refs(case, draw)
  S = _nsplit(case)
  y, dW, dx_pt, _ = _products(case, t)
  # extra = S: S - 1 additions of the K-slice partials and the bias (sup_fold_kernel); S = 1: the bias in the epilogue
  assert_within(y, y64, sc.forward_bound(case, Ay, S), "forward %s %s" % (case.name, draw), family="sup_fwd")
  assert_within(dW, dW64, sc.wgrad_bound(case, AdW), "dW %s %s" % (case.name, draw), family="sup_dW")
  b, lo, hi = sc.dx_bracket(case, dx64, Adx)
  share, floor = sc.decisive_share(lo, hi), sc.decisive_floor(case, draw)
  print("%s %s: nsplit %d, dx decisive share %.3f (floor %s)" % (case.name, draw, S, share, floor))
  if floor is not None:
    assert share >= floor, (share, floor)
  assert_in_bracket(sc.from_pt(dx_pt), lo, hi, "dx %s %s" % (case.name, draw), family="sup_dx", ref=dx64, b=b)
  assert_border(dx_pt, 1, 0.0, "dx %s %s" % (case.name, draw))
  print("worst |err| / bound:", {k: v for k, v in parity.WORST.items() if k.startswith("sup_")})


# ---- 3. BatchNorm1d + ReLU, cross-entropy --------------------------------------------------------------------------
def _bn_gpu(t, training, x=None):
  N, F = t["x"].shape
  d = {k: v.to(dev()) for k, v in t.items()}
  xin = d["x"] if x is None else x.to(dev())
  y, mean, inv = (torch.empty_like(xin), torch.empty(F, device=dev()), torch.empty(F, device=dev()))
  parity.ok("iic_sup_bn_relu_fwd", xin, d["gamma"], d["beta"], d["rm"], d["rv"], y, mean, inv, N, F, int(training),
            sc.BN_MOMENTUM, sc.BN_EPS)
  return d, y, mean, inv


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N,F", [(37, 192), (12, 2048), (2, 64)])
def test_bn_relu_vs_float64_torch(N, F, training):
  t = sc.bn_inputs(N, F, 1)
  x2 = sc.bn_inputs(N, F, 2)["x"]
  r = sc.bn_ref(t, training, x2=x2 if training else None)
  assert not bool(sc.bn_ambiguous(t, r).any())
  d, y, mean, inv = _bn_gpu(t, training)
  _, ez = sc.bn_fwd_bound(t, r)
  assert_within(y, r["y"], ez, "bn y", family="sup_bn_y")
  if training:
    uv1 = t["x"].double().var(0, unbiased=True)
    assert_within(d["rm"], r["rm1"], sc.bn_running_bound(t["rm"], [r["mean"]], N), "running_mean, 1 step")
    assert_within(d["rv"], r["rv1"], sc.bn_running_bound(t["rv"], [uv1], N), "running_var, 1 step")
  else:
    assert_bits(d["rm"], t["rm"], "running_mean untouched in eval mode")
    assert_bits(d["rv"], t["rv"], "running_var untouched in eval mode")
  dx, dg, db = (torch.empty_like(y), torch.empty(F, device=dev()), torch.empty(F, device=dev()))
  parity.ok("iic_sup_bn_relu_bwd", d["dout"], d["x"], y, d["gamma"], mean, inv, dx, dg, db, N, F, int(training))
  tdx, tdg, tdb = sc.bn_bwd_bounds(t, r, training)
  assert_within(dg, r["dgamma"], tdg, "bn dgamma", family="sup_bn_dg")
  assert_within(db, r["dbeta"], tdb, "bn dbeta", family="sup_bn_db")
  assert_within(dx, r["dx"], tdx, "bn dx", family="sup_bn_dx")
  if training:      # a second step on other data
    d2, _, _, _ = _bn_gpu(dict(t, rm=d["rm"].cpu(), rv=d["rv"].cpu()), True, x=x2)
    assert_within(d2["rm"], r["rm2"], sc.bn_running_bound(t["rm"], [r["mean"], r["mean2"]], N), "running_mean, 2 steps")
    assert_within(d2["rv"], r["rv2"], sc.bn_running_bound(t["rv"], [uv1, r["uvar2"]], N), "running_var, 2 steps")
  print("worst |err| / bound:", {k: v for k, v in parity.WORST.items() if k.startswith("sup_bn")})


def test_bn_training_with_one_row_raises():
  """Case C: N = 1 in training mode is an error (torch: 'Expected more than 1 value per channel'), in the library and in
  the module; evaluation mode serves it."""
  from iic_amd import _lib, semisup
  t = {k: v.to(dev()) for k, v in sc.bn_inputs(1, 64, 3).items()}
  y, m, i = torch.empty_like(t["x"]), torch.empty(64, device=dev()), torch.empty(64, device=dev())
  assert parity.call("iic_sup_bn_relu_fwd", t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], y, m, i, 1, 64, 1, 0.1,
                     1e-5) == -1
  with pytest.raises(ValueError):
    semisup.bn_relu_forward(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], True, 0.1, 1e-5)
  semisup.bn_relu_forward(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], False, 0.1, 1e-5)
  assert _lib.lib().iic_sup_fwd_nsplit(1, 64, 64, 1, 1) >= 1


@pytest.mark.parametrize("N,k", [(37, 10), (1, 10), (300, 3)])
def test_cross_entropy_vs_float64_torch(N, k):
  from iic_amd import semisup
  logits, targets = sc.ce_inputs(N, k, 1)
  loss64, dl64 = sc.ce_ref(logits, targets)
  tol_loss, tol_dl = sc.ce_bounds(logits, targets)
  lg = logits.to(dev()).requires_grad_(True)
  loss = semisup.cross_entropy(lg, targets)
  loss.backward()
  assert loss.shape == ()
  assert_within(loss.detach().view(1), loss64.view(1), tol_loss.view(1), "loss", family="sup_ce_loss")
  assert_within(lg.grad, dl64, tol_dl, "dlogits", family="sup_ce_dl")
  # the module twin and the upstream gradient
  lg2 = logits.to(dev()).requires_grad_(True)
  (semisup.CrossEntropyLoss()(lg2, targets.to(dev())) * 2.0).backward()
  assert_bits(lg2.grad, lg.grad * 2.0, "dlogits under an upstream factor")
  for bad in (-1, k):
    tb = targets.clone()
    tb[0] = bad
    with pytest.raises(IndexError):
      semisup.cross_entropy(lg.detach(), tb)
  print("worst |err| / bound:", {k_: v for k_, v in parity.WORST.items() if k_.startswith("sup_ce")})


# ---- 4. reproducibility ------------------------------------------------------------------------------------------
def test_backward_products_are_bit_reproducible():
  case = sc.CASE_B
  t = sc.inputs(case, "mixed")
  y1, dW1, dx1, _ = _products(case, t)
  y2, dW2, dx2, _ = _products(case, t)
  # other work queued on the stream in front of the third run
  a = torch.randn(1024, 1024, device=dev())
  for _ in range(4):
    a = a @ a * 1e-3
  x_pt = sc.to_pt(t["x"]).to(dev())
  wb, wt = _prep(case, t["w"])
  from iic_amd import linear
  dyb, dyt = linear.dy_cast(t["dy"].to(dev()))
  dx3, = linear.pt_linear_bwd_dx(dyb, wt, (torch.zeros_like(x_pt),))
  dW3 = linear.pt_linear_wgrad(dyt, (x_pt,))
  y3 = linear.pt_linear_forward((x_pt,), wb, t["b"].to(dev()), case.F)
  torch.cuda.synchronize()
  for name, u, v, w_ in (("y", y1, y2, y3), ("dW", dW1, dW2, dW3), ("dx", dx1, dx2, dx3)):
    assert_bits(u, v, name + " run 2")
    assert_bits(u, w_, name + " behind other work")


# ---- 5. ten-crop pixels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_rgb", [False, True])
def test_ten_crop_pixels_vs_pil(include_rgb):
  from iic_amd import semisup
  from oracle import augment_oracle as ao
  rng = np.random.default_rng(5)
  imgs = rng.integers(0, 256, (6, 96, 96, 3), dtype=np.uint8)
  ev = semisup.TenCropEvaluator(torch.from_numpy(imgs).to(dev()), np.arange(6) % 10, 64, include_rgb)
  idx = [4, 0, 5, 2, 1, 3]
  got = ev.crops(idx).cpu().numpy()
  S = 64
  c = int(round((96 - S) / 2.))
  boxes = [(0, 0), (96 - S, 0), (0, 96 - S), (96 - S, 96 - S), (c, c)]
  want = []
  for i in idx:
    for flip in (False, True):
      src = imgs[i][:, ::-1] if flip else imgs[i]        # TenCrop: five crops of the image, five of hflip(image)
      want += [ao.pil_pipeline(np.ascontiguousarray(src), xy, S, S, include_rgb) for xy in boxes]
  want = np.stack(want)
  assert got.shape == want.shape == (60, 4 if include_rgb else 1, S, S)
  assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- 6. ten-crop accuracy --------------------------------------------------------------------------------------------
def test_ten_crop_accumulator_vs_assess_acc_block():
  from iic_amd import semisup
  k = 10
  batches = [sc.tencrop_logits(7, k, 1), sc.tencrop_logits(300, k, 2), sc.tencrop_logits(5, k, 3)]
  rng = np.random.default_rng(6)
  targets = []
  for lg in batches:
    n = lg.shape[0] // 10
    al = lg.reshape(n, 10, k).astype(np.float64).sum(1)
    tg = np.where(rng.random(n) < 0.5, al.argmax(1), rng.integers(0, k, n))
    tg[0], tg[1] = 2, 1          # the tie's first index; the class only the float64 sum ranks first
    targets.append(tg.astype(np.int64))
  # the two special images are what they claim to be
  lg = batches[0].reshape(7, 10, k)
  assert lg[0, :, 2].sum() == lg[0, :, 5].sum() == lg[0].astype(np.float64).sum(0).max()
  f32 = np.zeros(k, np.float32)
  for q in range(10):
    f32 = f32 + lg[1, q]
  assert f32.argmax() == 3 and lg[1].astype(np.float64).sum(0).argmax() == 1
  want = sc.assess_acc_block_np(batches, targets)
  acc = semisup.TenCropAccumulator(dev())
  for lg_b, tg in zip(batches, targets):
    acc.update(torch.from_numpy(lg_b).to(dev()), torch.from_numpy(tg))
  assert acc.result() == want
  assert acc.accuracy() == want[0] / float(want[1])


# ---- 7. the whole module ---------------------------------------------------------------------------------------------
STATE_KEYS_HEAD = ["head.0.weight", "head.0.bias", "head.1.weight", "head.1.bias", "head.1.running_mean",
                   "head.1.running_var", "head.1.num_batches_tracked", "head.3.weight", "head.3.bias"]


def _cfg():
  return types.SimpleNamespace(in_channels=2, input_sz=32, batchnorm_track=True, num_sub_heads=2, output_k=10)


def _head_oracle(hp, feats, targets, training):
  """float64 torch.nn head and loss on the trunk oracle's features."""
  f = feats.double()
  h = f @ hp["head.0.weight"].double().t() + hp["head.0.bias"].double()
  bn = torch.nn.functional.batch_norm(h, hp["head.1.running_mean"].double().clone(), hp["head.1.running_var"].double().clone(),
                                     hp["head.1.weight"].double(), hp["head.1.bias"].double(), training, 0.1, 1e-5)
  if h.requires_grad:
    h.retain_grad()
  hp["_pre_bn"] = h
  logits = torch.relu(bn) @ hp["head.3.weight"].double().t() + hp["head.3.bias"].double()
  return logits, (torch.nn.functional.cross_entropy(logits, targets) if targets is not None else None)


@pytest.fixture(scope="module")
def module_setup():
  from iic_amd import archs, semisup
  from iic_amd.transforms import sobel_process
  from oracle import net_oracle
  params = net_oracle.make_net5g_params(2, 10, 2, True, seed=31, randomize_bn=True, head_std=0.3)
  imgs, _ = net_oracle.make_paired_batch(12, 32, 3, seed=32)
  xc = net_oracle.sobel_process(imgs, False)
  net = archs.ClusterNet5g(_cfg())
  net.load_state_dict(params, strict=True)
  net.to(dev())
  torch.manual_seed(7)
  sh = semisup.SupHead5(net, dlen=6400, gt_k=10)
  with torch.no_grad():       # (0.01-std weights give logits of 1e-2: scale the head so that the loss has structure)
    sh.head[3].weight.mul_(20.0)
    sh.head[1].weight.copy_(torch.rand(2048) + 0.5)
    sh.head[1].bias.copy_(torch.randn(2048) * 0.1)
  state = {k: v.detach().cpu().clone() for k, v in sh.state_dict().items()}
  x = sobel_process(imgs.to(dev()), False)
  targets = torch.from_numpy(np.random.default_rng(8).integers(0, 10, 12).astype(np.int64))
  return sh, state, params, x, xc, targets


def test_suphead5_state_dict_keys(module_setup):
  sh, state, params, _, _, _ = module_setup
  assert [k for k in state if k.startswith("head.")] == STATE_KEYS_HEAD
  assert sorted(k for k in state if k.startswith("trunk.")) == sorted("trunk." + k for k in params)
  assert state["head.0.weight"].shape == (2048, 6400) and state["head.3.weight"].shape == (10, 2048)


def test_suphead5_fp32_mode_vs_oracle(module_setup):
  from iic_amd import ops, semisup
  from oracle import net_oracle
  sh, state, params, x, xc, targets = module_setup
  sh.load_state_dict(state)
  sh.train()
  sh.zero_grad()
  rp = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
        for k, v in params.items()}
  hp = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
        for k, v in state.items() if k.startswith("head.")}
  feats = net_oracle.net5g_trunk(rp, xc, True, 32, penultimate_features=True)
  want_logits, want_loss = _head_oracle(hp, feats, targets, True)
  want_loss.backward()
  with ops.fp32_mode():
    logits = sh(x, penultimate_features=True)
    loss = semisup.cross_entropy(logits, targets)
  loss.backward()
  torch.cuda.synchronize()
  wl = want_logits.detach()
  assert (logits.detach().cpu().double() - wl).abs().max().item() <= 2e-4 * max(1.0, wl.abs().max().item())
  assert abs(float(loss.detach()) - float(want_loss.detach())) <= 2e-4 * max(1.0, abs(float(want_loss.detach())))
  for n, q in sh.named_parameters():
    if n.startswith("trunk.trunk.layer4") or n.startswith("trunk.head"):
      assert q.grad is None or float(q.grad.abs().max()) == 0.0, n
      continue
    ref = hp[n].grad if n.startswith("head.") else rp[n[len("trunk."):]].grad
    gn = scale = float(ref.double().norm())
    if n == "head.0.bias":
      # a bias in front of a batch-statistics BatchNorm has no gradient: the reference is a sum over the batch that
      # cancels to 1e-15.  The same 1e-2 applies at the scale the sum is taken at, its magnitude sum.
      scale = float(hp["_pre_bn"].grad.abs().sum(0).norm())
    assert abs(float(q.grad.double().norm()) - gn) <= 1e-2 * max(scale, 1e-6) + 1e-9, (n, float(q.grad.double().norm()), gn)


def test_suphead5_eval_forward_two_rows_vs_oracle(module_setup):
  """Case C: an evaluation-mode forward at N = 2 on the running statistics (exact tier)."""
  from iic_amd import ops
  from oracle import net_oracle
  sh, state, params, x, xc, _ = module_setup
  sh.load_state_dict(state)
  sh.eval()
  with torch.no_grad(), ops.fp32_mode():
    logits = sh(x[:2], penultimate_features=True)
  feats = net_oracle.net5g_trunk({k: v.clone() for k, v in params.items()}, xc[:2], False, 32, penultimate_features=True)
  want, _ = _head_oracle({k: v for k, v in state.items() if k.startswith("head.")}, feats.detach(), None, False)
  assert (logits.cpu().double() - want).abs().max().item() <= 2e-4 * max(1.0, want.abs().max().item())
  # the pooled 512 features take the fp32 GEMM too (another head: dlen = 512)
  from iic_amd import semisup
  sh512 = semisup.SupHead5(sh.trunk, dlen=512, gt_k=10).eval()
  with torch.no_grad():
    assert sh512(x[:2]).shape == (2, 10)


def test_suphead5_bf16_mode(module_setup):
  from iic_amd import optim, semisup
  sh, state, params, x, xc, targets = module_setup
  sh.load_state_dict(state)
  sh.train()
  sh.zero_grad()
  # the head's three products on the trunk's actual PT tensor, inside test 2's bounds
  with torch.no_grad():
    pt = sh._features(x, True)
    assert pt.dtype is BF16 and tuple(pt.shape) == (12, 7, 7, 256)
    pt = pt.clone()
  case = sc.CASE_B
  xin = sc.from_pt(pt)
  t = dict(x=xin, w=state["head.0.weight"], b=state["head.0.bias"], dy=sc.inputs(case, "mixed")["dy"])
  y64, Ay, dW64, AdW, dx64, Adx = sc.products64(xin, sc.bf16(t["w"]), t["b"], sc.bf16(t["dy"]))
  y, dW, dx_pt, _ = _products(case, t)
  assert_within(y, y64, sc.forward_bound(case, Ay, _nsplit(case)), "forward on the trunk's tensor")
  assert_within(dW, dW64, sc.wgrad_bound(case, AdW), "dW on the trunk's tensor")
  b, lo, hi = sc.dx_bracket(case, dx64, Adx)
  assert_in_bracket(sc.from_pt(dx_pt), lo, hi, "dx on the trunk's tensor")
  # two Adam steps, trunk and head each with its own optimiser, lower the loss on a fixed batch.  With sup_head5.py's
  # own initialisation (module_setup's 20-fold last layer undone): the fp32 CPU restatement of this step (oracle trunk,
  # torch.nn head, torch.optim.Adam, lr 1e-4 twice) goes 2.28 -> 1.32 -> 1.15 there, while at the 20-fold scale the
  # same restatement overshoots (6.7 -> 17.1 -> 14.5): Adam's first steps move every weight by lr whatever the gradient
  with torch.no_grad():
    sh.head[3].weight.div_(20.0)
  opt_t = optim.Adam(sh.trunk.parameters(), lr=1e-4)
  opt_h = optim.Adam(sh.head.parameters(), lr=1e-4)
  losses = []
  for step in range(3):
    sh.zero_grad()
    loss = semisup.cross_entropy(sh(x, penultimate_features=True), targets)
    losses.append(float(loss.detach()))
    if step == 2:
      break
    loss.backward()
    grads = [p.grad for n, p in sh.named_parameters()
             if not (n.startswith("trunk.trunk.layer4") or n.startswith("trunk.head"))]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    opt_t.step()
    opt_h.step()
  print("losses over two Adam steps:", losses)
  assert all(np.isfinite(losses)) and losses[2] < losses[0], losses
  assert int(sh.head[1].num_batches_tracked) == int(state["head.1.num_batches_tracked"]) + 3


def test_ten_crop_evaluator_matches_manual_batches(module_setup):
  from iic_amd import semisup
  from iic_amd.transforms import sobel_process
  sh, state, _, _, _, _ = module_setup
  sh.load_state_dict(state)
  sh.eval()
  rng = np.random.default_rng(9)
  imgs = torch.from_numpy(rng.integers(0, 256, (9, 48, 48, 3), dtype=np.uint8)).to(dev())
  tg = rng.integers(0, 10, 9)
  ev = semisup.TenCropEvaluator(imgs, tg, 32, False)
  got = ev.accuracy(sh, images_per_batch=4, penultimate_features=True)
  with torch.no_grad():
    logits = [sh(sobel_process(ev.crops(np.arange(s, min(9, s + 4))), False), penultimate_features=True).cpu().numpy()
              for s in range(0, 9, 4)]
  c, n = sc.assess_acc_block_np(logits, [tg[s:s + 4] for s in range(0, 9, 4)])
  assert n == 9 and got == c / 9.0


# ---- 8. unsupported shapes -------------------------------------------------------------------------------------------
def test_unsupported_shapes_return_the_error_code():
  from iic_amd import _lib, linear
  u = sc.UNSUPPORTED
  K = sc.K_of(u)
  assert _lib.lib().iic_sup_fwd_nsplit(u.N, u.F, u.C, u.H, u.W) == 0
  z = lambda *s, dt=BF16: torch.zeros(s, dtype=dt, device=dev())
  x_pt, wb, wt = z(u.N, u.H + 2, u.W + 2, u.C), z(u.F, K), z(K, u.F)
  y, dW, w = z(u.N, u.F, dt=F32), z(u.F, K, dt=F32), z(u.F, K, dt=F32)
  dyb, dyt = z(u.N, u.F), z(u.F, 64)
  for C, F in ((u.C, 128), (64, u.F), (u.C, u.F)):
    assert parity.call("iic_sup_weight_prep", w, wb, wt, F, C, u.H, u.W) == -3
    assert parity.call("iic_sup_linear_fwd", x_pt, wb, None, y, y, u.N, F, C, u.H, u.W) == -3
    assert parity.call("iic_sup_linear_bwd_dx", dyb, wt, x_pt, u.N, F, C, u.H, u.W) == -3
    assert parity.call("iic_sup_linear_wgrad", dyt, x_pt, dW, u.N, F, C, u.H, u.W) == -3
  assert float(x_pt.float().abs().sum()) == 0.0 and float(dW.abs().sum()) == 0.0 and float(y.abs().sum()) == 0.0
  with pytest.raises(_lib.IICLibraryError):
    linear.pt_linear_forward((x_pt,), wb, None, u.F)
