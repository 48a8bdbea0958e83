"""Non-finite values from a convolution's output to the loss, and through the Adam step, on the GPU: the class of every
output (finite / +inf / -inf / NaN) equals the float64 reference's and the finite ones stay within the bound the finite
test of the kernel applies (tests/nonfinite_cases.py: cases, references, the rule; tests/test_nonfinite_cpu.py: the
preconditions of every case and the proof that the rule rejects a ReLU and a window fold built on fmaxf).

DESIGN.md promises that a diverged run shows as NaN: "a non-finite loss propagates".  The reference scripts stop at a
non-finite loss, so a NaN has to reach it -- a ReLU or a max-pool written with fmaxf (one v_max_f32: returns the operand
that is not NaN) turns a poisoned channel into zeros and the run trains on with a dead channel and a finite loss.

Shapes are the smallest that reach every path of a kernel; output buffers start as parity.SENTINEL where a border must
survive.  pytest -m gpu."""
import ctypes
import math
import types

import pytest
import torch

from tests import nonfinite_cases as nf
from tests.parity import SENTINEL, U16, U32, assert_border, fma_acc_bound, interior, pt_of, stage_bound

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def dev():
  assert torch.cuda.is_available(), "no GPU visible"
  return torch.device("cuda:0")


def _gpu(t):
  return None if t is None else t.to(dev()).contiguous()


def _sentinel(N, H, W, P, C, dt):
  return torch.full((N, H + 2 * P, W + 2 * P, C), SENTINEL, dtype=dt, device=dev())


def _zeros_exactly(got, at, what):
  for i in at:
    assert float(got[i]) == 0.0, "%s: element %s must be exactly 0, got %r" % (what, i, float(got[i]))


# --------------------------------------------------------------------------------------
# ReLU and BatchNorm apply
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", nf.BN_MODES)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C", nf.BN_CS)
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_bn_apply_propagates_like_float64(fp32, C, relu, mode):
  """ops.bn_apply on bf16 PT tensors (iic_bn_apply) and on fp32 ones (iic_f32_bn_apply): a NaN, a +inf, a -inf, a +inf under
  a negative scale, +inf against -inf in the second operand, a channel with NaN coefficients; -inf and -1000 exactly 0
  after ReLU; the border keeps its sentinel."""
  from iic_amd import ops
  N, H, W, P = nf.BN_NHWP
  c = nf.bn_apply_case(C, relu, mode)
  dt = F32 if fp32 else BF16
  pt = lambda t: None if t is None else pt_of(t, P, dt)
  out = _sentinel(N, H, W, P, C, dt)
  ops.bn_apply(pt(c["y"]), _gpu(c["coef"]), out, N, H, W, P, C, res=pt(c["res"]), y2=pt(c["y2"]), coef2=_gpu(c["coef2"]),
               relu=bool(relu))
  torch.cuda.synchronize()
  got = interior(out, P).float()
  tol = 6 * U32 * c["A"] + (0.0 if fp32 else U16) * c["ref"].abs()
  what = "bn_apply %s C=%d relu=%d %s" % ("fp32" if fp32 else "bf16", C, relu, mode)
  nf.check(got, c["ref"], tol, what)
  _zeros_exactly(got, c["zero"], what)
  assert_border(out, P, SENTINEL, what)


@pytest.mark.parametrize("training", [True, False], ids=["batch-statistics", "running-statistics"])
def test_sup_bn_relu_propagates_like_float64(training):
  """semisup.bn_relu_forward (iic_sup_bn_relu_fwd) on [5, 40]: a full 32-feature block and a ragged one."""
  from iic_amd import semisup
  from tests import sup_head_cases as sh
  c = nf.sup_bn_case(training)
  t = c["t"]
  rm, rv = _gpu(t["rm"].clone()), _gpu(t["rv"].clone())
  y, _, _ = semisup.bn_relu_forward(_gpu(t["x"]), _gpu(t["gamma"]), _gpu(t["beta"]), rm, rv, training, sh.BN_MOMENTUM, sh.BN_EPS)
  torch.cuda.synchronize()
  what = "sup_bn_relu training=%d" % training
  nf.check(y.cpu(), c["ref"], c["tol"], what)
  _zeros_exactly(y.cpu(), c["zero"], what)


# --------------------------------------------------------------------------------------
# max-pools
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Pi,Po", nf.POOL_BORDERS)
@pytest.mark.parametrize("H,W", nf.POOL_HW)
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_maxpool2_propagates_like_torch(fp32, H, W, Pi, Po):
  """ops.maxpool2_fwd on bf16 (iic_maxpool2_fwd) and fp32 PT tensors (iic_f32_maxpool2_fwd): a NaN at each of the four
  window positions, +inf with NaN (NaN), an all -inf window (-inf), a NaN in the odd trailing row (nothing); finite
  outputs bit-equal."""
  from iic_amd import ops
  N, C = nf.POOL_N, nf.POOL_C
  c = nf.pool2_case(H, W)
  dt = F32 if fp32 else BF16
  out = _sentinel(N, H // 2, W // 2, Po, C, dt)
  ops.maxpool2_fwd(pt_of(c["x"], Pi, dt), out, N, H, W, Pi, Po, C)
  torch.cuda.synchronize()
  what = "maxpool2 %s %dx%d borders %d, %d" % (dt, H, W, Pi, Po)
  nf.check(interior(out, Po).float(), c["ref"], 0.0, what)
  assert_border(out, Po, SENTINEL, what)


@pytest.mark.parametrize("Pi,Po", nf.POOL_BORDERS)
@pytest.mark.parametrize("H,W", nf.POOL_HW)
def test_fused_bn_relu_maxpool_propagates_like_float64_and_like_the_two_pass_path(H, W, Pi, Po):
  """ops.bn_relu_maxpool2_fwd against maxpool(relu(bn)) in float64, and against ops.bn_apply followed by ops.maxpool2_fwd:
  the same class everywhere and the same bits where finite (the sibling of
  test_fused_bn_relu_maxpool_is_bit_identical_to_the_two_pass_path on non-finite data)."""
  from iic_amd import ops
  N, C = nf.POOL_N, nf.POOL_C
  c = nf.bn_pool2_case(H, W)
  Ho, Wo = H // 2, W // 2
  y, coef = pt_of(c["y"], Pi, BF16), _gpu(c["coef"])
  a = torch.zeros_like(y)
  ops.bn_apply(y, coef, a, N, H, W, Pi, C, relu=True)
  o_two, o_fus = _sentinel(N, Ho, Wo, Po, C, BF16), _sentinel(N, Ho, Wo, Po, C, BF16)
  ops.maxpool2_fwd(a, o_two, N, H, W, Pi, Po, C)
  ops.bn_relu_maxpool2_fwd(y, coef, o_fus, N, H, W, Pi, Po, C)
  torch.cuda.synchronize()
  what = "fused pool %dx%d borders %d, %d" % (H, W, Pi, Po)
  fus, two = interior(o_fus, Po).float(), interior(o_two, Po).float()
  nf.check(fus, c["ref"], c["tol"], what)
  nf.assert_classes(fus, two.double(), what + " against the two-pass path")
  fin = nf.cls(two) == nf.FIN
  assert torch.equal(fus[fin], two[fin]), what + ": finite elements differ from the two-pass path"
  assert_border(o_fus, Po, SENTINEL, what)


@pytest.mark.parametrize("H,W", nf.POOL_HW)
def test_f32_maxpool_s2p1_propagates_like_torch(H, W):
  """ops.f32_maxpool_s2p1_fwd: a NaN in a corner window that holds a single valid element, in the last pixel, next to a +inf;
  an all -inf window."""
  from iic_amd import ops
  N, C = nf.POOL_N, nf.POOL_C
  c = nf.pool_s2p1_case(H, W)
  out = _sentinel(N, H // 2 + 1, W // 2 + 1, 1, C, F32)
  ops.f32_maxpool_s2p1_fwd(pt_of(c["x"], 1, F32), out, N, H, W, C)
  torch.cuda.synchronize()
  nf.check(interior(out, 1), c["ref"], 0.0, "padded pool %dx%d" % (H, W))
  assert_border(out, 1, SENTINEL, "padded pool")


@pytest.mark.parametrize("kind", nf.STEM_KINDS)
def test_stem_apply_pool_propagates_like_float64(kind):
  """ops.stem_apply_pool on [3, 2, 8, 8]: a +inf and a NaN input pixel; then a finite input under NaN coefficients of one
  channel.  The pool inside the stem starts its fold at 0 (post-ReLU values): a NaN must still win."""
  from iic_amd import ops
  N, cin, S = nf.STEM_NCS
  c = nf.stem_case(kind)
  So = S // 2 + 1
  out = _sentinel(N, So, So, 1, 64, BF16)
  ops.stem_apply_pool(_gpu(c["x"]), _gpu(c["w"]), _gpu(c["coef"]), out)
  torch.cuda.synchronize()
  got = interior(out, 1).float().permute(0, 3, 1, 2)
  nf.assert_classes(got, c["ref"], "stem " + kind)
  nf.assert_in_bracket_where_finite(got, c["ref"], c["lo"], c["hi"], "stem " + kind)
  assert_border(out, 1, SENTINEL, "stem " + kind)


# --------------------------------------------------------------------------------------
# average pool, heads GEMM, softmax
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_avgpool_poisons_exactly_one_feature(fp32):
  from iic_amd import ops
  N, H, W, P, C = nf.AVG_SHAPE
  c = nf.avgpool_case(fp32)
  feats = ops.avgpool_fwd(pt_of(c["x"], P, F32 if fp32 else BF16), N, H, W, P, C)
  torch.cuda.synchronize()
  nf.check(feats.cpu(), c["ref"], c["tol"], "avgpool fp32=%d" % fp32)
  assert int((nf.cls(feats) == nf.ISNAN).sum()) == 1 and math.isnan(float(feats[1, 7]))


@pytest.mark.parametrize("run", nf.GEMM_RUNS)
@pytest.mark.parametrize("shape", nf.GEMM_SHAPES, ids=str)
def test_gemm_f32_poisons_rows_columns_and_single_outputs(shape, run):
  """ops.gemm_f32, one shape per kernel family: a NaN in a row of A and in bias; an inf in A against a 0 in B and a NaN
  already in C under accumulate; everything else within 2e-5 of the result's scale."""
  from iic_amd import ops
  M, N, K = shape
  c = nf.gemm_case(shape, run)
  A, B = _gpu(c["A"]), _gpu(c["B"])
  if run == "bias":
    C = torch.full((M, N), SENTINEL, device=dev())
    ops.gemm_f32(A, K, 1, B, 1, K, C, N, M, N, K, bias=_gpu(c["bias"]), accumulate=False)
  else:
    C = _gpu(c["C0"].clone())
    ops.gemm_f32(A, 1, M, B, N, 1, C, N, M, N, K, bias=None, accumulate=True)
  torch.cuda.synchronize()
  nf.check(C.cpu(), c["ref"], c["tol"], "gemm %s %s" % (shape, run))


@pytest.mark.parametrize("k", nf.SOFTMAX_KS)
def test_softmax_rows_propagate_like_torch(k):
  """ops.softmax_fwd, grouped kernels (k <= 32) and one wave per row: rows with a NaN or a +inf, and the all -inf row, are
  NaN; -inf entries are exactly 0 and the rest of their row sums to 1; the rows that share a wave stay finite."""
  from iic_amd import ops
  c = nf.softmax_case(k)
  p = ops.softmax_fwd(_gpu(c["x"]), nf.SOFTMAX_ROWS, k)
  torch.cuda.synchronize()
  p = p.cpu()
  nf.check(p, c["ref"], c["tol"], "softmax k=%d" % k)
  _zeros_exactly(p, c["zero"], "softmax k=%d" % k)
  fin = torch.isfinite(c["ref"]).all(1)
  assert float((p[fin].sum(1) - 1).abs().max()) <= 1e-6


# --------------------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------------------
def _iid_tol(ref64):
  return 1e-5 * ref64.abs() + 2e-7


def test_iid_loss_packed_heads_one_nan_probability():
  """H = 3 packed sub-heads, a NaN probability in head 1.  Stage by stage with the bounds of tests/test_gpu_iid_stages.py:
  the raw joint (class of every entry; finite ones within fma_acc_bound over bn terms), the k x k stage on the joint the
  GPU produced (parity.stage_bound).  Then the public entry: loss and both gradients of head 1 NaN, heads 0 and 2 finite
  and within the loss clause 1e-5 |ref| + 2e-7 and the gradient clause 1e-5 of the norm (tests/test_gpu_kernels.py)."""
  from iic_amd import _lib
  from iic_amd.losses import IID_loss_heads
  from tests import iid_stage_cases as sc
  from tests.test_gpu_iid_stages import run_stage
  H, bn, k = nf.IID_CASE
  c = nf.iid_case()
  L = _lib.lib()
  z, zt = _gpu(c["z"].permute(1, 0, 2)), _gpu(c["zt"].permute(1, 0, 2))      # packed [bn][H][k]
  ns = L.iic_iid_nsplit(bn)
  part = torch.full((ns, H, k, k), nf.NAN, device=dev())
  _lib.check(L.iic_iid_joint_raw(z.data_ptr(), zt.data_ptr(), part.data_ptr(), H, bn, k, k, H * k, ns, _lib.stream_ptr()),
             "iic_iid_joint_raw")
  torch.cuda.synchronize()
  R = part.cpu().double().sum(0)
  Rf = torch.nan_to_num(c["R"])
  nf.check(R, c["R"], fma_acc_bound(bn, Rf), "raw joint")
  ref = sc.stage_ref(part.cpu(), nf.IID_LAMB, 0)
  got = run_stage("iic_iid_loss_from_joint", part.cpu(), nf.IID_LAMB, 0)
  for name, mag in (("loss1", "M1"), ("loss2", "M2"), ("dR1", "mag1"), ("dR2", "mag2")):
    assert bool(torch.isnan(got[name][1]).all()) and bool(torch.isnan(ref[name][1]).all()), name
    keep = [0, 2]
    nf.check(got[name][keep], ref[name][keep], stage_bound(ref[name][keep], ref[mag][keep], k, ns), "k x k stage " + name)
  Z, ZT = z.clone().requires_grad_(True), zt.clone().requires_grad_(True)
  loss, loss_nl = IID_loss_heads(Z, ZT, lamb=nf.IID_LAMB)
  (loss.sum() + 0.5 * loss_nl.sum()).backward()
  torch.cuda.synchronize()
  nf.check(loss.detach().cpu(), c["loss"], _iid_tol(c["loss"]), "IID loss")
  nf.check(loss_nl.detach().cpu(), c["loss_nl"], _iid_tol(c["loss_nl"]), "IID loss without lambda")
  for mine, want, name in ((Z.grad, c["dz"], "dz"), (ZT.grad, c["dzt"], "dzt")):
    mine = mine.cpu().double().permute(1, 0, 2)
    nf.assert_classes(mine, want, "IID gradient " + name)
    for h in (0, 2):
      assert float((mine[h] - want[h]).norm() / want[h].norm()) <= 1e-5, (name, h)


@pytest.mark.parametrize("collapsed", [False, True], ids=["uncollapsed", "collapsed"])
def test_seg_loss_one_nan_pixel(collapsed):
  """(bn, k, h, w, T) = (2, 5, 6, 8, 1): one NaN pixel gives a NaN loss (both outputs), as oracle/iid_oracle.py in float64;
  the same maps without it give the finite loss within the clause of tests/test_gpu_seg_loss.py."""
  from iic_amd import seg_losses
  bn, k, h, w, T = nf.SEG_CASE
  c = nf.seg_case(collapsed)
  fn = seg_losses.IID_segmentation_loss if collapsed else seg_losses.IID_segmentation_loss_uncollapsed
  kw = dict(all_affine2_to_1=_gpu(torch.from_numpy(c["aff"])), all_mask_img1=_gpu(torch.from_numpy(c["mask"])), lamb=1.5,
            half_T_side_dense=T, half_T_side_sparse_min=0, half_T_side_sparse_max=0)
  got = []
  for x1 in (c["x1"], c["x1_clean"]):
    l, ln = fn(_gpu(torch.from_numpy(x1)).requires_grad_(True), _gpu(torch.from_numpy(c["x2"])).requires_grad_(True), **kw)
    got += [float(l.detach()), float(ln.detach())]
  got = torch.tensor(got, dtype=torch.float64)
  nf.check(got, c["ref"], 1e-5 * c["ref"].abs() + 2e-7, "segmentation loss collapsed=%d" % collapsed)


def test_sup_cross_entropy_one_nan_logit():
  """semisup.cross_entropy_raw (iic_sup_cross_entropy): a NaN logit gives a NaN mean loss and a NaN row of dlogits, as
  F.cross_entropy in float64; the other rows of dlogits within tests/sup_head_cases.py ce_bounds."""
  from iic_amd import semisup
  c = nf.ce_case()
  loss, dl = semisup.cross_entropy_raw(_gpu(c["logits"]), _gpu(c["targets"]))
  torch.cuda.synchronize()
  assert math.isnan(float(c["loss"])) and math.isnan(float(loss))
  nf.check(dl.cpu(), c["dl"], c["tol_dl"], "cross-entropy dlogits")


# --------------------------------------------------------------------------------------
# Adam
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["iic_adam_step", "iic_adam_step_dev"])
def test_adam_step_propagates_like_the_float64_restatement(entry):
  """Both entry points, two gradient sources, sizes [1, 257, 70001]: a NaN, a +inf, a -inf gradient and +inf against -inf;
  the class of p, m and v equals the float64 restatement of the kernel's expressions (an inf gradient: m = +-inf, v = +inf,
  p = NaN); every other element within the bounds of test_adam_step_dev_vs_float64_and_the_host_counter_variant."""
  from iic_amd import _lib
  c = nf.adam_case()
  n = len(nf.ADAM_SIZES)
  t = {name: [_gpu(x.clone()) for x in c["t"][name]] for name in ("p", "g", "g2", "m", "v")}
  VP, LP = ctypes.c_void_p * n, ctypes.c_long * n
  arr = lambda name: VP(*[x.data_ptr() for x in t[name]])
  lr, b1, b2, eps = nf.ADAM_HP
  if entry == "iic_adam_step":
    rc = _lib.lib().iic_adam_step(n, arr("p"), arr("g"), arr("g2"), arr("m"), arr("v"), LP(*nf.ADAM_SIZES), lr, b1, b2, eps,
                                  nf.ADAM_STEP, _lib.stream_ptr())
  else:
    steps = torch.full((1,), nf.ADAM_STEP - 1, dtype=torch.int32, device=dev())
    rc = _lib.lib().iic_adam_step_dev(n, arr("p"), arr("g"), arr("g2"), arr("m"), arr("v"), LP(*nf.ADAM_SIZES), lr, b1, b2,
                                      eps, steps.data_ptr(), _lib.stream_ptr())
  _lib.check(rc, entry)
  torch.cuda.synchronize()
  if entry == "iic_adam_step_dev":
    assert int(steps) == nf.ADAM_STEP
  for i in range(n):
    for j, name in enumerate(("p", "m", "v")):
      nf.check(t[name][i].cpu(), c["ref"][i][j], c["tol"][i][j], "%s %s of tensor %d" % (entry, name, i))


# --------------------------------------------------------------------------------------
# whole nets: a finite loss on a dead net is what the defect costs
# --------------------------------------------------------------------------------------
VARIANTS = ("inf-pixel", "nan-weight")


def _poison(params, x, variant, weight_name):
  params = {k: v.clone() for k, v in params.items()}
  x = x.clone()
  if variant == "inf-pixel":
    x[0, 0, x.shape[2] // 2, x.shape[3] // 3] = nf.INF
  else:
    w = params[weight_name]
    w[w.shape[0] // 2, w.shape[1] // 3, 1, 1] = nf.NAN
  return params, x


def _f64(params):
  return {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in params.items()}


_ORACLE = {}


def _cluster_oracle(key, make):
  """(probabilities per head, loss) of the float64 oracle, computed once per (net, variant, mode of the BatchNorm)."""
  if key not in _ORACLE:
    from oracle import iid_oracle
    outs = [o.detach() for o in make()]
    loss = sum(iid_oracle.IID_loss(o, o, lamb=1.0)[0] for o in outs) / len(outs)
    _ORACLE[key] = (outs, float(loss))
  return _ORACLE[key]


def _cluster_check(net, x, fp32, want, what):
  from iic_amd import ops
  from iic_amd.losses import IID_loss
  with torch.no_grad():
    if fp32:
      with ops.fp32_mode():
        got = net(x.to(dev()))
    else:
      got = net(x.to(dev()))
    loss = sum(IID_loss(o, o, lamb=1.0)[0] for o in got) / len(got)
  torch.cuda.synchronize()
  outs, lref = want
  assert math.isnan(lref), "the oracle's loss is finite: the case shows nothing"
  for i, (a, b) in enumerate(zip(got, outs)):
    nf.assert_classes(a.float().cpu(), b, "%s head %d" % (what, i))
    assert bool(torch.isnan(b).any())
  assert math.isnan(float(loss)), "%s: the loss is %r where the float64 oracle's is NaN" % (what, float(loss))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n_img,training", [(1, True), (2, False)], ids=["1-image-batch-statistics", "2-images-running-statistics"])
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_net5g_non_finite_reaches_every_head_and_the_loss(fp32, n_img, training, variant):
  """ClusterNet5g at the sizes of test_net5g_tiny_batches_and_batchnorm_modes_vs_oracle (32 x 32; one image on batch
  statistics, two in eval() on running statistics, where only the image that holds the +inf pixel may turn NaN): the heads'
  probabilities are NaN exactly where the float64 oracle's are, and the loss is NaN in both."""
  from iic_amd import archs
  from oracle import net_oracle
  params = net_oracle.make_net5g_params(2, 10, 2, True, seed=41, randomize_bn=True, head_std=0.3)
  g = torch.Generator().manual_seed(42 + n_img)
  xc = net_oracle.sobel_process(torch.rand(n_img, 1, 32, 32, generator=g), False)
  params, xc = _poison(params, xc, variant, "trunk.layer2.0.conv1.weight")
  want = _cluster_oracle(("5g", n_img, training, variant),
                         lambda: net_oracle.net5g_forward(_f64(params), xc.double(), training, 32, "head", 2))
  net = archs.ClusterNet5g(types.SimpleNamespace(in_channels=2, input_sz=32, batchnorm_track=True, num_sub_heads=2, output_k=10))
  net.load_state_dict(params, strict=True)
  net.to(dev()).train(training)
  _cluster_check(net, xc, fp32, want, "net5g %s" % variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_net6c_non_finite_reaches_every_head_and_the_loss(fp32, variant):
  """ClusterNet6c at the batch and size of test_net6c_input_sz_64_fp32_mode_vs_oracle (12 x 64 x 64, train())."""
  from iic_amd import archs
  from oracle import net_oracle
  params = net_oracle.make_net6c_params(1, 64, 10, 2, True, seed=9, randomize_bn=True, head_std=0.05)
  x6, _ = net_oracle.make_paired_batch(12, 64, 3, seed=10)
  mid = [idx for kind, idx, _, _ in net_oracle.vgg_feature_index(net_oracle.NET6C_CFG) if kind == "conv"][1]
  params, x6 = _poison(params, x6, variant, "trunk.features.%d.weight" % mid)
  want = _cluster_oracle(("6c", variant), lambda: net_oracle.net6c_forward(_f64(params), x6.double(), True, "head", 2))
  net = archs.ClusterNet6c(types.SimpleNamespace(in_channels=1, input_sz=64, batchnorm_track=True, num_sub_heads=2, output_k=10))
  net.load_state_dict(params, strict=True)
  net.to(dev()).train()
  _cluster_check(net, x6, fp32, want, "net6c %s" % variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
def test_net10a_non_finite_reaches_the_maps_and_the_loss(fp32, variant):
  """SegmentationNet10a at the size of its golden tests (2 x 4 x 24 x 24, train()): the maps are NaN where the float64
  oracle's are and IID_segmentation_loss is NaN in both."""
  from iic_amd import archs, ops, seg_losses
  from oracle import iid_oracle, net_oracle
  params = net_oracle.make_net10a_params(4, 3, 1, True, seed=5, randomize_bn=True)
  x = torch.rand(2, 4, 24, 24, generator=torch.Generator().manual_seed(3))
  mid = [idx for kind, idx, _, _ in net_oracle.vgg_feature_index(net_oracle.NET10A_CFG) if kind == "conv"][2]
  params, x = _poison(params, x, variant, "trunk.features.%d.weight" % mid)
  aff = torch.zeros(2, 2, 3)
  aff[:, 0, 0] = aff[:, 1, 1] = 1.0
  mask = torch.ones(2, 24, 24)
  key = ("10a", variant)
  if key not in _ORACLE:
    o = net_oracle.net10a_forward(_f64(params), x.double(), 24, True, "head", 1)[0].detach()
    l, _ = iid_oracle.IID_segmentation_loss(o, o, all_affine2_to_1=aff.double(), all_mask_img1=mask.double(), lamb=1.0,
                                            half_T_side_dense=1)
    _ORACLE[key] = (o, float(l))
  oref, lref = _ORACLE[key]
  assert math.isnan(lref) and bool(torch.isnan(oref).any())
  net = archs.SegmentationNet10a(types.SimpleNamespace(in_channels=4, input_sz=24, batchnorm_track=True, num_sub_heads=1,
                                                       output_k=3))
  net.load_state_dict(params, strict=True)
  net.to(dev()).train()
  if fp32:
    with ops.fp32_mode():
      out = net(x.to(dev()))[0]
  else:
    out = net(x.to(dev()))[0]
  # (the loss asserts that its inputs require a gradient, as the reference's does: no torch.no_grad() here)
  l, _ = seg_losses.IID_segmentation_loss(out, out, all_affine2_to_1=aff.to(dev()), all_mask_img1=mask.to(dev()), lamb=1.0,
                                          half_T_side_dense=1, half_T_side_sparse_min=0, half_T_side_sparse_max=0)
  torch.cuda.synchronize()
  nf.assert_classes(out.detach().float().cpu(), oref, "net10a %s" % variant)
  assert math.isnan(float(l.detach())), "net10a %s: the loss is %r where the float64 oracle's is NaN" % (variant, float(l.detach()))
