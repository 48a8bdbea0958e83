"""Exact-arithmetic tests of the kernels in front of and behind the bf16 convolutions: the ClusterNet5g stem
(csrc/stem.hip, csrc/stem_bwd2.hip), the VGG first convolution (csrc/firstconv2.hip and its first-generation fallback in
csrc/vgg.hip), the fused segmentation head and its unfused chain (csrc/seg_head.hip) and the fp32 GEMM family
(csrc/head.hip).  pytest -m gpu.

Inputs, weights and upstream gradients come from the {-1, 0, +1} lattice of tests/lattice.py; BatchNorm coefficients are
handed in as powers of two and half-integers (the finalisers' outputs are neither).  Every product and partial sum is then
a small multiple of 1/2 -- exact in fp32 under any summation order, exact in bf16 where a kernel stores bf16 -- so every
result must equal the float64 torch reference element for element: one input channel of one tap at one border column, the
last pixel of a ragged segment, a pool tie routed to the wrong element or the ragged last row of a chunk shows.  The
preconditions (|value| <= 255 where bf16 is stored, sums of magnitudes < 2^24) are asserted on the reference alone;
tests/test_first_layer_exact_cpu.py runs the same generators and preconditions without a GPU and proves the comparison.
"""
import ctypes
import functools

import pytest
import torch

from tests import lattice as L
from tests.lattice import assert_exact, record
from tests.test_gpu_kernels import HOOKS, hook

pytestmark = pytest.mark.gpu
IIC_ERR_UNSUPPORTED = -3
SENTINEL = 7.0


def dev():
  return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------------------------------
# stem
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem(case):
  inp = L.stem_inputs(case)
  return inp, L.stem_reference(inp)


def _run_stem(case, bwd2=True):
  """Every stem entry point on one case: those that serve its width against the float64 reference, exactly; the others
  must refuse it (tests/lattice.py stem_width_served restates the launch arithmetic)."""
  from iic_amd import ops
  from iic_amd._lib import lib, ptr, stream_ptr
  cin, H, W, N = case
  inp, ref = _stem(case)
  d = dev()
  x, w, coef, bcoef = (inp[k].to(d) for k in ("x", "w", "coef", "bcoef"))
  Ho, Wo = H // 2 + 1, W // 2 + 1
  ran = []
  # statistics
  st = ops.new_stats(64, d)
  ops.stem_stats(x, w, st)
  got = ops.stats_decode(st, 64)
  assert_exact(got[0], ref["sum_y"], "stem_stats sum y")
  assert_exact(got[1], ref["sum_yy"], "stem_stats sum y^2")
  # pooled activation, with its ring: the kernel writes the interior of a zeroed PT tensor
  out = torch.zeros((N, Ho + 2, Wo + 2, 64), dtype=torch.bfloat16, device=d)
  ops.stem_apply_pool(x, w, coef, out)
  assert_exact(out, L.to_pt64(ref["pool"], 1), "stem_apply_pool (PT, ring included)")
  # backward sums
  dpp = ops.pt_from_nchw(inp["dpool"].to(d), 1)
  sums = ops.new_stats(64, d)
  ops.stem_bwd_reduce(x, w, coef, dpp, sums)
  s = ops.stats_decode(sums, 64)
  assert_exact(s[0], ref["sum_g"], "stem_bwd_reduce sum g")
  assert_exact(s[1], ref["sum_gy"], "stem_bwd_reduce sum g*y")
  # weight gradient, two-pass form
  if L.stem_width_served("bwd_wgrad", cin, W):
    assert_exact(ops.stem_bwd_wgrad(x, w, coef, bcoef, dpp), ref["dW"], "stem_bwd_wgrad dW")
    ran.append("bwd_wgrad")
  else:
    part = ops._stem_partials(d)
    dW = torch.full_like(w, SENTINEL)
    rc = lib().iic_stem_bwd_wgrad(ptr(x), ptr(w), ptr(coef), ptr(bcoef), ptr(dpp), ptr(part), ptr(dW), N, cin, H, W,
                                  stream_ptr())
    assert rc == IIC_ERR_UNSUPPORTED and bool((dW == SENTINEL).all())
  # one-pass form
  if ops.stem_bwd_fused_ok(cin) or not L.stem_width_served("bwd_fused", cin, W, bwd2):
    if L.stem_width_served("bwd_fused", cin, W, bwd2):
      sums2 = ops.new_stats(64, d)
      h = ops.stem_bwd_fused(x, w, coef, dpp, sums2)
      s2 = ops.stats_decode(sums2, 64)
      assert_exact(s2[0], ref["sum_g"], "stem_bwd_fused sum g")
      assert_exact(s2[1], ref["sum_gy"], "stem_bwd_fused sum g*y")
      assert torch.equal(s2, s), "the sums of stem_bwd_fused and stem_bwd_reduce differ"
      assert_exact(ops.stem_wgrad_combine(h, bcoef, w), ref["dW"], "stem_wgrad_combine dW")
      ran.append("bwd_fused")
    else:
      sums2 = ops.new_stats(64, d)
      part = ops._stem_partials(d)
      nb = ctypes.c_int(-1)
      rc = lib().iic_stem_bwd_fused(ptr(x), ptr(w), ptr(coef), ptr(dpp), ptr(sums2), ptr(part), ctypes.byref(nb), N,
                                    cin, H, W, stream_ptr())
      assert rc == IIC_ERR_UNSUPPORTED and nb.value == -1 and int(sums2.abs().max()) == 0
  torch.cuda.synchronize()
  record(kernel="stem", ran=ran, **ref["figures"])


@pytest.mark.parametrize("case", L.STEM_CASES)
def test_stem_equals_float64_exactly(case):
  """(1, 4, 34, 700): 2100 (image, pooled row) items and 1400 statistic tile groups, both above the 1024 persistent
  workgroups -- every workgroup walks several; (5, 104, 104, 2): above the default LDS limit, ragged last segment;
  (4, 6, 34, 2): rectangular, two pixels in the last segment; (5, 2, 2, 1): the smallest legal image."""
  _run_stem(case)


# The largest width each entry point serves (derivation: tests/lattice.py stem_width_served, csrc/stem.hip stem_bwd_fits):
#   stats, apply_pool, bwd_reduce: W <= 256 (8 waves of 32 columns; 64 KB / 129 KB of LDS through the checked launch)
#   bwd_fused on the register-resident kernel (Cin <= 3): W <= 254 (W + 1 <= 256 columns with the odd origin)
#   bwd_wgrad, and bwd_fused elsewhere: static + dynamic LDS <= 160 KB -- W <= 204 at Cin = 1, W <= 186 at Cin = 5
STEM_WIDE_CASES = [(1, 4, 256, 2), (3, 4, 254, 2), (1, 4, 204, 2), (5, 4, 186, 2)]


@pytest.mark.parametrize("case", STEM_WIDE_CASES)
def test_stem_at_the_largest_served_widths(case):
  cin, H, W, N = case
  served = [e for e in ("stats", "apply_pool", "bwd_reduce", "bwd_wgrad", "bwd_fused") if L.stem_max_width(e, cin) == W]
  assert served, "no entry point has its limit at this width"
  _run_stem(case)


@pytest.mark.parametrize("entry,cin,W", [("stats", 1, 258), ("apply_pool", 1, 258), ("bwd_reduce", 1, 258),
                                         ("bwd_wgrad", 1, 206), ("bwd_wgrad", 5, 188), ("bwd_fused", 3, 256),
                                         ("bwd_fused", 4, 194), ("bwd_fused", 5, 188)])
def test_stem_first_refused_width_is_an_argument_error(entry, cin, W):
  """The first width past each entry point's limit: IIC_ERR_UNSUPPORTED, and no output is written."""
  from iic_amd import ops
  from iic_amd._lib import lib, ptr, stream_ptr
  assert L.stem_max_width(entry, cin) == W - 2 and not L.stem_width_served(entry, cin, W)
  d = dev()
  N, H = 1, 4
  Ho, Wo = H // 2 + 1, W // 2 + 1
  x, w = torch.zeros((N, cin, H, W), device=d), torch.zeros((64, cin, 3, 3), device=d)
  coef, bcoef = torch.ones((5, 64), device=d), torch.ones((3, 64), device=d)
  pt = torch.full((N, Ho + 2, Wo + 2, 64), SENTINEL, dtype=torch.bfloat16, device=d)
  st = ops.new_stats(64, d)
  part = ops._stem_partials(d)
  dW = torch.full_like(w, SENTINEL)
  nb = ctypes.c_int(-1)
  s = stream_ptr()
  rc = {
    "stats": lambda: lib().iic_stem_stats(ptr(x), ptr(w), ptr(st), N, cin, H, W, s),
    "apply_pool": lambda: lib().iic_stem_apply_pool(ptr(x), ptr(w), ptr(coef), ptr(pt), N, cin, H, W, s),
    "bwd_reduce": lambda: lib().iic_stem_bwd_reduce(ptr(x), ptr(w), ptr(coef), ptr(pt), ptr(st), N, cin, H, W, s),
    "bwd_wgrad": lambda: lib().iic_stem_bwd_wgrad(ptr(x), ptr(w), ptr(coef), ptr(bcoef), ptr(pt), ptr(part), ptr(dW), N,
                                                  cin, H, W, s),
    "bwd_fused": lambda: lib().iic_stem_bwd_fused(ptr(x), ptr(w), ptr(coef), ptr(pt), ptr(st), ptr(part),
                                                  ctypes.byref(nb), N, cin, H, W, s),
  }[entry]()
  torch.cuda.synchronize()
  assert rc == IIC_ERR_UNSUPPORTED
  assert int(st.abs().max()) == 0 and nb.value == -1
  assert bool((pt == SENTINEL).all()) and bool((dW == SENTINEL).all())


@HOOKS
def test_stem_fused_backward_fallback_equals_float64_exactly():
  """iic_debug_enable_stem_bwd2(0): iic_stem_bwd_fused runs stem_bwd_kernel<CIN, 2> at the flagship shape."""
  hook("iic_debug_enable_stem_bwd2", 0)
  try:
    _run_stem((2, 96, 96, 2), bwd2=False)
  finally:
    hook("iic_debug_enable_stem_bwd2", 1)


# ----------------------------------------------------------------------------------------------------------------------
# VGG first convolution
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.FIRSTCONV_CASES)
def test_firstconv_equals_float64_exactly(case):
  """Output (PT bf16, ring included), statistics and dW.  W % 4 != 0 takes the first-generation kernels; (4, 3, 200, 200,
  1) is the Potsdam width with a band count that does not divide the height; (8, 3, 36, 32, 2) one image row per tile."""
  from iic_amd import ops
  cin, K, H, W, N = case
  pad, P = (K - 1) // 2, 2
  inp = L.firstconv_inputs(case)
  ref = L.firstconv_reference(inp)
  d = dev()
  x = inp["x"].to(d)
  out = torch.zeros((N, H + 2 * P, W + 2 * P, 64), dtype=torch.bfloat16, device=d)
  st = ops.new_stats(64, d)
  ops.firstconv_fwd(x, inp["w"].to(d), out, st, K, pad, P)
  assert_exact(out, L.to_pt64(ref["y"], P), "firstconv_fwd (PT, ring included)")
  got = ops.stats_decode(st, 64)
  assert_exact(got[0], ref["sum_y"], "firstconv_fwd sum y")
  assert_exact(got[1], ref["sum_yy"], "firstconv_fwd sum y^2")
  dW = ops.firstconv_wgrad(x, ops.pt_from_nchw(inp["dy"].to(d), P), tuple(inp["w"].shape), K, pad, P)
  assert_exact(dW, ref["dW"], "firstconv_wgrad dW")
  record(kernel="firstconv", **ref["figures"])


# ----------------------------------------------------------------------------------------------------------------------
# segmentation head
# ----------------------------------------------------------------------------------------------------------------------
def _seg_setup(case):
  from iic_amd import ops
  C, k, N, Hf = case
  P = 3
  inp = L.seg_head_inputs(case)
  ref = L.seg_head_reference(inp)
  d = dev()
  xp = ops.pt_from_nchw(inp["f"].to(d), P)
  Hp = Hf + 2 * P
  geo = (N, Hf + 2, Hf + 2, Hp, Hp, P - 1)       # N, Hw, Ww, Hp, Wp, off as archs/seg.py::_head_probs derives them
  dx_ref = torch.full((N, Hp, Hp, C), SENTINEL, dtype=torch.float64)
  dx_ref[:, P:P + Hf, P:P + Hf] = ref["dx"].permute(0, 2, 3, 1)
  return inp, ref, xp, geo, dx_ref


@pytest.mark.parametrize("case", L.SEG_HEAD_CASES)
def test_seg_head_equals_float64_exactly(case):
  """iic_seg_head_fwd / _bwd_dx / _wgrad called directly.  M = 300: one ragged 256-row workgroup; M = 1083: two
  weight-gradient chunks, the second nearly empty; M = 1024: exactly one chunk.  pt_dx starts as a sentinel: the
  window's interior carries the gradient, everything else is left alone (include/iic_hip.h)."""
  from iic_amd._lib import check, lib, ptr, stream_ptr
  C, k, N, Hf = case
  inp, ref, xp, geo, dx_ref = _seg_setup(case)
  d, s, Lb = dev(), stream_ptr(), lib()
  M = geo[0] * geo[1] * geo[2]
  assert Lb.iic_seg_head_supported(C, k)
  w2 = inp["w"].reshape(k, C).contiguous().to(d)
  dlog = ref["dlog"].float().to(d)
  logits = torch.full((M, k), SENTINEL, device=d)
  check(Lb.iic_seg_head_fwd(ptr(xp), ptr(w2), ptr(logits), *geo, C, k, s), "iic_seg_head_fwd")
  assert_exact(logits, ref["logits"], "iic_seg_head_fwd logits")
  dx = torch.full(tuple(xp.shape), SENTINEL, dtype=torch.bfloat16, device=d)
  check(Lb.iic_seg_head_bwd_dx(ptr(dlog), ptr(w2), ptr(dx), *geo, C, k, s), "iic_seg_head_bwd_dx")
  assert_exact(dx, dx_ref, "iic_seg_head_bwd_dx (interior = gradient, the rest untouched)")
  nch = Lb.iic_seg_head_wgrad_chunks(M)
  part = torch.full((nch, k * C), SENTINEL, device=d)
  check(Lb.iic_seg_head_wgrad(ptr(dlog), ptr(xp), ptr(part), *geo, C, k, s), "iic_seg_head_wgrad")
  dW = torch.empty((k, C), device=d)
  check(Lb.iic_colsum_f32(ptr(part), ptr(dW), nch, k * C, 0, s), "iic_colsum_f32")
  assert_exact(dW, ref["dW"], "iic_seg_head_wgrad folded by iic_colsum_f32")
  record(kernel="seg_head", chunks=nch, **ref["figures"])


@pytest.mark.parametrize("case", L.SEG_CHAIN_CASES)
def test_seg_head_unfused_chain_equals_float64_exactly(case):
  """iic_seg_window_gather -> ops.gemm_f32 -> iic_gemm_f32_splitk / iic_seg_window_scatter, the calls of _head_probs and
  _SegHeadFn.backward with FUSED_HEAD off (C = 128 takes this chain always)."""
  from iic_amd import ops
  from iic_amd._lib import check, lib, ptr, stream_ptr
  C, k, N, Hf = case
  inp, ref, xp, geo, dx_ref = _seg_setup(case)
  d, s, Lb = dev(), stream_ptr(), lib()
  M = geo[0] * geo[1] * geo[2]
  w2 = inp["w"].reshape(k, C).contiguous().to(d)
  dlog = ref["dlog"].float().to(d)
  Fm = torch.full((M, C), SENTINEL, device=d)
  check(Lb.iic_seg_window_gather(ptr(xp), ptr(Fm), *geo, C, s), "iic_seg_window_gather")
  logits = torch.full((M, k), SENTINEL, device=d)
  ops.gemm_f32(Fm, C, 1, w2, 1, C, logits, k, M, k, C)
  assert_exact(logits, ref["logits"], "gather + gemm_f32 logits")
  dW = torch.zeros((k, C), device=d)
  splitk = max(1, min(512, M // 2048))
  check(Lb.iic_gemm_f32_splitk(ptr(dlog), 1, k, ptr(Fm), C, 1, ptr(dW), C, k, C, M, splitk, s), "iic_gemm_f32_splitk")
  assert_exact(dW, ref["dW"], "iic_gemm_f32_splitk dW")
  dF = torch.full((M, C), SENTINEL, device=d)
  ops.gemm_f32(dlog, k, 1, w2, C, 1, dF, C, M, C, k)
  dx = torch.full(tuple(xp.shape), SENTINEL, dtype=torch.bfloat16, device=d)
  check(Lb.iic_seg_window_scatter(ptr(dF), ptr(dx), *geo, C, s), "iic_seg_window_scatter")
  assert_exact(dx, dx_ref, "gemm_f32 + scatter (interior = gradient, the rest untouched)")
  record(kernel="seg_chain", splitk=splitk, **ref["figures"])


# ----------------------------------------------------------------------------------------------------------------------
# fp32 GEMM
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemm(shape):
  inp = L.gemm_inputs(shape)
  return inp, {(b, a): L.gemm_reference(inp, b, a) for b in (False, True) for a in (False, True)}


@pytest.mark.parametrize("a_kc", [True, False])
@pytest.mark.parametrize("b_kc", [True, False])
@pytest.mark.parametrize("shape", L.GEMM_SHAPES)
def test_gemm_f32_equals_float64_exactly(shape, a_kc, b_kc):
  """ops.gemm_f32 in the four operand-stride modes (unit stride along k, or along m / n), each with and without a bias
  and with and without accumulation onto a lattice-valued C.  (700, 250, 4608): four K-split groups."""
  from iic_amd import ops
  M, N, K = shape
  inp, refs = _gemm(shape)
  d = dev()
  A = (inp["A"] if a_kc else inp["A"].t()).contiguous().to(d)
  B = (inp["B"].t() if b_kc else inp["B"]).contiguous().to(d)
  sam, sak = (K, 1) if a_kc else (1, M)
  sbk, sbn = (1, K) if b_kc else (N, 1)
  bias = inp["bias"].to(d)
  for use_bias, acc in ((a_kc, b_kc), (not a_kc, not b_kc)):
    C = inp["C0"].clone().to(d) if acc else torch.full((M, N), SENTINEL, device=d)
    ops.gemm_f32(A, sam, sak, B, sbk, sbn, C, N, M, N, K, bias=bias if use_bias else None, accumulate=acc)
    assert_exact(C, refs[(use_bias, acc)], "gemm_f32 a_kc=%s b_kc=%s bias=%s accumulate=%s" % (a_kc, b_kc, use_bias, acc))
  record(kernel="gemm_f32", shape=list(shape), a_kc=a_kc, b_kc=b_kc, max_C=float(refs[(True, True)].abs().max()))


@pytest.mark.parametrize("splitk", [3, 1])
def test_gemm_f32_splitk_equals_float64_exactly(splitk):
  """iic_gemm_f32_splitk in the layout of _SegHeadFn.backward: dW[k][C] = dlog^T . F with k = 6, C = 512 over M = 6149
  rows -- splitk = M // 2048 = 3 with a ragged last slice -- added onto a zeroed C."""
  from iic_amd._lib import check, lib, ptr, stream_ptr
  k, C, M = L.SPLITK_CASE
  assert max(1, min(512, M // 2048)) == 3
  inp = L.gemm_inputs((k, C, M))      # A: [k][M] = dlog^T, B: [M][C] = F
  want = L.gemm_reference(inp, False, False)
  d = dev()
  dlog = inp["A"].t().contiguous().to(d)      # stored [M][k]
  Fm = inp["B"].to(d)
  dW = torch.zeros((k, C), device=d)
  check(lib().iic_gemm_f32_splitk(ptr(dlog), 1, k, ptr(Fm), C, 1, ptr(dW), C, k, C, M, splitk, stream_ptr()),
        "iic_gemm_f32_splitk")
  assert_exact(dW, want, "iic_gemm_f32_splitk splitk=%d" % splitk)
  record(kernel="gemm_f32_splitk", splitk=splitk, max_C=float(want.abs().max()))
