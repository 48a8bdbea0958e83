"""Inputs, float64 references, bounds and CPU emulations shared by tests/test_first_layer_f64_cpu.py (the proof, no GPU)
and tests/test_gpu_first_layer_f64.py (the kernels): the ClusterNet5g stem (csrc/stem.hip, csrc/stem_bwd2.hip), the VGG
first convolution (csrc/firstconv2.hip, csrc/vgg.hip) and the segmentation head (csrc/seg_head.hip).  A plain module.

tests/test_gpu_first_layer_exact.py feeds these kernels {-1, 0, +1} and power-of-two BatchNorm coefficients: exact under
any rounding, hence blind to a truncating store, to BatchNorm applied to a rounded conv output, to statistics or an
arg-max taken from rounded values and to a doubly rounded MFMA operand.  The general-value tests accept all of those
(1e-2 * max, 4e-3 * max, a cosine).  Here the operands carry full mantissas, the coefficients are what a finaliser
produces, and every output is held to a bound derived from the float64 reference of the same operands (tests/parity.py:
fma_acc_bound, pooled_bracket, bf16_bracket).  Every number below is U32, a term count, a magnitude sum or a bf16
spacing -- or a cap / floor stated here and asserted on the reference alone.

Draws.  Stem: `full` x ~ U(-1, 1) in fp32 with a full mantissa; `bf16x` the same draw with x rounded to bf16, so that the
patch operand of the weight-gradient GEMM is exact.  First conv and head: `mixed` and `pos` (absolute values: no
cancellation, the magnitude sum A equals |ref| and every bound is n * U32 relative).  w ~ U(-1, 1) / sqrt(taps * Cin) in
fp32; upstream gradients and the head's features are rounded to bf16.

What a bf16 rounding costs is charged as what it IS: the rounding of an input known exactly (the patch x) costs
|bf16_rne(x) - x| element by element; the rounding of a computed value v known to within e costs half the bf16 spacing
at |v| + e (parity.bf16_half_spacing) -- the kernels round to nearest even (pack_bf16x2 / f32_to_bf16, csrc/common.h).
A relative U16 / 2 would NOT be a bound: half a spacing is 2^-8 |v| just above a power of two.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.conv_f64_cases import (bf16, fold, shorten_mantissa, stat_bounds, stats_of, store_rne,      # noqa: F401
                                  store_truncating)
from tests.parity import (U32, bf16_bracket, bf16_half_spacing, bf16_rne, fma_acc_bound, pool_s2p1,
                          pooled_bracket)

CO = 64
BN_EPS = 1e-5
STEM_DRAWS = ("full", "bf16x")
DRAWS = ("mixed", "pos")
UNDECIDED_CAP = 2e-4        # share of pooling windows whose routing the reference cannot decide; see undecided_windows
DECISIVE_FLOOR = 0.95       # share of pooled-activation brackets that hold one bf16 value; see stem()
UNIT_BCOEF = {"G1": (1.0, 0.0, 0.0), "G2": (0.0, 1.0, 0.0), "G3": (0.0, 0.0, 1.0)}


def _u(rng, shape, scale=1.0):
  return torch.from_numpy((rng.uniform(-1.0, 1.0, shape) * scale).astype(np.float32))


def patches64(x, K=3, pad=1):
  """[N, Cin K K, H W] float64 patch matrix of conv2d(x, w, padding=pad), rows in (c, kh, kw) order."""
  return F.unfold(x.double(), K, padding=pad)


def wgp(patches, dy, K=3):
  """float64 weight gradient from a patch matrix: sum over images and pixels of dy[pix][co] * patch[pix][k]."""
  return torch.einsum("nkp,ncp->ck", patches, dy.double().flatten(2)).reshape(dy.shape[1], -1, K, K)


def wg64(x, dy, K=3, pad=1):
  return wgp(patches64(x, K, pad), dy, K)


# ----------------------------------------------------------------------------------------------------------------------
# pooling windows: position q = 2 rs + cs of window (ho, wo) is conv pixel (2 ho - 1 + rs, 2 wo - 1 + cs), scan order
# ----------------------------------------------------------------------------------------------------------------------
def windows(t, fill):
  """[N, C, H, W] (H, W even) -> [4, N, C, H/2+1, W/2+1]; positions outside the image hold `fill`."""
  tp = F.pad(t, (1, 1, 1, 1), value=fill)
  return torch.stack([tp[:, :, rs::2, cs::2] for rs in (0, 1) for cs in (0, 1)])


def unwindow(parts, H, W):
  """The inverse: four [N, C, Ho, Wo] tensors -> [N, C, H, W] (what fell outside the image is dropped)."""
  n, c = parts[0].shape[:2]
  tp = torch.zeros((n, c, H + 2, W + 2), dtype=parts[0].dtype)
  for q, p in enumerate(parts):
    tp[:, :, (q >> 1)::2, (q & 1)::2] = p
  return tp[:, :, 1:-1, 1:-1].contiguous()


def route(act, dpool):
  """The gradient of max_pool2d(2, 2, padding 1) o ReLU on the conv grid: dpool goes to the FIRST maximum of the window's
  activations in scan order (csrc/stem_common.h window_argmax; torch.argmax returns the first as well), and nowhere when
  that maximum is not positive.  act: the post-ReLU activations the comparison is made on."""
  win = windows(act, -1.0)
  best, am = win.max(0).values, win.argmax(0)
  zero = torch.zeros_like(dpool)
  return unwindow([torch.where((am == q) & (best > 0), dpool, zero) for q in range(4)], act.shape[2], act.shape[3])


def undecided_windows(z, bz):
  """[N, C, Ho, Wo] bool.  A window is undecided when the float64 reference cannot tell which way a kernel whose fp32 z
  lies within bz of it must route: another position's z + bz reaches the top's z - bz while the top can be positive, or
  the top's |z| lies within its bz of zero (routed or not).  The backward tests zero dpool there: the gradient is then
  zero whichever way the kernel routes -- a property of the input, computed from the reference alone."""
  zw, bw = windows(z, -float("inf")), windows(bz, 0.0)
  top, am = zw.max(0).values, zw.argmax(0)
  btop = bw.gather(0, am[None])[0]
  others = (zw + bw).scatter(0, am[None], -float("inf")).max(0).values
  return ((others >= top - btop) & (top + btop > 0)) | (top.abs() <= btop)


# ----------------------------------------------------------------------------------------------------------------------
# stem
# ----------------------------------------------------------------------------------------------------------------------
def stem_coefficients(y, rng):
  """coef [5][64] as a finaliser produces it from the float64 batch statistics of y: scale = gamma / sqrt(var + eps),
  shift = beta - mean * scale (rows 0, 1; the stem kernels read no other), gamma = 1 + 0.2 n with every 7th channel
  negated, beta = 0.1 n; general fp32 values."""
  mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
  gamma = 1.0 + 0.2 * torch.from_numpy(rng.standard_normal(CO))
  gamma[::7] = -gamma[::7]
  beta = 0.1 * torch.from_numpy(rng.standard_normal(CO))
  invstd = 1.0 / torch.sqrt(var + BN_EPS)
  scale = gamma * invstd
  return torch.stack([scale, beta - mean * scale, mean, invstd, var]).float()


def stem_bcoef(rng):
  """[3][64] general fp32 rows c1, c2, c3 of dy = c1 g + c2 y + c3 (bn_bwd_finalize's are of these sizes)."""
  return torch.stack([_u(rng, CO) * 0.5 + torch.sign(_u(rng, CO)), _u(rng, CO) * 0.1, _u(rng, CO) * 0.1])


def stem_reference(x, w, coef, dpool, case):
  """Everything the stem's checks need, from float64 alone.  dpool is zeroed in the undecided windows first."""
  cin, H, W, N = case
  s = dict(case=case, x=x, w=w, coef=coef)
  y = F.conv2d(x.double(), w.double(), padding=1)
  A = F.conv2d(x.double().abs(), w.double().abs(), padding=1)
  b = fma_acc_bound(9 * cin, A)
  sc, sh = (coef[i].double().view(1, -1, 1, 1) for i in (0, 1))
  z, bz, lo, hi = pooled_bracket(y, b, sc, sh)
  und = undecided_windows(z, bz)
  dpool = torch.where(und, torch.zeros_like(dpool), dpool)
  g = route(torch.relu(z), dpool.double())
  nw = N * (H // 2 + 1) * (W // 2 + 1)
  dims = (0, 2, 3)
  ag = g.abs()
  s.update(y=y, A=A, b=b, z=z, bz=bz, pool_lo=lo, pool_hi=hi, pool=pool_s2p1(torch.relu(z)), undecided=und,
           undecided_share=float(und.double().mean()), decisive=float((lo == hi).double().mean()), dpool=dpool, g=g,
           count=N * H * W, windows=nw)
  s["stat_tol"] = stat_bounds(y, b, N * H * W)
  # sum g: dpool values are bf16, the per-thread fp32 partial sums cost what an nw-term accumulation costs
  s["sum_g"], s["tol_sum_g"] = g.sum(dims), fma_acc_bound(nw, ag.sum(dims))
  # sum g*y on the fp32 accumulator: |g| b for the accumulator, then the products and their partial sums
  s["sum_gy"] = (g * y).sum(dims)
  s["tol_sum_gy"] = (ag * b).sum(dims) + fma_acc_bound(nw, (ag * (y.abs() + b)).sum(dims))
  return s


@functools.lru_cache(maxsize=4)
def stem(case, draw):
  assert draw in STEM_DRAWS
  cin, H, W, N = case
  rng = np.random.default_rng([7, cin, H, W, N])
  x = _u(rng, (N, cin, H, W))
  if draw == "bf16x":
    x = bf16(x)
  w = _u(rng, (CO, cin, 3, 3), 1.0 / math.sqrt(9 * cin))
  dpool = bf16(_u(rng, (N, CO, H // 2 + 1, W // 2 + 1)))
  coef = stem_coefficients(F.conv2d(x.double(), w.double(), padding=1), rng)
  s = stem_reference(x, w, coef, dpool, case)
  s["bcoef"] = stem_bcoef(rng)
  s["draw"] = draw
  return s


def _c(bcoef, i):
  return torch.as_tensor(bcoef, dtype=torch.float32)[i].double().view(1, -1, 1, 1)


def _exact_factor(c):
  return (c == 0) | (c.abs() == 1)


def stem_dw_two_pass(s, bcoef, exact_patch=False):
  """ref, tol of iic_stem_bwd_wgrad (stem_bwd_kernel<CIN, 1>): dW = sum bf16(fl(c1 g + c2 acc + c3)) * bf16(x) on the bf16
  MFMA, fp32 accumulation, partials folded in fp32.
    e32  |fl(c1 g + c2 acc + c3) - dy|: |c2| b for the accumulator, and at most four roundings (two products, two sums, any
         of them fused away), each within U32 of a partial result that m = |c1 g| + |c2| (|y| + b) + |c3| bounds.  A
         product by 0 or +-1 and a sum with 0 are exact: a channel with two such coefficients and a zero third has e32 = 0;
    e16  the RNE of that value: half a spacing at |dy| + e32 -- nothing where e32 = 0 and dy is a bf16 value (g is);
    ex   |bf16_rne(x) - x|, known exactly (zero in the bf16x draw);
  tol = wg(ex, |dy|) + wg(|xh|, e32 + e16) + fma_acc_bound(N H W, wg(|xh|, |dy| + e32 + e16)): the products of two bf16
  values are exact in fp32, the rest is the accumulation.
  exact_patch: x is an input, so bf16_rne(x) is known exactly; the reference is then the float64 sum dy * bf16_rne(x) and
  the wg(ex, |dy|) term falls away -- the sharper of the two checks (it implies the other by the triangle inequality)."""
  key = ("two", torch.as_tensor(bcoef, dtype=torch.float32).numpy().tobytes())
  if key not in s:
    c1, c2, c3 = (_c(bcoef, i) for i in range(3))
    g, y, b = s["g"], s["y"], s["b"]
    dy = c1 * g + c2 * y + c3
    m = (c1 * g).abs() + c2.abs() * (y.abs() + b) + c3.abs()
    nround = ((~_exact_factor(c1)).double() + (~_exact_factor(c2)).double() + ((c1 != 0) & (c2 != 0)).double() +
              (c3 != 0).double())
    e32 = c2.abs() * b + nround * U32 * m * (1 + 4 * U32)
    e16 = torch.where((e32 == 0) & (bf16_rne(dy) == dy), torch.zeros_like(dy), bf16_half_spacing(dy, e32))
    edy = e32 + e16
    P = _stem_patches(s)
    tol = wgp(P["axh"], edy) + fma_acc_bound(s["count"], wgp(P["axh"], dy.abs() + edy))
    s[key] = (wgp(P["x"], dy), tol + wgp(P["ex"], dy.abs()), wgp(P["xh"], dy), tol)
  return s[key][2:] if exact_patch else s[key][:2]


def _stem_patches(s):
  """Patch matrices of x, bf16_rne(x), its magnitude and the rounding's own error |bf16_rne(x) - x|, made once."""
  if "_patches" not in s:
    x = s["x"].double()
    xh = bf16_rne(x)
    s["_patches"] = dict(x=patches64(x), xh=patches64(xh), axh=patches64(xh.abs()), ex=patches64((xh - x).abs()))
  return s["_patches"]


def _g3_magnitude(x):
  """Per (c, kh, kw): the magnitudes that enter G3 = T - R[kh] - C[kw] + X[kh][kw] of stem_patch_sums_kernel."""
  a = x.double().abs()
  T = a.sum((0, 2, 3))
  rows = {0: a[:, :, -1].sum((0, 2)), 1: torch.zeros_like(T), 2: a[:, :, 0].sum((0, 2))}
  cols = {0: a[:, :, :, -1].sum((0, 2)), 1: torch.zeros_like(T), 2: a[:, :, :, 0].sum((0, 2))}
  mag = torch.zeros((x.shape[1], 3, 3), dtype=torch.float64)
  for kh in range(3):
    for kw in range(3):
      X = a[:, :, {0: -1, 2: 0}[kh], {0: -1, 2: 0}[kw]].sum(0) if kh != 1 and kw != 1 else torch.zeros_like(T)
      mag[:, kh, kw] = T + rows[kh] + cols[kw] + X
  return mag


def stem_dw_one_pass(s, bcoef, exact_patch=False):
  """ref, tol of iic_stem_bwd_fused + iic_stem_wgrad_combine (stem_bwd_kernel<CIN, 2> and stem_bwd2_kernel):
    G1 = sum bf16(g) bf16(x): g is a bf16 value -- with bf16x the products are exact and the bound is the accumulation's;
    G2 = sum bf16(acc) bf16(x): b + half a spacing at |y| + b on the y operand;
    G3 = T - R - C + X on fp32 sums of x (stem_patch_sums_kernel): the fp32 summation bound on the magnitudes that enter;
    dW = fl(c1 G1 + c2 G2 + c3 G3): five roundings, each within U32 (1 + U32)^4 < 1.2 U32 of the magnitudes' sum.
  exact_patch: G1 and G2 against the float64 sums over bf16_rne(x), as in stem_dw_two_pass (G3 never rounds x)."""
  c = [torch.as_tensor(bcoef, dtype=torch.float32)[i].double().view(-1, 1, 1, 1) for i in range(3)]
  key = ("one", bool(exact_patch))
  if key not in s:
    g, y, b = s["g"], s["y"], s["b"]
    n = s["count"]
    P = _stem_patches(s)
    ey = b + bf16_half_spacing(y, b)
    keep = 0.0 if exact_patch else 1.0
    xr = P["xh"] if exact_patch else P["x"]
    G = [wgp(xr, g), wgp(xr, y), wgp(P["x"], torch.ones_like(y))]
    t = [keep * wgp(P["ex"], g.abs()) + fma_acc_bound(n, wgp(P["axh"], g.abs())),
         keep * wgp(P["ex"], y.abs()) + wgp(P["axh"], ey) + fma_acc_bound(n, wgp(P["axh"], y.abs() + ey)),
         fma_acc_bound(n, _g3_magnitude(s["x"]), extra=3)[None].expand(CO, -1, -1, -1)]
    s[key] = (G, t)
  G, t = s[key]
  ref = sum(ci * Gi for ci, Gi in zip(c, G))
  mag = sum(ci.abs() * (Gi.abs() + ti) for ci, Gi, ti in zip(c, G, t))
  tol = sum(ci.abs() * ti for ci, ti in zip(c, t)) + 6 * U32 * mag
  return ref, tol


def unit_bcoef(which):
  return torch.tensor(UNIT_BCOEF[which]).view(3, 1).expand(3, CO).contiguous()


# ---- CPU emulation of the stem, correct by default, one seeded defect per knob ---------------------------------------
def stem_emulate(x, w, coef, bcoef, dpool, chunks=1, order=None, store=store_rne, bn_on_rounded=False,
                 stats_from_rounded=False, argmax_on_rounded=False, gy_with_rounded_y=False, patch_store=store_rne,
                 y_rounded_before_affine=False, wg_chunks=1, wg_order=None):
  """fp32 pipeline in the kernels' order and precision (F.conv2d in fp32 over `chunks` slices of the taps' channels,
  folded in `order`; unfused affine map; one RNE store; bf16 operands of the dW GEMMs exactly where the kernels round
  them).  Knobs: (a) store = store_truncating; (b) bn_on_rounded; (c) stats_from_rounded; (d) argmax_on_rounded; (e)
  gy_with_rounded_y; (f) patch_store = store_truncating, y_rounded_before_affine."""
  cin, H, W = x.shape[1], x.shape[2], x.shape[3]
  groups = torch.arange(cin).chunk(min(chunks, cin))
  acc = fold([F.conv2d(x[:, g_].contiguous(), w[:, g_].contiguous(), padding=1) for g_ in groups], order)
  sc, sh = (coef[i].view(1, -1, 1, 1) for i in (0, 1))
  zin = store_rne(acc) if bn_on_rounded else acc
  act = torch.relu(zin * sc + sh)
  out = dict(acc=acc, pool=pool_s2p1(store(act)), stats=stats_of(store_rne(acc) if stats_from_rounded else acc))
  g = route(store_rne(act) if argmax_on_rounded else torch.relu(acc * sc + sh), dpool)
  yq = store_rne(acc)
  out["g"] = g
  out["sum_g"] = g.double().sum((0, 2, 3))
  out["sum_gy"] = (g * (yq if gy_with_rounded_y else acc)).double().sum((0, 2, 3))
  c1, c2, c3 = (bcoef[i].view(1, -1, 1, 1) for i in range(3))
  xh = patch_store(x)

  def wg(t):
    parts = [torch.nn.grad.conv2d_weight(xh[i_].contiguous(), tuple(w.shape), t[i_].contiguous(), padding=1)
             for i_ in torch.arange(x.shape[0]).chunk(min(wg_chunks, x.shape[0]))]
    return fold(parts, wg_order)
  out["dW_two_pass"] = wg(store_rne(c1 * g + c2 * (yq if y_rounded_before_affine else acc) + c3))
  G1, G2 = wg(store_rne(g)), wg(yq)
  G3 = torch.nn.grad.conv2d_weight(x, tuple(w.shape), torch.ones_like(acc), padding=1)
  out.update(G1=G1, G2=G2, G3=G3)
  k1, k2, k3 = (bcoef[i].view(-1, 1, 1, 1) for i in range(3))
  out["dW_one_pass"] = k1 * G1 + k2 * G2 + k3 * G3
  return out


def stem_emulate_case(s, bcoef=None, **knobs):
  return stem_emulate(s["x"], s["w"], s["coef"], s["bcoef"] if bcoef is None else bcoef, s["dpool"], **knobs)


# ----------------------------------------------------------------------------------------------------------------------
# first conv
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def firstconv(case, draw):
  """Output bracket, statistic tolerances and the weight gradient's bound.  Forward: fp32 x and w on the exact-fp32 MFMA,
  K K Cin terms, one RNE store, statistics from the accumulators.  Weight gradient: bf16 dy widened exactly times fp32
  patches, N H W terms, fp32 partials folded in a fixed order (joins of partials of the same sum: fma_acc_bound)."""
  assert draw in DRAWS
  cin, K, H, W, N = case
  pad = (K - 1) // 2
  rng = np.random.default_rng([11, cin, K, H, W, N])
  x = _u(rng, (N, cin, H, W))
  w = _u(rng, (CO, cin, K, K), 1.0 / math.sqrt(K * K * cin))
  dy = bf16(_u(rng, (N, CO, H, W)))
  if draw == "pos":
    x, w, dy = x.abs(), w.abs(), dy.abs()
  y = F.conv2d(x.double(), w.double(), padding=pad)
  A = F.conv2d(x.double().abs(), w.double().abs(), padding=pad)
  b = fma_acc_bound(K * K * cin, A)
  lo, hi = bf16_bracket(y, b)
  s = dict(case=case, draw=draw, x=x, w=w, dy=dy, K=K, pad=pad, y=y, A=A, b=b, lo=lo, hi=hi, count=N * H * W,
           stat_tol=stat_bounds(y, b, N * H * W), decisive=float((lo == hi).double().mean()))
  s["dW"] = wg64(x, dy, K, pad)
  s["tol_dW"] = fma_acc_bound(N * H * W, wg64(x.abs(), dy.abs(), K, pad))
  return s


def firstconv_emulate(s, chunks=1, order=None, store=store_rne, stats_from_rounded=False, wg_chunks=2, wg_order=None,
                      on_part=None, wg_bands=1):
  """fp32 F.conv2d (chunked over the input channels), one store; the weight gradient as fp32 partials per image and band
  of output rows (dy zeroed outside the band) folded in `wg_order`, on_part(part0) damaging the first one (defect g)."""
  x, w, dy, pad = s["x"], s["w"], s["dy"], s["pad"]
  groups = torch.arange(x.shape[1]).chunk(min(chunks, x.shape[1]))
  acc = fold([F.conv2d(x[:, g_].contiguous(), w[:, g_].contiguous(), padding=pad) for g_ in groups], order)
  parts = []
  for i_ in torch.arange(x.shape[0]).chunk(min(wg_chunks, x.shape[0])):
    for rows in torch.arange(x.shape[2]).chunk(wg_bands):
      band = torch.zeros_like(dy[i_])
      band[:, :, rows] = dy[i_][:, :, rows]
      parts.append(torch.nn.grad.conv2d_weight(x[i_].contiguous(), tuple(w.shape), band, padding=pad))
  if on_part:
    parts[0] = on_part(parts[0])
  return dict(acc=acc, out=store(acc), stats=stats_of(store_rne(acc) if stats_from_rounded else acc),
              dW=fold(parts, wg_order))


# ----------------------------------------------------------------------------------------------------------------------
# segmentation head
# ----------------------------------------------------------------------------------------------------------------------
SHW_ROWS = 1024      # csrc/seg_head.hip: window rows per weight-gradient chunk


def seg_chunks(M):
  return (M + SHW_ROWS - 1) // SHW_ROWS


@functools.lru_cache(maxsize=4)
def seg_head(case, draw):
  """logits [M][k] (C terms, fp32), dx (k terms, RNE to bf16, interior of the window) and dW [k][C] (M terms and the
  chunk fold) of conv2d(f, w, 1x1, padding 1): bf16 features widened exactly, fp32 W, bf16 upstream gradient."""
  assert draw in DRAWS
  C, k, N, Hf = case
  rng = np.random.default_rng([13, C, k, N, Hf])
  f = bf16(_u(rng, (N, C, Hf, Hf)))
  w = _u(rng, (k, C, 1, 1), 1.0 / math.sqrt(C))
  dlog = bf16(_u(rng, (N, k, Hf + 2, Hf + 2)))
  if draw == "pos":
    f, w, dlog = f.abs(), w.abs(), dlog.abs()
  M = N * (Hf + 2) * (Hf + 2)
  rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, -1)
  f64, w64, d64 = f.double(), w.double().view(k, C), dlog.double()
  logits = rows(F.conv2d(f64, w.double(), padding=1))
  A_log = rows(F.conv2d(f64.abs(), w.double().abs(), padding=1))
  din = d64[:, :, 1:-1, 1:-1]                                        # the gradient that reaches the features
  dx = torch.einsum("njyx,jc->ncyx", din, w64)
  b_dx = fma_acc_bound(k, torch.einsum("njyx,jc->ncyx", din.abs(), w64.abs()))
  lo, hi = bf16_bracket(dx, b_dx)
  dW = torch.einsum("njyx,ncyx->jc", din, f64)
  A_dW = torch.einsum("njyx,ncyx->jc", din.abs(), f64.abs())
  return dict(case=case, draw=draw, f=f, w=w, dlog=dlog, M=M, logits=logits, dlog_rows=rows(d64).contiguous(),
              tol_logits=fma_acc_bound(C, A_log, extra=1), dx=dx, b_dx=b_dx, dx_lo=lo, dx_hi=hi,
              decisive=float((lo == hi).double().mean()), dW=dW, A_dW=A_dW)


def seg_dx_bracket(dlog_rows, w, N, Hw, Ww):
  """ref, b, lo, hi (NCHW, the window's interior) of the head's feature gradient dx[m][c] = sum_j dlog[m][j] W[j][c] for
  the fp32 dlog rows [N Hw Ww][k] a backward pass actually used: k products of fp32 operands, one RNE store."""
  k, C = w.shape[0], w.shape[1]
  din = dlog_rows.detach().cpu().double().view(N, Hw, Ww, k)[:, 1:-1, 1:-1]
  w64 = w.detach().cpu().double().view(k, C)
  dx = torch.einsum("nyxj,jc->ncyx", din, w64)
  b = fma_acc_bound(k, torch.einsum("nyxj,jc->ncyx", din.abs(), w64.abs()))
  return (dx, b) + bf16_bracket(dx, b)


def seg_dw_tol(s, folds):
  return fma_acc_bound(s["M"], s["A_dW"], extra=folds)


def seg_emulate(s, chunks=1, order=None, on_acc=None, store=store_rne, wg_chunks=2, wg_order=None, on_part=None):
  """fp32: logits over `chunks` slices of the channels folded in `order` (on_acc damages the running sum: defect h);
  dx stored once; dW as fp32 partials over runs of window rows (on_part damages the first: defect g)."""
  f, w, dlog = s["f"], s["w"], s["dlog"]
  C, k = w.shape[1], w.shape[0]
  groups = torch.arange(C).chunk(chunks)
  acc = fold([F.conv2d(f[:, g_].contiguous(), w[:, g_].contiguous(), padding=1) for g_ in groups], order, on_acc)
  din = dlog[:, :, 1:-1, 1:-1]
  dx = torch.einsum("njyx,jc->ncyx", din, w.view(k, C))
  dm, fm = din.permute(0, 2, 3, 1).reshape(-1, k), f.permute(0, 2, 3, 1).reshape(-1, C)
  parts = [dm[i_].t() @ fm[i_] for i_ in torch.arange(dm.shape[0]).chunk(wg_chunks)]
  if on_part:
    parts[0] = on_part(parts[0])
  return dict(logits=acc.permute(0, 2, 3, 1).reshape(s["M"], k), dx=store(dx), dW=fold(parts, wg_order))


# ----------------------------------------------------------------------------------------------------------------------
# the criteria the suite already had (tests/test_gpu_kernels.py test_stem_forward_backward, tests/test_gpu_vgg.py
# test_firstconv_forward_and_wgrad, tests/test_gpu_seg_net.py test_seg_head_forward_backward)
# ----------------------------------------------------------------------------------------------------------------------
def old_accepts_max(got, ref, rel):
  return float((got.double() - ref.double()).abs().max()) <= rel * float(ref.abs().max())


def old_accepts_stats(st, y, count, atol1, atol2):
  m1, m2 = y.mean((0, 2, 3)), (y * y).mean((0, 2, 3))
  return bool(((st[0] / count - m1).abs() <= atol1).all()) and bool(((st[1] / count - m2).abs() <= atol2 + 1e-4 * m2.abs()).all())


def old_accepts_cos(got, ref):
  a, r = got.double().flatten(), ref.double().flatten()
  return float((a * r).sum() / (a.norm() * r.norm())) >= 0.9999


def old_accepts_allclose(got, ref, rtol, atol_rel):
  return bool(((got.double() - ref).abs() <= atol_rel * float(ref.abs().max()) + rtol * ref.abs()).all())

