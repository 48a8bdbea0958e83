"""Cases, float64 restatements and derived bounds shared by tests/test_seg_baseline_cpu.py (the proof, no GPU) and
tests/test_gpu_seg_baseline.py (csrc/seg_patches.hip, the iic_pair_* entries of csrc/sup_head.hip,
csrc/seg_baseline_loss.hip, iic_amd/archs/seg_baselines.py, iic_amd/seg_baselines.py).  A plain module, not a test file.

What is restated, with the reference's lines:
  sample64 / adjoint64   code/archs/segmentation/baselines/net10a_isola.py:92 (F.interpolate, bilinear, align_corners=False)
                         followed by code/utils/segmentation/baselines/general.py:4-18 (get_patches), and its adjoint
  pair_products64        net10a_isola.py:52-58 + :29 (flatten both patches in (c, h, w) order, torch.cat, nn.Linear)
  isola_ref              code/utils/segmentation/baselines/isola_utils.py:27-72
  doersch_ref            code/utils/segmentation/baselines/doersch_utils.py:55-66

Bounds (U32 = 2^-24 per fp32 operation, U64 = 2^-53 per float64 operation, tests/parity.py):
  sampler forward   no bound: bit-equal to float64 on the dyadic lattice, bit-equal to bf16(iic_seg_feat_sample) elsewhere
  sampler adjoint   adjoint_bound: per element T terms g * (wy wx); a term passes through the roundings of 1 - l (one per
                    axis), of the sum of two taps that the far-edge clamp folds onto one row (one per axis), of wy wx, of
                    g w and of at most T additions: (T + 6) U32 / (1 - (T + 6) U32) * A, A = sum |g| wy wx in float64
                    with the fp32 interpolation weights (the kernel's own: they are inputs of the restatement, not
                    results).  One RNE store for bf16: parity.bf16_bracket.
  pair Linear       the bounds of tests/sup_head_cases.py with K -> 2 K: forward conv_acc_bound(2 K, A, extra = S), weight
                    gradient conv_acc_bound(N, A), backward-data bf16_bracket(ref, conv_acc_bound(F, A))
  losses            one fp32 rounding of a float64 computation: isola_bounds, doersch_bounds below
"""
import collections
import functools

import numpy as np
import torch

from tests.parity import U32, U64, bf16_bracket, conv_acc_bound

P_TRUNK = 3      # border of the trunk's PT tensors (SegmentationNet10aTrunk.P)
EPS = 2.0 ** -52      # sys.float_info.epsilon (isola_utils.py:11)


# ----------------------------------------------------------------------------------------------------------------------
# sampler
# ----------------------------------------------------------------------------------------------------------------------
SCase = collections.namedtuple("SCase", "name N C Hl S p centre other")
# S = 16 over Hl = 8: scale 1/2, interpolation weights 1/4 and 3/4 -- dyadic, so integer features stay exact
BASE = dict(N=2, C=64, Hl=8, S=16)
LATTICE_CASES = (
  SCase("inside_p3", centre=(6, 7), other=(10, 4), p=3, **BASE),
  SCase("top_left_p3", centre=(1, 1), other=(9, 9), p=3, **BASE),            # clamped taps at rows / columns 0
  SCase("bottom_right_p3", centre=(14, 14), other=(5, 6), p=3, **BASE),     # clamped taps at the far edges
  SCase("top_right_p5", centre=(2, 13), other=(13, 2), p=5, **BASE),        # the other two borders
  SCase("adjacent_p3", centre=(6, 6), other=(6, 9), p=3, **BASE),           # neighbouring blocks: footprints overlap
  SCase("same_p3", centre=(8, 8), other=(8, 8), p=3, **BASE),               # centre == other
  SCase("c512_p3", centre=(3, 12), other=(11, 5), p=3, N=2, C=512, Hl=8, S=16),
)
# the trunk's real ratio, Hl = S / 2 - 4: weights with full mantissas
RATIO_CASES = (
  SCase("ratio_p3", centre=(7, 9), other=(10, 12), p=3, N=2, C=64, Hl=6, S=20),
  SCase("ratio_p5", centre=(2, 17), other=(17, 2), p=5, N=2, C=64, Hl=6, S=20),
)


def src(d, size, S):
  """(i0, i1, lam) of destination index d: the operations of sk_src (csrc/seg_bilinear.h) in fp32.  The fused
  multiply-add is one rounding of the exact value, which float64 holds (at most 9 x 24 significant bits)."""
  scale = np.float32(size) / np.float32(S)
  s = np.float32(np.float64(np.float32(d) + np.float32(0.5)) * np.float64(scale) - 0.5)
  if s < 0:
    s = np.float32(0.0)
  i0 = min(int(s), size - 1)
  i1 = i0 + (1 if i0 < size - 1 else 0)
  return i0, i1, np.float32(s - np.float32(i0))


def taps(c, size, S, p):
  d = p // 2
  return [src(c - d + i, size, S) for i in range(p)]


def _axis_matrix(c, size, S, p, swap=False):
  """[p, size] float64: row i holds the two interpolation weights of patch index i (fp32 values, widened) -- summed where
  both taps fall on one source index; and the boolean 'touched' matrix."""
  W = np.zeros((p, size))
  T = np.zeros((p, size), dtype=bool)
  for i, (i0, i1, lam) in enumerate(taps(c, size, S, p)):
    w0, w1 = 1.0 - np.float64(lam), np.float64(lam)
    if swap:
      w0, w1 = w1, w0
    W[i, i0] += w0
    W[i, i1] += w1
    T[i, i0] = T[i, i1] = True
  return W, T


def points(case):
  return (case.centre, case.other)


def sample64(x, case, swap=False):
  """float64 [2 N, C, p, p] patches of x [N, C, Hl, Hl] (float64): images 0 .. N - 1 the centre patch.  swap: the
  seeded defect 'a swapped tap weight' (l and 1 - l exchanged along x)."""
  out = []
  for (cy, cx) in points(case):
    Wy, _ = _axis_matrix(cy, case.Hl, case.S, case.p)
    Wx, _ = _axis_matrix(cx, case.Hl, case.S, case.p, swap=swap)
    out.append(np.einsum("ih,nchw,jw->ncij", Wy, x, Wx))
  return np.concatenate(out, axis=0)


def adjoint64(g, case, patches=(0, 1)):
  """(dx, A, T): float64 adjoint of sample64 for g [2 N, C, p, p], the same sum over the magnitudes, and the number of
  contributing patch pixels per source pixel [Hl, Hl].  patches=(0,): the defect 'a missing second patch'."""
  N = case.N
  dx = np.zeros((N, case.C, case.Hl, case.Hl))
  A = np.zeros_like(dx)
  T = np.zeros((case.Hl, case.Hl), dtype=np.int64)
  for q, (cy, cx) in enumerate(points(case)):
    if q not in patches:
      continue
    Wy, Ty = _axis_matrix(cy, case.Hl, case.S, case.p)
    Wx, Tx = _axis_matrix(cx, case.Hl, case.S, case.p)
    gq = g[q * N:(q + 1) * N]
    dx += np.einsum("ih,ncij,jw->nchw", Wy, gq, Wx)
    A += np.einsum("ih,ncij,jw->nchw", Wy, np.abs(gq), Wx)
    T += Ty.sum(0)[:, None] * Tx.sum(0)[None, :]
  return dx, A, T


def adjoint_bound(A, T):
  n = (T + 6).astype(np.float64)[None, None]
  assert float(n.max()) * U32 < 1
  return n * U32 / (1.0 - n * U32) * A


def emu_adjoint_f32(g, case, patches=(0, 1)):
  """The gather of seg_patch_bwd_kernel in numpy float32, operation by operation and in its order: centre patch before
  other patch, patch pixels in ascending (i, j); acc <- acc + g * (wy wx), each rounded on its own."""
  N = case.N
  one = np.float32(1.0)
  acc = np.zeros((N, case.C, case.Hl, case.Hl), dtype=np.float32)
  for q, (cy, cx) in enumerate(points(case)):
    if q not in patches:
      continue
    ty, tx = taps(cy, case.Hl, case.S, case.p), taps(cx, case.Hl, case.S, case.p)
    gq = g[q * N:(q + 1) * N].astype(np.float32)
    for i, (y0, y1, ly) in enumerate(ty):
      for j, (x0, x1, lx) in enumerate(tx):
        for h in sorted({y0, y1}):
          wy = np.float32((one - ly if y0 == h else np.float32(0)) + (ly if y1 == h else np.float32(0)))
          for w in sorted({x0, x1}):
            wx = np.float32((one - lx if x0 == w else np.float32(0)) + (lx if x1 == w else np.float32(0)))
            acc[:, :, h, w] = acc[:, :, h, w] + gq[:, :, i, j] * np.float32(wy * wx)
  return acc


def lattice_features(case, seed=0):
  """Integers in -8 .. 8 as float64 [N, C, Hl, Hl]: with the lattice's weights (0, 1/4, 3/4, 1 per axis) every
  intermediate of the blend is a multiple of 1/16 of magnitude at most 8 -- exact in fp32 whatever is fused, and at most
  8 significant bits: a bf16 value."""
  rng = np.random.default_rng([21, case.N, case.C, case.Hl, case.p, seed])
  return rng.integers(-8, 9, (case.N, case.C, case.Hl, case.Hl)).astype(np.float64)


def lattice_grads(case, seed=0):
  """Integers in -4 .. 4 as float64 [2 N, C, p, p]."""
  rng = np.random.default_rng([22, case.N, case.C, case.Hl, case.p, seed])
  return rng.integers(-4, 5, (2 * case.N, case.C, case.p, case.p)).astype(np.float64)


def mantissa_features(case, seed=0):
  """bf16-valued full-range draws (float64)."""
  rng = np.random.default_rng([23, case.N, case.C, case.Hl, case.p, seed])
  x = torch.from_numpy(rng.uniform(-1.0, 1.0, (case.N, case.C, case.Hl, case.Hl)).astype(np.float32))
  return x.to(torch.bfloat16).double().numpy()


def mantissa_grads(case, seed=0):
  rng = np.random.default_rng([24, case.N, case.C, case.Hl, case.p, seed])
  g = torch.from_numpy(rng.uniform(-1.0, 1.0, (2 * case.N, case.C, case.p, case.p)).astype(np.float32))
  return g.to(torch.bfloat16).double().numpy()


def to_pt(x, P, dtype, fill=0.0):
  """[N, C, H, W] (numpy or tensor) -> PT tensor [N, H + 2P, W + 2P, C] on the host, border = fill."""
  x = torch.as_tensor(x)
  n, c, h, w = x.shape
  out = torch.full((n, h + 2 * P, w + 2 * P, c), fill, dtype=dtype)
  out[:, P:P + h, P:P + w] = x.permute(0, 2, 3, 1).to(dtype)
  return out


def from_pt(pt, P):
  """interior of a PT tensor -> [N, C, H, W] float64 numpy."""
  return pt[:, P:pt.shape[1] - P, P:pt.shape[2] - P].permute(0, 3, 1, 2).double().cpu().contiguous().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# joint Linear
# ----------------------------------------------------------------------------------------------------------------------
PCase = collections.namedtuple("PCase", "name N C p F")
PAIR_SHAPES = ((64, 3, 64), (64, 3, 128), (1024, 3, 1024))
PAIR_NS = (1, 3, 130)
PAIR_CASES = tuple(PCase("N%d_C%d_p%d_F%d" % (N, C, p, F), N, C, p, F) for (C, p, F) in PAIR_SHAPES for N in PAIR_NS)


def pair_K(case):
  return case.C * case.p * case.p


@functools.lru_cache(maxsize=2)
def pair_lattice(case):
  """a0, a1 in {-1, 0, 1, 2} [N, C, p, p], w in {-2 .. 2} [F, 2 K], b in {-3 .. 3}, dy in {-2 .. 2} [N, F]: every partial
  sum of the three products is an integer below 2^24 (2 K * 4 <= 73 728), exact in fp32 in any order.  Shared, never
  modified."""
  rng = np.random.default_rng([31, case.N, case.C, case.p, case.F])
  K = pair_K(case)
  f = lambda lo, hi, shape: torch.from_numpy(rng.integers(lo, hi, shape).astype(np.float32))
  return dict(a0=f(-1, 3, (case.N, case.C, case.p, case.p)), a1=f(-1, 3, (case.N, case.C, case.p, case.p)),
              w=f(-2, 3, (case.F, 2 * K)), b=f(-3, 4, (case.F,)), dy=f(-2, 3, (case.N, case.F)))


@functools.lru_cache(maxsize=2)
def pair_mantissa(case):
  """a0, a1 bf16-valued; w, b, dy with full fp32 mantissas (the kernels round w and dy)."""
  rng = np.random.default_rng([32, case.N, case.C, case.p, case.F])
  K = pair_K(case)
  u = lambda shape, s=1.0: torch.from_numpy((rng.uniform(-1.0, 1.0, shape) * s).astype(np.float32))
  b16 = lambda t: t.to(torch.bfloat16).float()
  return dict(a0=b16(u((case.N, case.C, case.p, case.p))), a1=b16(u((case.N, case.C, case.p, case.p))),
              w=u((case.F, 2 * K), 1.0 / np.sqrt(2 * K)), b=u((case.F,), 0.1), dy=u((case.N, case.F)))


def pair_products64(a0, a1, w, b, dy, exchange=False):
  """(y, Ay, dW, AdW, dx0, dx1, Adx0, Adx1) in float64 on the operands as given: the flatten of both activations in
  (c, h, w) order, concatenated (net10a_isola.py:52-58), against w [F, 2 K].  exchange: the defect 'the halves of w
  exchanged'."""
  N = a0.shape[0]
  cat = torch.cat([a0.reshape(N, -1), a1.reshape(N, -1)], dim=1).double()
  wd, dyd = w.double(), dy.double()
  K = cat.shape[1] // 2
  if exchange:
    wd = torch.cat([wd[:, K:], wd[:, :K]], dim=1)
  y = cat @ wd.t() + b.double()
  Ay = cat.abs() @ wd.abs().t() + b.double().abs()
  dW = dyd.t() @ cat
  AdW = dyd.abs().t() @ cat.abs()
  dx = dyd @ wd
  Adx = dyd.abs() @ wd.abs()
  sh = a0.shape
  return y, Ay, dW, AdW, dx[:, :K].reshape(sh), dx[:, K:].reshape(sh), Adx[:, :K].reshape(sh), Adx[:, K:].reshape(sh)


def pair_forward_bound(case, A, nsplit):
  return conv_acc_bound(2 * pair_K(case), A, extra=nsplit)


def pair_wgrad_bound(case, A):
  return conv_acc_bound(case.N, A)


def pair_dx_bracket(case, ref, A):
  b = conv_acc_bound(case.F, A)
  return (b,) + bf16_bracket(ref, b)


def emu_pair_forward(a0, a1, wb, b, chunks=1):
  """fp32 forward with the 2 K axis cut into `chunks` slices added in index order, then the bias."""
  N = a0.shape[0]
  cat = torch.cat([a0.reshape(N, -1), a1.reshape(N, -1)], dim=1)
  acc = None
  for g in torch.arange(cat.shape[1]).chunk(chunks):
    part = cat[:, g] @ wb[:, g].t()
    acc = part if acc is None else acc + part
  return acc + b


# ----------------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------------
LOSS_NS = (1, 5, 257)
S_MASK = 12
LOSS_POINTS = ((3, 4), (8, 2))      # (cy, cx), (oy, ox) inside the S_MASK map


def loss_mask(N, mode, seed=0):
  """uint8 [N, S, S] and the per-row mask it implies.  mode: 'mixed' -- rows cycle through neither / centre only / other
  only / both points set (values 1 or 255: the sum must not wrap) --, 'none', 'all'."""
  rng = np.random.default_rng([41, N, seed])
  mask = (rng.integers(0, 2, (N, S_MASK, S_MASK)) * rng.choice([1, 255], (N, S_MASK, S_MASK))).astype(np.uint8)
  (cy, cx), (oy, ox) = LOSS_POINTS
  for n in range(N):
    kind = {"mixed": (n + 1) % 4, "none": 0, "all": 3}[mode]
    mask[n, cy, cx] = (255 if n % 2 else 1) if kind & 1 else 0
    mask[n, oy, ox] = (255 if n % 3 else 1) if kind & 2 else 0
  m = ((mask[:, cy, cx].astype(np.int64) + mask[:, oy, ox].astype(np.int64)) > 0).astype(np.float64)
  return mask, m


def isola_probs(N, seed=0):
  """fp32 [N]: the special values first (0, EPS / 2, 2 EPS, 1 - 2^-24, 1 as far as N allows), then ordinary rows."""
  rng = np.random.default_rng([42, N, seed])
  p = rng.uniform(0.02, 0.98, N).astype(np.float32)
  special = np.array([0.0, EPS / 2, 2 * EPS, 1.0 - 2.0 ** -24, 1.0], dtype=np.float32)
  if N >= 5:
    p[:5] = special
  else:
    p[:N] = special[1:1 + N]
  return p


def isola_ref(p, m, adjacent):
  """(loss, dp, mag, dropped) in float64 (isola_utils.py:27-72): t = p or fl32(1 - p); dropped iff t < EPS; loss =
  -(1 / norm) sum m keep log t; dp = -+ m / (norm t), 0 for dropped rows.  mag = sum m keep |log t| / norm."""
  p = np.asarray(p, dtype=np.float32)
  t32 = p if adjacent else (np.float32(1.0) - p).astype(np.float32)
  drop = t32 < np.float32(EPS)
  t = np.where(drop, EPS, t32.astype(np.float64))
  keep = (~drop).astype(np.float64)
  norm = m.sum()
  with np.errstate(divide="ignore", invalid="ignore"):
    terms = m * keep * np.log(t)
    loss = -(1.0 / norm) * terms.sum()
    dp = np.where(drop, 0.0, (-1.0 if adjacent else 1.0) * (m / norm) / t)
    if norm == 0:
      dp = np.full_like(dp, np.nan)
    mag = np.abs(terms).sum() / norm
  return loss, dp, mag, drop


def isola_bounds(loss, dp, mag, N):
  """One fp32 rounding of a float64 computation.  Loss: per row log (charged 2), two products with 0 / 1 (exact), N
  additions, 1 / norm and the final product: n = N + 4, doubled for the restatement's own error.  dp: m / norm, the
  division by t and the sign: 3 roundings, doubled."""
  n = 2.0 * (N + 4)
  return U32 * abs(loss) + n * U64 / (1 - n * U64) * mag, U32 * np.abs(dp) + 6 * U64 * np.abs(dp)


def doersch_logits(N, k=9, seed=0):
  rng = np.random.default_rng([43, N, k, seed])
  return (rng.standard_normal((N, k)) * 3.0).astype(np.float32)


def doersch_ref(x, m, label, norm=None):
  """(loss, dlogits, mag, gmag) in float64 (doersch_utils.py:55-66): max-subtracted cross-entropy against the constant
  label, loss = sum m ce / norm, dlogits = (m / norm)(softmax - onehot).  norm: the defect 'norm = N instead of sum m'."""
  x = np.asarray(x, dtype=np.float64)
  N, k = x.shape
  norm = m.sum() if norm is None else norm
  mx = x.max(1, keepdims=True)
  e = np.exp(x - mx)
  s = e.sum(1, keepdims=True)
  ce = np.log(s[:, 0]) - (x[:, label] - mx[:, 0])
  onehot = np.zeros((N, k))
  onehot[:, label] = 1.0
  with np.errstate(divide="ignore", invalid="ignore"):
    loss = (m * ce).sum() / norm
    dl = (m / norm)[:, None] * (e / s - onehot)
    mag = (m * (np.abs(np.log(s[:, 0])) + np.abs(x[:, label] - mx[:, 0]) + 1.0)).sum() / norm
    gmag = (m / norm)[:, None] * (e / s + 1.0)
  return loss, dl, mag, gmag


def doersch_bounds(loss, dl, mag, gmag, N, k):
  """Loss: per row k exponentials (charged 2 each on the path of the sum: the relative error of s is an absolute error
  of log s, which `mag` charges as the + 1 per row), k - 1 additions, log (2), the subtraction, the product with m, N
  additions and the division: n = N + 3 k + 5, doubled.  dlogits: e / s carries (3 k + 2) roundings relative to e / s,
  the subtraction of the one-hot, the product with m / norm (2): n = 3 k + 6 relative to (m / norm)(e / s + 1), doubled."""
  n, g = 2.0 * (N + 3 * k + 5), 2.0 * (3 * k + 6)
  return U32 * abs(loss) + n * U64 / (1 - n * U64) * mag, U32 * np.abs(dl) + g * U64 * gmag
