"""Cases, generators, float64 references and preconditions for the stages of the two IID losses (csrc/iid_loss.hip,
csrc/seg_loss.hip, csrc/warp.hip), shared by tests/test_iid_stages_cpu.py (which proves them without a GPU) and
tests/test_gpu_iid_stages.py (which holds the kernels to them).  A helper module, not a test file.

Exact cases.  Maps take values in {0, 1/4, 1/2, 1}, masks in {0, 1/2, 1} (a binary mask has m^2 = m and hides a mask
applied twice or at the wrong pixel), the k x k gradient matrices in {-1, 0, +1} (not symmetric), the upstream gradients
in {1, -2, 1/2, 0}.  A masked map is a multiple of 1/8, a product of two of them a multiple of 2^-6; G = gl dR1 + gnl dR2
is a multiple of 1/2, G x (masked map) x mask a multiple of 2^-5.  With every sum of magnitudes below 2^24 of that unit
each product and each partial sum is exact in fp32 in any order and grouping -- and under the bf16 three-term split, whose
high term is the value itself (at most 3 significant bits).  The references assert those preconditions themselves.

References are written from the definitions of include/iic_hip.h in plain torch float64: explicit loops over the shifts,
one einsum per shift, nothing shared with the kernels or with iic_amd/."""
import functools
import sys

import numpy as np
import torch

from tests.lattice import F32_EXACT_BOUND

EPS = sys.float_info.epsilon
MAP_VALUES = (0.0, 0.25, 0.5, 1.0)
MASK_VALUES = (0.0, 0.5, 1.0)
DR_VALUES = (-1.0, 0.0, 1.0)
G_VALUES = (1.0, -2.0, 0.5, 0.0)
JOINT_DEN = 2 ** 6
GRAD_DEN = 2 ** 7

# (bn, k, h, w, T)
SEG_STREAM = [(4, 3, 5, 8, 1), (2, 16, 3, 132, 2), (4, 17, 3, 40, 2), (2, 24, 2, 200, 1), (2, 33, 3, 12, 1),
              (2, 48, 2, 136, 1)]      # TK = 1 / 2 / 3 at LW = 32 and 64
SEG_BF16 = [(4, 5, 7, 16, 5), (2, 16, 3, 200, 10), (1, 4, 2, 256, 10), (2, 2, 4, 8, 10)]      # default at k <= 16, T >= 5
SEG_GENERIC = [(4, 2, 9, 13, 0), (4, 15, 5, 13, 3), (2, 20, 3, 30, 1), (1, 33, 2, 202, 1), (2, 48, 3, 7, 2)]      # w % 4 != 0
# 64 < w <= 128: the gradient kernels' LW = 32 (one / two class tiles, and seg_grad_stream3_kernel)
SEG_GRAD_LW32 = [(2, 9, 2, 72, 2), (2, 20, 2, 96, 1), (1, 40, 2, 100, 1)]
SEG_CASES = SEG_STREAM + SEG_BF16 + SEG_GENERIC + SEG_GRAD_LW32
SEG_F64_CASES = SEG_STREAM + SEG_BF16 + SEG_GENERIC[1:4]
# (H, bn, k)
IID_CASES = [(1, 1, 2), (1, 3, 1), (2, 17, 31), (1, 64, 32), (3, 129, 33), (5, 255, 70), (1, 41, 97)]
IID_LAYOUTS = ("packed", "heads", "padded")
IID_F64_CASES = [(5, 255, 70), (1, 41, 97)]
# (H, k, nparts); 95 / 96: the two sides of IID_BIG_MIN_K
STAGE_CASES = [(1, 2, 1), (2, 3, 3), (9, 10, 2), (1, 48, 16), (5, 70, 4), (2, 95, 1), (2, 96, 1), (1, 97, 3), (1, 280, 2)]
STAGE_DRAWS = ("dense", "sparse", "dead")
STAGE_LAMBS = (1.0, 1.5)
# (N, K, H, W); the last: N H W = 1 326 = 5 blocks of 256 and 46 threads
WARP_SHAPES = [(3, 5, 17, 23), (1, 1, 1, 1), (2, 48, 5, 9), (2, 3, 17, 39)]


def draw(rng, values, shape):
  return torch.from_numpy(np.asarray(values, dtype=np.float32)[rng.integers(0, len(values), tuple(shape))])


def draw_dR(rng, H, k):
  """[H][k][k] from {-1, 0, +1}, never symmetric (k >= 2): entries (0, 1) and (1, 0) are +1 and -1."""
  t = draw(rng, DR_VALUES, (H, k, k))
  if k >= 2:
    t[:, 0, 1], t[:, 1, 0] = 1.0, -1.0
  return t


def assert_lattice(t, den, what):
  """Every value a multiple of 1 / den, every magnitude times den below 2^24.  Returns max |t|."""
  v = torch.as_tensor(t).double() * den
  assert torch.equal(v, v.round()), "%s: a value is no multiple of 1/%d" % (what, den)
  m = float(v.abs().max()) if v.numel() else 0.0
  assert m < F32_EXACT_BOUND, "%s: %g / %d reaches 2^24" % (what, m, den)
  return m / den


# ---- segmentation joint and gradients --------------------------------------------------------------------------------
def seg_flips(bn):
  """int32 [bn][2] (flip x, flip y): all four combinations from bn = 4 on, else starting at (1, 0)."""
  first = 0 if bn >= 4 else 1
  return torch.tensor([[i & 1, (i >> 1) & 1] for i in range(first, first + bn)], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def seg_inputs(case, seed=0):
  bn, k, h, w, T = case
  rng = np.random.default_rng(1000 * seed + 7 * k + w + T)
  nq = 2 * T + 1
  d = dict(case=case, x1=draw(rng, MAP_VALUES, (bn, k, h, w)), x2=draw(rng, MAP_VALUES, (bn, k, h, w)),
           mask=draw(rng, MASK_VALUES, (bn, h, w)), flips=seg_flips(bn))
  for name, H in (("c", 1), ("u", nq * nq)):      # collapsed: one matrix for every shift; uncollapsed: one per shift
    d["dR1" + name], d["dR2" + name] = draw_dR(rng, H, k), draw_dR(rng, H, k)
    d["gl" + name], d["gnl" + name] = draw(rng, G_VALUES, (H,)), draw(rng, G_VALUES, (H,))
  return d


@functools.lru_cache(maxsize=None)
def seg_f64_inputs(case, seed=0):
  """softmax(2 randn) maps floored at 2^-60 (full mantissas, no underflow in a product or in the split's low term) and a
  mask drawn from {0, 1/2, 1}."""
  bn, k, h, w, T = case
  g = torch.Generator().manual_seed(100 * seed + 3 * k + w + T)
  mk = lambda: torch.softmax(2 * torch.randn(bn, k, h, w, generator=g), 1).clamp_min(2.0 ** -60)
  mask = torch.randint(0, 3, (bn, h, w), generator=g).float() / 2
  return dict(case=case, x1=mk(), x2=mk(), mask=mask, flips=seg_flips(bn))


def shifted(a, ty, tx):
  """b(..., y, x) = a(..., y + ty, x + tx), zero where that leaves the image."""
  h, w = a.shape[-2:]
  out = torch.zeros_like(a)
  ys, ye, xs, xe = max(0, -ty), min(h, h - ty), max(0, -tx), min(w, w - tx)
  if ys < ye and xs < xe:
    out[..., ys:ye, xs:xe] = a[..., ys + ty:ye + ty, xs + tx:xe + tx]
  return out


def flip_samples(x, flips):
  """x2 -> x2_inv: per sample, the x / y mirror that `flips` asks for (its own inverse)."""
  out = x.clone()
  for n in range(x.shape[0]):
    dims = [d for d, f in ((2, int(flips[n, 0])), (1, int(flips[n, 1]))) if f]
    if dims:
      out[n] = torch.flip(x[n], dims)
  return out


def seg_maps(x1, x2, mask, flips):
  """x1m = x1 mask and x2m = flip(x2) mask, float64."""
  m = mask.double()[:, None]
  return x1.double() * m, flip_samples(x2.double(), flips) * m


def seg_joint_ref(x1m, x2m, T):
  """R[p][q][i][j] = sum_{n, y, x} x1m_i(y + p - T, x + q - T) x2m_j(y, x), float64 [2T+1][2T+1][k][k]."""
  nq, k = 2 * T + 1, x1m.shape[1]
  R = torch.zeros((nq, nq, k, k), dtype=torch.float64)
  for p in range(nq):
    for q in range(nq):
      R[p, q] = torch.einsum("nihw,njhw->ij", shifted(x1m, p - T, q - T), x2m)
  return R


def seg_terms(case):
  """[2T+1][2T+1]: pixel products of an entry of the joint at each shift (pairs of pixels both inside the image)."""
  bn, k, h, w, T = case
  t = torch.arange(-T, T + 1).abs()
  return (bn * (h - t).clamp_min(0)[:, None] * (w - t).clamp_min(0)[None, :]).double()


def seg_G(dR1, dR2, gl, gnl, T, k):
  """G[p][q] = gl dR1 + gnl dR2 per shift, [2T+1][2T+1][k][k] float64; H = 1 (collapsed): the same matrix at every shift."""
  nq = 2 * T + 1
  G = gl.double()[:, None, None] * dR1.double() + gnl.double()[:, None, None] * dR2.double()
  return G.expand(nq * nq, k, k).reshape(nq, nq, k, k)


def seg_grad_ref(x1m, x2m, mask, flips, G, T, which):
  """The closed forms of csrc/seg_loss.hip:19-21, float64.
  which = 0: dx1_i(v) = mask(v) sum_{p,q,j} G[p][q][i][j] x2m_j(v - t),      t = (p - T, q - T);
  which = 1: dx2m_j(u) =        sum_{p,q,i} G[p][q][i][j] x1m_i(u + t), then dx2(flip(u)) = mask(u) dx2m_j(u): x2m is
  flip(x2) mask, so the gradient lands at the flipped pixel."""
  nq = 2 * T + 1
  out = torch.zeros_like(x1m)
  for p in range(nq):
    for q in range(nq):
      if which == 0:
        out += torch.einsum("ij,njhw->nihw", G[p, q], shifted(x2m, -(p - T), -(q - T)))
      else:
        out += torch.einsum("ij,nihw->njhw", G[p, q], shifted(x1m, p - T, q - T))
  out = out * mask.double()[:, None]
  return out if which == 0 else flip_samples(out, flips)


@functools.lru_cache(maxsize=None)
def seg_exact_reference(case, seed=0):
  """R and the four gradients (collapsed / uncollapsed x which) of an exact case, the preconditions asserted."""
  bn, k, h, w, T = case
  inp = seg_inputs(case, seed)
  x1m, x2m = seg_maps(inp["x1"], inp["x2"], inp["mask"], inp["flips"])
  ref = dict(R=seg_joint_ref(x1m, x2m, T))
  fig = dict(case=list(case), max_R=assert_lattice(ref["R"], JOINT_DEN, "joint"))      # terms >= 0: R is its own magnitude sum
  for name in ("c", "u"):
    G = seg_G(inp["dR1" + name], inp["dR2" + name], inp["gl" + name], inp["gnl" + name], T, k)
    for which in (0, 1):
      ref["d%s%d" % (name, which)] = seg_grad_ref(x1m, x2m, inp["mask"], inp["flips"], G, T, which)
      mag = seg_grad_ref(x1m, x2m, inp["mask"], inp["flips"], G.abs(), T, which)
      fig["sum_abs_d%s%d" % (name, which)] = assert_lattice(mag, GRAD_DEN, "gradient magnitudes")
      assert_lattice(ref["d%s%d" % (name, which)], GRAD_DEN, "gradient")
  ref["figures"] = fig
  return ref


# ---- clustering joint and gradients ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def iid_inputs(case, seed=0):
  H, bn, k = case
  rng = np.random.default_rng(1000 * seed + 31 * H + bn + k)
  return dict(case=case, z=draw(rng, MAP_VALUES, (H, bn, k)), zt=draw(rng, MAP_VALUES, (H, bn, k)),
              dR1=draw_dR(rng, H, k), dR2=draw_dR(rng, H, k),
              gl=draw(rng, G_VALUES, (H,)), gnl=draw(rng, G_VALUES, (H,)))


def iid_joint_ref(z, zt):
  """R[h] = z_h^T z'_h, float64 [H][k][k]."""
  return torch.einsum("hni,hnj->hij", z.double(), zt.double())


def iid_grad_ref(z, zt, G):
  """dz[n][a] = sum_b G[a][b] z'[n][b];  dz'[n][a] = sum_b G[b][a] z[n][b]  (per head), float64."""
  return torch.einsum("hab,hnb->hna", G, zt.double()), torch.einsum("hba,hnb->hna", G, z.double())


def iid_G(inp, upstream):
  gl = inp["gl"].double() if upstream else torch.ones(inp["case"][0], dtype=torch.float64)
  gnl = inp["gnl"].double() if upstream else torch.zeros(inp["case"][0], dtype=torch.float64)
  return gl[:, None, None] * inp["dR1"].double() + gnl[:, None, None] * inp["dR2"].double()


@functools.lru_cache(maxsize=None)
def iid_exact_reference(case, seed=0):
  inp = iid_inputs(case, seed)
  ref = dict(R=iid_joint_ref(inp["z"], inp["zt"]))
  fig = dict(case=list(case), max_R=assert_lattice(ref["R"], JOINT_DEN, "joint"))
  for upstream in (True, False):
    G = iid_G(inp, upstream)
    ref["dz", upstream], ref["dzt", upstream] = iid_grad_ref(inp["z"], inp["zt"], G)
    for t in iid_grad_ref(inp["z"], inp["zt"], G.abs()):
      fig["sum_abs_grad"] = max(fig.get("sum_abs_grad", 0.0), assert_lattice(t, GRAD_DEN, "gradient magnitudes"))
  ref["figures"] = fig
  return ref


def iid_layout(case, layout):
  """(head_stride, ld, size, idx): element (h, n, i) of a [H][bn][k] tensor lives at idx[h][n][i] = h head_stride + n ld + i
  of a flat buffer of `size` floats.  packed: [bn][H][k] as the network's heads emit it; heads: [H][bn][k]; padded:
  [H][bn][k + 3], three pad floats per row that no kernel may touch."""
  H, bn, k = case
  hs, ld = {"packed": (k, H * k), "heads": (bn * k, k), "padded": (bn * (k + 3), k + 3)}[layout]
  idx = (torch.arange(H)[:, None, None] * hs + torch.arange(bn)[None, :, None] * ld + torch.arange(k)[None, None, :])
  size = H * bn * (k + 3) if layout == "padded" else H * bn * k
  assert int(idx.max()) < size and idx.unique().numel() == idx.numel()
  return hs, ld, size, idx


def iid_place(t, case, layout, fill):
  hs, ld, size, idx = iid_layout(case, layout)
  flat = torch.full((size,), fill, dtype=torch.float32)
  flat[idx.reshape(-1)] = t.reshape(-1).float()
  return flat


def iid_f64_inputs(case, seed=0):
  H, bn, k = case
  g = torch.Generator().manual_seed(seed + bn + k)
  mk = lambda: torch.softmax(2 * torch.randn(H, bn, k, generator=g), 2).clamp_min(2.0 ** -60)
  return dict(case=case, z=mk(), zt=mk())


# ---- the k x k stage -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_partials(case, kind, seed=0):
  """fp32 [nparts][H][k][k] raw-joint partials, every head its own draw.  dense: gamma(2) positives, full mantissas.
  sparse: a symmetric pattern of about half the off-diagonal entries is exactly 0 in every partial, so that P is 0 there
  and clamped (the diagonal stays: no empty joint).  dead: sparse, and the last class's row and column are 0 -- its
  marginal is 0 and clamped (at k = 2 one class remains)."""
  H, k, nparts = case
  rng = np.random.default_rng(1000 * seed + 97 * H + k + nparts + len(kind))
  part = rng.gamma(2.0, 1.0, (nparts, H, k, k))
  if kind in ("sparse", "dead"):
    keep = rng.random((H, k, k)) < 0.5
    keep = np.triu(keep, 1)
    keep = keep | keep.transpose(0, 2, 1) | np.eye(k, dtype=bool)[None]
    if kind == "dead":
      keep[:, k - 1, :] = False
      keep[:, :, k - 1] = False
    part = part * keep[None]
  return torch.from_numpy(part.astype(np.float32))


def stage_ref(partials, lamb, detach_norm, eps=EPS, log=torch.log, sum32=False):
  """The reference's formula (code/utils/cluster/IID_losses.py:6-33 as oracle/iid_oracle.py:42-62 restates it; the
  segmentation losses' k x k part is the same, with the normaliser detached for the collapsed one) from the raw joint, in
  torch float64 autograd: sum the partials in float64, symmetrise, normalise, marginals BEFORE the clamp, clamp (no
  gradient through a clamped value).  detach_norm: the normaliser is float(sum), a constant.
  Returns loss, loss_nl [H]; dR1, dR2 [H][k][k]; M1, M2 [H] and mag1, mag2 [H][k][k], the magnitudes of
  parity.stage_bound: M = sum Pc (|log Pc| + l |log p_i| + l |log p_j|) and, per entry of dR, the magnitudes of d's terms
  plus sum(those P), over S; P, pi, pj, S for the clamp-gap check.  `log` / `sum32` seed an fp32 intermediate."""
  def tot(t):      # the k k-term sums of the kernel (S, the two losses, g)
    return t.float().sum((1, 2), keepdim=True).double() if sum32 else t.sum((1, 2), keepdim=True)
  R = partials.double().sum(0).requires_grad_(True)
  Ps = 0.5 * (R + R.transpose(1, 2))
  S = tot(Ps)
  P = Ps / (S.detach() if detach_norm else S)
  pi, pj = P.sum(2, keepdim=True), P.sum(1, keepdim=True)
  e = torch.tensor(eps, dtype=torch.float64)
  mP, mi, mj = ~(P < eps), ~(pi < eps), ~(pj < eps)
  Pc, pic, pjc = torch.where(mP, P, e), torch.where(mi, pi, e), torch.where(mj, pj, e)
  lP, li, lj = log(Pc), log(pic), log(pjc)
  out = dict(P=P.detach(), pi=pi.detach()[:, :, 0], pj=pj.detach()[:, 0, :], S=S.detach()[:, 0, 0])
  for name, l in (("1", lamb), ("2", 1.0)):
    loss = -tot(Pc * (lP - l * lj - l * li))[:, 0, 0]
    out["loss" + name] = loss.detach()
    out["dR" + name] = torch.autograd.grad(loss.sum(), R, retain_graph=True)[0]
    with torch.no_grad():
      out["M" + name] = (Pc * (lP.abs() + l * li.abs() + l * lj.abs())).sum((1, 2))
      rc_i, rc_j = Pc.sum(2, keepdim=True), Pc.sum(1, keepdim=True)
      row = torch.where(mi, rc_i / pi, torch.zeros_like(pi))
      col = torch.where(mj, rc_j / pj, torch.zeros_like(pj))
      md = torch.where(mP, lP.abs() + l * lj.abs() + l * li.abs() + 1.0, torch.zeros_like(P)) + l * (row + col)
      mg = torch.zeros_like(S) if detach_norm else (md * P).sum((1, 2), keepdim=True)
      out["mag" + name] = (md + mg) / S.abs()
  return out


def clamp_gap(P, eps=EPS, rel=1e-6):
  """Smallest |v / eps - 1| over the entries of P: the clamp's branch must not hang on the last bit."""
  return float((P / eps - 1.0).abs().min())


# ---- bf16 three-term split (seg_split8 / seg_mfma6 of csrc/seg_loss.hip), emulated -----------------------------------------
def split3(x):
  """fp32 x -> (h, m, l) fp32 tensors holding bf16 values: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to
  nearest even (torch's float32 -> bfloat16), the subtractions in fp32."""
  x = x.float()
  h = x.to(torch.bfloat16).float()
  r = x - h
  m = r.to(torch.bfloat16).float()
  r = r - m
  return h, m, r.to(torch.bfloat16).float()


SIX = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))      # seg_mfma6's order: m m', l h', h l', m h', h m', h h'


def split_joint_emulated(x1m32, x2m32, T, products=SIX):
  """The joint from the kept products of the split operands, every product exact in fp32, accumulated in fp32."""
  a, b = split3(x1m32), split3(x2m32)
  nq, k = 2 * T + 1, x1m32.shape[1]
  R = torch.zeros((nq, nq, k, k), dtype=torch.float32)
  for p in range(nq):
    for q in range(nq):
      for ia, ib in products:
        R[p, q] += torch.einsum("nihw,njhw->ij", shifted(a[ia], p - T, q - T), b[ib])
  return R


# ---- affine warp ---------------------------------------------------------------------------------------------------------
def _warp_taps(M, N, H, W, sx, sy):
  """csrc/warp.hip:8-11 restated: per (n, output pixel) the four (source offset, weight, valid) of the bilinear sample at
  M_n (ox + sx, oy + sy, 1), all invalid where (ox + sx, oy + sy) leaves the image.  float64."""
  M = M.double()
  oy, ox = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
  qx, qy = (ox + sx).reshape(1, -1).double(), (oy + sy).reshape(1, -1).double()
  inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
  fx = M[:, 0:1] * qx + M[:, 1:2] * qy + M[:, 2:3]
  fy = M[:, 3:4] * qx + M[:, 4:5] * qy + M[:, 5:6]
  x0, y0 = torch.floor(fx), torch.floor(fy)
  ax, ay = fx - x0, fy - y0
  taps = []
  for dy in (0, 1):
    for dx in (0, 1):
      xi, yi = x0 + dx, y0 + dy
      valid = inside & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
      wgt = (ax if dx else 1 - ax) * (ay if dy else 1 - ay)
      idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
      taps.append((idx, torch.where(valid, wgt, torch.zeros_like(wgt))))
  return taps


def warp_fwd_ref(x, M, sx, sy):
  N, K, H, W = x.shape
  xf = x.double().reshape(N, K, H * W)
  out = torch.zeros_like(xf)
  for idx, wgt in _warp_taps(M, N, H, W, sx, sy):
    out += wgt[:, None] * torch.gather(xf, 2, idx[:, None].expand(N, K, H * W))
  return out.reshape(N, K, H, W)


def warp_bwd_ref(dout, M, sx, sy):
  """The adjoint of warp_fwd_ref: dx[s] = sum over the output pixels that sample s of weight x dout."""
  N, K, H, W = dout.shape
  g = dout.double().reshape(N, K, H * W)
  dx = torch.zeros_like(g)
  for idx, wgt in _warp_taps(M, N, H, W, sx, sy):
    dx.scatter_add_(2, idx[:, None].expand(N, K, H * W), wgt[:, None] * g)
  return dx.reshape(N, K, H, W)


def warp_matrices(shape):
  """[(name, M float32 [N][6], shift_x, shift_y)].  Sample n > 0 gets the matrix of sample 0 translated by a further
  (n, -n) pixels, so that a kernel reading another sample's matrix shows."""
  N, K, H, W = shape
  base = [("identity", (1, 0, 0, 0, 1, 0)), ("translate+", (1, 0, 2, 0, 1, 1)), ("translate-", (1, 0, -3, 0, 1, -2)),
          ("flip_x", (-1, 0, W - 1, 0, 1, 0)), ("flip_y", (1, 0, 0, 0, -1, H - 1)), ("flip_xy", (-1, 0, W - 1, 0, -1, H - 1)),
          ("transpose", (0, 1, 0, 1, 0, 0)), ("half_x", (1, 0, 0.5, 0, 1, 0)), ("half_xy", (1, 0, 0.5, 0, 1, 0.5)),
          ("half_neg", (1, 0, -0.5, 0, 1, -0.5)), ("scale2", (2, 0, 0, 0, 2, 0)), ("scale_half", (0.5, 0, 0, 0, 0.5, 0)),
          ("outside", (1, 0, 1000, 0, 1, 1000))]
  out = []
  for name, m in base:
    M = torch.tensor([m] * N, dtype=torch.float32)
    M[:, 2] += torch.arange(N)
    M[:, 5] -= torch.arange(N)
    shifts = [(0, 0), (3, -2), (-W, 0), (0, H)] if name.startswith("translate") else [(0, 0)]
    out += [("%s_s%d_%d" % (name, sx, sy), M, sx, sy) for sx, sy in shifts]
  return out


@functools.lru_cache(maxsize=None)
def warp_inputs(shape, seed=0):
  rng = np.random.default_rng(seed + sum(shape))
  return dict(x=draw(rng, MAP_VALUES, shape), dout=draw(rng, DR_VALUES, shape))


def pixel_to_theta(M, H, W):
  """The normalised-coordinate matrix [N][2][3] of F.affine_grid(align_corners=False) whose sampling positions are the
  pixel-space M's: ix = ((xs + 1) W - 1) / 2 with xs = t00 xn + t01 yn + t02, xn = (2 ox + 1) / W - 1."""
  M = M.double()
  t = torch.zeros((M.shape[0], 2, 3), dtype=torch.float64)
  t[:, 0, 0], t[:, 0, 1] = M[:, 0], M[:, 1] * H / W
  t[:, 1, 0], t[:, 1, 1] = M[:, 3] * W / H, M[:, 4]
  t[:, 0, 2] = (M[:, 2] + 0.5) * 2 / W - 1 - t[:, 0, 0] / W + t[:, 0, 0] - t[:, 0, 1] / H + t[:, 0, 1]
  t[:, 1, 2] = (M[:, 5] + 0.5) * 2 / H - 1 - t[:, 1, 0] / W + t[:, 1, 0] - t[:, 1, 1] / H + t[:, 1, 1]
  return t
