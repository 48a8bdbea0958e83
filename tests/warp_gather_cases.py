"""Cases and the host emulation of the gather-form backward of the general affine warp (csrc/warp.hip,
iic_affine_warp_bwd_gather), shared by tests/test_warp_gather_cpu.py (which proves the scheme without a GPU) and
tests/test_gpu_warp_gather.py (which holds the kernel to the emulation bit for bit).

The emulation restates the kernel, not the mathematics: the search box from the inverse of the 2x2 part in float64, the
forward's own tap arithmetic at every position of the box (coordinates round(round(m0 qx + m1 qy) + m2) in float64, the
fractions rounded to float32, the four weights as float32 products), membership by offset equality, and the sum
acc = fl32(acc + fl32(w g)) over the contributors in ascending (oy, ox) from acc = +0.0f."""
import functools

import numpy as np
import torch

from tests import iid_stage_cases as sc

CAP = 8                     # IIC_WARP_GATHER_CAP (include/iic_hip.h)
SLACK = 1.0 / 64
F32, F64 = np.float32, np.float64

# (N, K, H, W): H != W in both senses (the aspect factors of the pixel matrix), a published k, the smallest tensor
SHAPES = [(3, 5, 13, 20), (2, 1, 20, 9), (2, 24, 16, 16), (1, 1, 1, 1)]


class Case:
  """name; M float32 [N][6]; the shift; `served` (the library must say so); `exact` (every weight a dyadic fraction, so
  lattice inputs sum exactly in any order); `ref_range` (a matrix the reference's random_affine can draw); theta / ac
  (the normalised matrix and the align_corners convention M came from, for F.grid_sample) where there is one."""

  def __init__(self, name, M, sx=0, sy=0, served=True, exact=False, ref_range=False, theta=None, ac=False):
    self.name, self.M, self.sx, self.sy = name, M.contiguous(), int(sx), int(sy)
    self.served, self.exact, self.ref_range, self.theta, self.ac = served, exact, ref_range, theta, ac

  def __repr__(self):
    return self.name


def _per_sample(m, N):
  """Sample n > 0 gets the matrix of sample 0 translated by a further (n, -n) pixels (as iid_stage_cases.warp_matrices)."""
  M = torch.tensor([m] * N, dtype=torch.float32)
  M[:, 2] += torch.arange(N)
  M[:, 5] -= torch.arange(N)
  return M


@functools.lru_cache(maxsize=None)
def cases(shape):
  from iic_amd import seg_losses
  from oracle.gen_golden_seg2 import random_affines
  N, K, H, W = shape
  out = []
  # the reference's range: rotation +-30 deg, shear +-10 deg, scale 0.8-1.2, another matrix per sample; both grid_sample
  # conventions; with and without the x-flip of the second view
  for seed in (3, 11):
    aff = torch.from_numpy(random_affines(N, seed))
    for flip in (False, True):
      th = aff.clone()
      if flip:
        th[:, :, 0] *= -1.0
      for ac in (False, True):
        seg_losses.ALIGN_CORNERS[0] = ac
        try:
          M = seg_losses._pixel_matrices(th, H, W)
        finally:
          seg_losses.ALIGN_CORNERS[0] = False
        out.append(Case("affine%d%s%s" % (seed, "_flip" if flip else "", "_ac" if ac else ""), M, ref_range=True,
                        theta=th, ac=ac))
  for name, M, sx, sy in sc.warp_matrices(shape):
    out.append(Case("stage_" + name, M, sx, sy, exact=True))
  out.append(Case("half_pixel", _per_sample((1, 0, 0.5, 0, 1, -0.5), N), exact=True))
  out.append(Case("half_pixel_shift", _per_sample((1, 0, 0.5, 0, 1, -0.5), N), 2, -1, exact=True))
  out.append(Case("rot90", _per_sample((0, -1, H - 1, 1, 0, 0), N), exact=True))
  out.append(Case("rot90_shift", _per_sample((0, -1, H - 1, 1, 0, 0), N), -1, 1, exact=True))
  # refused: the LAST sample shrinks to a tenth (a box of 21 positions) / is singular; the others are served
  M = _per_sample((1, 0, 0, 0, 1, 0), N)
  M[N - 1] = torch.tensor([0.1, 0, 0, 0, 0.1, 0])
  out.append(Case("refused_tenth", M, served=False))
  M = _per_sample((1, 0, 0, 0, 1, 0), N)
  M[N - 1] = torch.tensor([1, 2, 0.25, 2, 4, 0.5])
  out.append(Case("refused_singular", M, served=False))
  return out


def served_cases(shape):
  return [c for c in cases(shape) if c.served]


def refused_cases(shape):
  return [c for c in cases(shape) if not c.served]


@functools.lru_cache(maxsize=None)
def random_dout(shape, seed=0):
  """Full-mantissa values of both signs."""
  g = torch.Generator().manual_seed(100 + seed + sum(shape))
  return torch.randn(shape, generator=g, dtype=torch.float32)


# ---- the library's range, restated -----------------------------------------------------------------------------------------------
def extents(M):
  """float64 [N] half-extents (ex, ey) of the search box, slack included, and `served` [N] (bool)."""
  m = M.numpy().astype(F64)
  a, b, c, d = m[:, 0], m[:, 1], m[:, 3], m[:, 4]
  with np.errstate(all="ignore"):
    det = a * d - b * c
    ex = (np.abs(d) + np.abs(b)) / np.abs(det) + SLACK
    ey = (np.abs(c) + np.abs(a)) / np.abs(det) + SLACK
    ok = (det != 0.0) & (2.0 * ex + 1.0 < CAP) & (2.0 * ey + 1.0 < CAP) & (np.abs(m[:, 2]) <= 3.0e38) & \
         (np.abs(m[:, 5]) <= 3.0e38)
  return ex, ey, ok


def supported(M):
  return bool(extents(M)[2].all())


# ---- the forward's taps ------------------------------------------------------------------------------------------------------------
def taps(m, qx, qy, H, W):
  """csrc/warp.hip warp_taps_at: m float32 [..., 6] and integer qx, qy broadcast against each other ->
  [(offset int64, weight float32)] x 4, offset -1 = outside."""
  m = m.astype(F64)
  qxd, qyd = qx.astype(F64), qy.astype(F64)
  fx = (m[..., 0] * qxd + m[..., 1] * qyd) + m[..., 2]
  fy = (m[..., 3] * qxd + m[..., 4] * qyd) + m[..., 5]
  x0d, y0d = np.floor(fx), np.floor(fy)
  inside = (x0d >= -1.0) & (x0d < W) & (y0d >= -1.0) & (y0d < H)
  x0 = np.where(inside, x0d, -1.0).astype(np.int64)
  y0 = np.where(inside, y0d, -1.0).astype(np.int64)
  ax, ay = (fx - x0d).astype(F32), (fy - y0d).astype(F32)
  one = F32(1.0)
  vx0, vx1, vy0, vy1 = inside & (x0 >= 0), inside & (x0 + 1 < W), y0 >= 0, y0 + 1 < H
  zero = np.zeros_like(ax)
  return [(np.where(vx0 & vy0, y0 * W + x0, -1), np.where(inside, (one - ax) * (one - ay), zero)),
          (np.where(vx1 & vy0, y0 * W + x0 + 1, -1), np.where(inside, ax * (one - ay), zero)),
          (np.where(vx0 & vy1, (y0 + 1) * W + x0, -1), np.where(inside, (one - ax) * ay, zero)),
          (np.where(vx1 & vy1, (y0 + 1) * W + x0 + 1, -1), np.where(inside, ax * ay, zero))]


def scatter_members(M, H, W, sx, sy):
  """The full scatter: bool [N][source pixel][output pixel], True where one of the output pixel's four taps is the
  source pixel.  Independent of any search box."""
  N = M.shape[0]
  oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
  qx, qy = (ox + sx).reshape(1, -1), (oy + sy).reshape(1, -1)
  inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
  S = np.zeros((N, H * W, H * W), dtype=bool)
  nn, oo = np.meshgrid(np.arange(N), np.arange(H * W), indexing="ij")
  for off, _ in taps(M.numpy()[:, None, :], qx, qy, H, W):
    ok = inside & (off >= 0)
    S[nn[ok], off[ok], oo[ok]] = True
  return S


# ---- the kernel, restated ----------------------------------------------------------------------------------------------------------
def emulate(dout, M, sx, sy, slack=SLACK, clamp_cap=True):
  """dict(dx float32 [N][K][H][W], members bool [N][source pixel][output pixel], width / height: the largest box of any
  pixel before the cap cuts it, count: the most contributors of one pixel)."""
  N, K, H, W = dout.shape
  g = dout.numpy().reshape(N, K, H * W)
  m32 = M.numpy()
  m = m32.astype(F64)
  a, b, c, d = (m[:, i].reshape(N, 1, 1) for i in (0, 1, 3, 4))
  with np.errstate(all="ignore"):
    det = a * d - b * c
    ex = (np.abs(d) + np.abs(b)) / np.abs(det) + slack
    ey = (np.abs(c) + np.abs(a)) / np.abs(det) + slack
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    du, dv = u[None].astype(F64) - m[:, 2].reshape(N, 1, 1), v[None].astype(F64) - m[:, 5].reshape(N, 1, 1)
    cx, cy = (d * du - b * dv) / det, (a * dv - c * du) / det
    qx_min, qx_max = max(0, sx), min(W - 1, W - 1 + sx)
    qy_min, qy_max = max(0, sy), min(H - 1, H - 1 + sy)
    x_lo = np.minimum(np.maximum(np.ceil(cx - ex), qx_min), qx_max + 1.0).astype(np.int64)
    y_lo = np.minimum(np.maximum(np.ceil(cy - ey), qy_min), qy_max + 1.0).astype(np.int64)
    x_hi = np.maximum(np.minimum(np.floor(cx + ex), qx_max), x_lo - 1.0).astype(np.int64)
    y_hi = np.maximum(np.minimum(np.floor(cy + ey), qy_max), y_lo - 1.0).astype(np.int64)
  width, height = int((x_hi - x_lo + 1).max()), int((y_hi - y_lo + 1).max())
  span_x, span_y = max(width, 1), max(height, 1)
  if clamp_cap:
    x_hi, y_hi = np.minimum(x_hi, x_lo + CAP - 1), np.minimum(y_hi, y_lo + CAP - 1)
    span_x, span_y = min(span_x, CAP), min(span_y, CAP)
  r = (v * W + u)[None]
  acc = np.zeros((N, K, H * W), dtype=F32)
  members = np.zeros((N, H * W, H * W), dtype=bool)
  count = np.zeros((N, H, W), dtype=np.int64)
  nn = np.broadcast_to(np.arange(N).reshape(N, 1, 1), (N, H, W))
  rr = np.broadcast_to(r, (N, H, W))
  for j in range(span_y):                 # ascending (oy, ox): oy = qy - sy, ox = qx - sx
    for i in range(span_x):
      qx, qy = x_lo + i, y_lo + j
      inbox = (qx <= x_hi) & (qy <= y_hi)
      qxc, qyc = np.where(inbox, qx, qx_min if qx_min <= qx_max else 0), np.where(inbox, qy, qy_min if qy_min <= qy_max else 0)
      hit = np.zeros((N, H, W), dtype=bool)
      w = np.zeros((N, H, W), dtype=F32)
      for off, wt in taps(m32[:, None, None, :], qxc, qyc, H, W):
        first = inbox & (off == r) & ~hit
        w = np.where(first, wt, w)
        hit |= first
      o = np.where(hit, (qyc - sy) * W + (qxc - sx), 0)
      members[nn[hit], rr[hit], o[hit]] = True
      count += hit
      gq = np.take_along_axis(g, np.broadcast_to(o.reshape(N, 1, H * W), (N, K, H * W)), axis=2)
      with np.errstate(all="ignore"):
        step = (acc + (w.reshape(N, 1, H * W) * gq).astype(F32)).astype(F32)
      acc = np.where(hit.reshape(N, 1, H * W), step, acc)
  return dict(dx=torch.from_numpy(acc.reshape(N, K, H, W)), members=members, width=width, height=height,
              count=int(count.max()), counts=count)


def adjoint_f64(dout, M, sx, sy):
  """The float64 adjoint with the kernel's own float32 weights removed: iid_stage_cases.warp_bwd_ref."""
  return sc.warp_bwd_ref(dout, M, sx, sy)


def accumulation_bound(dout, M, sx, sy, counts):
  """Per element, how far the float32 fixed-order sum may lie from the float64 adjoint.  A weight is a product of two
  factors ax | 1 - ax, each off by at most 2^-25 (the fraction is rounded to float32, and so is 1 - ax), and is rounded
  once more: at most 2.5 x 2^-24 absolute.  A term fl32(w g) adds 2^-24 |w g|, and each of the c additions 2^-24 of a
  partial sum that is at most sum |w g|.  With |w| <= 1:  (4 + c) 2^-24 sum |g| over the pixel's contributors."""
  N, K, H, W = dout.shape
  # sum |g| over a pixel's contributors: the adjoint of |dout| with every weight replaced by 1
  S = scatter_members(M, H, W, sx, sy)
  gsum = np.einsum("nro,nko->nkr", S.astype(F64), dout.abs().double().numpy().reshape(N, K, H * W)).reshape(N, K, H, W)
  c = counts.reshape(N, 1, H, W).astype(F64)
  return torch.from_numpy((4.0 + c) * 2.0 ** -24 * gsum)
