"""Cases, float64 restatements, the fp32 emulation and the derived bounds shared by tests/test_seg_kmeans_cpu.py and
tests/test_gpu_seg_kmeans.py (a helper module, not a test file).

The label bracket.  The device takes fp32 dot products d_j = x.c_j at the trunk's resolution, up-samples them with
bilinear_fwd_kernel's operations and takes the arg-min of  cnorm_j - 2 up_j.  The reference interpolates the C-channel
features and then takes the distance to every centre; the two are the same function in exact arithmetic (both linear in
x).  With u = 2^-24,
  A  = max over low-resolution pixels and centres of sum_t |x_t c_jt|        (>= D = max |x.c_j|)
  Cn = max_j ||c_j||^2,  Lmax = max(Hl, Wl)
the fp32 score differs from the float64 one by at most
  e = u [ (C + 2) (2 A + Cn)            C products and additions per dot product and per ||c||^2, two spare; the dot's
                                        error is doubled by the score
        + (16 + 24 Lmax) D              the blend: at most 8 roundings of magnitudes <= D (1 - lx, 1 - ly, four
                                        products, two sums), doubled; the fp32 source coordinate fma(d + .5, scale, -.5)
                                        with scale = fp32(Hl / S) is within 3 u Lmax of the exact one, which moves the
                                        value by at most 2 D per unit per axis (continuous across a change of the
                                        neighbour pair): 2 axes x 2 D x 3 u Lmax, doubled
        + Cn + 2 D ]                    the one rounding of the subtraction
A pixel is UNDER THE GAP when the float64 difference between its best and second-best score is <= 2 e: fp32 may then
pick either.  Everywhere else the label must be the float64 arg-min.  On the integer lattice with S = 2 Hl every weight
is 0, 1/4, 3/4 or 1 and every number an exact fp32: no pixel is left out there.
"""
import numpy as np

U = 2.0 ** -24
GAP_CAP = 0.02       # at most this share of pixels may fall under the gap: a condition on the inputs, float64 alone

# fused kernel against iic_bilinear_fwd + argmin + iic_seg_contingency_acc: (Hl, Wl, S, k, N).  The first four are the
# issue's; (10, 10, 28, 255, 1) halves its tile until the staged rows fit the LDS budget.  The kernel has one variant
# switch, LDS-staged sources against global reads when not even one quad's sources (2 rows x 25 columns x k here) fit
# the 40 KB budget: (30, 30, 4, 204, 1) is the last k that stages (10200 floats), (30, 30, 4, 205, 1) the first that does
# not.  test_gpu_seg_kmeans.py asserts which side each case is on with iic_seg_kmeans_label_lds_floats.
FUSED_CASES = [(8, 8, 24, 3, 2), (8, 8, 16, 6, 2), (7, 9, 18, 27, 1), (10, 10, 28, 255, 1), (30, 30, 4, 204, 1),
               (30, 30, 4, 205, 1)]
GLOBAL_FORM = {(30, 30, 4, 205, 1)}
SAMPLE_M = [0, 1, 257]
# bracket test against the reference's order in float64: clustered features, real geometry Hl = S / 2 - 4 and an odd one
BRACKET_CASES = [dict(N=2, Hl=8, Wl=8, S=24, C=512, k=3, seed=31), dict(N=1, Hl=7, Wl=9, S=18, C=64, k=27, seed=32)]
LATTICE_CASE = dict(N=2, Hl=8, Wl=8, S=16, C=512, k=6, seed=33)


# ---- bilinear, align_corners=False: float64 and the kernel's fp32 operation order ----------------------------------------------
def src64(S, L, align_corners=False):
  d = np.arange(S, dtype=np.float64)
  s = d * ((L - 1) / max(S - 1, 1)) if align_corners else np.maximum((d + 0.5) * (float(L) / S) - 0.5, 0.0)
  i0 = np.minimum(np.floor(s).astype(np.int64), L - 1)
  i1 = i0 + (i0 < L - 1)
  return i0, i1, s - i0


def _fma32(a, b, c):
  return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def src32(S, L):
  """sk_src: s = fma(d + .5, scale, -.5) with scale = fp32(L) / fp32(S), clamped at 0; lam = s - i0."""
  scale = np.float32(L) / np.float32(S)
  d = np.arange(S, dtype=np.float32) + np.float32(0.5)
  s = np.maximum(_fma32(d, np.full_like(d, scale), np.full_like(d, -0.5)), np.float32(0))
  i0 = np.minimum(s.astype(np.int64), L - 1)
  i1 = i0 + (i0 < L - 1)
  return i0, i1, (s - i0.astype(np.float32)).astype(np.float32)


def up64(v, S, align_corners=False):
  """v [N, Hl, Wl, K] -> float64 [N, S, S, K]."""
  v = np.asarray(v, dtype=np.float64)
  y0, y1, ly = src64(S, v.shape[1], align_corners)
  x0, x1, lx = src64(S, v.shape[2], align_corners)
  ly, lx = ly[None, :, None, None], lx[None, None, :, None]
  top = v[:, y0][:, :, x0] * (1 - lx) + v[:, y0][:, :, x1] * lx
  bot = v[:, y1][:, :, x0] * (1 - lx) + v[:, y1][:, :, x1] * lx
  return top * (1 - ly) + bot * ly


def up32(v, S, defect=None):
  """The kernel's operation order in numpy fp32: top = fma(v01, lx, v00 (1 - lx)), bot = fma(v10, 1 - lx, v11 lx),
  out = (1 - ly) top + ly bot.  defect "neighbour": the right neighbour is taken one column too far."""
  v = np.asarray(v, dtype=np.float32)
  y0, y1, ly = src32(S, v.shape[1])
  x0, x1, lx = src32(S, v.shape[2])
  if defect == "neighbour":
    x1 = np.minimum(x1 + 1, v.shape[2] - 1)
  ly, lx = ly[None, :, None, None], lx[None, None, :, None]
  one = np.float32(1)
  v00, v01, v10, v11 = v[:, y0][:, :, x0], v[:, y0][:, :, x1], v[:, y1][:, :, x0], v[:, y1][:, :, x1]
  top = _fma32(v01, np.broadcast_to(lx, v01.shape), v00 * (one - lx))
  bot = _fma32(v10, np.broadcast_to(one - lx, v10.shape), v11 * lx)
  return ((one - ly) * top + ly * bot).astype(np.float32)


def labels32(X, C, S, defect=None):
  """numpy fp32 emulation of the device path on features X [N, Hl, Wl, C] and centres [k, C]: uint8-range labels."""
  X32, C32 = np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32)
  dots = (X32.reshape(-1, X32.shape[3]) @ C32.T).reshape(X32.shape[:3] + (C32.shape[0],))
  cn = (C32 * C32).sum(1, dtype=np.float32)
  if defect == "align_corners":
    up = up64(dots, S, align_corners=True).astype(np.float32)
  else:
    up = up32(dots, S, defect)
  if defect == "cnorm":
    cn = np.zeros_like(cn)
  score = cn[None, None, None] - np.float32(2) * up
  return rule_argmin(score)


def rule_argmin(score):
  """arg-min over the last axis with the kernel's rule: a NaN never beats a number, lowest index on a tie, all NaN: 0."""
  return np.argmin(np.where(np.isnan(score), np.inf, score), axis=-1)


def scores64(X, C, S):
  """The reference's order in float64: interpolate the features, then the squared distance to every centre, less the
  pixel's own ||x||^2 (common to all centres): [N, S, S, k]."""
  xu = up64(X, S)
  C64 = np.asarray(C, dtype=np.float64)
  return (C64 * C64).sum(1)[None, None, None] - 2.0 * (xu @ C64.T)


def score_error(X, C):
  """e of the module docstring."""
  X64, C64 = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
  Cc = X64.shape[3]
  flat = X64.reshape(-1, Cc)
  A = (np.abs(flat) @ np.abs(C64).T).max()
  D = np.abs(flat @ C64.T).max()
  Cn = (C64 * C64).sum(1).max()
  Lmax = max(X64.shape[1], X64.shape[2])
  return U * ((Cc + 2) * (2 * A + Cn) + (16 + 24 * Lmax) * D + Cn + 2 * D)


def under_gap(S64, e):
  """bool [N, S, S]: the float64 gap between the best and the second-best score is <= 2 e."""
  if S64.shape[-1] == 1:
    return np.zeros(S64.shape[:-1], dtype=bool)
  part = np.partition(S64, 1, axis=-1)
  return (part[..., 1] - part[..., 0]) <= 2 * e


def clustered_features(N, Hl, Wl, C, k, seed, sep=3.0, noise=0.05, bf16=False):
  """Features around k well-separated centres of different norms (centre j is scaled by 1 + j / k), constant over
  blocks of the low-resolution map: X fp32 [N, Hl, Wl, C] (bf16-representable on request), centres fp32 [k, C]."""
  rng = np.random.RandomState(seed)
  cen = rng.standard_normal((k, C)) * sep / np.sqrt(C) * (1.0 + np.arange(k) / float(k))[:, None]
  cen = cen.astype(np.float32)
  which = rng.randint(0, k, (N, (Hl + 2) // 3, (Wl + 2) // 3))
  which = np.repeat(np.repeat(which, 3, axis=1), 3, axis=2)[:, :Hl, :Wl]
  X = cen[which] + (noise / np.sqrt(C)) * rng.standard_normal((N, Hl, Wl, C))
  X = X.astype(np.float32)
  if bf16:
    X = to_bf16(X)
  return X, cen


def to_bf16(a):
  """fp32 values rounded to bf16 (round to nearest even), still as fp32."""
  b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
  b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
  return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def lattice_features(N, Hl, Wl, C, k, seed):
  """Integers in {-2 .. 2} (X) and {-1, 0, 1} (centres), sparse: with S = 2 Hl every interpolated dot product is a
  multiple of 1/16 below 2^12, exact in fp32 in any order."""
  rng = np.random.RandomState(seed)
  X = rng.randint(-2, 3, (N, Hl, Wl, C)) * (rng.random_sample((N, Hl, Wl, C)) < 0.1)
  Cn = rng.randint(-1, 2, (k, C)) * (rng.random_sample((k, C)) < 0.2)
  return X.astype(np.float32), Cn.astype(np.float32)


def counts64(labels, targets, mask, k, k_gt):
  """iic_seg_contingency_acc's layout: [k k_gt + 1], the selected pixels in the last cell."""
  sel = np.ones(labels.shape, dtype=bool) if mask is None else (mask != 0)
  out = np.zeros(k * k_gt + 1, dtype=np.int64)
  ok = sel & (targets < k_gt)
  np.add.at(out, labels[ok].astype(np.int64) * k_gt + targets[ok], 1)
  out[-1] = sel.sum()
  return out


# ---- mini-batch k-means in float64 ---------------------------------------------------------------------------------------
def assign64(X, C):
  X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
  S = (C * C).sum(1)[None] - 2.0 * (X @ C.T)
  labels = np.argmin(S, axis=1)
  return labels, np.maximum(0.0, (X * X).sum(1) + S[np.arange(X.shape[0]), labels])


def mini_batch_step64(Xb, C, w, random_reassign=False, reassignment_ratio=0.01, choice=None):
  """One dense mini-batch step (sklearn _mini_batch_step) in float64: (new centres, new weight sums, batch inertia,
  reassigned mask).  The inertia is that of the assignment, which uses the old centres.  ``choice(n_rows, size)``
  supplies the reassignment picks."""
  Xb, C, w = np.asarray(Xb, dtype=np.float64), np.array(C, dtype=np.float64), np.array(w, dtype=np.float64)
  labels, mind = assign64(Xb, C)
  k = C.shape[0]
  cnt = np.bincount(labels, minlength=k).astype(np.float64)
  sums = np.zeros_like(C)
  np.add.at(sums, labels, Xb)
  upd = cnt > 0
  C[upd] = (C[upd] * w[upd, None] + sums[upd]) / (w[upd] + cnt[upd])[:, None]
  w = w + cnt
  to = np.zeros(k, dtype=bool)
  if random_reassign and reassignment_ratio > 0:
    to = w < reassignment_ratio * w.max()
    if to.sum() > 0.5 * Xb.shape[0]:
      to[np.argsort(w)[int(0.5 * Xb.shape[0]):]] = False
    if to.sum():
      C[to] = Xb[np.asarray(choice(Xb.shape[0], int(to.sum())))]
    w[to] = np.min(w[~to])
  return C, w, float(mind.sum()), to


class Schedule64(object):
  """MiniBatchKMeans._random_reassign and _mini_batch_convergence as plain float64 bookkeeping."""

  def __init__(self, n_clusters, batch_size, n_samples, max_no_improvement=10, tol=0.0):
    self.k, self.batch, self.n, self.max_no_improvement, self.tol = n_clusters, batch_size, n_samples, max_no_improvement, tol
    self.ewa = self.ewa_min = None
    self.no_improvement = 0
    self.n_since = 0
    self.min_margin = np.inf      # smallest relative distance of a smoothed inertia from the minimum it was compared with

  def random_reassign(self, w):
    self.n_since += self.batch
    if (np.asarray(w) == 0).any() or self.n_since >= 10 * self.k:
      self.n_since = 0
      return True
    return False

  def converged(self, step, shift, batch_inertia):
    bi = batch_inertia / self.batch
    if step + 1 == 1:
      return False
    if self.ewa is None:
      self.ewa = bi
    else:
      alpha = min(self.batch * 2.0 / (self.n + 1), 1)
      self.ewa = self.ewa * (1 - alpha) + bi * alpha
    if self.tol > 0.0 and shift <= self.tol:
      return True
    if self.ewa_min is not None:
      self.min_margin = min(self.min_margin, abs(self.ewa - self.ewa_min) / max(abs(self.ewa), 1e-300))
    if self.ewa_min is None or self.ewa < self.ewa_min:
      self.no_improvement = 0
      self.ewa_min = self.ewa
    else:
      self.no_improvement += 1
    return self.max_no_improvement is not None and self.no_improvement >= self.max_no_improvement


def fit64(X, C0, batches, max_no_improvement=10, reassignment_ratio=0.01, choice=None):
  """The step loop of MiniBatchKMeans.fit on forced batches: per-step centres, weights, and the step it stopped at."""
  X = np.asarray(X, dtype=np.float64)
  C, w = np.array(C0, dtype=np.float64), np.zeros(len(C0))
  sch = Schedule64(len(C0), len(batches[0]), X.shape[0], max_no_improvement)
  hist, reassigned = [], []
  for i, idx in enumerate(batches):
    rr = sch.random_reassign(w)
    C, w, inertia, to = mini_batch_step64(X[idx], C, w, rr, reassignment_ratio, choice)
    hist.append((C.copy(), w.copy(), inertia))
    reassigned.append(to)
    if sch.converged(i, 0.0, inertia):
      break
  return dict(hist=hist, n_steps=i + 1, reassigned=reassigned, centres=C, w=w, schedule=sch)


def centre_bound_step(err_prev, w_prev, Xb, labels, C_new):
  """[k, d]: how far the device's fp32 centres may be from the float64 restatement's after a step on which the labels
  agree, given the bound before it.  The new centre is (c w + s) / (w + m): the incoming error shrinks by
  w / (w + m) <= 1; the fp32 sum s of the m batch rows is within (m + 2) u sum |x| (tests/kmeans_cases.sum_bound); the
  float64 quotient is rounded to fp32 once (u |c|).  A centre without rows keeps its value and its bound."""
  Xb = np.asarray(Xb, dtype=np.float64)
  k = C_new.shape[0]
  m = np.bincount(labels, minlength=k).astype(np.float64)
  mag = np.zeros(C_new.shape)
  np.add.at(mag, labels, np.abs(Xb))
  wn = np.maximum(w_prev + m, 1.0)[:, None]
  new = (err_prev * w_prev[:, None] + (m[:, None] + 2) * U * mag) / wn + U * np.abs(C_new)
  return np.where(m[:, None] > 0, new, err_prev)


def blobs(n, d, k, seed, sep=6.0):
  rng = np.random.RandomState(seed)
  cen = rng.standard_normal((k, d)) * sep / np.sqrt(2.0)
  which = rng.randint(0, k, n)
  which[:k] = np.arange(k)
  return (cen[which] + rng.standard_normal((n, d))).astype(np.float32), which, cen.astype(np.float32)


def lattice_blobs(n, d, k, seed):
  """Integer data: k centres in {0, 8}^d, points = centre + {-1, 0, 1} noise.  Sums and weights stay exact in fp32."""
  rng = np.random.RandomState(seed)
  cen = 8 * rng.randint(0, 2, (k, d))
  while len(set(map(tuple, cen))) < k:
    cen = 8 * rng.randint(0, 2, (k, d))
  which = np.arange(n) % k
  return (cen[which] + rng.randint(-1, 2, (n, d))).astype(np.float32), which, cen.astype(np.float32)


# ---- the reference's sampling lines, literally (kmeans_segmentation_eval.py:30, :78-81, :88) ---------------------------------
def reference_budget(max_num_kmeans_samples, num_imgs):
  return int(max_num_kmeans_samples / num_imgs)


def reference_select(x_out_masked, num_imgs_batch, max_num_pixels_per_img, rng):
  """Lines :78-91 on the masked feature rows [num_unmasked, C]: the block written into features_all."""
  num_unmasked = x_out_masked.shape[0]
  num_selected = min(num_unmasked, num_imgs_batch * max_num_pixels_per_img)
  selected = rng.choice(num_selected, replace=False)
  x_out = x_out_masked[selected, :]
  block = np.zeros((num_selected, x_out_masked.shape[1]), dtype=np.float32)
  block[0:num_selected, :] = x_out
  return num_selected, block
