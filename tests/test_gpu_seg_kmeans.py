"""Segmentation k-means evaluation on the device (csrc/seg_kmeans.hip, iic_amd/seg_kmeans.py,
iic_amd.kmeans.MiniBatchKMeans) against the parts already trusted and the float64 restatements of
tests/seg_kmeans_cases.py.

Entry points: iic_seg_kmeans_label_acc (label_acc, apply_trained_kmeans), iic_seg_kmeans_label_lds_floats,
iic_seg_feat_sample (feat_sample, train_kmeans), iic_kmeans_minibatch_update (MiniBatchKMeans).  Bit-for-bit tier: the
fused kernel against iic_bilinear_fwd + arg-min + iic_seg_contingency_acc, the sampler against gather + iic_bilinear_fwd.
Float64 tier: labels outside the derived gap, dots and centres inside derived bounds.  No scikit-learn here: the
restatements' equality with it is tests/test_seg_kmeans_cpu.py's."""
import types

import numpy as np
import pytest
import torch

from tests import kmeans_cases as kc
from tests import seg_kmeans_cases as sc

pytestmark = pytest.mark.gpu
P = 3      # border of the segmentation trunk's PT tensors


def dev():
  return torch.device("cuda:0")


def _g(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bilinear(dots, S):
  from iic_amd._lib import check, lib, ptr, stream_ptr
  N, Hl, Wl, k = dots.shape
  out = torch.empty((N, k, S, S), dtype=torch.float32, device=dots.device)
  check(lib().iic_bilinear_fwd(ptr(dots), ptr(out), N, Hl, Wl, k, S, stream_ptr()), "iic_bilinear_fwd")
  return out


def _contingency(labels, targets, mask, k, k_gt, counts=None):
  from iic_amd._lib import check, lib, ptr, stream_ptr
  if counts is None:
    counts = torch.zeros((k * k_gt + 1,), dtype=torch.long, device=labels.device)
  check(lib().iic_seg_contingency_acc(ptr(labels), ptr(targets), ptr(mask), labels.numel(), k, k_gt, ptr(counts),
                                      stream_ptr()), "iic_seg_contingency_acc")
  return counts


def _parts(dots, cnorm, S):
  """uint8 [N, S, S]: argmin_j (cnorm - 2 iic_bilinear_fwd(dots)), taken with torch on the existing kernel's output."""
  score = cnorm[None, :, None, None] - 2.0 * _bilinear(dots, S)
  return torch.argmin(score, dim=1).to(torch.uint8).contiguous()


def _fused_inputs(case, seed=0):
  Hl, Wl, S, k, N = case
  rng = np.random.RandomState(seed + Hl + 7 * S + k)
  k_gt = min(k, 5)
  dots = _g(rng.standard_normal((N, Hl, Wl, k)).astype(np.float32))
  cnorm = _g((0.5 * rng.random_sample(k)).astype(np.float32))
  targets = rng.randint(0, k_gt, (N, S, S)).astype(np.uint8)
  targets[rng.random_sample((N, S, S)) < 0.05] = 255      # out of range: selected, but in no cell
  mask = (rng.random_sample((N, S, S)) < 0.8) * rng.randint(1, 256, (N, S, S))
  return dots, cnorm, _g(targets), _g(mask.astype(np.uint8)), k_gt


# ---- fused kernel against the parts, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.FUSED_CASES, ids=lambda c: "%dx%d_S%d_k%d_N%d" % c)
def test_fused_equals_bilinear_argmin_contingency(case):
  from iic_amd import _lib, seg_kmeans
  Hl, Wl, S, k, N = case
  floats = _lib.lib().iic_seg_kmeans_label_lds_floats(Hl, Wl, k, S)
  assert (floats == 0) == (case in sc.GLOBAL_FORM), floats      # which side of the kernel's variant switch
  dots, cnorm, targets, mask, k_gt = _fused_inputs(case)
  want_labels = _parts(dots, cnorm, S)
  want_counts = _contingency(want_labels, targets, mask, k, k_gt)
  counts = torch.zeros((k * k_gt + 1,), dtype=torch.long, device=dev())
  labels = torch.full((N, S, S), 255, dtype=torch.uint8, device=dev())
  seg_kmeans.label_acc(dots, cnorm, targets, mask, k_gt, counts, S, labels_u8=labels)
  assert torch.equal(labels, want_labels)
  assert torch.equal(counts, want_counts)
  assert int(counts[-1]) == int((mask != 0).sum()) and int(counts[:-1].sum()) <= int(counts[-1])
  # no label map asked for: the same counts
  counts2 = torch.zeros_like(counts)
  seg_kmeans.label_acc(dots, cnorm, targets, mask, k_gt, counts2, S)
  assert torch.equal(counts2, want_counts)


def test_fused_mask_forms_unaligned_labels_and_accumulation():
  from iic_amd import seg_kmeans
  case = sc.FUSED_CASES[0]
  Hl, Wl, S, k, N = case
  dots, cnorm, targets, mask, k_gt = _fused_inputs(case, seed=5)
  want_labels = _parts(dots, cnorm, S)
  nb = k * k_gt
  # null mask: every pixel selected
  counts = torch.zeros((nb + 1,), dtype=torch.long, device=dev())
  seg_kmeans.label_acc(dots, cnorm, targets, None, k_gt, counts, S)
  assert torch.equal(counts, _contingency(want_labels, targets, None, k, k_gt)) and int(counts[-1]) == N * S * S
  # all-zero mask: nothing is counted
  counts = torch.zeros((nb + 1,), dtype=torch.long, device=dev())
  seg_kmeans.label_acc(dots, cnorm, targets, torch.zeros_like(mask), k_gt, counts, S)
  assert int(counts.abs().sum()) == 0
  # a label map at an odd address (S % 4 == 0 here: only the base is unaligned), sentinels around it untouched
  buf = torch.full((N * S * S + 8,), 77, dtype=torch.uint8, device=dev())
  labels = buf[3:3 + N * S * S].view(N, S, S)
  assert labels.data_ptr() % 4 != 0
  counts = torch.zeros((nb + 1,), dtype=torch.long, device=dev())
  seg_kmeans.label_acc(dots, cnorm, targets, mask, k_gt, counts, S, labels_u8=labels)
  assert torch.equal(labels, want_labels) and bool((buf[:3] == 77).all()) and bool((buf[3 + N * S * S:] == 77).all())
  # two calls accumulate into one counts
  once = counts.clone()
  seg_kmeans.label_acc(dots, cnorm, targets, mask, k_gt, counts, S)
  assert torch.equal(counts, 2 * once)
  assert torch.equal(once, _contingency(want_labels, targets, mask, k, k_gt))


def test_ties_and_non_finite_scores():
  from iic_amd import seg_kmeans
  Hl, Wl, S, k, N = 8, 8, 24, 4, 3
  rng = np.random.RandomState(2)
  d = rng.standard_normal((N, Hl, Wl, k)).astype(np.float32)
  d[0, :, :, 2] = d[0, :, :, 1] = np.abs(d[0, :, :, 1]) + 5.0      # image 0: centres 1 and 2 equal and best everywhere
  d[1, :, :, 0] = np.nan                                            # image 1: channel 0 is NaN and must never win
  d[2] = np.nan                                                     # image 2: every score NaN: label 0
  cn = np.array([0.3, 0.1, 0.1, 0.2], dtype=np.float32)
  dots, cnorm = _g(d), _g(cn)
  targets = torch.zeros((N, S, S), dtype=torch.uint8, device=dev())
  counts = torch.zeros((k + 1,), dtype=torch.long, device=dev())
  labels = torch.full((N, S, S), 255, dtype=torch.uint8, device=dev())
  seg_kmeans.label_acc(dots, cnorm, targets, None, 1, counts, S, labels_u8=labels)
  got = labels.cpu().numpy()
  score = (cnorm[None, :, None, None] - 2.0 * _bilinear(dots, S)).permute(0, 2, 3, 1).cpu().numpy()
  assert np.array_equal(got, sc.rule_argmin(score))
  assert (got[0] == 1).all()
  assert (got[1] != 0).all()
  assert (got[2] == 0).all()
  assert counts.cpu().tolist() == [int((got == j).sum()) for j in range(k)] + [N * S * S]


# ---- against the reference's order of operations in float64 ---------------------------------------------------------------------
def _device_labels(X, C, S):
  """The device path on features X [N, Hl, Wl, C] (numpy fp32): gather-free GEMM dots, then the fused kernel."""
  from iic_amd import ops, seg_kmeans
  N, Hl, Wl, Cc = X.shape
  k = C.shape[0]
  Xg, Cg = _g(X.reshape(-1, Cc)), _g(C)
  dots = torch.empty((N, Hl, Wl, k), dtype=torch.float32, device=dev())
  ops.gemm_f32(Xg, Cc, 1, Cg, 1, Cc, dots, k, N * Hl * Wl, k, Cc)
  cnorm = (Cg * Cg).sum(1).contiguous()
  targets = torch.zeros((N, S, S), dtype=torch.uint8, device=dev())
  counts = torch.zeros((k + 1,), dtype=torch.long, device=dev())
  labels = torch.empty((N, S, S), dtype=torch.uint8, device=dev())
  seg_kmeans.label_acc(dots, cnorm, targets, None, 1, counts, S, labels_u8=labels)
  return labels.cpu().numpy().astype(np.int64), counts.cpu().numpy()


@pytest.mark.parametrize("case", sc.BRACKET_CASES, ids=lambda c: "%dx%dx%d_k%d" % (c["Hl"], c["Wl"], c["S"], c["k"]))
def test_labels_equal_float64_argmin_outside_the_gap(case):
  X, C = sc.clustered_features(case["N"], case["Hl"], case["Wl"], case["C"], case["k"], case["seed"])
  S64 = sc.scores64(X, C, case["S"])
  gap = sc.under_gap(S64, sc.score_error(X, C))
  assert gap.mean() <= sc.GAP_CAP      # a condition on the inputs (tests/test_seg_kmeans_cpu.py asserts it too)
  got, _ = _device_labels(X, C, case["S"])
  want = np.argmin(S64, axis=-1)
  print("under the gap %d of %d pixels; off the float64 arg-min %d" % (gap.sum(), gap.size, (got != want).sum()))
  assert (got[~gap] == want[~gap]).all()


def test_lattice_with_dyadic_weights_leaves_no_pixel_out():
  c = sc.LATTICE_CASE
  X, C = sc.lattice_features(c["N"], c["Hl"], c["Wl"], c["C"], c["k"], c["seed"])
  want = np.argmin(sc.scores64(X, C, c["S"]), axis=-1)
  got, counts = _device_labels(X, C, c["S"])
  assert np.array_equal(got, want)
  assert counts.tolist() == np.bincount(want.reshape(-1), minlength=c["k"]).tolist() + [want.size]


# ---- the sampler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("C", [512, 5])
def test_feat_sample_equals_indexed_bilinear(C, dtype):
  from iic_amd import seg_kmeans
  N, Hl, Wl, S = 2, 5, 6, 14
  rng = np.random.RandomState(C)
  pt = torch.from_numpy(rng.standard_normal((N, Hl + 2 * P, Wl + 2 * P, C)).astype(np.float32)).to(dev())
  if dtype == "bf16":
    pt = pt.to(torch.bfloat16)
  interior = pt[:, P:P + Hl, P:P + Wl, :].float().contiguous()      # the fp32-converted interior
  full = _bilinear(interior, S)      # [N, C, S, S]
  special = [(0, 0, 0), (0, 0, S - 1), (1, S - 1, 0), (1, S - 1, S - 1), (0, 0, 5), (1, 7, 0), (0, S - 1, 4), (1, 6, S - 1),
             (1, 3, 3), (1, 3, 3)]      # corners, edges, a repeated pixel
  for m in sc.SAMPLE_M:
    coords = np.array(special, dtype=np.int32)[:m]
    if m > len(special):
      more = np.stack([rng.randint(0, N, m - len(special)), rng.randint(0, S, m - len(special)),
                       rng.randint(0, S, m - len(special))], axis=1).astype(np.int32)
      coords = np.concatenate([coords, more])
    out = torch.full((m + 1, C), -7.0, device=dev())
    got = seg_kmeans.feat_sample(pt, coords, S, out=out[:m])
    assert tuple(got.shape) == (m, C) and bool((out[m] == -7.0).all())      # m = 0 writes nothing
    if m:
      ci = torch.from_numpy(coords.astype(np.int64)).to(dev())
      want = full[ci[:, 0], :, ci[:, 1], ci[:, 2]]
      assert torch.equal(got, want)
      if m > 9:
        assert torch.equal(got[8], got[9])


# ---- the dots: fused head kernel at off = P, and gather + GEMM ----------------------------------------------------------------
@pytest.mark.parametrize("k", [27, 33])
def test_trunk_dots_inside_the_gemm_bound(k):
  from iic_amd import _lib, seg_kmeans
  from tests.parity import fma_acc_bound
  N, Hl, Wl, C = 2, 8, 9, 512
  assert bool(_lib.lib().iic_seg_head_supported(C, k)) == (k == 27)      # both paths are exercised
  rng = np.random.RandomState(k)
  pt = torch.from_numpy(rng.standard_normal((N, Hl + 2 * P, Wl + 2 * P, C)).astype(np.float32)).to(dev()).to(torch.bfloat16)
  cen = _g(rng.standard_normal((k, C)).astype(np.float32))
  dots = seg_kmeans.trunk_dots(pt, cen)
  assert tuple(dots.shape) == (N, Hl, Wl, k)
  x64 = pt[:, P:P + Hl, P:P + Wl, :].double().reshape(-1, C)
  want = x64 @ cen.double().t()
  tol = fma_acc_bound(C, x64.abs() @ cen.double().abs().t(), extra=1)
  err = (dots.reshape(-1, k).double() - want).abs()
  print("dots k=%d: largest error / bound %.3f" % (k, float((err / tol).max())))
  assert bool((err <= tol).all())


# ---- MiniBatchKMeans ------------------------------------------------------------------------------------------------------------
def _mb_data(n, d, k, seed):
  X, which, cen = sc.blobs(n, d, k, seed)
  C0 = (cen + 0.1 * np.random.RandomState(seed + 1).standard_normal(cen.shape)).astype(np.float32)
  return X, C0


@pytest.mark.parametrize("n,d,k,batch", [(300, 512, 3, 40), (64, 7, 27, 32)])
def test_minibatch_steps_inside_float64_bounds(n, d, k, batch):
  from iic_amd import kmeans
  X, C0 = _mb_data(n, d, k, seed=n + k)
  rng = np.random.RandomState(4)
  batches = [rng.randint(0, n, batch) for _ in range(5)]
  want = sc.fit64(X, C0, batches, max_no_improvement=None, reassignment_ratio=0.0)
  Xg = _g(X)
  km = kmeans.MiniBatchKMeans(k, init=C0, reassignment_ratio=0.0, max_no_improvement=None)
  err = np.zeros((k, d))
  C_prev, w_prev = C0.astype(np.float64), np.zeros(k)
  for step, idx in enumerate(batches):
    km.partial_fit(Xg[torch.from_numpy(idx).to(dev())])
    C64, w64, inertia64 = want["hist"][step]
    S, E = kc.score_bounds(X[idx], C_prev)
    assert not kc.ambiguity(S, E)[0].any()      # a condition on the data: the labels of the step are then determined
    labels, mind64 = sc.assign64(X[idx], C_prev)
    # the batch inertia is taken against the device's own centres, within `err` of C_prev: every distance moves by at
    # most 2 |x - c| |dc| + |dc|^2; the score bound E is evaluated at C_prev (1.001: the centres' own 1e-7 shift in it)
    dc = np.sqrt((err * err).sum(1))[labels]
    inertia_tol = 1.001 * (kc.mind_bound(X[idx], E, labels) + 2 * np.sqrt(mind64) * dc + dc * dc).sum()
    err = sc.centre_bound_step(err, w_prev, X[idx], labels, C64)
    got_C = km.cluster_centers_.cpu().numpy().astype(np.float64)
    assert np.array_equal(km.counts_.cpu().numpy(), w64)      # w is exact
    print("step %d: largest centre error / bound %.3f" % (step, float((np.abs(got_C - C64) / np.maximum(err, 1e-300)).max())))
    assert (np.abs(got_C - C64) <= err).all()
    assert abs(km.batch_inertia_ - inertia64) <= inertia_tol
    C_prev, w_prev = C64, w64
  assert km.n_steps_ == 5
  # fit on the same forced batches walks the same steps: the same bits as the partial_fit chain
  fit = kmeans.MiniBatchKMeans(k, init=C0, reassignment_ratio=0.0, max_no_improvement=None).fit(Xg, batches=batches)
  assert fit.n_steps_ == 5
  assert torch.equal(fit.cluster_centers_, km.cluster_centers_) and torch.equal(fit.counts_, km.counts_)
  assert torch.equal(fit.labels_, fit.predict(Xg))
  lab64, mind64 = sc.assign64(X, want["centres"])
  assert np.array_equal(fit.labels_.cpu().numpy(), lab64)
  assert abs(fit.inertia_ - mind64.sum()) <= 1e-3 * mind64.sum()


def test_early_stop_fires_at_the_same_step_on_lattice_data():
  from iic_amd import kmeans
  n, d, k, batch = 240, 16, 3, 30
  X, _, cen = sc.lattice_blobs(n, d, k, seed=6)
  rng = np.random.RandomState(8)
  batches = [rng.randint(0, n, batch) for _ in range(60)]
  want = sc.fit64(X, cen, batches, max_no_improvement=3, reassignment_ratio=0.0)
  print("float64 stops after %d steps; smallest decision margin %.2e" % (want["n_steps"], want["schedule"].min_margin))
  assert 4 < want["n_steps"] < len(batches)      # the early stop really fires
  assert want["schedule"].min_margin > 1e-4      # no comparison of the smoothed inertia is within fp32's reach of a tie
  for ce in (1, 8):
    km = kmeans.MiniBatchKMeans(k, init=cen, max_no_improvement=3, reassignment_ratio=0.0, check_every=ce)
    km.fit(_g(X), batches=batches)
    assert km.n_steps_ == want["n_steps"]
    assert np.array_equal(km.counts_.cpu().numpy(), want["w"])
    # every fp32 distance is a sum of d + 2 = 18 rounded terms (1.1e-6 relative), the centres carry a few u more: 1e-5
    assert abs(km.ewa_inertia_ - want["schedule"].ewa) <= 1e-5 * want["schedule"].ewa


def test_under_weighted_centre_pauses_and_lands_where_the_restatement_puts_it():
  from iic_amd import kmeans
  n, d, k, batch = 200, 8, 4, 50
  X, _, cen = sc.blobs(n, d, 3, seed=3, sep=8.0)
  C0 = np.concatenate([cen, np.full((1, d), 1e3, dtype=np.float32)])      # the last centre attracts no point
  rng = np.random.RandomState(1)
  batches = [rng.randint(0, n, batch) for _ in range(4)]
  choice = lambda nb, size: np.arange(7, 7 + size)
  want = sc.fit64(X, C0, batches, max_no_improvement=None, choice=choice)
  assert want["reassigned"][0].tolist() == [False, False, False, True]      # step 1: w_3 = 0 < 1 % of the heaviest
  assert not any(r.any() for r in want["reassigned"][1:])
  fits = []
  for ce in (1, 8):
    km = kmeans.MiniBatchKMeans(k, init=C0, max_no_improvement=None, check_every=ce)
    km._choice = choice
    fits.append(km.fit(_g(X), batches=batches))
    assert km.n_steps_ == 4 and km.n_pauses_ == 1      # the device raised `pause` once, at the first step
    assert np.array_equal(km.counts_.cpu().numpy(), want["w"])
    got = km.cluster_centers_.cpu().numpy().astype(np.float64)
    # per step the fp32 sum of m <= 50 rows is within (m + 2) u m max |x|, divided by w + m >= m, and the quotient is
    # rounded once (u |c| <= u max |x|); incoming errors only shrink: 4 (52 + 1) u max |x| per coordinate
    assert (np.abs(got - want["centres"]) <= 212 * sc.U * np.abs(X).max()).all()
  assert torch.equal(fits[0].cluster_centers_, fits[1].cluster_centers_)
  # one step alone: the reassigned centre IS the picked batch row, bit for bit, and takes the smallest remaining weight
  km = kmeans.MiniBatchKMeans(k, init=C0, max_no_improvement=None)
  km._choice = choice
  km.partial_fit(_g(X[batches[0]]))
  assert np.array_equal(km.cluster_centers_[3].cpu().numpy(), X[batches[0]][7])
  assert np.array_equal(km.counts_.cpu().numpy(), want["hist"][0][1])


def test_two_fits_identical_and_check_every_invisible():
  from iic_amd import kmeans
  X, _, _ = sc.blobs(1500, 40, 6, seed=9, sep=1.5)
  X[:3] += 60.0      # three far points: k-means++ seeds one, most mini-batches miss them -- its weight stays 0: a pause
  Xg = _g(X)
  fits = [kmeans.MiniBatchKMeans(6, seed=3, max_iter=2, check_every=ce).fit(Xg) for ce in (8, 8, 1)]
  print("n_steps %s, pauses %s" % ([f.n_steps_ for f in fits], [f.n_pauses_ for f in fits]))
  assert fits[0].n_pauses_ >= 1      # the host really rewound its RandomState and dropped the batches drawn ahead
  for f in fits[1:]:
    assert f.n_pauses_ == fits[0].n_pauses_
    assert f.n_steps_ == fits[0].n_steps_ and f.inertia_ == fits[0].inertia_
    assert torch.equal(f.cluster_centers_, fits[0].cluster_centers_)
    assert torch.equal(f.counts_, fits[0].counts_)
    assert torch.equal(f.labels_, fits[0].labels_)
  assert torch.equal(fits[0].fit_predict(Xg), fits[0].labels_)


def test_refusals_enqueue_nothing():
  from iic_amd import _lib, kmeans, seg_kmeans
  L, Pp, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
  dots = torch.zeros((1, 4, 4, 3), device=dev())
  cn = torch.zeros((3,), device=dev())
  tg = torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev())
  counts = torch.full((3 * 3 + 1,), -7, dtype=torch.long, device=dev())
  assert L.iic_seg_kmeans_label_acc(Pp(dots), Pp(cn), Pp(tg), None, 1, 4, 4, 256, 8, 3, Pp(counts), None, s) == -3
  assert L.iic_seg_kmeans_label_acc(Pp(dots), Pp(cn), Pp(tg), None, 1, 4, 4, 255, 8, 65, Pp(counts), None, s) == -3
  assert L.iic_seg_kmeans_label_acc(Pp(dots), Pp(cn), None, None, 1, 4, 4, 3, 8, 3, Pp(counts), None, s) == -1
  assert L.iic_seg_feat_sample(Pp(dots), 1, None, 4, Pp(dots), 1, 4, 4, 4, 4, 1, 3, 8, s) == -1
  assert L.iic_kmeans_minibatch_update(Pp(dots), Pp(dots), Pp(dots), Pp(counts), Pp(dots), 10, 8, 257, 0, Pp(dots),
                                       Pp(dots), s) == -3
  torch.cuda.synchronize()
  assert bool((counts == -7).all())
  with pytest.raises(ValueError, match="served range"):
    seg_kmeans.label_acc(torch.zeros((1, 2, 2, 200), device=dev()), torch.zeros((200,), device=dev()),
                         torch.zeros((1, 4, 4), dtype=torch.uint8, device=dev()), None, 100,
                         torch.zeros((20001,), dtype=torch.long, device=dev()), 4)
  with pytest.raises(ValueError, match="no CPU fallback"):
    seg_kmeans.trunk_dots(torch.zeros((1, 8, 8, 512)), torch.zeros((3, 512)))
  with pytest.raises(ValueError, match="should be >= n_clusters"):
    kmeans.MiniBatchKMeans(9).fit(torch.zeros((4, 3), device=dev()))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
class _Loader(object):
  """What the reference's test dataloader offers the routine: len(loader.dataset), iteration over CPU batches."""

  def __init__(self, batches, num_imgs):
    self.batches, self.dataset = batches, list(range(num_imgs))

  def __len__(self):
    return len(self.batches)

  def __iter__(self):
    return iter(self.batches)


def _e2e_config(**kw):
  c = dict(in_channels=3, input_sz=24, batchnorm_track=True, num_sub_heads=1, output_k=3, gt_k=3, no_sobel=True,
           include_rgb=True, using_IR=False, max_num_kmeans_samples=600, verbose=0)
  c.update(kw)
  return types.SimpleNamespace(**c)


@pytest.mark.parametrize("arch", ["SegmentationNet10aFeatures", "SegmentationNet10aTwoHead"])
def test_eval_equals_the_literal_composition(arch):
  from iic_amd import archs, eval_metrics, kmeans, seg_kmeans
  from iic_amd.archs import seg as seg_archs
  config = _e2e_config(output_k_A=6, output_k_B=3)
  torch.manual_seed(0)
  net = getattr(archs, arch)(config).to(dev())
  S, gt_k, n_img, bs = config.input_sz, config.gt_k, 5, 2
  rng = np.random.RandomState(12)
  imgs = rng.random_sample((n_img, 3, S, S)).astype(np.float32)
  imgs[:, :, : S // 2] += 1.5 * rng.random_sample((n_img, 3, 1, 1)).astype(np.float32)      # structure for the trunk
  targets = rng.randint(0, gt_k, (n_img, S, S)).astype(np.int32)
  mask = rng.random_sample((n_img, S, S)) < 0.85
  batches = [(torch.from_numpy(imgs[i:i + bs]), torch.from_numpy(targets[i:i + bs]), torch.from_numpy(mask[i:i + bs]))
             for i in range(0, n_img, bs)]      # the reference's CPU tensors; the last batch is ragged
  loader = _Loader(batches, n_img)
  km = kmeans.MiniBatchKMeans(gt_k, seed=1)
  np.random.seed(3)
  acc, nmi, ari, masses = seg_kmeans.kmeans_segmentation_eval(config, net, loader, sampling="uniform", kmeans=km)
  assert not net.training and (nmi, ari) == (-1., -1.)
  centres = km.cluster_centers_
  # the literal composition: forward(penultimate=True) -> mask -> the same centres -> KMeans.predict -> match / _acc
  kp = kmeans.KMeans(gt_k)
  kp.cluster_centers_ = centres
  preds, tgts, n_gap, n_pix = [], [], 0, 0
  with torch.no_grad():
    for b_imgs, b_t, b_m in batches:
      if arch == "SegmentationNet10aFeatures":
        x_out = net(b_imgs.to(dev()), penultimate=True)
        assert tuple(x_out.shape) == (b_imgs.shape[0], 512, S, S) and x_out.dtype == torch.float32
      else:
        x_out = seg_archs.upsampled_features(seg_archs.trunk_pt(net, b_imgs.to(dev())), S)
      rows = x_out.permute(0, 2, 3, 1)[b_m.to(dev())].contiguous()
      preds.append(kp.predict(rows))
      tgts.append(b_t.to(dev())[b_m.to(dev())])
      # float64, for the gap: the features at the trunk's resolution
      pt = seg_archs.trunk_pt(net, b_imgs.to(dev()))
      feats = pt[:, P:-P, P:-P, :].float().cpu().numpy()
      S64 = sc.scores64(feats, centres.cpu().numpy(), S)
      n_gap += int((sc.under_gap(S64, sc.score_error(feats, centres.cpu().numpy())) & b_m.numpy()).sum())
      n_pix += int(b_m.sum())
  preds, tgts = torch.cat(preds), torch.cat(tgts)
  print("%d of %d selected pixels under the gap" % (n_gap, n_pix))
  assert n_gap <= sc.GAP_CAP * n_pix
  want_counts = eval_metrics._counts(preds, tgts, gt_k, gt_k)
  got_counts, n = seg_kmeans._apply_counts(config, net, loader, km)
  assert n == n_pix == int(mask.sum())
  assert np.abs(got_counts - want_counts).sum() <= 2 * n_gap      # a pixel under the gap may sit in another cell
  match = eval_metrics._hungarian_match(preds, tgts, preds_k=gt_k, targets_k=gt_k)
  reordered = torch.zeros_like(preds)
  for pred_i, target_i in match:
    reordered[preds == pred_i] = target_i
  want_acc = eval_metrics._acc(reordered, tgts, gt_k)
  want_masses = np.array([float((reordered == c).sum()) / n_pix for c in range(gt_k)])
  if n_gap == 0:
    assert acc == want_acc and np.array_equal(masses, want_masses)
  else:
    assert abs(acc - want_acc) <= n_gap / float(n_pix) and np.abs(masses - want_masses).max() <= n_gap / float(n_pix)
  # the reference's selection line: every batch contributes copies of ONE pixel -- 3 batches, 3 distinct rows
  np.random.seed(3)
  ref = seg_kmeans.train_kmeans(config, net, loader, sampling="reference", kmeans=kmeans.MiniBatchKMeans(gt_k, seed=1))
  assert ref.cluster_centers_.shape == (gt_k, 512)
  stats = seg_kmeans.apply_trained_kmeans(config, net, loader, km, get_nmi_ari=True)
  assert stats[0] == acc and 0.0 <= stats[1] <= 1.0 and -1.0 <= stats[2] <= 1.0


def test_device_resident_batches_are_consumed_as_they_are():
  """uint8 targets and mask already on the device (what SegTestPreparer / seg_mapping_dataloader yield) give the counts of
  the reference's CPU tensors."""
  from iic_amd import archs, kmeans, seg_kmeans
  config = _e2e_config()
  torch.manual_seed(2)
  net = archs.SegmentationNet10aFeatures(config).to(dev()).eval()
  S, gt_k = config.input_sz, config.gt_k
  rng = np.random.RandomState(5)
  imgs = torch.from_numpy(rng.random_sample((2, 3, S, S)).astype(np.float32))
  targets = rng.randint(0, gt_k, (2, S, S))
  mask = rng.random_sample((2, S, S)) < 0.5
  km = types.SimpleNamespace(cluster_centers_=rng.standard_normal((gt_k, 512)).astype(np.float32) * 0.05)
  cpu = _Loader([(imgs, torch.from_numpy(targets.astype(np.int32)), torch.from_numpy(mask))], 2)
  gpu = _Loader([(imgs.to(dev()), _g(targets.astype(np.uint8)), _g(mask.astype(np.uint8)))], 2)
  a, na = seg_kmeans._apply_counts(config, net, cpu, km)
  b, nb = seg_kmeans._apply_counts(config, net, gpu, km)
  assert np.array_equal(a, b) and na == nb == int(mask.sum())
