"""k-means on the device (csrc/kmeans.hip, iic_amd/kmeans.py) against the float64 oracle of tests/kmeans_cases.py.

Entry points: iic_kmeans_assign and iic_kmeans_update (lloyd_step, KMeans), iic_kmeans_seed_potential (seed_potentials,
kmeans_plusplus), and the host-side queries iic_kmeans_supported / iic_kmeans_workspace_bytes (supported,
workspace_bytes).  Exact tier: the integer lattice, no tolerance.  Float64 tier: random cases, every figure inside the
derived bounds of kmeans_cases.  No scikit-learn here: the oracle's equality with it is tests/test_kmeans_cpu.py's."""
import types

import numpy as np
import pytest
import torch

from tests import kmeans_cases as kc
from tests.lattice import assert_exact

pytestmark = pytest.mark.gpu


def dev():
  return torch.device("cuda:0")


def _g(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _step(X, C):
  from iic_amd import kmeans
  labels, sums, counts, mind = kmeans.lloyd_step(X, C)
  torch.cuda.synchronize()
  return labels.cpu().numpy().astype(np.int64), sums.cpu().numpy(), counts.cpu().numpy(), mind.cpu().numpy()


# ---- exact tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", kc.LATTICE_SHAPES + ["ldx"], ids=lambda s: s if isinstance(s, str) else "%dx%dx%d" % s)
def test_lattice_step_is_exact(shape):
  if shape == "ldx":
    n, d, k = kc.LDX_CASE
    X, C = kc.lattice_case(kc.LDX_CASE)
    wide = torch.full((n, d + kc.LDX_PAD), 7.0, device=dev())      # the padding must never be read into a result
    wide[:, :d] = _g(X)
    Xg = wide[:, :d]
    assert Xg.stride(0) == d + kc.LDX_PAD
  else:
    n, d, k = shape
    X, C = kc.lattice_case(shape)
    Xg = _g(X)
  want_labels, want_mind = kc.assign64(X, C)
  want_sums, want_counts = kc.accumulate64(X, want_labels, k)
  kc.lattice_preconditions(X, C, want_labels, want_sums)
  labels, sums, counts, mind = _step(Xg, _g(C))
  assert labels.min() >= 0 and labels.max() < k
  assert_exact(labels, want_labels, "labels")
  assert_exact(counts, want_counts, "counts")
  assert_exact(sums, want_sums, "sums")
  assert_exact(mind, want_mind, "mind")


# ---- float64 tier -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.RANDOM_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_random_step_inside_float64_bounds(case):
  X, C = kc.random_case(case)
  n, d, k = case[:3]
  S, E = kc.score_bounds(X, C)
  amb, allowed = kc.ambiguity(S, E)
  assert amb.mean() <= kc.AMBIGUOUS_CAP
  labels, sums, counts, mind = _step(_g(X), _g(C))
  rows = np.arange(n)
  print("ambiguous rows %d, labels off the float64 arg-min %d" % (amb.sum(), (labels != np.argmin(S, 1)).sum()))
  assert labels.min() >= 0 and labels.max() < k
  assert (labels[~amb] == np.argmin(S, axis=1)[~amb]).all()
  assert allowed[rows, labels].all()
  assert np.array_equal(counts, np.bincount(labels, minlength=k))
  sums64, _ = kc.accumulate64(X, labels, k)
  err = np.abs(sums - sums64)
  bound = kc.sum_bound(X, labels, k)
  print("sums: largest error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()))
  assert (err <= bound).all()
  X64 = X.astype(np.float64)
  mind64 = np.maximum(0.0, (X64 * X64).sum(1) + S[rows, labels])
  merr, mb = np.abs(mind - mind64), kc.mind_bound(X, E, labels)
  print("mind: largest error / bound %.3f" % float((merr / mb).max()))
  assert (merr <= mb).all()


# ---- reproducibility, latch -----------------------------------------------------------------------------------------------------
def test_two_steps_and_two_fits_are_bit_identical():
  from iic_amd import kmeans
  X, C = kc.random_case(kc.RANDOM_CASES[0])
  Xg, Cg = _g(X), _g(C)
  a = kmeans.lloyd_step(Xg, Cg)
  b = kmeans.lloyd_step(Xg, Cg)
  for p, q in zip(a, b):
    assert torch.equal(p, q)
  Xb, _ = kc.blobs(1500, 40, 6, seed=9, sep=1.5)
  fits = [kmeans.KMeans(6, n_init=2, seed=3).fit(_g(Xb)) for _ in range(2)]
  assert torch.equal(fits[0].cluster_centers_, fits[1].cluster_centers_)
  assert torch.equal(fits[0].labels_, fits[1].labels_)
  assert fits[0].inertia_ == fits[1].inertia_ and fits[0].n_iter_ == fits[1].n_iter_


def test_latch_makes_check_every_invisible():
  from iic_amd import kmeans
  X, _ = kc.blobs(3000, 24, 9, seed=11, sep=0.8)      # overlapping: a dozen or more iterations
  C0 = X[np.random.RandomState(2).choice(3000, 9, replace=False)]
  fits = [kmeans.KMeans(9, init=C0, check_every=ce).fit(_g(X)) for ce in (1, 3, 8)]
  print("n_iter %s" % [f.n_iter_ for f in fits])
  assert fits[0].n_iter_ > 3
  for f in fits[1:]:
    assert f.n_iter_ == fits[0].n_iter_
    assert torch.equal(f.cluster_centers_, fits[0].cluster_centers_)
    assert torch.equal(f.labels_, fits[0].labels_)
    assert f.inertia_ == fits[0].inertia_


# ---- whole fits -----------------------------------------------------------------------------------------------------------------
def _check_fit(X, C0, km, want):
  k = C0.shape[0]
  labels = km.labels_.cpu().numpy().astype(np.int64)
  centres = km.cluster_centers_.cpu().numpy().astype(np.float64)
  assert km.n_iter_ == want["n_iter"]
  assert np.array_equal(labels, want["labels"])
  # the centres are fp32 sums of the final labels' rows over their count: the sum bound over the count (its two spare
  # roundings cover the division's)
  m = np.bincount(labels, minlength=k)
  bound = kc.sum_bound(X, labels, k) / np.maximum(m, 1)[:, None]
  assert (np.abs(centres - want["centres"]) <= bound).all()
  # inertia: the sum of mind against the fit's own centres, every term inside mind's bound
  S, E = kc.score_bounds(X, centres)
  X64 = X.astype(np.float64)
  rows = np.arange(X.shape[0])
  mind64 = np.maximum(0.0, (X64 * X64).sum(1) + S[rows, labels])
  assert abs(km.inertia_ - mind64.sum()) <= kc.mind_bound(X, E, labels).sum()
  assert abs(km.inertia_ - want["inertia"]) <= 1e-3 * want["inertia"]


@pytest.mark.parametrize("shape", kc.FIT_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_whole_fit_equals_oracle(shape):
  from iic_amd import kmeans
  n, d, k = shape
  X, which = kc.blobs(n, d, k, seed=21, sep=6.0)
  C0 = X[np.random.RandomState(1).choice(n, k, replace=False)]
  want = kc.lloyd64(X, C0, tol=0.0)
  km = kmeans.KMeans(k, init=C0, tol=0.0).fit(_g(X))
  _check_fit(X, C0, km, want)
  assert torch.equal(km.predict(_g(X)), km.labels_)


def test_empty_cluster_is_relocated_as_the_oracle_does():
  from iic_amd import kmeans
  X, C0 = kc.empty_cluster_case()
  want = kc.lloyd64(X, C0, tol=0.0)
  assert want["relocations"] >= 1
  for ce in (1, 8):
    km = kmeans.KMeans(C0.shape[0], init=C0, tol=0.0, check_every=ce).fit(_g(X))
    _check_fit(X, C0, km, want)


# ---- seeding ------------------------------------------------------------------------------------------------------------------
def test_seed_potentials_teacher_forced():
  from iic_amd import kmeans
  X, _ = kc.blobs(1000, 513, 5, seed=4, sep=2.0)
  rng = np.random.RandomState(0)
  mind = (rng.random_sample(1000) * 2000.0).astype(np.float32)
  cand = np.array([3, 999, 0, 512, 77, 3, 640, 1], dtype=np.int64)
  Xg, mg = _g(X), _g(mind)
  pot = kmeans.seed_potentials(Xg, _g(cand), mg).cpu().numpy()
  assert torch.equal(mg, _g(mind))      # write=False leaves mind alone
  dist = kc.seed_dist64(X, cand)
  want = np.minimum(mind.astype(np.float64)[:, None], dist).sum(0)
  bound = kc.seed_potential_bound(X, cand)
  print("potential: largest error / bound %.3f" % float((np.abs(pot - want) / bound).max()))
  assert (np.abs(pot - want) <= bound).all()
  assert pot[0] == pot[5]      # the same candidate in two slots: the same bits
  one = kmeans.seed_potentials(Xg, _g(cand[1:2]), mg, write=True).cpu().numpy()
  assert one[0] == pot[1]
  new = mg.cpu().numpy().astype(np.float64)
  d1 = dist[:, 1]
  assert (np.abs(new - np.minimum(mind, d1)) <= (X.shape[1] + 2) * kc.U * d1 + 1e-30).all()


def test_kmeans_plusplus_properties():
  from iic_amd import kmeans
  sb = kc.SEED_BLOBS
  X, which = kc.blobs(sb["n"], sb["d"], sb["k"], sb["data_seed"], sep=sb["sep"])
  Xg = _g(X)
  picks = {}
  for seed in kc.SEEDS_ONE_PER_BLOB:
    chosen = kmeans.kmeans_plusplus(Xg, sb["k"], np.random.RandomState(seed)).cpu().numpy()
    again = kmeans.kmeans_plusplus(Xg, sb["k"], np.random.RandomState(seed)).cpu().numpy()
    assert np.array_equal(chosen, again)      # deterministic in the seed
    assert chosen.min() >= 0 and chosen.max() < sb["n"]      # centres are rows of X
    assert len(set(chosen.tolist())) == sb["k"]      # and distinct
    assert sorted(which[chosen]) == list(range(sb["k"])), (seed, which[chosen])      # one per blob
    picks[seed] = tuple(chosen.tolist())
  assert len(set(picks.values())) > 1      # the seed matters
  km = kmeans.KMeans(sb["k"], n_init=1, seed=0).fit(Xg)
  assert sorted(np.bincount(km.labels_.cpu().numpy(), minlength=sb["k"])) == sorted(np.bincount(which))


# ---- non-finite input, refusals -------------------------------------------------------------------------------------------------
def test_nan_row_keeps_its_label_in_range_and_fit_raises():
  from iic_amd import kmeans
  X, C = kc.random_case(kc.RANDOM_CASES[3])
  X = X.copy()
  X[5, 3] = np.nan
  X[70] = np.nan
  X[200, 0] = np.inf
  labels, _, counts, mind = _step(_g(X), _g(C))
  assert labels.min() >= 0 and labels.max() < C.shape[0]
  assert counts.sum() == X.shape[0]
  assert not np.isfinite(mind[[5, 70, 200]]).any()
  with pytest.raises(ValueError, match="non-finite features"):
    kmeans.KMeans(C.shape[0], init=C, max_iter=4).fit(_g(X))


def test_refusals_leave_the_outputs_untouched():
  from iic_amd import _lib, kmeans
  L = _lib.lib()
  n, d, k = 64, 8, 3
  X = torch.zeros((n, d), device=dev())
  C = torch.zeros((k, d), device=dev())
  labels = torch.full((n,), -7, dtype=torch.int32, device=dev())
  mind = torch.full((n,), -7.0, device=dev())
  sums = torch.full((k, d), -7.0, device=dev())
  counts = torch.full((k,), -7, dtype=torch.long, device=dev())
  ws = torch.zeros((kmeans.workspace_bytes(n, d, k),), dtype=torch.uint8, device=dev())
  P, s = _lib.ptr, _lib.stream_ptr()
  for nn, dd, kk, ldx, rc in [(n, 32769, k, 32769, -3), (n, d, 257, d, -3), (0, d, k, d, -3), (2 ** 31, d, k, d, -3),
                              (n, d, k, d - 1, -1)]:
    assert not kmeans.supported(nn, dd, kk) or ldx < dd
    assert L.iic_kmeans_assign(P(X), ldx, P(C), nn, dd, kk, P(labels), P(mind), P(sums), P(counts), None, P(ws), None,
                               s) == rc
  state = torch.zeros((64,), dtype=torch.uint8, device=dev())
  assert L.iic_kmeans_update(P(C), P(sums), P(counts), n, d, 257, 0, P(ws), P(state), s) == -3
  cand = torch.zeros((9,), dtype=torch.long, device=dev())
  pot = torch.full((9,), -7.0, dtype=torch.float64, device=dev())
  assert L.iic_kmeans_seed_potential(P(X), d, n, d, P(cand), 9, P(mind), 0, P(pot), P(ws), s) == -1
  assert L.iic_kmeans_seed_potential(P(X), d, n, d, P(cand), 2, P(mind), 1, P(pot), P(ws), s) == -1
  torch.cuda.synchronize()
  for t in (labels, mind, sums, counts, pot):
    assert bool((t == -7).all())
  assert int(state.sum()) == 0 and float(C.abs().sum()) == 0.0
  km = kmeans.KMeans(n + 1)
  with pytest.raises(ValueError, match="should be >= n_clusters"):
    km.fit(X)
  assert not hasattr(km, "labels_") and not hasattr(km, "cluster_centers_")


# ---- on the nets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["ClusterNet5g", "ClusterNet6c"])
def test_kmeans_on_net_features(arch):
  from iic_amd import archs, eval_metrics, kmeans
  gt_k, n_img, bs = 4, 48, 16
  if arch == "ClusterNet5g":
    cfg = types.SimpleNamespace(in_channels=2, input_sz=32, batchnorm_track=True, num_sub_heads=2, output_k=gt_k)
    net, chans, sz = archs.ClusterNet5g(cfg), 2, 32
  else:
    cfg = types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, num_sub_heads=2, output_k=gt_k)
    net, chans, sz = archs.ClusterNet6c(cfg), 1, 24
  torch.manual_seed(0)
  net.to(dev()).train()
  rng = np.random.RandomState(6)
  targets = rng.randint(0, gt_k, n_img).astype(np.int64)
  # class-dependent images, so that the features cluster
  base = rng.random_sample((gt_k, chans, sz, sz)).astype(np.float32)
  imgs = base[targets] + 0.05 * rng.standard_normal((n_img, chans, sz, sz)).astype(np.float32)
  loader = list((torch.from_numpy(imgs[i:i + bs]), torch.from_numpy(targets[i:i + bs])) for i in range(0, n_img, bs))
  config = types.SimpleNamespace(batch_sz=bs, gt_k=gt_k, include_rgb=False, output_k=gt_k)
  # the features, copied out for the oracle
  net.eval()
  with torch.no_grad():
    feats = torch.cat([net(b[0].to(dev()), kmeans_use_features=True)[0].float() for b in loader]).cpu().numpy()
  net.train()
  assert feats.ndim == 2 and feats.shape[0] == n_img
  C0 = feats[[int(np.nonzero(targets == c)[0][0]) for c in range(gt_k)]]
  want = kc.lloyd64(feats, C0)
  S, E = kc.score_bounds(feats, want["centres"])
  assert not kc.ambiguity(S, E)[0].any()      # a condition on the features: the comparison below is then exact
  stats = kmeans.kmeans_eval(config, net, loader, False, kmeans=kmeans.KMeans(gt_k, init=C0))
  assert net.training      # bracketed with eval() / train()
  # host computation on the oracle's labels
  from scipy.optimize import linear_sum_assignment
  counts = np.zeros((gt_k, gt_k), dtype=np.int64)
  np.add.at(counts, (want["labels"], targets), 1)
  r, c = linear_sum_assignment(n_img - counts)
  acc = counts[r, c].sum() / float(n_img)
  nmi, ari = eval_metrics.nmi_ari_from_counts(counts)
  print("acc %.3f nmi %.3f ari %.3f, n_iter %d" % (acc, nmi, ari, want["n_iter"]))
  assert stats["acc"] == acc and stats["nmi"] == nmi and stats["ari"] == ari
  assert stats["mass"].shape == (1, gt_k) and stats["mass"].sum() == n_img
  assert stats["per_class_acc"].sum() == counts[r, c].sum()


def test_predictions_on_eval_features_equal_the_oracle():
  """get_data_kmeans_on_features itself, on a net already in eval() mode (what triplets_eval does before calling it)."""
  from iic_amd import archs, kmeans
  gt_k, n_img, bs = 3, 40, 20
  cfg = types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, num_sub_heads=1, output_k=gt_k)
  torch.manual_seed(1)
  net = archs.ClusterNet6c(cfg).to(dev()).eval()
  rng = np.random.RandomState(8)
  targets = rng.randint(0, gt_k, n_img).astype(np.int64)
  base = rng.random_sample((gt_k, 1, 24, 24)).astype(np.float32)
  imgs = base[targets] + 0.05 * rng.standard_normal((n_img, 1, 24, 24)).astype(np.float32)
  loader = list((torch.from_numpy(imgs[i:i + bs]), torch.from_numpy(targets[i:i + bs])) for i in range(0, n_img, bs))
  config = types.SimpleNamespace(batch_sz=bs, gt_k=gt_k, include_rgb=False, output_k=gt_k)
  with torch.no_grad():
    feats = torch.cat([net(b[0].to(dev()), kmeans_use_features=True)[0].float() for b in loader]).cpu().numpy()
  C0 = feats[[int(np.nonzero(targets == c)[0][0]) for c in range(gt_k)]]
  want = kc.lloyd64(feats, C0)
  preds, _ = kmeans.get_data_kmeans_on_features(config, net, loader, False, kmeans=kmeans.KMeans(gt_k, init=C0))
  S, E = kc.score_bounds(feats, want["centres"])
  assert not kc.ambiguity(S, E)[0].any()      # a condition on the features: the comparison below is then exact
  assert np.array_equal(preds.cpu().numpy(), want["labels"])


# ---- NMI / ARI on device tensors -----------------------------------------------------------------------------------------------
def test_nmi_ari_on_device_tensors():
  from iic_amd import eval_metrics
  rng = np.random.RandomState(3)
  t = rng.randint(0, 7, 5000)
  p = np.where(rng.random_sample(5000) < 0.6, (t + 2) % 7, rng.randint(0, 9, 5000))
  counts = np.zeros((p.max() + 1, t.max() + 1), dtype=np.int64)
  np.add.at(counts, (p, t), 1)
  nmi, ari = eval_metrics.nmi_ari_from_counts(counts)
  assert 0.0 < nmi < 1.0 and 0.0 < ari < 1.0
  assert eval_metrics._nmi(_g(p.astype(np.int32)), _g(t.astype(np.int32))) == nmi
  assert eval_metrics._ari(_g(p.astype(np.int32)), _g(t.astype(np.int32))) == ari
