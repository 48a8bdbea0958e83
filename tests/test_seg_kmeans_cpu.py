"""Host side of the segmentation k-means evaluation (iic_amd/seg_kmeans.py, iic_amd.kmeans.MiniBatchKMeans): the
float64 restatements of tests/seg_kmeans_cases.py against scikit-learn's own functions, the sampling arithmetic against
the reference's lines evaluated literally, and the label bracket proved on a numpy fp32 emulation of the kernel's
operation order -- correct arithmetic inside it, seeded defects outside.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import seg_kmeans_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["iic_seg_kmeans_label_acc", "iic_seg_kmeans_label_lds_floats", "iic_seg_feat_sample",
               "iic_kmeans_minibatch_update"]


# ---- the mini-batch step and its bookkeeping against scikit-learn -----------------------------------------------------------
def _sk_step(Xb, C, w, rng, random_reassign, ratio=0.01):
  km = pytest.importorskip("sklearn.cluster._kmeans")
  centres_new = np.empty_like(C)
  w = w.copy()
  inertia = km._mini_batch_step(Xb, np.ones(Xb.shape[0]), C.copy(), centres_new, w, rng, random_reassign=random_reassign,
                                reassignment_ratio=ratio)
  return centres_new, w, inertia


@pytest.mark.parametrize("n,d,k", [(100, 512, 3), (64, 7, 27)])
def test_step64_equals_sklearn(n, d, k):
  X, _, _ = sc.blobs(n, d, k, seed=n + d, sep=4.0)
  X = X.astype(np.float64)
  rng = np.random.RandomState(0)
  C = X[rng.choice(n, k, replace=False)].copy()
  w = np.zeros(k)
  for step in range(3):      # the second and third steps carry non-zero weights
    Xb = X[rng.randint(0, n, 40)]
    want_C, want_w, want_inertia = _sk_step(Xb, C, w, np.random.RandomState(1), False)
    got_C, got_w, got_inertia, to = sc.mini_batch_step64(Xb, C, w)
    assert not to.any()
    assert np.array_equal(got_w, want_w)
    np.testing.assert_allclose(got_C, want_C, rtol=1e-12, atol=1e-13)
    assert abs(got_inertia - want_inertia) <= 1e-10 * want_inertia
    C, w = got_C, got_w


def test_step64_reassignment_equals_sklearn():
  n, d, k = 60, 7, 5
  X, _, _ = sc.blobs(n, d, k, seed=5, sep=5.0)
  X = X.astype(np.float64)
  C = np.concatenate([X[:4], np.full((1, d), 1e3)])      # the last centre attracts nothing
  w = np.array([400.0, 300.0, 3.0, 350.0, 0.0])          # ... so its weight stays 0, under 1 % of the heaviest
  Xb = X[10:50]
  want_C, want_w, want_inertia = _sk_step(Xb, C, w, np.random.RandomState(7), True)
  got_C, got_w, got_inertia, to = sc.mini_batch_step64(
    Xb, C, w, random_reassign=True, choice=lambda nb, size: np.random.RandomState(7).choice(nb, replace=False, size=size))
  assert to[4] and not to[[0, 1, 3]].any()      # the reassignment test really fires
  assert np.array_equal(got_w, want_w)
  np.testing.assert_allclose(got_C, want_C, rtol=1e-12, atol=1e-13)
  assert abs(got_inertia - want_inertia) <= 1e-10 * want_inertia
  # with the ratio at 0 nothing is reassigned, whatever the weights
  _, w0, _, to0 = sc.mini_batch_step64(Xb, C, w, random_reassign=True, reassignment_ratio=0.0)
  assert not to0.any() and w0[4] == 0.0


def test_convergence_bookkeeping_equals_sklearn():
  cl = pytest.importorskip("sklearn.cluster")
  n, batch, k = 1000, 100, 3
  rng = np.random.RandomState(2)
  falling = list(5000.0 / (1 + np.arange(12)))
  plateau = list(400.0 + 20.0 * rng.random_sample(120))      # long enough for the smoothed inertia to stop falling
  for max_ni, seq in [(10, falling + plateau), (3, falling + plateau), (None, falling + plateau[:8])]:
    sk = cl.MiniBatchKMeans(n_clusters=k, batch_size=batch, max_no_improvement=max_ni)
    sk._batch_size, sk._tol = batch, 0.0
    sk._ewa_inertia = sk._ewa_inertia_min = None
    sk._no_improvement = 0
    mine = sc.Schedule64(k, batch, n, max_ni)
    stopped = None
    for step, inertia in enumerate(seq):
      a = sk._mini_batch_convergence(step, len(seq), n, 0, inertia)
      b = mine.converged(step, 0.0, inertia)
      assert a == b, step
      assert mine.ewa == sk._ewa_inertia and mine.ewa_min == sk._ewa_inertia_min
      assert mine.no_improvement == sk._no_improvement
      if a:
        stopped = step
        break
    assert (stopped is None) == (max_ni is None)
  # the tolerance branch returns before the minimum is touched
  sk = cl.MiniBatchKMeans(n_clusters=k, batch_size=batch)
  sk._batch_size, sk._tol = batch, 1e-3
  sk._ewa_inertia = sk._ewa_inertia_min = None
  sk._no_improvement = 0
  mine = sc.Schedule64(k, batch, n, 10, tol=1e-3)
  for step, (shift, inertia) in enumerate([(1.0, 900.0), (0.5, 800.0), (1e-4, 700.0)]):
    assert sk._mini_batch_convergence(step, 3, n, shift, inertia) == mine.converged(step, shift, inertia) == (step == 2)
  assert mine.ewa_min == sk._ewa_inertia_min


def test_reassignment_schedule_equals_sklearn():
  cl = pytest.importorskip("sklearn.cluster")
  for k, batch in [(3, 100), (27, 100), (27, 64)]:
    sk = cl.MiniBatchKMeans(n_clusters=k, batch_size=batch)
    sk._batch_size, sk._n_since_last_reassign = batch, 0
    mine = sc.Schedule64(k, batch, 1000)
    for step in range(12):
      w = np.ones(k)
      if step in (0, 7):
        w[k // 2] = 0.0
      sk._counts = w
      assert sk._random_reassign() == mine.random_reassign(w)
      assert sk._n_since_last_reassign == mine.n_since


# ---- sampling: the reference's lines, literally ---------------------------------------------------------------------------
def test_budget_and_sampling_against_the_reference_lines():
  from iic_amd import seg_kmeans
  for total, num_imgs in [(10000, 7), (100, 300), (5400, 5400), (1, 1)]:
    assert seg_kmeans.sample_budget(total, num_imgs) == sc.reference_budget(total, num_imgs)
  rng = np.random.RandomState(3)
  mask = rng.random_sample((3, 8, 8)) < 0.7
  x_out = rng.standard_normal((3, 5, 8, 8)).astype(np.float32)       # NCHW, as the net returns it
  masked = x_out.transpose((0, 2, 3, 1))[mask, :]                     # :64-66
  for per_img in (4, 1000):      # the budget binds / the unmasked count binds
    want_n, want_block = sc.reference_select(masked, 3, per_img, np.random.RandomState(11))
    n_sel, ordinals = seg_kmeans.sample_indices(int(mask.sum()), 3, per_img, "reference", np.random.RandomState(11))
    assert n_sel == want_n == min(int(mask.sum()), 3 * per_img) and ordinals.shape == (1,)
    coords = seg_kmeans.ordinals_to_coords(mask, ordinals)
    row = x_out[coords[0, 0], :, coords[0, 1], coords[0, 2]]
    assert np.array_equal(np.broadcast_to(row, want_block.shape), want_block)      # n_sel copies of one pixel
    n_uni, ordinals = seg_kmeans.sample_indices(int(mask.sum()), 3, per_img, "uniform", np.random.RandomState(11))
    assert n_uni == want_n and ordinals.shape == (n_uni,) and len(set(ordinals.tolist())) == n_uni
    assert ordinals.min() >= 0 and ordinals.max() < mask.sum()
    coords = seg_kmeans.ordinals_to_coords(mask, ordinals)
    assert np.array_equal(coords, np.argwhere(mask)[ordinals])
    assert mask[coords[:, 0], coords[:, 1], coords[:, 2]].all()
  if per_img == 1000:
    assert sorted(ordinals.tolist()) == list(range(int(mask.sum())))      # every unmasked pixel, once
  with pytest.raises(ValueError):
    seg_kmeans.sample_indices(10, 1, 5, "nearest")


# ---- the label bracket on the fp32 emulation ------------------------------------------------------------------------------
def _bracket(case, defect=None):
  X, C = sc.clustered_features(case["N"], case["Hl"], case["Wl"], case["C"], case["k"], case["seed"])
  S64 = sc.scores64(X, C, case["S"])
  gap = sc.under_gap(S64, sc.score_error(X, C))
  got = sc.labels32(X, C, case["S"], defect)
  return gap, got, np.argmin(S64, axis=-1)


@pytest.mark.parametrize("case", sc.BRACKET_CASES, ids=lambda c: "%dx%dx%d_k%d" % (c["Hl"], c["Wl"], c["S"], c["k"]))
def test_bracket_holds_correct_arithmetic_and_the_exclusion_cap(case):
  gap, got, want = _bracket(case)
  print("under the gap: %d of %d pixels" % (gap.sum(), gap.size))
  assert gap.mean() <= sc.GAP_CAP      # float64 alone: the inputs are clustered well enough
  assert (got[~gap] == want[~gap]).all()


@pytest.mark.parametrize("defect", ["neighbour", "cnorm", "align_corners"])
def test_bracket_rejects_seeded_defects(defect):
  gap, got, want = _bracket(sc.BRACKET_CASES[0], defect)
  wrong = (got != want) & ~gap
  print("%s: %d pixels off outside the gap" % (defect, wrong.sum()))
  assert wrong.any()


def test_lattice_with_dyadic_weights_is_exact_everywhere():
  c = sc.LATTICE_CASE
  assert c["S"] == 2 * c["Hl"] == 2 * c["Wl"]
  X, C = sc.lattice_features(c["N"], c["Hl"], c["Wl"], c["C"], c["k"], c["seed"])
  S64 = sc.scores64(X, C, c["S"])
  assert np.array_equal(S64 * 16, np.round(S64 * 16)) and np.abs(S64).max() < 2 ** 12      # exact in fp32 in any order
  assert (np.partition(S64, 1, axis=-1)[..., 0] == np.partition(S64, 1, axis=-1)[..., 1]).any()      # real ties
  assert np.array_equal(sc.labels32(X, C, c["S"]), np.argmin(S64, axis=-1))      # no pixel left out


def test_rule_argmin_nan_and_ties():
  s = np.array([[np.nan, 2.0, 2.0], [np.nan, np.nan, np.nan], [np.nan, np.inf, 1.0], [3.0, 3.0, np.nan]])
  assert sc.rule_argmin(s).tolist() == [1, 0, 2, 0]


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_header_binding_and_docs_name_the_new_entry_points():
  from iic_amd import _lib
  header = open(os.path.join(ROOT, "include", "iic_hip.h")).read()
  for name in NEW_SYMBOLS:
    assert name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"\b(?:int|long)\s+%s\s*\(" % name, header)
  assert "kmeans_segmentation_eval.py:" in header      # every entry cites the reference lines it replaces
  src = open(os.path.join(ROOT, "iic_amd", "csrc", "seg_kmeans.hip")).read()
  assert "atomicAdd(float" not in src.replace(" ", "") and "unsafeAtomicAdd" not in src      # integer atomics only
  assert "seg_kmeans.hip" in open(os.path.join(ROOT, "iic_amd", "csrc", "Makefile")).read()
  assert "## 5i. Segmentation k-means evaluation" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_feature_net_refuses_the_unbuilt_heads_and_loader_filters_keys():
  import types

  import torch
  from iic_amd.archs import seg
  cfg = types.SimpleNamespace(in_channels=3, input_sz=24, batchnorm_track=True)
  net = seg.SegmentationNet10aFeatures(cfg)
  assert net.features_sz == 512
  with pytest.raises(NotImplementedError, match="not built"):
    net(torch.zeros(1, 3, 24, 24))
  src = seg.SegmentationNet10aFeatures(cfg)
  sd = dict(src.state_dict())
  sd["isola_head.layers.0.weight"] = torch.zeros(3)
  seg.load_trunk_state_dict(net, sd)
  for key, val in src.state_dict().items():
    assert torch.equal(net.state_dict()[key], val)
  iic = {"module.trunk." + key[len("features."):]: val for key, val in src.state_dict().items()}
  iic["module.head_B.heads.0.0.weight"] = torch.zeros(3)
  seg.load_trunk_state_dict(net, iic)
  with pytest.raises(ValueError, match="unexpected key"):
    seg.load_trunk_state_dict(net, dict(sd, **{"classifier.weight": torch.zeros(1)}))
