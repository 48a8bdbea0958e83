"""k-means without a GPU: the float64 oracle against scikit-learn, NMI / ARI against sklearn.metrics, the condition on the
random cases (ambiguity cap), the bounds against a numpy fp32 emulation and against seeded defects, the library's
host-side queries and the argument checks that must fire before any launch."""
import numpy as np
import pytest
import torch

from tests import kmeans_cases as kc


# ---- the oracle is scikit-learn's Lloyd -------------------------------------------------------------------------------------
def _sk_fit(X, C0, tol):
  cluster = pytest.importorskip("sklearn.cluster")
  km = cluster.KMeans(n_clusters=C0.shape[0], init=C0.astype(np.float64), n_init=1, algorithm="lloyd", tol=tol)
  return km.fit(X.astype(np.float64))


@pytest.mark.parametrize("name", ["separated", "overlapping_tol0", "empty_cluster"])
def test_oracle_equals_sklearn_lloyd(name):
  if name == "separated":
    X, _ = kc.blobs(500, 16, 5, seed=1, sep=8.0)
    C0, tol = X[[3, 77, 140, 300, 451]].astype(np.float64), 1e-4
  elif name == "overlapping_tol0":
    X, _ = kc.blobs(600, 6, 7, seed=2, sep=1.0)
    C0, tol = X[np.random.RandomState(0).choice(600, 7, replace=False)].astype(np.float64), 0.0
  else:
    (X, C0), tol = kc.empty_cluster_case(), 1e-4
  sk = _sk_fit(X, C0, tol)
  got = kc.lloyd64(X, C0, tol=tol)
  if name == "empty_cluster":
    assert got["relocations"] >= 1
  assert got["n_iter"] == sk.n_iter_
  assert np.array_equal(got["labels"], sk.labels_)
  assert np.abs(got["centres"] - sk.cluster_centers_).max() <= 1e-10
  assert abs(got["inertia"] - sk.inertia_) <= 1e-9 * max(1.0, sk.inertia_)


# ---- NMI / ARI -----------------------------------------------------------------------------------------------------------------
def _count_matrix(p, t):
  c = np.zeros((p.max() + 1, t.max() + 1), dtype=np.int64)
  np.add.at(c, (p, t), 1)
  return c


@pytest.mark.parametrize("name", ["random", "perfect", "single", "single_vs_many", "permuted"])
def test_nmi_ari_equal_sklearn(name):
  metrics = pytest.importorskip("sklearn.metrics")
  from iic_amd.eval_metrics import nmi_ari_from_counts
  rng = np.random.RandomState(4)
  t = rng.randint(0, 6, 500)
  p = {"random": rng.randint(0, 9, 500), "perfect": t.copy(), "single": np.zeros(500, dtype=np.int64),
       "single_vs_many": np.zeros(500, dtype=np.int64), "permuted": (t * 5 + 1) % 6}[name]
  if name == "single":
    t = np.zeros(500, dtype=np.int64)
  nmi, ari = nmi_ari_from_counts(_count_matrix(p, t))
  assert abs(nmi - metrics.normalized_mutual_info_score(t, p)) <= 1e-12
  assert abs(ari - metrics.adjusted_rand_score(t, p)) <= 1e-12


# ---- the random cases satisfy their condition; the bounds hold for fp32 and catch defects ----------------------------------
@pytest.fixture(scope="module", params=kc.RANDOM_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def rcase(request):
  X, C = kc.random_case(request.param)
  S, E = kc.score_bounds(X, C)
  return X, C, S, E


def test_ambiguity_cap(rcase):
  X, C, S, E = rcase
  amb, allowed = kc.ambiguity(S, E)
  print("ambiguous share %.4f" % amb.mean())
  assert amb.mean() <= kc.AMBIGUOUS_CAP
  assert (allowed.sum(1) >= 1).all() and (allowed[~amb].sum(1) == 1).all()


def test_fp32_emulation_inside_bounds(rcase):
  X, C, S, E = rcase
  S32 = kc.scores32(X, C).astype(np.float64)
  assert (np.abs(S32 - S) <= E).all(), float((np.abs(S32 - S) / E).max())
  amb, allowed = kc.ambiguity(S, E)
  lab32 = np.argmin(S32, axis=1)
  assert allowed[np.arange(X.shape[0]), lab32].all()
  # sums and mind of the emulation's labels
  sums32 = np.zeros(C.shape, dtype=np.float32)
  for j in range(C.shape[0]):
    sums32[j] = X[lab32 == j].sum(0, dtype=np.float32)
  sums64, _ = kc.accumulate64(X, lab32, C.shape[0])
  assert (np.abs(sums32 - sums64) <= kc.sum_bound(X, lab32, C.shape[0])).all()
  xn32 = (X * X).sum(1, dtype=np.float32)
  mind32 = np.maximum(np.float32(0), xn32 + S32[np.arange(X.shape[0]), lab32].astype(np.float32))
  X64 = X.astype(np.float64)
  mind64 = np.maximum(0.0, (X64 * X64).sum(1) + S[np.arange(X.shape[0]), lab32])
  assert (np.abs(mind32 - mind64) <= kc.mind_bound(X, E, lab32)).all()


def test_seeded_defects_fall_outside(rcase):
  X, C, S, E = rcase
  dropped = kc.scores64(X[:, :-1], C[:, :-1])      # a dropped feature
  assert (np.abs(dropped - S) > E).any()
  if C.shape[0] > 1:      # the norm of the neighbouring centroid
    C64 = C.astype(np.float64)
    wrong = S - (C64 * C64).sum(1)[None, :] + np.roll((C64 * C64).sum(1), 1)[None, :]
    assert (np.abs(wrong - S) > E).any()


def test_highest_index_tie_break_shows_on_the_lattice():
  X, C = kc.lattice_case((257, 511, 10))
  C[7] = C[2]      # an exact tie wherever either is the arg-min
  S = kc.scores64(X, C)
  low = np.argmin(S, axis=1)
  high = S.shape[1] - 1 - np.argmin(S[:, ::-1], axis=1)
  assert (low != high).any()
  labels, _ = kc.assign64(X, C)
  assert np.array_equal(labels, low)


def test_lattice_cases_meet_their_preconditions():
  for shape in kc.LATTICE_SHAPES + [kc.LDX_CASE]:
    X, C = kc.lattice_case(shape)
    labels, _ = kc.assign64(X, C)
    sums, _ = kc.accumulate64(X, labels, shape[2])
    kc.lattice_preconditions(X, C, labels, sums)


def test_seeds_pick_one_centre_per_blob_in_float64():
  sb = kc.SEED_BLOBS
  X, which = kc.blobs(sb["n"], sb["d"], sb["k"], sb["data_seed"], sep=sb["sep"])
  for seed in kc.SEEDS_ONE_PER_BLOB:
    chosen = kc.kmeanspp64(X, sb["k"], seed)
    assert sorted(which[chosen]) == list(range(sb["k"])), (seed, which[chosen])


# ---- host-side queries and refusals, no GPU ------------------------------------------------------------------------------------
def test_host_queries_answer_the_documented_range():
  from iic_amd import kmeans
  for n, d, k in [(1, 1, 1), (13000, 512, 10), (70000, 4608, 10), (2 ** 31 - 1, 32768, 256), (500, 32, 256)]:
    assert kmeans.supported(n, d, k)
    assert kmeans.workspace_bytes(n, d, k) > 0
  for n, d, k in [(0, 4, 2), (2 ** 31, 4, 2), (10, 0, 2), (10, 32769, 2), (10, 4, 0), (10, 4, 257)]:
    assert not kmeans.supported(n, d, k)
    assert kmeans.workspace_bytes(n, d, k) == 0
  # the workspace holds one [k][d] partial per workgroup of at most 4096 rows, and no more than ~1/8 of X beyond a floor
  assert kmeans.workspace_bytes(1000000, 512, 27) <= 1000000 * 512 * 4 // 8 + (1 << 22)


def test_every_value_error_fires_before_a_launch(monkeypatch):
  from iic_amd import kmeans

  def no_launch(*a, **k):
    raise AssertionError("a launch was attempted")
  monkeypatch.setattr(kmeans, "_assign", no_launch)
  monkeypatch.setattr(kmeans, "_update", no_launch)
  monkeypatch.setattr(kmeans, "seed_potentials", no_launch)
  X = torch.zeros((20, 8))
  with pytest.raises(ValueError, match="no CPU fallback"):
    kmeans.KMeans(3).fit(X)
  with pytest.raises(ValueError, match="no CPU fallback"):
    kmeans.lloyd_step(X, torch.zeros((3, 8)))
  with pytest.raises(ValueError, match="float32"):
    kmeans.KMeans(3).fit(X.double())
  with pytest.raises(ValueError, match="inner stride"):
    kmeans.KMeans(3).fit(torch.zeros((8, 20)).t())
  with pytest.raises(ValueError, match="should be >= n_clusters"):
    kmeans.KMeans(21).fit(X)
  with pytest.raises(ValueError, match="served range"):
    kmeans.KMeans(257).fit(torch.zeros((300, 8)))
  with pytest.raises(ValueError, match="served range"):
    kmeans.KMeans(2).fit(torch.zeros((4, 32769)))
  with pytest.raises(ValueError, match="init has shape"):
    kmeans.KMeans(3, init=np.zeros((3, 7))).fit(X)
  with pytest.raises(ValueError):
    kmeans.KMeans(3, init="random")
  assert kmeans.KMeans(3, init=np.zeros((3, 8)), n_init=10).n_init == 1
