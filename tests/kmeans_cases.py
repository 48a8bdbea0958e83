"""Cases, float64 oracle, bounds and the ambiguity computation shared by tests/test_kmeans_cpu.py and
tests/test_gpu_kmeans.py (a helper module, not a test file).

The kernel assigns with the score form  score_ij = ||c_j||^2 - 2 x_i.c_j  in fp32.  With u = 2^-24 the bounds are derived,
not measured:
  |score32 - score64| <= e_ij = (d + 2) u (||c_j||^2 + 2 sum_t |x_it c_jt|)      (d products and additions per sum, one more
                                                                                  rounding for the scale and the add)
  a cluster sum of m rows is within (m + 2) u sum |x| per coordinate
  mind_i is within e_i,label + (d + 2) u ||x_i||^2
A row is AMBIGUOUS when the float64 gap between its best and second-best score is <= the sum of their two e: fp32 may
then legitimately pick either; its in-bound candidates are the j whose score64 - e reaches below the best's score64 + e.
"""
import numpy as np

U = 2.0 ** -24
AMBIGUOUS_CAP = 0.01      # a condition on the INPUTS of every random case, asserted on the float64 reference alone

# exact tier: (n, d, k) on the integer lattice {-1, 0, 1}; LDX_CASE reads a [n, d] view of a [n, d + 5] matrix
LATTICE_SHAPES = [(1, 1, 1), (7, 3, 7), (193, 17, 2), (257, 511, 10), (300, 512, 16), (300, 513, 17), (129, 4608, 10),
                  (37, 32768, 3), (2000, 64, 65), (500, 32, 256), (70001, 16, 27)]
LDX_CASE = (300, 64, 10)
LDX_PAD = 5

# float64 tier: (n, d, k, how the centroids are made)
RANDOM_CASES = [(2000, 512, 10, "rows"), (1500, 513, 33, "rows"), (4000, 64, 64, "rows"), (3000, 17, 27, "rows"),
                (300, 4608, 10, "update")]
FIT_CASES = [(600, 512, 10), (400, 4608, 10)]


def blobs(n, d, k, seed, sep=4.0):
  """n points with unit Gaussian noise around k centres drawn as sep / sqrt(2) * N(0, 1) per coordinate (two centres
  differ by sep * N(0, 1) per coordinate): float32 [n, d] and the blob of every point, int [n]."""
  rng = np.random.RandomState(seed)
  centres = rng.standard_normal((k, d)) * sep / np.sqrt(2.0)
  which = rng.randint(0, k, n)
  which[:k] = np.arange(k)      # every blob has a point
  X = centres[which] + rng.standard_normal((n, d))
  return X.astype(np.float32), which


def random_case(case, seed=0):
  """X float32 [n, d] and centroids float32 [k, d] of a float64-tier case."""
  n, d, k, how = case
  X, _ = blobs(n, d, k, seed + 17 * d + k, sep=1.0)
  rng = np.random.RandomState(seed + 1)
  C = X[rng.choice(n, k, replace=False)].astype(np.float64)
  if how == "update":      # one float64 Lloyd update: data rows as centroids are ambiguous for 6-36 % of rows at d >= 4608
    labels, _ = assign64(X, C)
    sums, counts = accumulate64(X, labels, k)
    C = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], C)
  return X, C.astype(np.float32)


def lattice_case(shape, seed=0):
  """X, C float32 with values in {-1, 0, 1}: every score and every sum is an integer below 2^24 (asserted by
  lattice_preconditions), so fp32 arithmetic is exact in any order and the comparison needs no tolerance."""
  n, d, k = shape
  rng = np.random.RandomState(seed + n + d + k)
  density = min(0.5, 2000.0 / d)
  def draw(rows):
    u = rng.random_sample((rows, d))
    return np.where(u < 0.5 * density, -1.0, np.where(u < density, 1.0, 0.0)).astype(np.float32)
  return draw(n), draw(k)


def lattice_preconditions(X, C, labels, sums):
  X64, C64 = X.astype(np.float64), C.astype(np.float64)
  bound = (C64 * C64).sum(1).max() + 2 * (np.abs(X64) @ np.abs(C64).T).max() + (X64 * X64).sum(1).max()
  assert bound < 2 ** 24, bound
  m = np.zeros(C.shape, dtype=np.float64)
  np.add.at(m, labels, np.abs(X64))
  assert m.max() < 2 ** 24 and np.abs(sums).max() < 2 ** 24


def empty_cluster_case():
  """X and four initial centres of which the last attracts no point: the first iteration relocates it."""
  X, _ = blobs(200, 8, 3, seed=3, sep=8.0)
  return X, np.concatenate([X[:3].astype(np.float64), np.full((1, 8), 1e3)]).astype(np.float32)


# ---- the float64 oracle -------------------------------------------------------------------------------------------------
def scores64(X, C):
  X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
  return (C * C).sum(1)[None, :] - 2.0 * (X @ C.T)


def assign64(X, C):
  """labels (ties to the lowest j: np.argmin takes the first minimum) and mind = max(0, ||x||^2 + score)."""
  X = np.asarray(X, dtype=np.float64)
  S = scores64(X, C)
  labels = np.argmin(S, axis=1)
  mind = np.maximum(0.0, (X * X).sum(1) + S[np.arange(X.shape[0]), labels])
  return labels, mind


def accumulate64(X, labels, k):
  X = np.asarray(X, dtype=np.float64)
  sums = np.zeros((k, X.shape[1]), dtype=np.float64)
  np.add.at(sums, labels, X)
  return sums, np.bincount(labels, minlength=k).astype(np.int64)


def relocate64(X, C, labels, sums, counts):
  """Empty clusters, in index order, take the points farthest from their assigned centre (ties to the lowest index);
  the points leave their old clusters.  In place; returns the relocated row indices."""
  X = np.asarray(X, dtype=np.float64)
  empty = np.nonzero(counts == 0)[0]
  if empty.size == 0:
    return []
  dist = ((X - C[labels]) ** 2).sum(1)
  far = np.argsort(-dist, kind="stable")[:empty.size]
  for e, i in zip(empty, far):
    old = labels[i]
    sums[old] -= X[i]
    sums[e] = X[i]
    counts[old] -= 1
    counts[e] = 1
  return list(far)


def lloyd64(X, C0, max_iter=300, tol=1e-4):
  """scikit-learn's Lloyd loop in float64: dict(centres, labels, inertia, n_iter, relocations)."""
  X = np.asarray(X, dtype=np.float64)
  C = np.asarray(C0, dtype=np.float64).copy()
  k = C.shape[0]
  tol_s = tol * np.mean(np.var(X, axis=0))
  old, strict, reloc = None, False, 0
  for it in range(max_iter):
    labels, _ = assign64(X, C)
    sums, counts = accumulate64(X, labels, k)
    reloc += len(relocate64(X, C, labels, sums, counts))
    Cn = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], C)
    shift = ((Cn - C) ** 2).sum()
    C = Cn
    if old is not None and np.array_equal(labels, old):
      strict = True
      break
    if shift <= tol_s:
      break
    old = labels
  if not strict:
    labels, _ = assign64(X, C)
  inertia = float(((X - C[labels]) ** 2).sum())
  return dict(centres=C, labels=labels, inertia=inertia, n_iter=it + 1, relocations=reloc)


# ---- bounds ---------------------------------------------------------------------------------------------------------------
def score_bounds(X, C):
  """(score64 [n, k], e [n, k])."""
  X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
  d = X.shape[1]
  e = (d + 2) * U * ((C * C).sum(1)[None, :] + 2.0 * (np.abs(X) @ np.abs(C).T))
  return scores64(X, C), e


def ambiguity(S, E):
  """(ambiguous [n] bool, allowed [n, k] bool): allowed[i, j] says label j is an in-bound candidate of row i (for an
  unambiguous row that is the float64 arg-min alone)."""
  n, k = S.shape
  best = np.argmin(S, axis=1)
  rows = np.arange(n)
  ceiling = S[rows, best] + E[rows, best]
  if k == 1:
    return np.zeros(n, dtype=bool), np.ones((n, 1), dtype=bool)
  S2 = S.copy()
  S2[rows, best] = np.inf
  second = np.argmin(S2, axis=1)
  amb = (S[rows, second] - S[rows, best]) <= (E[rows, best] + E[rows, second])
  allowed = (S - E) <= ceiling[:, None]
  allowed[~amb] = False
  allowed[rows, best] = True
  return amb, allowed


def sum_bound(X, labels, k):
  """[k, d]: (m + 2) u sum |x| of every cluster's rows, m its count."""
  X = np.asarray(X, dtype=np.float64)
  mag = np.zeros((k, X.shape[1]), dtype=np.float64)
  np.add.at(mag, labels, np.abs(X))
  m = np.bincount(labels, minlength=k)
  return (m[:, None] + 2) * U * mag


def mind_bound(X, E, labels):
  X = np.asarray(X, dtype=np.float64)
  return E[np.arange(X.shape[0]), labels] + (X.shape[1] + 2) * U * (X * X).sum(1)


def scores32(X, C):
  """numpy fp32 emulation of the kernel's score form (fp32 products and sums, in BLAS's order)."""
  X, C = np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32)
  cn = (C * C).sum(1, dtype=np.float32)
  return cn[None, :] - np.float32(2.0) * (X @ C.T)


# ---- seeding ----------------------------------------------------------------------------------------------------------------
def seed_dist64(X, idx):
  X = np.asarray(X, dtype=np.float64)
  return ((X[:, None, :] - X[None, np.atleast_1d(idx), :]) ** 2).sum(2)      # [n, ncand]


def seed_potential_bound(X, idx):
  """[ncand]: sum_i (d + 2) u ||x_i - x_cand||^2 -- each fp32 distance is a d-term sum of squares of rounded differences
  (relative error (d + 2) u), min(., mind) does not widen it, the float64 sum adds nothing at this size."""
  d = np.asarray(X).shape[1]
  return (d + 2) * U * seed_dist64(X, idx).sum(0)


def kmeanspp64(X, k, seed):
  """Greedy k-means++ in float64 with the package's use of the random stream: chosen row indices."""
  X = np.asarray(X, dtype=np.float64)
  n = X.shape[0]
  rng = np.random.RandomState(seed)
  trials = 2 + int(np.log(k))
  chosen = [int(rng.randint(n))]
  mind = seed_dist64(X, chosen[0])[:, 0]
  pot = mind.sum()
  for _ in range(1, k):
    u = rng.uniform(size=trials)
    cand = np.minimum(np.searchsorted(np.cumsum(mind), u * pot), n - 1)
    dist = np.minimum(mind[:, None], seed_dist64(X, cand))
    best = int(np.argmin(dist.sum(0)))
    chosen.append(int(cand[best]))
    mind = dist[:, best]
    pot = mind.sum()
  return chosen


SEED_BLOBS = dict(n=400, d=64, k=8, data_seed=5, sep=12.0)
SEEDS_ONE_PER_BLOB = (0, 1, 2)      # asserted on the float64 emulation by tests/test_kmeans_cpu.py
