"""k-means on a net's pre-head features, on the device -- opt-in twin of the reference's host-side fit.

The reference copies the features off the GPU batch by batch and runs ``KMeans(n_clusters=config.gt_k).fit`` of
scikit-learn on the host (code/utils/cluster/baselines/triplets.py:134-173; ``triplets_eval`` :176-228 matches and scores
the labels).  Here the features stay where the net wrote them: a Lloyd iteration is one launch chain of csrc/kmeans.hip over
them, the k-means++ potentials come from the same file, and only the 64-byte state block crosses to the host, once per
``check_every`` iterations.

``KMeans`` follows scikit-learn's Lloyd: tolerance scaled by the mean per-feature variance, strict convergence when no
label changes, a final assignment so that ``labels_`` match ``cluster_centers_``, the best of ``n_init`` runs by inertia,
empty clusters relocated to the points farthest from their centre.  Distances are fp32 in the score form
||c||^2 - 2 x.c (exact-fp32 MFMA dot products); every sum has a fixed order, so two fits give the same bits.

``MiniBatchKMeans`` is scikit-learn's mini-batch algorithm on the same assignment kernel, with the centre update, the
reassignment schedule and the early-stopping bookkeeping of csrc/seg_kmeans.hip; the reference fits it on sampled pixel
features (code/utils/segmentation/baselines/kmeans_segmentation_eval.py:104; iic_amd/seg_kmeans.py).

``install()`` does not rebind anything to this module; a script opts in -- INTEGRATION.md sections 5g and 5i.
"""
import math

import numpy as np
import torch

from . import eval_metrics
from ._lib import check, lib, ptr, stream_ptr

__all__ = ["KMeans", "MiniBatchKMeans", "lloyd_step", "seed_potentials", "supported", "workspace_bytes",
           "get_data_kmeans_on_features", "kmeans_eval"]
F32 = torch.float32
MAX_K, MAX_D = 256, 32768
STATE_BYTES = 64
MB_STATE_BYTES = 128      # csrc/seg_kmeans.hip mb_state: 10 int32, then 8 float64 from byte 40


def supported(n, d, k):
  """Whether the kernels serve (n, d, k): 1 <= k <= 256, 1 <= d <= 32768, 1 <= n < 2^31.  Host only."""
  return bool(lib().iic_kmeans_supported(int(n), int(d), int(k)))


def workspace_bytes(n, d, k):
  """Bytes of scratch the launches for (n, d, k) need (the seeding calls use the k = 1 layout).  Host only."""
  L = lib()
  own = int(L.iic_kmeans_workspace_bytes(int(n), int(d), int(k)))
  return max(own, int(L.iic_kmeans_workspace_bytes(int(n), int(d), 1))) if own else 0


def _check_X(X, what="X", need_device=True):
  """Everything the kernels cannot know about X; raises ValueError before anything is enqueued.  The device check comes
  last (need_device=False leaves it to the caller, who has further host-side checks to make first)."""
  if not torch.is_tensor(X):
    raise ValueError("kmeans (HIP): %s must be a torch tensor on the device, got %s" % (what, type(X).__name__))
  if X.dtype != F32:
    raise ValueError("kmeans (HIP): %s must be float32, got %s" % (what, X.dtype))
  if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
    raise ValueError("kmeans (HIP): %s must be [n, d] with n, d >= 1, got %s" % (what, tuple(X.shape)))
  if X.shape[1] > 1 and X.stride(1) != 1:
    raise ValueError("kmeans (HIP): the inner stride of %s must be 1, got %d" % (what, X.stride(1)))
  if X.shape[0] > 1 and X.stride(0) < X.shape[1]:
    raise ValueError("kmeans (HIP): the row stride of %s (%d) is below d = %d" % (what, X.stride(0), X.shape[1]))
  if need_device and not X.is_cuda:
    raise ValueError("kmeans (HIP): %s is a CPU tensor -- there is no CPU fallback" % what)
  return X.shape[0], X.shape[1], (X.stride(0) if X.shape[0] > 1 else X.shape[1])


def _check_shape(n, d, k):
  if not (1 <= k <= MAX_K and 1 <= d <= MAX_D and 1 <= n < 2 ** 31) or not supported(n, d, k):
    raise ValueError("kmeans (HIP): (n, d, k) = (%d, %d, %d) is outside the served range 1 <= k <= %d, 1 <= d <= %d, "
                     "1 <= n < 2^31" % (n, d, k, MAX_K, MAX_D))


def _check_C(C, d):
  if not (torch.is_tensor(C) and C.is_cuda and C.dtype == F32 and C.dim() == 2 and C.shape[1] == d and C.is_contiguous()):
    raise ValueError("kmeans (HIP): centres must be a contiguous float32 [k, %d] device tensor" % d)
  return C.shape[0]


class _Buffers(object):
  """Outputs and scratch of the launches for one (X, k)."""

  def __init__(self, X, k, with_sums=True):
    n, d, _ = _check_X(X)
    _check_shape(n, d, k)
    dev = X.device
    self.n, self.d, self.k = n, d, k
    self.labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    self.mind = torch.empty((n,), dtype=F32, device=dev)
    self.sums = torch.empty((k, d), dtype=F32, device=dev) if with_sums else None
    self.counts = torch.empty((k,), dtype=torch.long, device=dev) if with_sums else None
    self.inertia = torch.zeros((1,), dtype=torch.float64, device=dev)
    self.ws = torch.empty((workspace_bytes(n, d, k),), dtype=torch.uint8, device=dev)


def _assign(X, C, buf, state=None, with_sums=True, inertia=False):
  n, d, ldx = _check_X(X)
  check(lib().iic_kmeans_assign(ptr(X), ldx, ptr(C), n, d, buf.k, ptr(buf.labels), ptr(buf.mind),
                                ptr(buf.sums) if with_sums else None, ptr(buf.counts) if with_sums else None,
                                ptr(buf.inertia) if inertia else None, ptr(buf.ws), ptr(state), stream_ptr()),
        "iic_kmeans_assign")


def _update(C, buf, state, force=0):
  check(lib().iic_kmeans_update(ptr(C), ptr(buf.sums), ptr(buf.counts), buf.n, buf.d, buf.k, int(force), ptr(buf.ws),
                                ptr(state), stream_ptr()), "iic_kmeans_update")


def lloyd_step(X, C):
  """One assignment + accumulation of X [n, d] against the centres C [k, d]: (labels int32 [n], sums fp32 [k, d],
  counts int64 [k], mind fp32 [n]).  labels_i = arg-min_j ||c_j||^2 - 2 x_i.c_j with ties to the lowest j."""
  _, d, _ = _check_X(X)
  k = _check_C(C, d)
  buf = _Buffers(X, k)
  _assign(X, C, buf)
  return buf.labels, buf.sums, buf.counts, buf.mind


def seed_potentials(X, cand, mind, write=False, ws=None):
  """float64 [len(cand)] device tensor: sum_i min(mind_i, ||x_i - x_cand||^2) per candidate row index (int64 device
  tensor, at most 8).  write=True (one candidate): mind <- min(mind, distance to it) as well."""
  n, d, ldx = _check_X(X)
  _check_shape(n, d, 1)
  if not (torch.is_tensor(cand) and cand.is_cuda and cand.dtype == torch.long and cand.dim() == 1 and
          1 <= cand.numel() <= 8 and cand.is_contiguous()):
    raise ValueError("kmeans (HIP): candidates must be 1 to 8 int64 row indices on the device")
  if write and cand.numel() != 1:
    raise ValueError("kmeans (HIP): write=True takes one candidate")
  if not (torch.is_tensor(mind) and mind.is_cuda and mind.dtype == F32 and mind.is_contiguous() and mind.numel() == n):
    raise ValueError("kmeans (HIP): mind must be %d contiguous float32 device values" % n)
  if ws is None:
    ws = torch.empty((workspace_bytes(n, d, 1),), dtype=torch.uint8, device=X.device)
  pot = torch.empty((cand.numel(),), dtype=torch.float64, device=X.device)
  check(lib().iic_kmeans_seed_potential(ptr(X), ldx, n, d, ptr(cand), cand.numel(), ptr(mind), int(bool(write)), ptr(pot),
                                        ptr(ws), stream_ptr()), "iic_kmeans_seed_potential")
  return pot


def kmeans_plusplus(X, k, rng, ws=None):
  """Greedy k-means++ (2 + int(log k) local trials) on the device: int64 [k] device tensor of the chosen row indices.
  The uniforms come from ``rng`` (a numpy RandomState) in scikit-learn's order -- randint(n), then one vector of trials
  per further centre -- but the draws cannot replay scikit-learn's stream: its distances are float64, ours fp32, so the
  cumulative sums the uniforms are searched in differ in the last bits and so, now and then, does a pick.  Nothing here
  waits for the device."""
  n, d, _ = _check_X(X)
  dev = X.device
  trials = 2 + int(math.log(k))
  if ws is None:
    ws = torch.empty((workspace_bytes(n, d, 1),), dtype=torch.uint8, device=dev)
  mind = torch.full((n,), float("inf"), dtype=F32, device=dev)
  chosen = torch.empty((k,), dtype=torch.long, device=dev)
  first = torch.tensor([int(rng.randint(n))], dtype=torch.long, device=dev)
  chosen[0:1] = first
  pot = seed_potentials(X, first, mind, write=True, ws=ws)      # mind = distance to the first centre
  for c in range(1, k):
    u = torch.from_numpy(rng.uniform(size=trials)).to(dev)
    cand = torch.searchsorted(torch.cumsum(mind.double(), 0), u * pot[0]).clamp_(max=n - 1)
    pots = seed_potentials(X, cand.contiguous(), mind, ws=ws)
    best = cand[torch.argmin(pots)].reshape(1)
    chosen[c:c + 1] = best
    pot = seed_potentials(X, best, mind, write=True, ws=ws)
  return chosen


def _relocate(X, buf):
  """scikit-learn's _relocate_empty_clusters_dense on the sums and counts of the current assignment: the empty clusters,
  in index order, take the points farthest from their assigned centre (ties to the lowest index), which leave their old
  clusters.  A rare path: a top-k and a few torch ops."""
  empty = torch.nonzero(buf.counts == 0).reshape(-1)
  ne = int(empty.numel())
  if ne == 0:
    return
  # farthest first, ties to the lowest index: a stable descending sort
  far = torch.sort(buf.mind, descending=True, stable=True).indices[:ne]
  for e in range(ne):
    i = far[e]
    old = buf.labels[i].long()
    x = X[i]
    buf.sums[old] -= x
    buf.sums[empty[e]] = x
    buf.counts[old] -= 1
    buf.counts[empty[e]] = 1


class KMeans(object):
  """scikit-learn's ``KMeans`` (Lloyd) for fp32 features resident on the device; the defaults are scikit-learn's, which
  the reference's ``KMeans(n_clusters=gt_k)`` implies.  ``init``: "k-means++" or a [k, d] array / tensor (n_init is
  then 1).  After ``fit``: ``cluster_centers_`` (device fp32 [k, d]), ``labels_`` (device int32 [n]), ``inertia_``,
  ``n_iter_``.  ``check_every`` Lloyd iterations are enqueued between two reads of the device's state block; a latch on
  the device makes the result identical to checking after every iteration.

  The k-means++ draws cannot replay scikit-learn's random stream for the same seed: scikit-learn's distances are
  float64 (see ``kmeans_plusplus``)."""

  def __init__(self, n_clusters, n_init=10, max_iter=300, tol=1e-4, init="k-means++", seed=0, check_every=8):
    if isinstance(init, str):
      if init != "k-means++":
        raise ValueError("kmeans (HIP): init must be 'k-means++' or a [k, d] array, got %r" % init)
    else:
      n_init = 1
    if n_clusters < 1 or n_init < 1 or max_iter < 1 or check_every < 1 or tol < 0:
      raise ValueError("kmeans (HIP): n_clusters, n_init, max_iter, check_every >= 1 and tol >= 0 required")
    self.n_clusters, self.n_init, self.max_iter, self.tol = int(n_clusters), int(n_init), int(max_iter), float(tol)
    self.init, self.seed, self.check_every = init, seed, int(check_every)

  def _init_centres(self, X, rng, buf):
    k, d = self.n_clusters, X.shape[1]
    if isinstance(self.init, str):
      return X[kmeans_plusplus(X, k, rng, ws=buf.ws)].contiguous()
    C = torch.as_tensor(self.init)
    if tuple(C.shape) != (k, d):
      raise ValueError("kmeans (HIP): init has shape %s, expected %s" % (tuple(C.shape), (k, d)))
    return C.to(device=X.device, dtype=F32).contiguous().clone()

  def _read(self, state):
    host = state.cpu()      # the one transfer of a chunk
    ints = host[:16].view(torch.int32)
    dbl = host[16:40].view(torch.float64)
    return dict(iter=int(ints[0]), converged=int(ints[1]), pause=int(ints[2]), shift=float(dbl[0]), inertia=float(dbl[1]))

  def _one_run(self, X, C, buf, tol_dev):
    dev = X.device
    state = torch.zeros((STATE_BYTES,), dtype=torch.uint8, device=dev)
    state[32:40].view(torch.float64).copy_(tol_dev.reshape(1))
    buf.labels.fill_(-1)
    st = dict(iter=0, converged=0, pause=0)
    while st["iter"] < self.max_iter and not st["converged"]:
      for _ in range(min(self.check_every, self.max_iter - st["iter"])):
        _assign(X, C, buf, state=state)
        _update(C, buf, state)
      st = self._read(state)
      if st["pause"]:
        _relocate(X, buf)
        state[8:12].view(torch.int32).zero_()
        _update(C, buf, state, force=1)
        st = self._read(state)
    if st["converged"] == 1:
      inertia = st["inertia"]      # no label moved: the centres are the ones the labels were assigned with
    else:
      _assign(X, C, buf, with_sums=False, inertia=True)
      inertia = float(buf.inertia.cpu()[0])
    return inertia, st["iter"]

  def fit(self, X):
    n, d, _ = _check_X(X, need_device=False)
    k = self.n_clusters
    if n < k:
      raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, k))
    _check_shape(n, d, k)
    if not isinstance(self.init, str) and tuple(torch.as_tensor(self.init).shape) != (k, d):
      raise ValueError("kmeans (HIP): init has shape %s, expected %s" % (tuple(torch.as_tensor(self.init).shape), (k, d)))
    _check_X(X)
    buf = _Buffers(X, k)
    # scikit-learn's _tolerance: tol * mean of the per-feature variances; stays on the device
    if n > 1:
      tol_dev = X.var(dim=0, unbiased=False).double().mean() * self.tol
    else:
      tol_dev = torch.zeros((), dtype=torch.float64, device=X.device)
    rng = np.random.RandomState(self.seed)
    best = None
    for _ in range(self.n_init):
      C = self._init_centres(X, rng, buf)
      inertia, n_iter = self._one_run(X, C, buf, tol_dev)
      if not math.isfinite(inertia):
        raise ValueError("non-finite features")
      if best is None or inertia < best[0]:
        best = (inertia, n_iter, C, buf.labels.clone())
    self.inertia_, self.n_iter_, self.cluster_centers_, self.labels_ = best
    return self

  def predict(self, X):
    _, d, _ = _check_X(X)
    C = self.cluster_centers_
    if d != C.shape[1]:
      raise ValueError("kmeans (HIP): X has %d features, the centres %d" % (d, C.shape[1]))
    buf = _Buffers(X, C.shape[0], with_sums=False)
    _assign(X, C, buf, with_sums=False)
    return buf.labels

  def fit_predict(self, X):
    return self.fit(X).labels_


class MiniBatchKMeans(object):
  """scikit-learn's ``MiniBatchKMeans`` for fp32 features resident on the device.  The defaults are those of the
  scikit-learn era the reference's bare ``MiniBatchKMeans(n_clusters=gt_k)`` implies (batch_size=100, n_init=3,
  max_iter=100, max_no_improvement=10, reassignment_ratio=0.01, tol=0.0) -- the choice ``KMeans`` made with n_init=10.

  The algorithm is sklearn/cluster/_kmeans.py's, step for step: a validation subset of ``init_size`` random rows,
  ``n_init`` initialisations (k-means++ on a fresh random subset each) of which the one with the lowest validation
  inertia is kept, ``n_steps = max_iter * n // batch_size`` steps on ``randint(0, n, batch_size)`` mini-batches drawn
  from a host ``RandomState``, the reassignment schedule of ``_random_reassign``, the early stopping of
  ``_mini_batch_convergence``, a final full assignment for ``labels_`` and ``inertia_``.  A step is a gather of the
  batch rows into a reused [batch, d] buffer, iic_kmeans_assign and iic_kmeans_minibatch_update; ``check_every`` steps
  are enqueued between two reads of the 128-byte state block, and the latch on the device makes the result identical to
  checking after every step (the host rewinds its RandomState to the paused step before it draws the reassignment).  The
  rare reassignment itself is a few torch ops on the host's side, as ``KMeans`` relocates empty clusters.

  The same caveat as ``KMeans``: the random stream of scikit-learn cannot be replayed -- its k-means++ distances are
  float64 (see ``kmeans_plusplus``).  ``batches``: an optional sequence of index arrays that replaces the random
  mini-batches (one step each).  After ``fit``: ``cluster_centers_``, ``labels_``, ``inertia_``, ``n_steps_``,
  ``n_iter_``, ``counts_`` (float64 [k] on the device), ``n_pauses_`` (steps that waited for a reassignment)."""

  def __init__(self, n_clusters, batch_size=100, max_iter=100, n_init=3, init_size=None, max_no_improvement=10,
               reassignment_ratio=0.01, tol=0.0, init="k-means++", seed=0, check_every=8):
    if isinstance(init, str):
      if init != "k-means++":
        raise ValueError("kmeans (HIP): init must be 'k-means++' or a [k, d] array, got %r" % init)
    else:
      n_init = 1
    if n_clusters < 1 or batch_size < 1 or n_init < 1 or max_iter < 1 or check_every < 1 or tol < 0:
      raise ValueError("kmeans (HIP): n_clusters, batch_size, n_init, max_iter, check_every >= 1 and tol >= 0 required")
    if reassignment_ratio < 0:
      raise ValueError("reassignment_ratio should be >= 0, got %r instead." % reassignment_ratio)
    self.n_clusters, self.batch_size, self.max_iter, self.n_init = int(n_clusters), int(batch_size), int(max_iter), int(n_init)
    self.init_size, self.max_no_improvement = init_size, max_no_improvement
    self.reassignment_ratio, self.tol = float(reassignment_ratio), float(tol)
    self.init, self.seed, self.check_every = init, seed, int(check_every)
    self._choice = None      # tests inject the reassignment picks: callable(n_rows, size) -> indices
    self._bufs = {}

  # ---- pieces -----------------------------------------------------------------------------------------------------------
  def _init_size_for(self, n, batch):
    k = self.n_clusters
    size = self.init_size
    if size is None:
      size = 3 * batch
      if size < k:
        size = 3 * k
    elif size < k:
      size = 3 * k
    return min(int(size), n)

  def _init_centroids(self, X, rng, init_size):
    """_BaseKMeans._init_centroids: a random subset of init_size rows (drawn even for an array init), then k-means++."""
    n, k = X.shape[0], self.n_clusters
    Xi = X
    if init_size is not None and init_size < n:
      Xi = X[torch.from_numpy(rng.randint(0, n, init_size)).to(X.device)]
    if isinstance(self.init, str):
      return Xi[kmeans_plusplus(Xi, k, rng)].contiguous()
    return torch.as_tensor(self.init).to(device=X.device, dtype=F32).contiguous().clone()

  def _buf(self, Xb):
    key = (Xb.shape[0], Xb.shape[1], Xb.device)
    if key not in self._bufs:
      self._bufs[key] = _Buffers(Xb, self.n_clusters)
    return self._bufs[key]

  def _new_state(self, dev, norm, alpha, tol, max_no_improvement):
    host = torch.zeros((MB_STATE_BYTES,), dtype=torch.uint8)
    ints, dbl = host[:40].view(torch.int32), host[40:104].view(torch.float64)
    ints[8] = 10 * self.n_clusters
    ints[9] = -1 if max_no_improvement is None else int(max_no_improvement)
    dbl[4], dbl[5], dbl[6], dbl[7] = tol, alpha, self.reassignment_ratio, norm
    return host.to(dev)

  @staticmethod
  def _read(state):
    host = state.cpu()      # the one transfer of a chunk
    ints, dbl = host[:40].view(torch.int32), host[40:104].view(torch.float64)
    return dict(step=int(ints[0]), converged=int(ints[1]), pause=int(ints[2]), n_since=int(ints[4]),
                no_improvement=int(ints[5]), inertia=float(dbl[0]), ewa=float(dbl[1]) if int(ints[6]) else None,
                ewa_min=float(dbl[2]) if int(ints[7]) else None, shift=float(dbl[3]))

  def _step(self, Xb, C, Cold, w, buf, state, resume=0):
    if not resume:
      _assign(Xb, C, buf, state=state)
    check(lib().iic_kmeans_minibatch_update(ptr(C), ptr(Cold), ptr(buf.sums), ptr(buf.counts), ptr(w), buf.n, buf.d,
                                            buf.k, int(resume), ptr(buf.ws), ptr(state), stream_ptr()),
          "iic_kmeans_minibatch_update")

  def _reassign(self, Xs, C, w, rng):
    """The tail of _mini_batch_step (sklearn/cluster/_kmeans.py) on the weights the step left: centres below
    reassignment_ratio * max w (at most half a batch of them, the lightest) move to random rows of the batch, and take
    the smallest remaining weight."""
    wh = w.cpu().numpy().copy()
    nb = Xs.shape[0]
    to = wh < self.reassignment_ratio * wh.max()
    if to.sum() > 0.5 * nb:
      to[np.argsort(wh)[int(0.5 * nb):]] = False
    nre = int(to.sum())
    if nre:
      picks = self._choice(nb, nre) if self._choice is not None else rng.choice(nb, replace=False, size=nre)
      dev = C.device
      C[torch.from_numpy(np.nonzero(to)[0]).to(dev)] = Xs[torch.as_tensor(np.asarray(picks, dtype=np.int64)).to(dev)]
    wh[to] = np.min(wh[~to])
    w.copy_(torch.from_numpy(wh))

  def _resume(self, Xs, C, Cold, w, buf, state, rng):
    self._reassign(Xs, C, w, rng)
    state[8:12].view(torch.int32).zero_()      # pause
    self._step(None, C, Cold, w, buf, state, resume=1)
    return self._read(state)

  # ---- public -----------------------------------------------------------------------------------------------------------
  def fit(self, X, batches=None):
    n, d, _ = _check_X(X, need_device=False)
    k = self.n_clusters
    if n < k:
      raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, k))
    batch = min(self.batch_size, n)
    if batches is not None:
      batches = [np.asarray(b, dtype=np.int64) for b in batches]
      if not batches or any(b.ndim != 1 or b.shape != batches[0].shape or b.size < 1 for b in batches) or \
         any(b.min() < 0 or b.max() >= n for b in batches):
        raise ValueError("kmeans (HIP): batches must be equally long 1-d index arrays into X")
      batch = int(batches[0].size)
    _check_shape(n, d, k)
    _check_shape(batch, d, k)
    if not isinstance(self.init, str) and tuple(torch.as_tensor(self.init).shape) != (k, d):
      raise ValueError("kmeans (HIP): init has shape %s, expected %s" % (tuple(torch.as_tensor(self.init).shape), (k, d)))
    _check_X(X)
    dev = X.device
    rng = np.random.RandomState(self.seed)
    init_size = self._init_size_for(n, batch)
    tol = 0.0
    if self.tol > 0 and n > 1:
      tol = float(X.var(dim=0, unbiased=False).double().mean()) * self.tol
    # validation set, then the best of n_init initialisations on it
    Xv = X[torch.from_numpy(rng.randint(0, n, init_size)).to(dev)]
    vbuf = _Buffers(Xv, k, with_sums=False)
    cands, inertias = [], []
    for _ in range(self.n_init):
      Ci = self._init_centroids(X, rng, init_size)
      _assign(Xv, Ci, vbuf, with_sums=False, inertia=True)
      cands.append(Ci)
      inertias.append(vbuf.inertia.clone())
    best, best_inertia = 0, None
    for i, v in enumerate(torch.cat(inertias).cpu().tolist()):
      if not math.isfinite(v):
        raise ValueError("non-finite features")
      if best_inertia is None or v < best_inertia:
        best, best_inertia = i, v
    C = cands[best]
    Cold = torch.empty_like(C)
    w = torch.zeros((k,), dtype=torch.float64, device=dev)
    n_steps = (self.max_iter * n) // batch if batches is None else len(batches)
    state = self._new_state(dev, float(batch), min(batch * 2.0 / (n + 1), 1.0), tol, self.max_no_improvement)
    Xb = torch.empty((batch, d), dtype=F32, device=dev)
    buf = self._buf(Xb)
    buf.labels.fill_(-1)
    st = dict(step=0, converged=0, pause=0, ewa=None)
    self.n_pauses_ = 0
    while st["step"] < n_steps and not st["converged"]:
      i0 = st["step"]
      ce = min(self.check_every, n_steps - i0)
      idxs, rstates = [], []
      for j in range(ce):
        if batches is None:
          idxs.append(rng.randint(0, n, batch))
          rstates.append(rng.get_state())
        else:
          idxs.append(batches[i0 + j])
      idx_dev = torch.from_numpy(np.stack(idxs).astype(np.int64)).to(dev)
      for j in range(ce):
        torch.index_select(X, 0, idx_dev[j], out=Xb)
        self._step(Xb, C, Cold, w, buf, state)
      st = self._read(state)
      if st["pause"]:
        j = st["step"] - i0      # the steps behind it were latched out: their draws are taken back
        if batches is None:
          rng.set_state(rstates[j])
        self.n_pauses_ += 1
        st = self._resume(X[idx_dev[j]], C, Cold, w, buf, state, rng)
    self.cluster_centers_, self.counts_ = C, w
    self.n_steps_ = st["step"]
    self.n_iter_ = int(np.ceil((st["step"] * batch) / float(n)))
    self.ewa_inertia_ = st["ewa"]
    fbuf = _Buffers(X, k, with_sums=False)
    _assign(X, C, fbuf, with_sums=False, inertia=True)
    self.labels_ = fbuf.labels
    self.inertia_ = float(fbuf.inertia.cpu()[0])
    if not math.isfinite(self.inertia_):
      raise ValueError("non-finite features")
    self._w, self._rng = w, rng
    return self

  def partial_fit(self, X):
    """One mini-batch step on the rows of X (the first call initialises the centres on them).  Reads the state block
    once: a reassignment, when the step asks for one, is completed before the call returns."""
    n, d, _ = _check_X(X)
    k = self.n_clusters
    _check_shape(n, d, k)
    dev = X.device
    if not hasattr(self, "_rng"):
      self._rng = np.random.RandomState(self.seed)
    if not hasattr(self, "cluster_centers_"):
      if n < k:
        raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n, k))
      if not isinstance(self.init, str) and tuple(torch.as_tensor(self.init).shape) != (k, d):
        raise ValueError("kmeans (HIP): init has shape %s, expected %s" % (tuple(torch.as_tensor(self.init).shape), (k, d)))
      self.cluster_centers_ = self._init_centroids(X, self._rng, self._init_size_for(n, min(self.batch_size, n)))
      self._w = self.counts_ = torch.zeros((k,), dtype=torch.float64, device=dev)
      self.n_steps_ = 0
    if not hasattr(self, "_pstate"):
      # never latches on convergence: tol 0 and no max_no_improvement; n_since carries the reassignment schedule
      self._pstate = self._new_state(dev, float(n), 1.0, 0.0, None)
      self._pstate[0:4].view(torch.int32).fill_(int(self.n_steps_))
      self._pold = torch.empty_like(self.cluster_centers_)
    C = self.cluster_centers_
    if d != C.shape[1]:
      raise ValueError("kmeans (HIP): X has %d features, the centres %d" % (d, C.shape[1]))
    Xc = X if X.is_contiguous() else X.contiguous()
    buf = self._buf(Xc)
    buf.labels.fill_(-1)
    self._step(Xc, C, self._pold, self._w, buf, self._pstate)
    st = self._read(self._pstate)
    if st["pause"]:
      st = self._resume(Xc, C, self._pold, self._w, buf, self._pstate, self._rng)
    self.n_steps_ = st["step"]
    self.batch_inertia_ = st["inertia"]
    return self

  predict = KMeans.predict
  fit_predict = KMeans.fit_predict


def _features(config, net, dataloader, sobel):
  """Every batch's pre-head features, written into one device matrix; flat int32 targets next to it."""
  from .transforms import sobel_process
  num_batches = len(dataloader)
  dev = torch.device("cuda", torch.cuda.current_device())
  total = num_batches * config.batch_sz
  flat_targets_all = torch.zeros(total, dtype=torch.int32, device=dev)
  features_all = None
  num_test = 0
  for b_i, batch in enumerate(dataloader):
    imgs = batch[0].cuda()
    if sobel:
      imgs = sobel_process(imgs, config.include_rgb)
    flat_targets = batch[1]
    with torch.no_grad():
      x_outs = net(imgs, kmeans_use_features=True)
    feats = x_outs if torch.is_tensor(x_outs) else x_outs[0]      # our IIC nets return one copy per sub-head
    assert (len(feats.shape) == 2)
    if features_all is None:
      features_all = torch.zeros((total, feats.shape[1]), dtype=F32, device=dev)
    num_test_curr = flat_targets.shape[0]
    assert (num_test_curr <= config.batch_sz and feats.shape[0] == num_test_curr)
    start_i = b_i * config.batch_sz
    features_all[start_i:(start_i + num_test_curr), :] = feats.float()
    flat_targets_all[start_i:(start_i + num_test_curr)] = flat_targets.to(dev)
    num_test += num_test_curr
  return features_all[:num_test], flat_targets_all[:num_test]


def get_data_kmeans_on_features(config, net, dataloader, sobel, kmeans=None):
  """Twin of the reference's triplets_get_data_kmeans_on_features (triplets.py:134-173): same signature, same return
  value -- flat predictions and flat targets on the device.  The features never leave the device.  ``kmeans``: a
  configured ``KMeans`` to use instead of the default ``KMeans(n_clusters=config.gt_k)``."""
  features_all, flat_targets_all = _features(config, net, dataloader, sobel)
  km = kmeans if kmeans is not None else KMeans(n_clusters=config.gt_k)
  flat_preds_all = km.fit(features_all).labels_
  assert (flat_targets_all.shape == flat_preds_all.shape)
  return flat_preds_all, flat_targets_all


def kmeans_eval(config, net, dataloader, sobel, kmeans=None):
  """The k-means branch of the reference's triplets_eval (triplets.py:176-228) as a function: net.eval() / net.train()
  around the pass, Hungarian match of the k-means labels, then a dict with ``acc``, ``mass`` and ``per_class_acc``
  ([1, gt_k] arrays as triplets_eval computes them), ``nmi`` and ``ari`` -- all from one count matrix."""
  net.eval()
  flat_preds_all, flat_targets_all = get_data_kmeans_on_features(config, net, dataloader, sobel, kmeans=kmeans)
  net.train()
  gt_k = config.gt_k
  num_samples = flat_preds_all.shape[0]
  match = eval_metrics._hungarian_match(flat_preds_all, flat_targets_all, preds_k=gt_k, targets_k=gt_k)
  assert (len(set(p for p, _ in match)) == gt_k)      # each class must get mapped
  counts = eval_metrics._counts(flat_preds_all, flat_targets_all, gt_k, gt_k)      # iic_contingency: [pred][target]
  mass = np.zeros((1, gt_k))
  per_class_acc = np.zeros((1, gt_k))
  for pred_i, target_i in match:
    mass[0, target_i] = counts[pred_i].sum()
    per_class_acc[0, target_i] = counts[pred_i, target_i]
  nmi, ari = eval_metrics.nmi_ari_from_counts(counts)
  return {"acc": per_class_acc.sum() / float(num_samples), "mass": mass, "per_class_acc": per_class_acc,
          "nmi": nmi, "ari": ari, "match": match}
