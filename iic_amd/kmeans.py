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

``install()`` does not rebind anything to this module; a script opts in -- INTEGRATION.md section 5g.
"""
import math

import numpy as np
import torch

from . import eval_metrics
from ._lib import check, lib, ptr, stream_ptr

__all__ = ["KMeans", "lloyd_step", "seed_potentials", "supported", "workspace_bytes", "get_data_kmeans_on_features",
           "kmeans_eval"]
F32 = torch.float32
MAX_K, MAX_D = 256, 32768
STATE_BYTES = 64


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
