"""Segmentation k-means evaluation on the device -- opt-in twin of
code/utils/segmentation/baselines/kmeans_segmentation_eval.py, the routine that scores the reference's three segmentation
baselines (isola.py, doersch.py, kmeans_and_sift.py) and the way to ask what plain k-means makes of an IIC trunk.

The reference runs the net with ``penultimate=True`` -- the 10a trunk bilinearly up-sampled to input_sz, an fp32
``[N, 512, S, S]`` tensor (6.1 GB per Potsdam batch) -- copies it to the host, transposes and masks it, and hands it to
scikit-learn: a ``MiniBatchKMeans`` fit on a sample of pixels (``train_kmeans``), then ``predict`` on every unmasked pixel
(``apply_trained_kmeans``).  Here the up-sampled feature map never exists:

* ``train_kmeans`` interpolates only the sampled pixels (iic_seg_feat_sample) into one device matrix and fits
  ``iic_amd.kmeans.MiniBatchKMeans`` on it;
* ``apply_trained_kmeans`` uses that a k-means score ``||c_j||^2 - 2 x.c_j`` is linear in x, as bilinear interpolation is:
  the dot products are taken at the trunk's own resolution (the fused head GEMM on the bf16 PT window, or gather +
  iic_gemm_f32) and up-sampled as gt_k channels; iic_seg_kmeans_label_acc up-samples, takes the arg-min and folds the label
  with the batch's targets and mask into a device-resident count matrix -- one launch per batch, one host
  synchronisation per pass.  Accuracy, masses, NMI and ARI are functions of that matrix.

``install()`` does not rebind anything to this module; a script opts in -- INTEGRATION.md section 5i.
"""
import numpy as np
import torch

from . import eval_metrics, ops
from ._lib import check, lib, ptr, stream_ptr
from .archs import seg as seg_archs
from .kmeans import MiniBatchKMeans
from .transforms import sobel_process

__all__ = ["kmeans_segmentation_eval", "train_kmeans", "apply_trained_kmeans", "trunk_dots", "label_acc", "feat_sample",
           "sample_indices", "sample_budget", "stats_from_counts"]
F32, U8 = torch.float32, torch.uint8
GET_NMI_ARI = False      # kmeans_segmentation_eval.py:11
MAX_K, MAX_BINS = 255, 16384
P = seg_archs.SegmentationNet10aTrunk.P


# ---- host-side index generation (kmeans_segmentation_eval.py:29-30, :78-81) --------------------------------------------------
def sample_budget(max_num_kmeans_samples, num_imgs):
  """max_num_pixels_per_img of train_kmeans (:30)."""
  return int(max_num_kmeans_samples / num_imgs)


def sample_indices(num_unmasked, num_imgs_batch, max_num_pixels_per_img, sampling="reference", rng=None):
  """(num_selected, ordinals): which of a batch's unmasked pixels (numbered in the order ``x_out[mask, :]`` lists them)
  make up its num_selected feature rows.

  ``sampling="reference"`` is the reference's line :79, ``np.random.choice(num_selected, replace=False)``: without a
  ``size`` it returns ONE integer below num_selected, and ``x_out[selected, :]`` is then one row that the assignment at
  :88 broadcasts -- the batch contributes num_selected copies of one pixel's features.  ``ordinals`` is that single
  integer, shape [1].  ``sampling="uniform"`` draws num_selected distinct pixels among all num_unmasked, which is what
  the comment above that line describes; ``ordinals`` has shape [num_selected].  ``rng``: np.random (the reference's
  global stream) unless given."""
  rng = np.random if rng is None else rng
  num_selected = int(min(num_unmasked, num_imgs_batch * max_num_pixels_per_img))
  if sampling == "reference":
    if num_selected < 1:
      raise ValueError("a must be greater than 0 unless no samples are taken")      # what np.random.choice(0) raises
    return num_selected, np.asarray([rng.choice(num_selected, replace=False)], dtype=np.int64)
  if sampling == "uniform":
    if num_selected < 1:
      return 0, np.zeros((0,), dtype=np.int64)
    return num_selected, np.asarray(rng.choice(int(num_unmasked), size=num_selected, replace=False), dtype=np.int64)
  raise ValueError("sampling must be 'reference' or 'uniform', got %r" % (sampling,))


def ordinals_to_coords(mask_np, ordinals):
  """int32 [m, 3] (n, y, x) of the unmasked pixels with the given ordinals; mask_np: bool [N, S, S]."""
  flat = np.flatnonzero(mask_np.reshape(-1))[ordinals]
  S2 = mask_np.shape[1] * mask_np.shape[2]
  n, r = flat // S2, flat % S2
  return np.stack([n, r // mask_np.shape[2], r % mask_np.shape[2]], axis=1).astype(np.int32)


# ---- device pieces -------------------------------------------------------------------------------------------------------
def _check_pt(pt):
  if not (torch.is_tensor(pt) and pt.is_cuda and pt.dim() == 4 and pt.is_contiguous() and
          pt.dtype in (torch.bfloat16, F32)):
    raise ValueError("seg k-means (HIP): the PT feature tensor must be a contiguous bf16 or fp32 [N, Hp, Wp, C] device "
                     "tensor -- there is no CPU fallback")
  N, Hp, Wp, C = pt.shape
  if Hp <= 2 * P or Wp <= 2 * P:
    raise ValueError("seg k-means (HIP): PT tensor %s has no interior inside its border of %d" % (tuple(pt.shape), P))
  return N, Hp, Wp, C


def _check_centres(centres, C):
  if not (torch.is_tensor(centres) and centres.is_cuda and centres.dtype == F32 and centres.dim() == 2 and
          centres.shape[1] == C and centres.is_contiguous()):
    raise ValueError("seg k-means (HIP): centres must be a contiguous float32 [k, %d] device tensor" % C)
  k = centres.shape[0]
  if not 1 <= k <= MAX_K:
    raise ValueError("seg k-means (HIP): k = %d is outside the served range 1 <= k <= %d" % (k, MAX_K))
  return k


def trunk_dots(pt, centres):
  """fp32 [N, Hl, Wl, k]: x.c_j for every interior pixel of the PT feature tensor.  bf16 tensors with C in {256, 512} and
  k <= 32 take iic_seg_head_fwd on the interior window (off = P, exact-fp32 MFMA); everything else gathers the window
  (iic_seg_window_gather, or the f32 gather on the parity path) and multiplies with iic_gemm_f32."""
  N, Hp, Wp, C = _check_pt(pt)
  k = _check_centres(centres, C)
  Hl, Wl = Hp - 2 * P, Wp - 2 * P
  M = N * Hl * Wl
  L, s = lib(), stream_ptr()
  dots = torch.empty((N, Hl, Wl, k), dtype=F32, device=pt.device)
  if pt.dtype != F32 and bool(L.iic_seg_head_supported(C, k)):
    check(L.iic_seg_head_fwd(ptr(pt), ptr(centres), ptr(dots), N, Hl, Wl, Hp, Wp, P, C, k, s), "iic_seg_head_fwd")
    return dots
  if pt.dtype != F32 and C % 8 != 0:
    raise ValueError("seg k-means (HIP): a bf16 PT tensor needs C % 8 == 0, got C = %d" % C)
  Fm = torch.empty((M, C), dtype=F32, device=pt.device)
  if pt.dtype == F32:
    check(L.iic_f32_window_gather(ptr(pt), ptr(Fm), N, Hl, Wl, Hp, Wp, P, C, s), "iic_f32_window_gather")
  else:
    check(L.iic_seg_window_gather(ptr(pt), ptr(Fm), N, Hl, Wl, Hp, Wp, P, C, s), "iic_seg_window_gather")
  ops.gemm_f32(Fm, C, 1, centres, 1, C, dots, k, M, k, C)
  return dots


def _u8_map(t, dev, shape, what, is_mask=False):
  """uint8 [N, S, S] on the device: SegTestPreparer's tensors as they are, the reference's CPU tensors copied."""
  t = t.to(dev, non_blocking=True)
  if t.dtype == torch.bool:
    t = t.view(U8) if t.is_contiguous() else t.to(U8)
  elif t.dtype != U8:
    t = (t != 0).to(U8) if is_mask else t.to(U8)
  if tuple(t.shape) != tuple(shape):
    raise ValueError("seg k-means (HIP): %s has shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
  return t.contiguous()


def label_acc(dots, cnorm, targets_u8, mask_u8, k_gt, counts, S, labels_u8=None):
  """One iic_seg_kmeans_label_acc launch: counts (int64 [k * k_gt + 1], accumulated) += the batch's labels against its
  targets under its mask (None: every pixel); labels_u8 (optional uint8 [N, S, S]) receives the label map."""
  if not (torch.is_tensor(dots) and dots.is_cuda and dots.dtype == F32 and dots.dim() == 4 and dots.is_contiguous()):
    raise ValueError("seg k-means (HIP): dots must be a contiguous float32 [N, Hl, Wl, k] device tensor")
  N, Hl, Wl, k = dots.shape
  if not (1 <= k <= MAX_K and k_gt >= 1 and k * k_gt <= MAX_BINS):
    raise ValueError("seg k-means (HIP): (k, k_gt) = (%d, %d) is outside the served range 1 <= k <= %d, k * k_gt <= %d"
                     % (k, k_gt, MAX_K, MAX_BINS))
  if N < 1 or Hl < 1 or Wl < 1 or S < 1:
    raise ValueError("seg k-means (HIP): empty geometry N, Hl, Wl, S = %s" % ((N, Hl, Wl, S),))
  if not (cnorm.is_cuda and cnorm.dtype == F32 and cnorm.is_contiguous() and cnorm.numel() == k):
    raise ValueError("seg k-means (HIP): cnorm must be %d contiguous float32 device values" % k)
  if not (counts.is_cuda and counts.dtype == torch.long and counts.is_contiguous() and counts.numel() == k * k_gt + 1):
    raise ValueError("seg k-means (HIP): counts must be %d contiguous int64 device values" % (k * k_gt + 1))
  for t, what in ((targets_u8, "targets"), (mask_u8, "mask"), (labels_u8, "labels")):
    if t is not None and not (t.is_cuda and t.dtype == U8 and t.is_contiguous() and t.numel() == N * S * S):
      raise ValueError("seg k-means (HIP): %s must be %d contiguous uint8 device values" % (what, N * S * S))
  if targets_u8 is None:
    raise ValueError("seg k-means (HIP): targets are required")
  check(lib().iic_seg_kmeans_label_acc(ptr(dots), ptr(cnorm), ptr(targets_u8), ptr(mask_u8), N, Hl, Wl, k, S, k_gt,
                                       ptr(counts), ptr(labels_u8), stream_ptr()), "iic_seg_kmeans_label_acc")


def feat_sample(pt, coords, S, out=None):
  """fp32 [m, C]: the up-sampled features of the pixels coords (int32 [m, 3] = (n, y, x) at resolution S, numpy or
  device tensor) -- the numbers gather + iic_bilinear_fwd would store there.  ``out``: a contiguous [m, C] device view
  to write into."""
  N, Hp, Wp, C = _check_pt(pt)
  if not torch.is_tensor(coords):
    coords = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32))
  if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 3:
    raise ValueError("seg k-means (HIP): coords must be int32 [m, 3]")
  coords = coords.to(pt.device).contiguous()
  m = coords.shape[0]
  if out is None:
    out = torch.empty((m, C), dtype=F32, device=pt.device)
  elif not (out.is_cuda and out.dtype == F32 and out.is_contiguous() and tuple(out.shape) == (m, C)):
    raise ValueError("seg k-means (HIP): out must be a contiguous float32 [%d, %d] device tensor" % (m, C))
  check(lib().iic_seg_feat_sample(ptr(pt), 1 if pt.dtype == F32 else 0, ptr(coords), m, ptr(out), N, Hp - 2 * P,
                                  Wp - 2 * P, Hp, Wp, P, C, S, stream_ptr()), "iic_seg_feat_sample")
  return out


def _trunk(config, net, imgs):
  imgs = imgs.cuda()
  if not config.no_sobel:
    imgs = sobel_process(imgs, config.include_rgb, using_IR=getattr(config, "using_IR", False))
  with torch.no_grad():
    return seg_archs.trunk_pt(net, imgs)


def _num_imgs(loader):
  ds = getattr(loader, "dataset", None)
  return len(ds) if ds is not None else int(loader.n)      # seg_mapping_dataloader has no dataset object


def _centres_of(kmeans, dev):
  c = kmeans.cluster_centers_
  c = c if torch.is_tensor(c) else torch.from_numpy(np.asarray(c))
  return c.to(device=dev, dtype=F32).contiguous()


# ---- the twins -----------------------------------------------------------------------------------------------------------
def train_kmeans(config, net, test_dataloader, sampling="reference", kmeans=None, rng=None):
  """Twin of train_kmeans (kmeans_segmentation_eval.py:28-107): the same sample budget arithmetic, the sampled rows
  interpolated on the device and written straight into the device matrix the fit runs on.  Returns the fitted
  ``MiniBatchKMeans`` (``kmeans``: a configured one to use instead of ``MiniBatchKMeans(n_clusters=config.gt_k)``).
  ``sampling``: see ``sample_indices`` -- "reference" reproduces the reference's selection line, "uniform" what its
  comment describes."""
  num_imgs = _num_imgs(test_dataloader)
  max_num_pixels_per_img = sample_budget(config.max_num_kmeans_samples, num_imgs)
  dev = torch.device("cuda", torch.cuda.current_device())
  features_all = None
  actual_num_features = 0
  for tup in test_dataloader:
    imgs, _, mask = tup
    mask_np = (mask.cpu().numpy() != 0)
    num_unmasked = int(mask_np.sum())
    pt = _trunk(config, net, imgs)
    if features_all is None:
      features_all = torch.zeros((config.max_num_kmeans_samples, pt.shape[3]), dtype=F32, device=dev)
    num_selected, ordinals = sample_indices(num_unmasked, pt.shape[0], max_num_pixels_per_img, sampling, rng)
    assert (actual_num_features + num_selected <= config.max_num_kmeans_samples)
    block = features_all[actual_num_features:actual_num_features + num_selected]
    coords = ordinals_to_coords(mask_np, ordinals)
    if sampling == "reference":
      block[:] = feat_sample(pt, coords, config.input_sz)      # one row, broadcast as :88 does
    else:
      feat_sample(pt, coords, config.input_sz, out=block)
    actual_num_features += num_selected
  assert (actual_num_features <= config.max_num_kmeans_samples)
  features_all = features_all[:actual_num_features, :]
  km = kmeans if kmeans is not None else MiniBatchKMeans(n_clusters=config.gt_k)
  return km.fit(features_all)


def stats_from_counts(counts, gt_k, get_nmi_ari=False):
  """(acc, nmi, ari, reordered_masses, match) of apply_trained_kmeans (:162-186) from the [gt_k, gt_k] count matrix
  counts[pred][target]: permutation match, accuracy of the reordered predictions, the mass of every class."""
  from scipy.optimize import linear_sum_assignment
  counts = np.asarray(counts)
  n = int(counts.sum())
  rows, cols = linear_sum_assignment(n - counts)      # eval_metrics._hungarian_match
  match = [(int(p), int(t)) for p, t in zip(rows, cols)]
  acc = int(sum(int(counts[p, t]) for p, t in match)) / float(n)
  reordered_masses = np.zeros(gt_k)
  for p, t in match:
    reordered_masses[t] = float(counts[p].sum()) / n
  nmi, ari = eval_metrics.nmi_ari_from_counts(counts) if get_nmi_ari else (-1., -1.)
  return acc, nmi, ari, reordered_masses, match


def _apply_counts(config, net, test_dataloader, kmeans):
  gt_k = config.gt_k
  dev = torch.device("cuda", torch.cuda.current_device())
  centres = _centres_of(kmeans, dev)
  k = centres.shape[0]
  if not (1 <= k <= MAX_K and k * gt_k <= MAX_BINS):
    raise ValueError("seg k-means (HIP): (k, gt_k) = (%d, %d) is outside the served range" % (k, gt_k))
  cnorm = (centres * centres).sum(1).contiguous()
  counts = torch.zeros((k * gt_k + 1,), dtype=torch.long, device=dev)
  S = config.input_sz
  for tup in test_dataloader:
    imgs, targets, mask = tup
    pt = _trunk(config, net, imgs)
    shape = (pt.shape[0], S, S)
    label_acc(trunk_dots(pt, centres), cnorm, _u8_map(targets, dev, shape, "targets"),
              _u8_map(mask, dev, shape, "mask", is_mask=True), gt_k, counts, S)
  host = counts.cpu().numpy()      # the one synchronisation of the pass
  return host[:-1].reshape(k, gt_k).copy(), int(host[-1])


def apply_trained_kmeans(config, net, test_dataloader, kmeans, get_nmi_ari=None):
  """Twin of apply_trained_kmeans (kmeans_segmentation_eval.py:110-188): (acc, nmi, ari, reordered_masses).  ``kmeans``:
  anything with ``cluster_centers_`` [gt_k, 512].  nmi and ari are -1. as in the reference unless get_nmi_ari (default:
  the module's GET_NMI_ARI); then eval_metrics.nmi_ari_from_counts of the same matrix."""
  counts, n = _apply_counts(config, net, test_dataloader, kmeans)
  assert (counts.shape[0] == config.gt_k)      # permutation, not many-to-one
  assert (int(counts.sum()) == n)      # _acc's asserts: every selected target is a valid class
  acc, nmi, ari, masses, _ = stats_from_counts(counts, config.gt_k, GET_NMI_ARI if get_nmi_ari is None else get_nmi_ari)
  return acc, nmi, ari, masses


def kmeans_segmentation_eval(config, net, test_dataloader, sampling="reference", kmeans=None, get_nmi_ari=None):
  """Twin of kmeans_segmentation_eval (kmeans_segmentation_eval.py:18-25)."""
  net.eval()
  km = train_kmeans(config, net, test_dataloader, sampling=sampling, kmeans=kmeans)
  return apply_trained_kmeans(config, net, test_dataloader, km, get_nmi_ari=get_nmi_ari)
