"""Segmentation evaluation on the device (csrc/seg_eval.hip, iic_amd/seg_eval.py, predict_labels): the label-map kernel
against the arg-max of the existing up-sampling kernel (bit for bit) and against float64, the streaming count kernel
against numpy and iic_contingency, predict_labels against forward, and segmentation_eval against the reference's
procedure assembled by hand from the flat arrays.  pytest -m gpu."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (Hl, Wl, S, k, N).  The first six are the square cases of the feature's specification: non-integer scales, clamped
# first / last rows, k above one wave's worth, a multi-row-tile case at k = 255, the real Potsdam width.  Then: source
# columns tiled because two rows of k = 255 do not fit the kernel's LDS budget (30 -> 64), the global-memory path (a
# 10x reduction: one quad's sources alone exceed the budget), S % 4 != 0 (byte stores: 18, 21), a non-square source.
CASES = [(7, 7, 16, 5, 2), (10, 10, 24, 3, 2), (12, 12, 24, 24, 2), (9, 9, 20, 45, 2), (6, 6, 12, 255, 1),
         (102, 102, 200, 24, 1),
         (30, 30, 64, 255, 1), (40, 40, 4, 200, 1), (9, 9, 18, 5, 2), (7, 7, 21, 3, 2), (7, 11, 20, 6, 2)]


def dev():
  return torch.device("cuda:0")


def _probs(Hl, Wl, k, N):
  g = torch.Generator().manual_seed(1234 + k)
  return F.softmax(torch.randn((N, k, Hl, Wl), generator=g) * 3, dim=1)        # NCHW fp32, CPU


def _label_map(p_nchw, S):
  from iic_amd._lib import check, lib, stream_ptr
  N, k, Hl, Wl = p_nchw.shape
  xin = p_nchw.permute(0, 2, 3, 1).contiguous().to(dev())                       # [N][Hl][Wl][k]
  lab = torch.full((N, S, S), 255, dtype=torch.uint8, device=dev())
  check(lib().iic_seg_label_map(xin.data_ptr(), lab.data_ptr(), N, Hl, Wl, k, S, stream_ptr()), "iic_seg_label_map")
  return xin, lab


@functools.lru_cache(maxsize=None)
def _case(Hl, Wl, S, k, N):
  """(CPU probabilities, labels of iic_seg_label_map, the existing kernel's up-sampled maps) -- computed once a case."""
  from iic_amd._lib import check, lib, stream_ptr
  p = _probs(Hl, Wl, k, N)
  xin, lab = _label_map(p, S)
  out = torch.empty((N, k, S, S), device=dev())
  check(lib().iic_bilinear_fwd(xin.data_ptr(), out.data_ptr(), N, Hl, Wl, k, S, stream_ptr()), "iic_bilinear_fwd")
  torch.cuda.synchronize()
  return p, lab.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("Hl,Wl,S,k,N", CASES)
def test_label_map_equals_argmax_of_existing_upsampling(Hl, Wl, S, k, N):
  """array_equal against numpy argmax(axis=1) (first maximum) of iic_bilinear_fwd's output."""
  _, lab, out = _case(Hl, Wl, S, k, N)
  want = out.argmax(axis=1)
  assert lab.shape == want.shape and lab.dtype == np.uint8
  assert np.array_equal(lab, want), "%d of %d labels differ" % (int((lab != want).sum()), lab.size)


@pytest.mark.parametrize("Hl,Wl,S,k,N", CASES)
def test_label_map_vs_float64(Hl, Wl, S, k, N):
  """Oracle: F.interpolate in float64 on the CPU, then arg-max.  A three-level fp32 convex combination of values <= 1
  errs by less than 5e-7 per class, so a float64 top-two gap of 2e-6 or more cannot flip: those pixels must be equal;
  the others are left out, and may be at most 0.5 % of a case.  (On the CPU, with these seeds: no pixel of any case
  is below the gap; the smallest gap is 6.8e-6, in the Potsdam-width case, then 7.3e-6 in the second.)"""
  p, lab, _ = _case(Hl, Wl, S, k, N)
  o = F.interpolate(p.double(), size=S, mode="bilinear", align_corners=False)
  top2 = o.topk(2, dim=1).values
  sure = ((top2[:, 0] - top2[:, 1]) >= 2e-6).numpy()
  left_out = 1.0 - sure.mean()
  print("left out %d of %d pixels" % (int((~sure).sum()), sure.size))
  assert left_out <= 0.005
  assert np.array_equal(lab[sure], o.argmax(dim=1).numpy()[sure])


def _sources(S, L):
  """Source index pair of every output index (align_corners=False), in float64."""
  s = np.maximum((np.arange(S) + 0.5) * L / S - 0.5, 0.0)
  i0 = np.minimum(np.floor(s).astype(np.int64), L - 1)
  return i0, np.minimum(i0 + 1, L - 1)


@pytest.mark.parametrize("Hl,S,k", [(6, 12, 5), (7, 18, 9), (10, 24, 255)])
def test_label_map_ties_go_to_the_lowest_index(Hl, S, k):
  rng = np.random.default_rng(Hl)
  # two classes exactly equal and on top: the lower one wins, whichever pair it is
  lo, hi = 1, k - 2
  p = torch.from_numpy(rng.random((2, k, Hl, Hl)).astype(np.float32)) * 0.25
  top = torch.from_numpy(rng.random((2, Hl, Hl)).astype(np.float32)) * 0.5 + 0.3
  p[:, lo] = top
  p[:, hi] = top
  _, lab = _label_map(p, S)
  assert bool((lab == lo).all())
  # all classes exactly equal: class 0
  _, lab = _label_map(torch.full((2, k, Hl, Hl), 1.0 / k), S)
  assert bool((lab == 0).all())
  # a one-hot map (3 x 3 blocks of one label): the label is one of its four sources' labels, and THE label where the
  # four agree
  nb = (Hl + 2) // 3
  low = rng.integers(0, k, (2, nb, nb)).repeat(3, axis=1).repeat(3, axis=2)[:, :Hl, :Hl]
  p = F.one_hot(torch.from_numpy(low), k).permute(0, 3, 1, 2).float()
  _, lab = _label_map(p, S)
  lab = lab.cpu().numpy()
  i0, i1 = _sources(S, Hl)
  src = np.stack([low[:, a][:, :, b] for a in (i0, i1) for b in (i0, i1)])      # [4][N][S][S]
  assert bool((src == lab[None]).any(axis=0).all())
  agree = (src == src[0]).all(axis=0)
  assert agree.mean() > 0.1
  assert np.array_equal(lab[agree], src[0][agree])


def _acc_call(p, t, m, n, kp, kt, counts):
  from iic_amd._lib import lib, stream_ptr
  return lib().iic_seg_contingency_acc(p.data_ptr(), t.data_ptr(), None if m is None else m.data_ptr(), n, kp, kt,
                                       counts.data_ptr(), stream_ptr())


def _np_counts(p, t, m, kp, kt):
  sel = np.ones(p.shape, bool) if m is None else (m != 0)
  ok = sel & (p < kp) & (t < kt)
  c = np.zeros((kp, kt), np.int64)
  np.add.at(c, (p[ok].astype(np.int64), t[ok].astype(np.int64)), 1)
  return c, int(sel.sum())


@pytest.mark.parametrize("kp,kt", [(3, 3), (24, 3), (45, 15), (255, 64)])
def test_contingency_accumulation(kp, kt):
  """Two successive calls into one buffer == numpy's count of the concatenation == iic_contingency on the masked,
  widened arrays; the last element is the number of selected samples.  Labels >= k are injected on both sides."""
  from iic_amd._lib import check, lib, stream_ptr
  rng = np.random.default_rng(kp * 100 + kt)
  sizes = (1, 15, 16, 17, 4099)
  for n1, n2 in zip(sizes, sizes[1:] + sizes[:1]):
    for mask_mode in ("none", "zero", "random"):
      parts = []
      counts = torch.zeros(kp * kt + 1, dtype=torch.long, device=dev())
      for n in (n1, n2):
        p = np.minimum(rng.integers(0, kp + 3, n), 255).astype(np.uint8)
        t = np.minimum(rng.integers(0, kt + 3, n), 255).astype(np.uint8)
        p[0], t[-1] = 255, 255
        m = {"none": None, "zero": np.zeros(n, np.uint8),
             "random": (rng.integers(0, 3, n) * 127).astype(np.uint8)}[mask_mode]          # 0, 127, 254: != 0 selects
        parts.append((p, t, m))
        dp, dt = torch.from_numpy(p).to(dev()), torch.from_numpy(t).to(dev())
        dm = None if m is None else torch.from_numpy(m).to(dev())
        check(_acc_call(dp, dt, dm, n, kp, kt, counts), "iic_seg_contingency_acc")
      p, t = np.concatenate([a[0] for a in parts]), np.concatenate([a[1] for a in parts])
      m = None if mask_mode == "none" else np.concatenate([a[2] for a in parts])
      want, nsel = _np_counts(p, t, m, kp, kt)
      got = counts.cpu().numpy()
      assert np.array_equal(got[:-1].reshape(kp, kt), want), (n1, n2, mask_mode)
      assert int(got[-1]) == nsel, (n1, n2, mask_mode)
      # the existing kernel on the selected samples, widened to int64
      sel = np.ones(p.shape, bool) if m is None else (m != 0)
      old = torch.empty((kp, kt), dtype=torch.long, device=dev())
      wp, wt = torch.from_numpy(p[sel].astype(np.int64)).to(dev()), torch.from_numpy(t[sel].astype(np.int64)).to(dev())
      check(lib().iic_contingency(wp.data_ptr() if nsel else old.data_ptr(), wt.data_ptr() if nsel else old.data_ptr(),
                                  nsel, kp, kt, old.data_ptr(), stream_ptr()), "iic_contingency")
      assert np.array_equal(old.cpu().numpy(), want)


def test_contingency_unaligned_streams_empty_call_and_limits():
  from iic_amd._lib import check
  rng = np.random.default_rng(7)
  kp, kt, n = 24, 3, 1000
  p, t = rng.integers(0, kp, n + 1).astype(np.uint8), rng.integers(0, kt, n + 1).astype(np.uint8)
  m = rng.integers(0, 2, n + 1).astype(np.uint8)
  dp, dt, dm = (torch.from_numpy(a).to(dev())[1:] for a in (p, t, m))            # data pointers off 16-byte alignment
  counts = torch.zeros(kp * kt + 1, dtype=torch.long, device=dev())
  check(_acc_call(dp, dt, dm, n, kp, kt, counts), "iic_seg_contingency_acc")
  want, nsel = _np_counts(p[1:], t[1:], m[1:], kp, kt)
  check(_acc_call(dp, dt, dm, 0, kp, kt, counts), "iic_seg_contingency_acc")     # n == 0: a no-op that succeeds
  got = counts.cpu().numpy()
  assert np.array_equal(got[:-1].reshape(kp, kt), want) and int(got[-1]) == nsel
  assert _acc_call(dp, dt, dm, n, 255, 65, counts) == -3                         # 16 575 bins > 16 384: unsupported
  assert np.array_equal(counts.cpu().numpy(), got)


def _seg_cfg(two_head=False, **kw):
  c = dict(in_channels=4, input_sz=24, batchnorm_track=True, num_sub_heads=2, output_k=6)
  if two_head:
    c.update(output_k_A=6, output_k_B=3)
  c.update(kw)
  return types.SimpleNamespace(**c)


def _np_argmax(outs):
  return [o.detach().cpu().numpy().argmax(axis=1).astype(np.uint8) for o in outs]


@pytest.mark.parametrize("two_head", [False, True])
def test_predict_labels_equals_argmax_of_forward(two_head):
  from iic_amd import archs, ops
  torch.manual_seed(3)
  net = (archs.SegmentationNet10aTwoHead if two_head else archs.SegmentationNet10a)(_seg_cfg(two_head)).to(dev())
  x = torch.from_numpy(np.random.default_rng(2).random((3, 4, 24, 24)).astype(np.float32)).to(dev())
  heads = [dict(head="A"), dict(head="B")] if two_head else [dict()]
  net.train()
  with pytest.raises(AssertionError):
    net.predict_labels(x)                                     # grad enabled: inference only
  start = {k: v.clone() for k, v in net.state_dict().items()}

  def both(kw):
    """(labels of predict_labels, arg-max of forward, state after each) from the same starting state."""
    net.load_state_dict(start)
    with torch.no_grad():
      labs = net.predict_labels(x, **kw)
    torch.cuda.synchronize()
    s1 = {k: v.clone() for k, v in net.state_dict().items()}
    net.load_state_dict(start)
    with torch.no_grad():
      outs = net(x, **kw)
    torch.cuda.synchronize()
    s2 = {k: v.clone() for k, v in net.state_dict().items()}
    return labs, outs, s1, s2

  for kw in heads:
    for mode in ("eval", "train", "fp32"):
      net.train(mode == "train")
      if mode == "fp32":
        with ops.fp32_mode():
          labs, outs, s1, s2 = both(kw)
      else:
        labs, outs, s1, s2 = both(kw)
      assert len(labs) == len(outs) == 2
      for lab, want in zip(labs, _np_argmax(outs)):
        assert lab.dtype == torch.uint8 and tuple(lab.shape) == (3, 24, 24) and lab.is_cuda
        assert np.array_equal(lab.cpu().numpy(), want), (kw, mode)
      # BatchNorm state: exactly what forward leaves behind -- nothing at all in eval mode
      assert all(torch.equal(s1[k], s2[k]) for k in start), (kw, mode)
      if mode != "train":
        assert all(torch.equal(s1[k], start[k]) for k in start), (kw, mode)
      else:
        assert all(torch.equal(s1[k], start[k]) for k in start if "running" not in k and "num_batches" not in k)


def _loader(seed, gt_k, sizes=(4, 4, 2)):
  rng = np.random.default_rng(seed)
  return [(torch.from_numpy(rng.random((b, 4, 24, 24)).astype(np.float32)),
           torch.from_numpy(rng.integers(0, gt_k, (b, 24, 24)).astype(np.int32)),
           torch.from_numpy((rng.random((b, 24, 24)) < 0.7).astype(np.uint8))) for b in sizes]


def _by_hand(config, net, assign, test):
  """cluster_subheads_eval (cluster_eval.py:101-145, :187-228) on the flat arrays, with the package's drop-in matchers
  and the reference's reorder loop."""
  from iic_amd import eval_metrics, seg_eval
  matcher = eval_metrics._hungarian_match if config.eval_mode == "hung" else eval_metrics._original_match

  def reordered_acc(preds, targets, match):
    r = torch.zeros(targets.shape[0], dtype=preds.dtype).cuda()
    for pred_i, target_i in match:
      r[preds == pred_i] = target_i
    return eval_metrics._acc(r, targets, config.gt_k, verbose=0)

  preds, targets = seg_eval._segmentation_get_data(config, net, assign, sobel=False)
  matches, train_accs = [], np.zeros(config.num_sub_heads, dtype=np.float32)
  for i in range(config.num_sub_heads):
    matches.append(matcher(preds[i], targets, preds_k=config.output_k, targets_k=config.gt_k))
    train_accs[i] = reordered_acc(preds[i], targets, matches[i])
  best = np.argmax(train_accs)
  if config.mode == "IID":
    test_accs = train_accs
  else:
    preds, targets = seg_eval._segmentation_get_data(config, net, test, sobel=False)
    test_accs = np.zeros(config.num_sub_heads, dtype=np.float32)
    for i in range(config.num_sub_heads):
      test_accs[i] = reordered_acc(preds[i], targets, matches[i])
  return {"test_accs": list(test_accs), "avg": np.mean(test_accs), "std": np.std(test_accs), "best": test_accs[best],
          "worst": test_accs.min(), "best_train_sub_head": best, "best_train_sub_head_match": matches[best],
          "train_accs": list(train_accs)}


@functools.lru_cache(maxsize=None)
def _eval_net(k):
  from iic_amd import archs
  torch.manual_seed(11 + k)
  return archs.SegmentationNet10a(_seg_cfg(output_k=k)).to(dev()).train()


@pytest.mark.parametrize("mode", ["IID", "IID+"])
@pytest.mark.parametrize("eval_mode,k", [("orig", 6), ("hung", 3)])
def test_segmentation_eval_end_to_end(eval_mode, k, mode):
  from iic_amd import seg_eval
  gt_k = 3
  net = _eval_net(k)
  config = _seg_cfg(output_k=k, gt_k=gt_k, batch_sz=4, eval_mode=eval_mode, mode=mode, include_rgb=True,
                    mapping_assignment_partitions=["a"], mapping_test_partitions=["a"], epoch_stats=[], epoch_acc=[],
                    epoch_avg_subhead_acc=[])
  assign, test = _loader(5, gt_k), _loader(6, gt_k, sizes=(4, 3))
  got = seg_eval.segmentation_eval(config, net, assign, test, sobel=False, return_only=True)
  assert net.training and config.epoch_acc == []
  net.eval()
  want = _by_hand(config, net, assign, test)
  assert set(got) == set(want)
  for key in ("test_accs", "train_accs"):
    assert all(type(v) is np.float32 for v in got[key])
    assert np.array(got[key]).tobytes() == np.array(want[key]).tobytes(), (key, got[key], want[key])
  for key in ("avg", "std", "best", "worst"):
    assert type(got[key]) is type(want[key]) and np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
  assert int(got["best_train_sub_head"]) == int(want["best_train_sub_head"])
  assert got["best_train_sub_head_match"] == want["best_train_sub_head_match"]

  # the flat arrays of the compatible form == the reference's procedure (segmentation_eval.py:75-128) with torch.argmax
  preds, targets = seg_eval._segmentation_get_data(config, net, assign, sobel=False)
  ref_p, ref_t, ref_m = [[] for _ in range(config.num_sub_heads)], [], []
  for imgs, flat_targets, mask in assign:
    with torch.no_grad():
      x_outs = net(imgs.cuda())
    for i in range(config.num_sub_heads):
      ref_p[i].append(torch.argmax(x_outs[i], dim=1).view(-1).to(torch.uint8))
    ref_t.append(flat_targets.view(-1).cuda().to(torch.uint8))
    ref_m.append(mask.view(-1).cuda().bool())
  sel = torch.cat(ref_m)
  assert targets.dtype == torch.uint8 and torch.equal(targets, torch.cat(ref_t)[sel])
  for i in range(config.num_sub_heads):
    assert preds[i].dtype == torch.uint8 and torch.equal(preds[i], torch.cat(ref_p[i])[sel])
  assert targets.shape[0] == int(sel.sum())

  # the bookkeeping form: same dict appended, is_best from the accuracies so far, net back in train mode
  config.epoch_acc.append(-1.0)
  assert seg_eval.segmentation_eval(config, net, assign, test, sobel=False) == bool(got["best"] > -1.0)
  assert net.training and len(config.epoch_stats) == 1 and config.epoch_acc[-1] == got["best"]
  assert config.epoch_avg_subhead_acc == [got["avg"]]
  net.train()


def test_seg_eval_accumulator_streams_without_flat_arrays():
  """SegEvalAccumulator.add on label maps + counts(): equals numpy on the concatenated batches, every sub-head."""
  from iic_amd.seg_eval import SegEvalAccumulator
  rng = np.random.default_rng(9)
  acc = SegEvalAccumulator(2, 6, 3, dev())
  want, nsel = np.zeros((2, 6, 3), np.int64), 0
  for b in (3, 2):
    maps = [rng.integers(0, 6, (b, 24, 24)).astype(np.uint8) for _ in range(2)]
    t, m = rng.integers(0, 3, (b, 24, 24)).astype(np.int32), rng.random((b, 24, 24)) < 0.5
    acc.add([torch.from_numpy(a).to(dev()) for a in maps], torch.from_numpy(t).to(dev()), torch.from_numpy(m).to(dev()))
    for h in range(2):
      c, s = _np_counts(maps[h].ravel(), t.ravel().astype(np.uint8), m.ravel(), 6, 3)
      want[h] += c
    nsel += s
  got, n = acc.counts()
  assert got.dtype == np.int64 and np.array_equal(got, want) and n == nsel
  with pytest.raises(AssertionError):
    acc.add([torch.zeros((1, 24, 24), dtype=torch.uint8)] * 2, torch.zeros((1, 24, 24)), None)      # CPU tensors
