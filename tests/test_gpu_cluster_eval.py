"""Clustering evaluation on the device (csrc/eval_metrics.hip::cluster_argmax_acc_kernel, iic_amd/cluster_eval.py): the
arg-max + count kernel through the C ABI (iic_cluster_argmax_acc) against torch.argmax, numpy and iic_contingency; ties
and non-finite rows; the accumulation contract; cluster_subheads_eval / cluster_eval / _clustering_get_data against the
reference's flat-array flow assembled by hand on iic_amd.eval_metrics; the real nets' outputs read in place; and
get_subhead_using_loss against the reference's `+= loss.item()` loop.  Every comparison is exact.  pytest -m gpu."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, H, k, gt_k): k below, at and above one / several lane strides of 64; row counts that do not fill a workgroup
CASES = [(1, 1, 1, 1), (7, 1, 3, 3), (33, 5, 10, 10), (65, 5, 70, 10), (130, 2, 140, 20), (50, 3, 280, 20),
         (257, 1, 64, 64)]
LAYOUTS = ["packed", "padded", "list"]


def dev():
  return torch.device("cuda:0")


def _call(probs_ptr, ld, hs, n, H, k, targets, gt_k, counts, labels, label_stride):
  from iic_amd._lib import lib, stream_ptr
  return lib().iic_cluster_argmax_acc(probs_ptr, ld, hs, n, H, k, None if targets is None else targets.data_ptr(), gt_k,
                                      None if counts is None else counts.data_ptr(),
                                      None if labels is None else labels.data_ptr(), label_stride, stream_ptr())


def _np_counts(preds, targets, k, gt_k):
  """preds [H][n], targets [n] (any integers) -> (int64 [H][k][gt_k], n)."""
  ok = (targets >= 0) & (targets < gt_k)
  c = np.zeros((preds.shape[0], k, gt_k), np.int64)
  for h in range(preds.shape[0]):
    np.add.at(c[h], (preds[h][ok].astype(np.int64), targets[ok].astype(np.int64)), 1)
  return c, int(targets.shape[0])


@functools.lru_cache(maxsize=None)
def _case(n, H, k, gt_k):
  """(host softmax outputs [n][H][k] fp32, host targets int64 [n]) -- made once a case; quantised so that ties occur."""
  rng = np.random.default_rng(1000 * k + n)
  x = torch.softmax(torch.from_numpy(rng.standard_normal((n, H, k)).astype(np.float32)) * 2, dim=2).numpy()
  x = np.round(x * 64).astype(np.float32) / 64          # many equal maxima: the first index must win
  t = rng.integers(0, gt_k, n).astype(np.int64)
  x.setflags(write=False)
  t.setflags(write=False)
  return x, t


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,H,k,gt_k", CASES)
def test_argmax_and_counts_vs_numpy(n, H, k, gt_k, layout):
  from iic_amd import cluster_eval
  from iic_amd._lib import check, lib, stream_ptr
  x, t = _case(n, H, k, gt_k)
  dt = torch.tensor(t).to(dev())
  if layout == "packed":
    dx = torch.tensor(x).to(dev())
    heads = [dx[:, h, :] for h in range(H)]
    src, ld, hs = dx.data_ptr(), H * k, k
  elif layout == "padded":
    ld = H * k + 5
    buf = torch.full((n, ld), float("nan"), device=dev())           # the padding must never be read: NaN would win
    buf[:, :H * k] = torch.tensor(x).to(dev()).view(n, H * k)
    dx = buf.as_strided((n, H, k), (ld, k, 1))
    heads = [dx[:, h, :] for h in range(H)]
    src, hs = buf.data_ptr(), k
  else:
    heads = [torch.tensor(x[:, h, :]).to(dev()) for h in range(H)]                  # separate allocations
  want = np.stack([x[:, h, :].argmax(axis=1) for h in range(H)])                                   # [H][n]
  for h in range(H):
    assert np.array_equal(torch.argmax(heads[h], dim=1).cpu().numpy(), want[h])
  want_counts, _ = _np_counts(want, t, k, gt_k)

  if layout == "list":
    # the wrapper's stack path: labels through _clustering_get_data's launch, counts through the accumulator
    labels = torch.full((H, n + 3), -7, dtype=torch.int32, device=dev())
    got = cluster_eval._argmax_acc(heads, None, 0, None, labels, 1, n + 3)
    assert got == (n, H, k)
    if H > 1:
      assert cluster_eval._rows(heads)[1] not in [a.data_ptr() for a in heads]                     # stacked once
    acc = cluster_eval.ClusterEvalAccumulator(H, k, gt_k, dev())
    acc.add(heads, dt)
    counts, total = acc.counts()
    lab = labels.cpu().numpy()
    assert np.array_equal(lab[:, 1:n + 1], want) and (lab[:, 0] == -7).all() and (lab[:, n + 1:] == -7).all()
  else:
    labels = torch.full((H, n + 3), -7, dtype=torch.int32, device=dev())
    cbuf = torch.zeros((H, k * gt_k + 1), dtype=torch.long, device=dev())
    check(_call(src, ld, hs, n, H, k, dt, gt_k, cbuf, labels, n + 3), "iic_cluster_argmax_acc")
    lab = labels.cpu().numpy()
    assert np.array_equal(lab[:, :n], want) and (lab[:, n:] == -7).all()
    host = cbuf.cpu().numpy()
    counts, total = host[:, :-1].reshape(H, k, gt_k), int(host[0, -1])
    assert (host[:, -1] == n).all()
    # the wrapper on the same memory: views of one storage are read in place
    acc = cluster_eval.ClusterEvalAccumulator(H, k, gt_k, dev())
    acc.add(heads, dt)
    assert cluster_eval._rows(heads)[1:4] == (src, ld, hs if H > 1 else 0)
    c2, n2 = acc.counts()
    assert np.array_equal(c2, want_counts) and n2 == n
  assert counts.dtype == np.int64 and np.array_equal(counts, want_counts) and total == n
  # the existing contingency kernel on the widened labels
  for h in range(H):
    old = torch.empty((k, gt_k), dtype=torch.long, device=dev())
    wp = torch.from_numpy(want[h].astype(np.int64)).to(dev())
    check(lib().iic_contingency(wp.data_ptr(), dt.data_ptr(), n, k, gt_k, old.data_ptr(), stream_ptr()), "iic_contingency")
    assert np.array_equal(old.cpu().numpy(), counts[h])


def test_ties_and_non_finite_rows():
  """torch's and numpy's rule for every input: the first maximal index wins, a NaN counts as maximal, the first NaN
  wins (seg_label_map_kernel's strict `>` differs on NaN)."""
  from iic_amd._lib import check
  k = 140
  nan, inf = float("nan"), float("inf")
  rng = np.random.default_rng(3)
  rows, want = [], []

  def base():
    return (rng.random(k) * 0.5).astype(np.float32)
  for a, b in ((3, 67), (0, 139), (64, 128)):           # equal maxima: within a lane's stride, across lanes, across both
    r = base()
    r[a] = r[b] = 0.75
    rows.append(r)
    want.append(a)
  rows.append(np.full(k, 1.0 / k, np.float32)); want.append(0)                  # noqa: E702   all equal
  r = base(); r[5] = nan; r[100] = 3.0; r[2] = 2.0; rows.append(r); want.append(5)      # noqa: E702   NaN beats larger finite values
  r = base(); r[70] = nan; r[9] = nan; rows.append(r); want.append(9)           # noqa: E702   first NaN
  r = base(); r[77] = inf; r[13] = inf; rows.append(r); want.append(13)         # noqa: E702   first +inf
  rows.append(np.full(k, -inf, np.float32)); want.append(0)                     # noqa: E702   all -inf
  r = base(); r[:] = -1.0; r[66] = -0.0; r[130] = 0.0; rows.append(r); want.append(66)  # noqa: E702   -0.0 == 0.0
  x = np.stack(rows)
  n = x.shape[0]
  dx = torch.from_numpy(x).to(dev())
  labels = torch.full((n,), -1, dtype=torch.int32, device=dev())
  check(_call(dx.data_ptr(), k, k, n, 1, k, None, 0, None, labels, n), "iic_cluster_argmax_acc")
  got = labels.cpu().numpy()
  assert np.array_equal(got, np.array(want))
  assert np.array_equal(got, torch.argmax(dx, dim=1).cpu().numpy())
  assert np.array_equal(got, np.argmax(x, axis=1))


def test_accumulation_contract():
  from iic_amd._lib import check
  H, k, gt_k = 3, 10, 4
  rng = np.random.default_rng(5)
  parts = []
  cbuf = torch.zeros((H, k * gt_k + 1), dtype=torch.long, device=dev())
  for n in (37, 6):
    x = rng.random((n, H, k)).astype(np.float32)
    t = rng.integers(-1, gt_k + 1, n).astype(np.int64)              # -1 and gt_k: counted in the last cell only
    t[0], t[-1] = -1, gt_k
    parts.append((x, t))
    dx, dt = torch.from_numpy(x).to(dev()), torch.from_numpy(t).to(dev())
    check(_call(dx.data_ptr(), H * k, k, n, H, k, dt, gt_k, cbuf, None, 0), "iic_cluster_argmax_acc")     # counts only
  x, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
  preds = np.stack([x[:, h, :].argmax(axis=1) for h in range(H)])
  want, n_all = _np_counts(preds, t, k, gt_k)
  got = cbuf.cpu().numpy()
  assert np.array_equal(got[:, :-1].reshape(H, k, gt_k), want) and (got[:, -1] == n_all).all()
  assert int(want[0].sum()) == int(((t >= 0) & (t < gt_k)).sum()) < n_all

  # out-of-range targets alone raise only the last cell
  before = got
  dx = torch.from_numpy(x[:2]).to(dev())
  dt = torch.tensor([-1, gt_k], dtype=torch.long, device=dev())
  check(_call(dx.data_ptr(), H * k, k, 2, H, k, dt, gt_k, cbuf, None, 0), "iic_cluster_argmax_acc")
  after = cbuf.cpu().numpy()
  assert np.array_equal(after[:, :-1], before[:, :-1]) and (after[:, -1] == before[:, -1] + 2).all()

  # n == 0: IIC_OK, nothing written
  labels = torch.full((H, 4), -3, dtype=torch.int32, device=dev())
  assert _call(dx.data_ptr(), H * k, k, 0, H, k, dt, gt_k, cbuf, labels, 4) == 0
  # both outputs NULL, counts without targets: IIC_ERR_ARG, nothing launched
  assert _call(dx.data_ptr(), H * k, k, 2, H, k, dt, gt_k, None, None, 0) == -1
  assert _call(dx.data_ptr(), H * k, k, 2, H, k, None, gt_k, cbuf, labels, 4) == -1
  assert np.array_equal(cbuf.cpu().numpy(), after) and bool((labels == -3).all())
  # labels only
  check(_call(dx.data_ptr(), H * k, k, 2, H, k, None, 0, None, labels, 4), "iic_cluster_argmax_acc")
  lab = labels.cpu().numpy()
  assert np.array_equal(lab[:, :2], preds[:, :2]) and (lab[:, 2:] == -3).all()
  assert np.array_equal(cbuf.cpu().numpy(), after)


def test_mismatched_sizes_raise_before_the_launch():
  """The C entry cannot know the size of counts, targets or labels: the wrappers hold (n, H, k) against them and raise
  before anything is enqueued -- the count buffer and the memory on both sides of it stay as they were."""
  from iic_amd import cluster_eval
  H, k, gt_k, n = 2, 6, 3, 9
  rng = np.random.default_rng(11)

  def heads(h, kk, rows=n):
    return [torch.from_numpy(rng.random((rows, kk)).astype(np.float32)).to(dev()) for _ in range(h)]
  t = torch.from_numpy(rng.integers(0, gt_k, n).astype(np.int64)).to(dev())
  acc = cluster_eval.ClusterEvalAccumulator(H, k, gt_k, dev())
  guard = torch.zeros((H + 4, k * gt_k + 1), dtype=torch.long, device=dev())      # the buffer with two rows on each side
  acc.buf = guard[2:2 + H]
  acc.add(heads(H, k), t)
  before = guard.cpu().numpy().copy()
  assert (before[2:2 + H, -1] == n).all() and not before[:2].any() and not before[2 + H:].any()
  for bad_outs, bad_t in ((heads(H + 1, k), t),                     # more sub-heads than the buffer has rows
                          (heads(H - 1, k), t),
                          (heads(H, k + 1), t),                     # a larger k: bins past a row's end
                          (heads(H, k - 1), t),
                          (torch.stack(heads(H + 2, k), dim=1), t), # the packed form
                          (heads(H, k), t[:n - 1]),                 # targets shorter than the rows: a read out of bounds
                          (heads(H, k), torch.cat([t, t])),
                          (heads(H, k, rows=n + 1), t)):
    with pytest.raises(ValueError):
      acc.add(bad_outs, bad_t)
  torch.cuda.synchronize()
  assert np.array_equal(guard.cpu().numpy(), before)
  c, total = acc.counts()
  assert total == n and int(c.sum()) == H * n

  # the labels output: a buffer that cannot hold H rows of n at the offset
  labels = torch.full((H, n + 2), -7, dtype=torch.int32, device=dev())
  for off, stride, outs in ((3, n + 2, heads(H, k)),                # offset + n past a row
                            (0, n + 2, heads(H + 1, k)),            # a row past the buffer
                            (0, n - 1, heads(H, k)),                # rows that overlap
                            (-1, n + 2, heads(H, k))):
    with pytest.raises(ValueError):
      cluster_eval._argmax_acc(outs, None, 0, None, labels, off, stride)
  with pytest.raises(ValueError):
    cluster_eval._argmax_acc(heads(H, k), None, 0, None, labels, 0, n + 2, expect=(H, k + 1))
  assert bool((labels == -7).all())

  # _clustering_get_data: a net with more sub-heads than the config names, and a batch whose targets are short
  net, assign, _ = _stub_setup(H + 1, k, gt_k, seed=13)
  config = _config(H, k, gt_k, "orig", "IID")
  with pytest.raises(ValueError):
    cluster_eval._clustering_get_data(config, net, assign, sobel=False)
  with pytest.raises(ValueError):
    cluster_eval.cluster_subheads_eval(config, net, assign, assign, sobel=False)
  net, assign, _ = _stub_setup(H, k, gt_k, seed=13)
  short = [(imgs, targets[:-1]) for imgs, targets in assign]
  with pytest.raises(AssertionError):
    cluster_eval._clustering_get_data(config, net, short, sobel=False)
  with pytest.raises(ValueError):
    cluster_eval.cluster_subheads_eval(config, net, short, short, sobel=False)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: a stub net that returns fixed device softmax lists
# ---------------------------------------------------------------------------------------------------------------------
class _StubNet(torch.nn.Module):
  """Maps each batch (recognised by its first pixel) to a fixed list of separately allocated [n, k] softmax tensors."""

  def __init__(self, table):
    super(_StubNet, self).__init__()
    self.table = table
    self.calls = []

  def forward(self, x, head="B"):
    self.calls.append(self.training)
    return [t.clone() for t in self.table[int(x.reshape(-1)[0].item())]]


def _stub_setup(H, k, gt_k, seed, sizes_assign=(4, 4, 3), sizes_test=(4, 2)):
  rng = np.random.default_rng(seed)
  table, loaders, key = {}, [], 0
  for sizes in (sizes_assign, sizes_test):
    loader = []
    for b in sizes:
      imgs = torch.full((b, 1, 2, 2), float(key))
      targets = torch.from_numpy(rng.integers(0, gt_k, b).astype(np.int64))
      outs = torch.softmax(torch.from_numpy(rng.standard_normal((H, b, k)).astype(np.float32)) * 2, dim=2)
      table[key] = [outs[h].contiguous().to(dev()) for h in range(H)]
      loader.append((imgs, targets))
      key += 1
    loaders.append(loader)
  return _StubNet(table), loaders[0], loaders[1]


def _ref_get_data(config, net, loader):
  """cluster_eval.py:23-67 as the reference writes it: per-sub-head torch.argmax slice-assigned into flat int32 arrays."""
  nb = len(loader)
  ft = torch.zeros(nb * config.batch_sz, dtype=torch.int32).cuda()
  fp = [torch.zeros(nb * config.batch_sz, dtype=torch.int32).cuda() for _ in range(config.num_sub_heads)]
  soft = [torch.zeros((nb * config.batch_sz, config.output_k), dtype=torch.float32).cuda()
          for _ in range(config.num_sub_heads)]
  num = 0
  for b_i, batch in enumerate(loader):
    with torch.no_grad():
      x_outs = net(batch[0].cuda())
    cur = batch[1].shape[0]
    num += cur
    s = b_i * config.batch_sz
    for i in range(config.num_sub_heads):
      fp[i][s:s + cur] = torch.argmax(x_outs[i], dim=1)
      soft[i][s:s + cur, :] = x_outs[i]
    ft[s:s + cur] = batch[1].cuda()
  return [p[:num] for p in fp], ft[:num], [s[:num] for s in soft]


def _by_hand(config, net, assign, test, use_sub_head=None):
  """cluster_subheads_eval (cluster_eval.py:101-145, :187-228) on the flat arrays, with the package's drop-in matchers
  and the reference's reorder loop."""
  from iic_amd import eval_metrics
  matcher = eval_metrics._hungarian_match if config.eval_mode == "hung" else eval_metrics._original_match

  def reordered_acc(preds, targets, match):
    r = torch.zeros(targets.shape[0], dtype=preds.dtype).cuda()
    for pred_i, target_i in match:
      r[preds == pred_i] = target_i
    return eval_metrics._acc(r, targets, config.gt_k, verbose=0)

  preds, targets, _ = _ref_get_data(config, net, assign)
  matches, train_accs = [], np.zeros(config.num_sub_heads, dtype=np.float32)
  for i in range(config.num_sub_heads):
    matches.append(matcher(preds[i], targets, preds_k=config.output_k, targets_k=config.gt_k))
    train_accs[i] = reordered_acc(preds[i], targets, matches[i])
  best = np.argmax(train_accs)
  if config.num_sub_heads > 1 and use_sub_head is not None:
    best = use_sub_head
  if config.mode == "IID":
    test_accs = train_accs
  else:
    preds, targets, _ = _ref_get_data(config, net, test)
    test_accs = np.zeros(config.num_sub_heads, dtype=np.float32)
    for i in range(config.num_sub_heads):
      test_accs[i] = reordered_acc(preds[i], targets, matches[i])
  return {"test_accs": list(test_accs), "avg": np.mean(test_accs), "std": np.std(test_accs), "best": test_accs[best],
          "worst": test_accs.min(), "best_train_sub_head": best, "best_train_sub_head_match": matches[best],
          "train_accs": list(train_accs)}


def _same_dict(got, want):
  assert set(got) == set(want)
  for key in ("test_accs", "train_accs"):
    assert all(type(v) is np.float32 for v in got[key])
    assert np.array(got[key]).tobytes() == np.array(want[key]).tobytes(), (key, got[key], want[key])
  for key in ("avg", "std", "best", "worst"):
    assert type(got[key]) is type(want[key]) and np.asarray(got[key]).tobytes() == np.asarray(want[key]).tobytes(), key
  assert int(got["best_train_sub_head"]) == int(want["best_train_sub_head"])
  assert got["best_train_sub_head_match"] == want["best_train_sub_head_match"]


def _config(H, k, gt_k, eval_mode, mode, **kw):
  c = dict(num_sub_heads=H, output_k=k, gt_k=gt_k, batch_sz=4, eval_mode=eval_mode, mode=mode, include_rgb=False,
           mapping_assignment_partitions=["a"], mapping_test_partitions=["a"], epoch_stats=[], epoch_acc=[],
           epoch_avg_subhead_acc=[], double_eval=False, double_eval_stats=[], double_eval_acc=[],
           double_eval_avg_subhead_acc=[])
  c.update(kw)
  return types.SimpleNamespace(**c)


@pytest.mark.parametrize("use_sub_head", [None, 1])
@pytest.mark.parametrize("mode", ["IID", "IID+"])
@pytest.mark.parametrize("eval_mode,k", [("orig", 6), ("hung", 3)])
def test_cluster_subheads_eval_end_to_end(eval_mode, k, mode, use_sub_head):
  from iic_amd import cluster_eval
  H, gt_k = 3, 3
  net, assign, test = _stub_setup(H, k, gt_k, seed=17 + k)
  config = _config(H, k, gt_k, eval_mode, mode)
  got = cluster_eval.cluster_subheads_eval(config, net, assign, test, sobel=False, use_sub_head=use_sub_head)
  want = _by_hand(config, net, assign, test, use_sub_head=use_sub_head)
  _same_dict(got, want)
  if use_sub_head is not None:
    assert got["best_train_sub_head"] == use_sub_head

  def own(config, net, loader, sobel=False, using_IR=False, verbose=0):
    return _ref_get_data(config, net, loader)[:2]
  # a caller's own get_data_fn: the flat-array flow, same dict
  _same_dict(cluster_eval.cluster_subheads_eval(config, net, assign, test, sobel=False, get_data_fn=own,
                                                use_sub_head=use_sub_head), want)


@pytest.mark.parametrize("double_eval", [False, True])
def test_cluster_eval_bookkeeping(double_eval):
  from iic_amd import cluster_eval
  H, k, gt_k = 3, 6, 3
  net, assign, test = _stub_setup(H, k, gt_k, seed=29)
  config = _config(H, k, gt_k, "orig", "IID+", double_eval=double_eval)
  want = _by_hand(config, net, assign, test)
  net.train()
  del net.calls[:]
  assert cluster_eval.cluster_eval(config, net, assign, test, sobel=False) is False          # no accuracy so far
  assert net.training
  nb = len(assign) + len(test)
  # the double_eval pass runs in whatever mode the net was in (train), the main pass in eval mode
  assert net.calls == ([True] * nb if double_eval else []) + [False] * nb
  assert len(config.epoch_stats) == 1 and config.epoch_acc == [want["best"]]
  assert config.epoch_avg_subhead_acc == [want["avg"]]
  _same_dict(config.epoch_stats[0], want)
  if double_eval:
    assert len(config.double_eval_stats) == 1 and config.double_eval_acc == [want["best"]]
    assert config.double_eval_avg_subhead_acc == [want["avg"]]
    _same_dict(config.double_eval_stats[0], want)
  else:
    assert config.double_eval_stats == [] and config.double_eval_acc == []
  # is_best: against the accuracies so far
  config.epoch_acc[0] = -1.0
  assert bool(cluster_eval.cluster_eval(config, net, assign, test, sobel=False)) is True
  config.epoch_acc[:] = [2.0]
  assert bool(cluster_eval.cluster_eval(config, net, assign, test, sobel=False)) is False
  assert len(config.epoch_stats) == 3
  # print_stats: nothing appended, nothing returned
  assert cluster_eval.cluster_eval(config, net, assign, test, sobel=False, print_stats=True) is None
  assert len(config.epoch_stats) == 3 and len(config.double_eval_stats) == (3 if double_eval else 0)


def test_clustering_get_data_equals_reference_flow():
  from iic_amd import cluster_eval
  H, k, gt_k = 3, 6, 3
  net, assign, _ = _stub_setup(H, k, gt_k, seed=31)
  config = _config(H, k, gt_k, "orig", "IID")
  rp, rt, rs = _ref_get_data(config, net, assign)
  preds, targets = cluster_eval._clustering_get_data(config, net, assign, sobel=False)
  assert len(preds) == H and targets.dtype == torch.int32 and torch.equal(targets, rt)
  for i in range(H):
    assert preds[i].dtype == torch.int32 and preds[i].shape == rt.shape and torch.equal(preds[i], rp[i])
  preds, targets, soft = cluster_eval._clustering_get_data(config, net, assign, sobel=False, get_soft=True)
  assert torch.equal(targets, rt) and len(soft) == H
  for i in range(H):
    assert torch.equal(preds[i], rp[i]) and torch.equal(soft[i], rs[i])


# ---------------------------------------------------------------------------------------------------------------------
# the real nets: their head outputs are views of one packed tensor and are read in place
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["5g_two_head_A", "5g_two_head_B", "6c"])
def test_real_net_outputs_are_read_in_place(which):
  from iic_amd import archs, cluster_eval
  torch.manual_seed(7)
  if which == "6c":
    cfg = types.SimpleNamespace(in_channels=1, input_sz=24, batchnorm_track=True, num_sub_heads=2, output_k=10)
    net, kw, H, k = archs.ClusterNet6c(cfg), {}, 2, 10
    x = torch.rand(12, 1, 24, 24)
  else:
    cfg = types.SimpleNamespace(in_channels=2, input_sz=32, batchnorm_track=True, num_sub_heads=3, output_k_A=20,
                                output_k_B=10)
    net, head = archs.ClusterNet5gTwoHead(cfg), which[-1]
    kw, H, k = dict(head=head), 3, (20 if head == "A" else 10)
    x = torch.rand(8, 2, 32, 32)
  net.to(dev()).eval()
  gt_k = 10
  t = torch.from_numpy(np.random.default_rng(1).integers(0, gt_k, x.shape[0]).astype(np.int64)).to(dev())
  with torch.no_grad():
    outs = net(x.to(dev()), **kw)
  assert len(outs) == H and tuple(outs[0].shape) == (x.shape[0], k)
  keep, p, ld, hs, n, h2, k2 = cluster_eval._rows(outs)
  assert keep is outs[0] and p == outs[0].data_ptr() and (ld, hs, n, h2, k2) == (H * k, k, x.shape[0], H, k)   # no stack
  acc = cluster_eval.ClusterEvalAccumulator(H, k, gt_k, dev())
  acc.add(outs, t)
  counts, total = acc.counts()
  preds = np.stack([o.cpu().numpy().argmax(axis=1) for o in outs])
  want, _ = _np_counts(preds, t.cpu().numpy(), k, gt_k)
  assert np.array_equal(counts, want) and total == x.shape[0]
  with pytest.raises(AssertionError):
    acc.add([o.cpu() for o in outs], t.cpu())                       # CPU tensors: no fallback


def test_get_subhead_using_loss_equals_reference_sums():
  from iic_amd import cluster_eval
  from iic_amd.losses import IID_loss
  H, k, lamb = 3, 10, 1.5
  rng = np.random.default_rng(41)
  table, loader_a, loader_b = {}, [], []
  for key, b in ((0, 6), (1, 6), (2, 4), (3, 4)):                   # keys 0, 2: plain batches; 1, 3: their transformed twins
    outs = torch.softmax(torch.from_numpy(rng.standard_normal((H, 2 * b, k)).astype(np.float32)) * 2, dim=2)
    table[key] = [outs[h].contiguous().to(dev()) for h in range(H)]
    (loader_a if key % 2 == 0 else loader_b).append((torch.full((b, 1, 2, 2), float(key)),))
  net = _StubNet(table)
  config = types.SimpleNamespace(num_sub_heads=H, in_channels=1, batch_sz=12, input_sz=2, num_dataloaders=2,
                                 include_rgb=False)
  loaders = [loader_a, loader_b, loader_b]                          # num_dataloaders = 2 transformed loaders
  # the reference's loop (cluster_eval.py:245-293): one host read per sub-head and batch
  want = np.zeros(H)
  for key in (0, 2):
    for i in range(H):
      with torch.no_grad():
        loss, _ = IID_loss(table[key][i], table[key + 1][i], lamb=lamb)
      want[i] += loss.item()
  net.eval()
  sums = cluster_eval._subhead_loss_sums(config, loaders, net, sobel=False, lamb=lamb)
  assert sums.dtype == np.float64 and sums.tobytes() == want.tobytes(), (sums, want)
  net.train()
  del net.calls[:]
  best = cluster_eval.get_subhead_using_loss(config, loaders, net, sobel=False, lamb=lamb)
  assert net.training and net.calls == [False] * 4
  assert int(best) == int(np.argmin(want))
