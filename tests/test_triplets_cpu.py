"""The triplets baseline without a GPU: the conditions on the float64 references, the derived bounds proven on a numpy
emulation of the kernel's arithmetic (correct arithmetic inside, seeded defects outside), the agreement of header,
exports.map and binding table, the host-side queries at the range edges, the nets' state_dict against the reference's
names and shapes, and triplets_eval's host logic against a numpy restatement of baselines/triplets.py:176-228."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import triplets_cases as tc

KEYS = ("loss", "d_a", "d_b", "d_c")
SYMBOLS = ("iic_triplets_loss", "iic_triplets_supported", "iic_triplets_workspace_bytes")


# ---- conditions on the inputs, asserted on the references alone --------------------------------------------------------
@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_autograd_form_is_finite_and_equals_the_closed_form(case):
  a, b, c = tc.inputs(case)
  r = tc.refs(case)
  auto = tc.autograd64(a, b, c)
  for key, got in zip(KEYS, auto):
    assert bool(torch.isfinite(got).all()), key
    scale = float(r[key].abs().max())
    diff = float((got - r[key]).abs().max())
    print("%s %s: |autograd - closed| / max |closed| = %.2e" % (case.name, key, diff / scale if scale else 0.0))
    assert diff <= 1e-12 * scale, (key, diff, scale)


def test_wide_row_underflows_in_fp32_only():
  assert np.exp(np.float32(-tc.WIDE_SPREAD)) == 0.0 and np.exp(-tc.WIDE_SPREAD) > 0.0
  assert np.exp(-tc.HUGE_SPREAD) == 0.0
  case = tc.CASES[2]
  a, b, c = tc.inputs(case)
  row = tc.wide_row(case)
  assert float(b[row].max() - b[row].min()) == tc.WIDE_SPREAD and float(c[row].max() - c[row].min()) == tc.WIDE_SPREAD


def test_spread_1600_torch_is_nan_where_the_closed_form_is_finite():
  """The deviation on record: float64 torch's target gradients are 0 * (-inf) = NaN once a softmax entry underflows;
  its loss and d_a agree with the closed form, which is finite everywhere."""
  a, b, c = tc.inputs(tc.HUGE_CASE)
  r = tc.closed64(a, b, c)
  loss, d_a, d_b, d_c = tc.autograd64(a, b, c)
  assert all(bool(torch.isfinite(r[key]).all()) for key in KEYS)
  assert bool(torch.isnan(d_b).any()) and bool(torch.isnan(d_c).any())
  row = tc.wide_row(tc.HUGE_CASE)
  others = [i for i in range(tc.HUGE_CASE.N) if i != row]
  assert bool(torch.isfinite(d_b[others]).all()) and bool(torch.isfinite(d_c[others]).all())
  assert abs(float(loss - r["loss"])) <= 1e-12 * abs(float(r["loss"]))
  assert float((d_a - r["d_a"]).abs().max()) <= 1e-12 * float(r["d_a"].abs().max())


# ---- the bounds: correct arithmetic inside, seeded defects outside -----------------------------------------------------
def _np(case):
  return [t.numpy() for t in tc.inputs(case)]


def _ref_tol(case):
  if case is tc.HUGE_CASE:
    a, b, c = tc.inputs(case)
    r = tc.closed64(a, b, c)
    return r, tc.bounds(a, b, c, r)
  return tc.refs(case), tc.case_bounds(case)


@pytest.mark.parametrize("case", tc.CASES + [tc.HUGE_CASE], ids=tc.case_id)
def test_emulated_kernel_arithmetic_is_inside_the_bounds(case):
  r, tol = _ref_tol(case)
  got = tc.emulate(*_np(case))
  for key in KEYS:
    w = tc.worst(got[key], r[key], tol[key])
    print("%s %s: worst |err| / bound = %.3f" % (case.name, key, w))
    assert tc.outside(got[key], r[key], tol[key]) == 0, (key, w)


@pytest.mark.parametrize("case", [c for c in tc.CASES + [tc.HUGE_CASE] if c.k > 1], ids=tc.case_id)
def test_seeded_defects_fall_outside_the_bounds(case):
  r, tol = _ref_tol(case)
  x = _np(case)

  def out(defect, rows=None):
    got = tc.emulate(*x, defect=defect, defect_rows=rows)
    return {key: tc.outside(got[key], r[key], tol[key]) for key in KEYS}
  o = out("fp32_exp")
  assert o["d_a"] > 0 and o["d_b"] > 0, o
  o = out("div_n")
  assert all(o[key] > 0 for key in KEYS), o
  o = out("sign_dc")
  assert o["d_c"] > 0 and o["loss"] == 0 and o["d_a"] == 0 and o["d_b"] == 0, o
  row = tc.wide_row(case)
  if row is not None:
    # log(softmax) in place of the log-space form, in the wide row only: fp32 loses it at spread 160, float64 at 1600
    o = out("log_exp", [row])
    assert o["d_b"] > 0 and o["d_c"] > 0, o
    o = out("log_exp64", [row])
    if case is tc.HUGE_CASE:
      assert o["d_b"] > 0 and o["d_c"] > 0, o
    else:
      assert all(o[key] == 0 for key in KEYS), o      # float64 still resolves exp(-160)


def test_constants_follow_the_sources():
  text = open(os.path.join(tc.ROOT, "iic_amd", "csrc", "triplets.hip")).read()
  assert int(re.search(r"#define TR_ROWS (\d+)", text).group(1)) == tc.ROWS_PER_WG
  assert int(re.search(r"#define TR_MAXK (\d+)", text).group(1)) == 1024
  # no flushing flag in the build: the subnormal term of the bounds is one fp32 subnormal spacing
  assert not tc.flushes_denormals() and tc.subnormal_term() == 2.0 ** -149
  n = tc.CASES[9].N
  assert tc.CASES[9].name == "wg_plus_one" and n % tc.ROWS_PER_WG == 1 and n > tc.ROWS_PER_WG


# ---- header, exports.map and binding table ---------------------------------------------------------------------------
def test_header_exports_map_and_binding_table_agree():
  import ctypes
  import fnmatch
  from iic_amd import _lib
  header = open(os.path.join(tc.ROOT, "include", "iic_hip.h")).read()
  code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
  protos = {m.group(2): (m.group(1), m.group(3)) for m in
            re.finditer(r"\b(int|long)\s+(iic_triplets_\w+)\s*\(([^;]*?)\)\s*;", code, flags=re.S)}
  assert sorted(protos) == sorted(SYMBOLS)
  ctype = {"int": ctypes.c_int, "long": ctypes.c_long}
  for name, (res, args) in protos.items():
    sig = _lib._SIGNATURES[name]
    assert name in _lib.EXPORTED_SYMBOLS
    assert sig[0] is ctype[res], name
    want = [ctypes.c_void_p if "*" in a else ctype[a.split()[0]] for a in args.split(",")]
    assert sig[1] == want, (name, sig[1], want)
  # the reference lines every entry point replaces are cited next to it
  assert "baselines/triplets.py:231-238" in header
  # exports.map: a global pattern that covers the three names and hides everything else
  emap = open(os.path.join(tc.ROOT, "iic_amd", "csrc", "exports.map")).read()
  emap = re.sub(r"/\*.*?\*/", " ", emap, flags=re.S)
  globs = [g.strip() for g in re.search(r"global:(.*?);", emap, flags=re.S).group(1).split(";") if g.strip()]
  assert all(any(fnmatch.fnmatchcase(name, g) for g in globs) for name in SYMBOLS)
  assert re.search(r"local:\s*\*\s*;", emap)
  # the Makefile compiles the source
  assert re.search(r"^SRCS =.*\btriplets\.hip\b", open(os.path.join(tc.ROOT, "iic_amd", "csrc", "Makefile")).read(), re.M)
  # and the built library exports them
  L = _lib.lib()
  for name in SYMBOLS:
    assert hasattr(L, name)


def test_supported_and_workspace_at_the_range_edges():
  from iic_amd import triplets
  for N, k in [(1, 1), (700, 10), (660, 280), (2, 1024), (2 ** 21 - 1, 1024), (2 ** 31 - 1, 1)]:
    assert triplets.supported(N, k), (N, k)
    ws = triplets.workspace_bytes(N, k)
    assert ws >= 8 * ((N + tc.ROWS_PER_WG - 1) // tc.ROWS_PER_WG) and ws % 256 == 0
  for N, k in [(1, 1025), (0, 10), (10, 0), (2 ** 21, 1024), (2 ** 31, 1), (2 ** 30, 2), (-1, 4)]:
    assert not triplets.supported(N, k), (N, k)
    assert triplets.workspace_bytes(N, k) == 0


def test_cpu_tensors_and_bad_arguments_raise_before_a_launch(monkeypatch):
  from iic_amd import _lib, triplets

  class NoLaunch(object):
    def __getattr__(self, name):
      if name == "iic_triplets_loss":
        raise AssertionError("a launch was attempted")
      return getattr(_lib.lib(), name)
  monkeypatch.setattr(triplets, "lib", lambda: NoLaunch())
  x = torch.zeros((4, 6))
  with pytest.raises(ValueError, match="no CPU fallback"):
    triplets.triplets_loss(x, x, x)
  with pytest.raises(ValueError, match="float32"):
    triplets.triplets_loss(x.double(), x.double(), x.double())
  with pytest.raises(ValueError, match="outs_orig is"):
    triplets.triplets_loss(x, x[:, :5], x)
  with pytest.raises(ValueError, match=r"\[N, k\]"):
    triplets.triplets_loss(x[0], x[0], x[0])


# ---- state_dict names and shapes ---------------------------------------------------------------------------------------
def test_state_dict_names_and_shapes_equal_the_references(golden_dir):
  from iic_amd import archs
  golden = json.load(open(os.path.join(golden_dir, "triplets_state_keys.json")))
  assert sorted(set(v["class"] for v in golden.values())) == ["TripletsNet5g", "TripletsNet6c"]
  for key, ent in sorted(golden.items()):
    net = archs.__dict__[ent["class"]](types.SimpleNamespace(**ent["config"]))
    got = [[n, list(t.shape), str(t.dtype)] for n, t in net.state_dict().items()]
    assert got == ent["state"], key
    assert "head.head.weight" in net.state_dict() and "head.head.bias" in net.state_dict()
    # the reference's initialisers: Linear weight N(0, 0.01), bias 0; BatchNorm 1 / 0
    assert float(net.head.head.bias.detach().abs().max()) == 0.0
    assert 0.005 < float(net.head.head.weight.detach().std()) < 0.02
    bn = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert all(bool((m.weight == 1).all()) and bool((m.bias == 0).all()) for m in bn)
    assert all(m.track_running_stats == ent["config"]["batchnorm_track"] for m in bn)


# ---- triplets_eval's host logic ----------------------------------------------------------------------------------------
class _FakeNet(object):
  def __init__(self):
    self.calls = []

  def eval(self):
    self.calls.append("eval")

  def train(self):
    self.calls.append("train")


def _counts_np(flat_preds, flat_targets, preds_k, targets_k):
  c = np.zeros((preds_k, targets_k), dtype=np.int64)
  np.add.at(c, (flat_preds.numpy().astype(np.int64), flat_targets.numpy().astype(np.int64)), 1)
  return c


def test_triplets_eval_host_logic_equals_the_numpy_restatement(monkeypatch):
  from iic_amd import eval_metrics, triplets
  gt_k = 4
  logits, targets = tc.eval_batches(gt_k=gt_k, sizes=(8, 8, 5))
  tie = logits[0][3]
  assert tie[1] == tie[3] == tie.max()      # one exact tie: the lower index is the prediction
  passes = []

  def fake_get_data(config, net, dataloader, sobel):
    assert net.calls[-1:] == ["eval"]      # the pass runs between net.eval() and net.train()
    lg = np.concatenate([b[0] for b in dataloader], 0)
    passes.append(lg)
    preds = torch.from_numpy(np.argmax(lg, axis=1).astype(np.int32))
    return preds, torch.from_numpy(np.concatenate([b[1] for b in dataloader], 0).astype(np.int32))
  monkeypatch.setattr(triplets, "triplets_get_data", fake_get_data)
  monkeypatch.setattr(triplets, "triplets_get_data_kmeans_on_features", fake_get_data)
  monkeypatch.setattr(eval_metrics, "_counts", _counts_np)
  config = types.SimpleNamespace(kmeans_on_features=False, output_k=gt_k, gt_k=gt_k, batch_sz=8, epoch_acc=[],
                                 masses=None, per_class_acc=None)
  net = _FakeNet()
  loader = list(zip(logits, targets))
  assert triplets.triplets_eval(config, net, loader, sobel=False) is False      # the first epoch never is best
  assert net.calls == ["eval", "train"]
  all_targets = np.concatenate(targets)
  preds = np.argmax(np.concatenate(logits, 0), axis=1)
  assert preds[3] == 1
  acc, mass, pca = tc.eval_np(preds, all_targets, gt_k)
  assert config.epoch_acc == [acc]
  assert np.array_equal(config.masses, mass) and np.array_equal(config.per_class_acc, pca)
  assert mass.sum() == 21 and config.masses.shape == (1, gt_k)
  # a second epoch whose predictions follow the targets through a permutation: better, so is_best
  better = [np.eye(gt_k, dtype=np.float32)[(t + 1) % gt_k] for t in targets]
  assert triplets.triplets_eval(config, net, list(zip(better, targets)), sobel=False) is True
  acc2, mass2, pca2 = tc.eval_np((all_targets + 1) % gt_k, all_targets, gt_k)
  assert acc2 == 1.0 and config.epoch_acc == [acc, 1.0]
  assert np.array_equal(config.masses, np.concatenate((mass, mass2), 0))
  assert np.array_equal(config.per_class_acc, np.concatenate((pca, pca2), 0))
  # a third that is no better is not best
  assert triplets.triplets_eval(config, net, list(zip(better, targets)), sobel=False) is False
  assert net.calls == ["eval", "train"] * 3
  # the arg-max branch insists on output_k == gt_k, the k-means branch does not
  config.output_k = 7
  with pytest.raises(AssertionError):
    triplets.triplets_eval(config, net, loader, sobel=False)
  net.calls.append("train")
  config.kmeans_on_features = True
  n_before = len(config.epoch_acc)
  triplets.triplets_eval(config, net, loader, sobel=False)
  assert len(config.epoch_acc) == n_before + 1 and config.masses.shape == (n_before + 1, gt_k)
