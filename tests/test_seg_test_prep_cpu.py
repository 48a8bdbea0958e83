"""Host logic of the test-time half of iic_amd/seg_augment.py against the reference-generated fixture
tests/golden/seg_test_prep.npz (tools/gen_golden_seg_test_prep.py: the reference's own `_prepare_test` and
`_filter_label`).  No GPU: the two 256-entry tables, the numpy restatement `prepare_test_host` (bit for bit, all three
outputs, every pixel), the mapping loader and the constructor's refusals."""
import json
import os
import types

import numpy as np
import pytest
import torch

from iic_amd import seg_augment as sa

G = os.path.join(os.path.dirname(__file__), "golden", "seg_test_prep.npz")
POTSDAM_FINE_TO_COARSE = {0: 0, 4: 0, 1: 1, 5: 1, 2: 2, 3: 2}       # potsdam.py:418-421


def _fixture():
  return np.load(G)


def _cases(g):
  for name in g["names"]:
    yield str(name), json.loads(str(g[str(name) + "/meta"]))


def _keys(g, name):
  return ["%s/%dx%d" % (name, h, w) for h, w in g["sizes"]]


def u8_labels(lab_i16):
  return (lab_i16.astype(np.int64) % 256).astype(np.uint8)         # -1 -> 255, the resident form


def filter_label_of(g, name, meta):
  """The shape of the case's `_filter_label`, restated: what it returns (labels alone / a tuple), what it does in
  place, what it starts its map from and what it refuses.  The per-class values of the two COCO dictionaries (the
  reference generates them from its class hierarchy) are read back from the fixture's table; everything else --
  -1, the entries that are no fine label, thing classes of a stuff-only set, Potsdam's assert -- is the method's."""
  table = g[name + "/targets_table"].astype(np.int8).astype(np.int32)      # low 8 bits -> signed
  kind, gt_k = meta["kind"], meta["gt_k"]
  if kind == "potsdam":
    def potsdam(label):                                              # potsdam.py:429-439
      if meta["use_coarse_labels"]:
        new = np.zeros(label.shape, dtype=label.dtype)
        for c in range(6):
          new[label == c] = POTSDAM_FINE_TO_COARSE[c]
        return new
      assert (label.max() < gt_k)
      return label
    return potsdam
  if kind == "coco_few":
    def few(label):                                                  # cocostuff.py:734-760: the map starts from zeros
      new = np.zeros(label.shape, dtype=label.dtype)
      for c in range(182):
        new[label == c] = table[c]
      return new, (new >= 0)
    return few
  first = 12 if meta["use_coarse_labels"] else 91

  def full(label):                                                   # cocostuff.py:629-656: subtracts in place
    if meta["use_coarse_labels"]:
      new = np.zeros(label.shape, dtype=label.dtype)                 # _fine_to_coarse (:605-615), from zeros too
      for c in range(182):
        new[label == c] = table[c] + first
      label = new
    mask = (label >= first)
    label -= first
    return label, mask
  return full


def test_tables_match_the_reference_for_every_case():
  g = _fixture()
  kinds = set()
  for name, meta in _cases(g):
    fl = filter_label_of(g, name, meta)
    t = sa.label_table(fl)
    assert t.dtype == np.uint8 and t.shape == (256,) and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t, g[name + "/targets_table"]), name
    if meta["kind"] == "potsdam":
      assert name + "/relevance" not in g.files                      # potsdam.py:342: the mask is all ones
    else:
      assert np.array_equal(sa.relevance_table(fl), g[name + "/relevance"]), name
    kinds.add((meta["kind"], meta["gt_k"]))
  assert kinds >= {("potsdam", 3), ("potsdam", 6), ("coco_few", 3), ("coco_full", 91)}


def test_table_values_the_reference_documents():
  g = _fixture()
  by = {n: (g[n + "/targets_table"], g[n + "/relevance"] if n + "/relevance" in g.files else None) for n, _ in _cases(g)}
  t, _ = by["potsdam_coarse_nosobel"]
  assert list(t[:6]) == [0, 1, 2, 2, 0, 1] and not t[6:].any()       # everything else stays in the zero map
  t, _ = by["potsdam_fine_sobel_rgb"]
  assert list(t[:6]) == [0, 1, 2, 3, 4, 5] and (t[6:182] == 255).all()      # refused by the reference's assert
  assert (t[182:] == 255).all()                                      # -1 passes the assert unchanged
  t, r = by["coco_fine_nosobel"]
  assert np.array_equal(t[:182], (np.arange(182) - 91) & 255) and (t[182:] == ((-1 - 91) & 255)).all()
  assert not r[:91].any() and r[91:182].all() and not r[182:].any()
  t, r = by["coco_few_sobel"]
  assert (t[182:] == 0).all() and (r[182:] == 1).all()               # the quirk: -1 is class 0 with mask 1
  assert set(t[:182]) == {0, 1, 2, 255} and np.array_equal(r[:182], (t[:182] != 255).astype(np.uint8))
  if "coco_coarse_sobel_rgb" in by:
    t, r = by["coco_coarse_sobel_rgb"]
    assert (t[182:] == ((0 - 12) & 255)).all() and not r[182:].any()        # _fine_to_coarse: -1 falls to coarse 0
    assert set(t[91:182]) == set(range(15)) and r[91:182].all() and not r[:91].any()


def test_prepare_test_host_matches_the_fixture_bit_for_bit():
  g = _fixture()
  layouts, n = set(), 0
  for name, meta in _cases(g):
    cfg = meta["config"]
    ttab = g[name + "/targets_table"]
    rel = g[name + "/relevance"] if meta["kind"] != "potsdam" else None
    for key in _keys(g, name):
      imgs, labs = g[key + "/images"], u8_labels(g[key + "/labels"])
      for i in range(imgs.shape[0]):
        img, tgt, mask = sa.prepare_test_host(imgs[i], labs[i], cfg["input_sz"], cfg["no_sobel"], cfg["include_rgb"],
                                              ttab, rel)
        want = g[key + "/imgs"][i]
        assert img.dtype == np.float32 and img.shape == want.shape, key
        assert img.tobytes() == want.tobytes(), (key, i, float(np.abs(img - want).max()))
        assert tgt.dtype == np.uint8 and np.array_equal(tgt, g[key + "/targets"][i].astype(np.uint8)), (key, i)
        assert mask.dtype == np.uint8 and np.array_equal(mask, g[key + "/mask"][i]), (key, i)
        layouts.add(img.shape[0])
        n += 1
  assert layouts == {1, 2, 3, 4, 5} and n == len(g["names"]) * len(g["sizes"]) * 2


def test_fixture_covers_what_the_kernel_must_get_right():
  g = _fixture()
  assert [tuple(s) for s in g["sizes"]] == [(24, 24), (32, 32), (37, 37), (48, 48), (24, 48), (48, 24)]
  for name, meta in _cases(g):
    if meta["kind"] == "potsdam":
      continue
    labs = np.concatenate([g[k + "/labels"].ravel() for k in _keys(g, name)])
    assert (labs == -1).any() and ((labs >= 0) & (labs <= 90)).any() and (labs >= 91).any(), name
    masks = np.concatenate([g[k + "/mask"].ravel() for k in _keys(g, name)])
    assert set(np.unique(masks)) == {0, 1}, name
    tg = np.concatenate([g[k + "/targets"].ravel() for k in _keys(g, name)])
    if meta["kind"] == "coco_full":
      assert (tg < 0).any(), name                                    # the reference leaves negatives where masked out


def _cfg(**kw):
  c = dict(input_sz=32, no_sobel=True, include_rgb=False, pre_scale_all=False, mask_input=False)
  c.update(kw)
  return types.SimpleNamespace(**c)


def _prep(B=11, H=40, W=40, cs=4, cfg=None, **kw):
  return sa.SegTestPreparer(torch.zeros(B, H, W, cs, dtype=torch.uint8), torch.zeros(B, H, W, dtype=torch.uint8),
                            cfg or _cfg(), np.arange(256, dtype=np.uint8), **kw)


def test_constructor_refusals():
  with pytest.raises(NotImplementedError, match="multiple of 4"):
    _prep(cfg=_cfg(input_sz=30))
  with pytest.raises(AssertionError):
    _prep(cfg=_cfg(mask_input=True))
  with pytest.raises(NotImplementedError, match="pre_scale_all"):
    _prep(cfg=_cfg(pre_scale_all=True), prescaled=False)
  _prep(cfg=_cfg(pre_scale_all=True))                                # the resident arrays are the pre-scaled ones
  ok = np.tile(np.array([[40, 17]]), (11, 1))
  assert _prep(sizes=ok).sizes.dtype == torch.int32
  for bad in ([41, 17], [40, 41], [0, 17], [40, -3]):
    sz = ok.copy()
    sz[5] = bad
    with pytest.raises(ValueError, match="sizes out of range"):
      _prep(sizes=sz)
  with pytest.raises(ValueError, match="one .h, w. per image"):
    _prep(sizes=ok[:10])
  with pytest.raises(AssertionError):
    sa.SegTestPreparer(torch.zeros(2, 40, 40, 3, dtype=torch.uint8), torch.zeros(2, 40, 41, dtype=torch.uint8), _cfg(),
                       np.arange(256, dtype=np.uint8))
  with pytest.raises(AssertionError):
    _prep(relevance=np.ones(255, np.uint8))
  p = _prep()
  assert p.out_channels == 4 and _prep(cs=3, cfg=_cfg(no_sobel=False)).out_channels == 1
  with pytest.raises(AssertionError, match="out of range"):
    p.batch([0, 11])                                                 # refused on the host, never launched
  with pytest.raises(AssertionError, match="out of range"):
    p.batch([-1])
  with pytest.raises(AssertionError, match="resident on the GPU"):
    p.batch([0, 1])                                                  # no CPU path


def test_mapping_loader_length_order_and_ragged_last_batch():
  p = _prep()
  calls = []

  def stub_batch(idx):
    calls.append(list(idx))
    n = len(idx)
    return torch.zeros(n, 4, 32, 32), torch.zeros(n, 32, 32, dtype=torch.uint8), torch.ones(n, 32, 32, dtype=torch.uint8)
  p.batch = stub_batch
  loader = sa.seg_mapping_dataloader(p, 4)
  assert len(loader) == 3
  for _ in range(2):                                                 # re-iterable, as a DataLoader is every epoch
    del calls[:]
    shapes = [(imgs.shape[0], t.shape[0], m.shape[0]) for imgs, t, m in loader]
    assert shapes == [(4, 4, 4), (4, 4, 4), (3, 3, 3)]
    assert calls == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]
  assert len(sa.seg_mapping_dataloader(p, 11)) == 1 and len(sa.seg_mapping_dataloader(p, 12)) == 1


def test_exported_from_the_package():
  import iic_amd
  assert iic_amd.SegTestPreparer is sa.SegTestPreparer
  assert iic_amd.seg_mapping_dataloader is sa.seg_mapping_dataloader
