"""RandomAffine on the host side (no GPU): the numpy specification of csrc/aug_stages.h::aug_affine_bilinear equals
Pillow's own transform bit for bit on the case list the GPU test launches, that list can tell every seeded defect, and
PairedAugmenter's affine draws have the reference's distributions without disturbing the existing random stream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import augment_affine_cases as ac   # noqa: E402


@pytest.fixture(scope="module")
def evaluated():
  """Per case of every shape: (crop pixels, source image, origin, matrix, Pillow's result)."""
  out = []
  for shape in ac.SHAPES:
    crop = shape[2]
    imgs, rows = ac.shape_cases(shape)
    for r in rows:
      if r["m"] is None:
        continue
      x0, y0 = r["xy"]
      a = imgs[r["src"]][y0:y0 + crop, x0:x0 + crop]
      out.append((r["name"], a, imgs[r["src"]], r["xy"], r["m"], ac.pil_affine(a, r["m"])))
  return out


def test_specification_equals_pillow_bit_for_bit(evaluated):
  total = 0
  for name, a, _, _, m, want in evaluated:
    got = ac.np_affine_bilinear(a, m)
    assert np.array_equal(got, want), (name, a.shape, m, int((got != want).sum()))
    total += want.size
  assert total > 500000


def test_hand_made_rows_do_what_they_are_for(evaluated):
  by_name = {}
  for name, a, _, _, m, want in evaluated:
    by_name.setdefault(name, []).append((a, m, want))
  for a, m, want in by_name["identity"] + by_name["identity_draw"]:
    assert np.array_equal(want, a)
  for a, m, want in by_name["all_out"]:
    assert not want.any() and a.any()
  for a, m, want in by_name["shift_half_up"]:          # X == w exactly at the last column: zero fill there only
    assert not want[:, -1].any() and not want[-1, :].any() and want[:-1, :-1].any()
  for a, m, want in by_name["shift_int"]:
    assert np.array_equal(want[3:, :-2], a[:-3, 2:])


@pytest.mark.parametrize("defect", ac.DEFECTS)
def test_case_list_tells_each_seeded_defect(defect, evaluated):
  """What makes the GPU comparison able to fail: a kernel with this defect would differ from Pillow on the list."""
  changed = 0
  for name, a, src, xy, m, want in evaluated:
    changed += int((ac.np_affine_bilinear(a, m, defect=defect, source=src, origin=xy) != want).sum())
  print("%s: %d values change" % (defect, changed))
  assert changed >= 1, defect


def test_each_family_catches_what_the_other_cannot(evaluated):
  def count(defect, prefix):
    return sum(int((ac.np_affine_bilinear(a, m, defect=defect) != want).sum())
               for name, a, _, _, m, want in evaluated if name.startswith(prefix))
  assert count("fused_coordinates", "draw") >= 1
  assert count("fused_interpolation", "structured") >= 1


def test_identity_draw_is_exactly_the_identity():
  from iic_amd.augment import inverse_affine_matrix
  for crop in (7, 20, 36, 84):
    m = inverse_affine_matrix(ac.crop_center(crop), 0.0, (0.0, 0.0), 1.0, 0.0)
    assert tuple(m) == (1, 0, 0, 0, 1, 0), m


def test_host_matrix_equals_the_restated_formula():
  from iic_amd.augment import inverse_affine_matrix
  rng = np.random.default_rng(5)
  for crop in (20, 36, 84):
    for _ in range(50):
      p = ac.random_affine_params(rng, crop)
      assert inverse_affine_matrix(ac.crop_center(crop), *p) == ac.inverse_affine_matrix(ac.crop_center(crop), *p)


def _augmenter(**kw):
  from iic_amd.augment import PairedAugmenter
  imgs = torch.zeros((8, 40, 40, 3), dtype=torch.uint8)         # draws need no device
  return PairedAugmenter(imgs, 36, 24, True, seed=9, **kw)


def test_draw_ranges_and_share():
  from iic_amd.augment import inverse_affine_matrix
  p = 0.3
  aug = _augmenter(random_affine=True, affine_p=p)
  n = 4000
  ip, fp, mats = aug.draw(np.arange(n) % 8, "jittered")
  assert ip.shape == (n, 20) and fp.shape == (n, 4) and mats.shape == (n, 6) and mats.dtype == np.float64
  do = (ip[:, 11] & 2) != 0
  assert abs(do.mean() - p) < 4 * np.sqrt(p * (1 - p) / n)      # four standard deviations of a binomial share
  la = aug.last_affine
  assert la.shape == (n, 5) and np.isnan(la[~do]).all() and np.isfinite(la[do]).all()
  ang, tx, ty, sc, sh = la[do].T
  assert (np.abs(ang) <= 18).all() and np.abs(ang).max() > 16
  assert (tx == np.round(tx)).all() and (ty == np.round(ty)).all()            # integer-valued translations
  assert np.abs(tx).max() <= 4 and np.abs(ty).max() <= 4                       # round(U(-3.6, 3.6))
  assert set(np.unique(tx)) == set(float(v) for v in range(-4, 5))
  assert (sc >= 0.9).all() and (sc <= 1.1).all() and sc.max() - sc.min() > 0.18
  assert (np.abs(sh) <= 10).all() and np.abs(sh).max() > 9
  assert (mats[~do] == np.asarray(ac.IDENTITY)).all()
  for i in np.nonzero(do)[0][:50]:
    want = inverse_affine_matrix(ac.crop_center(36), la[i, 0], (la[i, 1], la[i, 2]), la[i, 3], la[i, 4])
    assert tuple(mats[i]) == tuple(want)
  assert (ip[:, 11] & 1 == 0).all()                             # no fluid_warp: no rotation bit


def test_without_the_keywords_the_stream_is_unchanged():
  idx = np.arange(64) % 8
  for kw in (dict(), dict(cutout=True, cutout_p=0.5, cutout_max_box=0.7),
             dict(fluid_warp=True, rot_val=25.0, rand_crop_szs_tf=[36, 30])):
    a, b = _augmenter(**kw), _augmenter(random_affine=False, affine_p=0.9, affine_degrees=30, **kw)
    for mode in ("jittered", "plain", "jittered", "center"):
      da, db = a.draw(idx, mode), b.draw(idx, mode)
      assert len(da) == len(db) == 2
      assert np.array_equal(da[0], db[0]) and np.array_equal(da[1], db[1])


def test_draw_order_affine_after_crop_before_cutout():
  """The affine consumes the stream between the crop and the cutout: crops agree with an augmenter without it, and the
  translation range follows the row's crop size under fluid_warp."""
  idx = np.arange(200) % 8
  kw = dict(fluid_warp=True, rot_val=25.0, rand_crop_szs_tf=[36, 20])
  a, b = _augmenter(**kw), _augmenter(random_affine=True, affine_p=1.0, **kw)
  (ia, _), (ib, _, mats) = a.draw(idx, "jittered"), b.draw(idx, "jittered")
  assert np.array_equal(ia[:, [1, 2, 10]], ib[:, [1, 2, 10]])
  assert np.array_equal(ia[:, 11], ib[:, 11] & 1) and (ib[:, 11] & 2 != 0).all()
  small = ib[:, 10] == b.crop_szs.index(20)
  assert small.any() and np.abs(b.last_affine[small, 1]).max() <= 2 and np.abs(b.last_affine[~small, 1]).max() > 2


def test_apply_refuses_bad_matrices_before_any_launch():
  aug = _augmenter(random_affine=True, affine_p=1.0)
  ip, fp, mats = aug.draw(np.arange(4), "jittered")
  with pytest.raises(ValueError):
    aug.apply(ip, fp)                                            # affine rows without matrices
  bad = mats.copy()
  bad[2, 2] = np.nan
  with pytest.raises(ValueError):
    aug.apply(ip, fp, bad)
  bad[2, 2] = np.inf
  with pytest.raises(ValueError):
    aug.apply(ip, fp, bad)
  with pytest.raises(ValueError):
    aug.apply(ip, fp, mats[:, :5])


class _FakeAugmenter(object):
  B = 23

  def jittered(self, idx):
    return torch.as_tensor(np.asarray(idx))


def test_train_loader_shuffles_and_keeps_the_ragged_batch():
  from iic_amd.semisup import train_loader
  targets = torch.arange(23) * 10
  loader = train_loader(_FakeAugmenter(), targets, 5, seed=1)
  assert len(loader) == 5
  epochs = []
  for _ in range(2):
    seen = []
    sizes = []
    for imgs, t in loader:
      assert torch.equal(t, imgs * 10)                           # targets[idx] of the batch's own indices
      sizes.append(len(t))
      seen += imgs.tolist()
    assert sizes == [5, 5, 5, 5, 3] and sorted(seen) == list(range(23))
    epochs.append(seen)
  assert epochs[0] != epochs[1] and epochs[0] != list(range(23))
