"""csrc/augment_affine.hip (iic_augment_affine) against Pillow: RandomAffine of sobel_make_transforms
(code/utils/cluster/transforms.py:152-161) between the crop and the cutout / Resize, every float32 output equal to the
composed PIL oracle of tests/augment_affine_cases.py for the same parameters -- no tolerance, no exclusions."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import augment_affine_cases as ac   # noqa: E402
from augment_affine_cases import ao   # noqa: E402

pytestmark = pytest.mark.gpu

IIC_ERR_ARG, IIC_ERR_UNSUPPORTED = -1, -3


def _launch(aug, ip, fp, ap, out=None, null_aparams=False):
  """iic_augment_affine through the C ABI with the augmenter's dataset and tables; returns (rc, out)."""
  from iic_amd import _lib
  dev = aug.images.device
  n = ip.shape[0]
  ipd = torch.from_numpy(np.ascontiguousarray(ip, dtype=np.int32)).to(dev)
  fpd = torch.from_numpy(np.ascontiguousarray(fp, dtype=np.float32)).to(dev)
  apd = torch.from_numpy(np.ascontiguousarray(ap, dtype=np.float64)).to(dev)
  if out is None:
    out = torch.empty(n, aug.out_channels, aug.S, aug.S, device=dev, dtype=torch.float32)
  rc = _lib.lib().iic_augment_affine(
    aug.images.data_ptr(), aug.B, aug.H, aug.W, aug.channels, ipd.data_ptr(), fpd.data_ptr(),
    None if null_aparams else apd.data_ptr(), n, aug.tables_host.ctypes.data, len(aug.crop_szs), aug.bounds.data_ptr(),
    aug.kk.data_ptr(), aug.S, aug.lut.data_ptr(), out.data_ptr(), int(aug.include_rgb),
    None if aug.norm is None else aug.norm.data_ptr(), _lib.stream_ptr())
  torch.cuda.synchronize()
  return rc, out


def _oracle_from_params(imgs, aug, ip, fp, ap, angles=None, norm=None):
  """The composed PIL oracle for rows given as kernel parameters (what PairedAugmenter.draw returns)."""
  out = []
  for i in range(ip.shape[0]):
    jit = dict(flip=bool(ip[i, 3]), order=[int(o) for o in ip[i, 5:5 + ip[i, 4]]],
               factors={op: float(fp[i, op]) for op in range(4)})
    assert ao.hue_delta(float(fp[i, 3])) == ip[i, 9]
    box = None
    if ip[i, 19] != 0:
      box = (ip[i, 18] & 0xffff, ip[i, 18] >> 16, ip[i, 19] & 0xffff, ip[i, 19] >> 16)
    ang = None if angles is None or np.isnan(angles[i]) else float(angles[i])
    assert (ang is not None) == bool(ip[i, 11] & 1)
    out.append(ac.composed_oracle(imgs[ip[i, 0]], (int(ip[i, 1]), int(ip[i, 2])), aug.crop_szs[ip[i, 10]], aug.S,
                                  aug.include_rgb, tuple(ap[i]) if ip[i, 11] & 2 else None, jit, angle=ang,
                                  cutout_box=box, norm=norm))
  return np.stack(out)


def _assert_equal(got, want, what):
  assert got.shape == want.shape and got.dtype == want.dtype == np.float32
  bad = [i for i in range(got.shape[0]) if not np.array_equal(got[i], want[i])]
  assert not bad, (what, len(bad), bad[:8], float(np.abs(got - want).max()))


@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: "H%dW%d_crop%d_S%d_%s" % (s[:4] + ("rgb" if s[4] else "grey",)))
def test_affine_bit_exact_vs_pil(shape):
  """Both case families and the hand-made rows, flips and full jitter, one launch per shape."""
  from iic_amd.augment import PairedAugmenter
  H, W, crop, S, include_rgb = shape
  imgs, rows = ac.shape_cases(shape)
  assert len(rows) == 48
  jit = ac.jitter_rows(np.random.default_rng(crop * 100 + S), len(rows))
  ip, fp, ap = ac.kernel_params(rows, jit)
  aug = PairedAugmenter(torch.from_numpy(imgs).cuda(), crop, S, include_rgb)
  rc, out = _launch(aug, ip, fp, ap)
  assert rc == 0
  want = np.stack([ac.composed_oracle(imgs[r["src"]], r["xy"], crop, S, include_rgb, r["m"], j)
                   for r, j in zip(rows, jit)])
  _assert_equal(out.cpu().numpy(), want, [r["name"] for r in rows])
  # the public path launches the same entry for these rows
  assert torch.equal(aug.apply(ip, fp, ap), out)


def test_affine_without_jitter_shows_the_resampled_pixels():
  """No flip, no ColorJitter, crop size = input size: the output IS the affined crop / 255 -- nothing downstream can
  mask a wrong pixel."""
  from iic_amd.augment import PairedAugmenter
  shape = (40, 40, 36, 36, True)
  imgs, rows = ac.shape_cases(shape)
  jit = [dict(flip=False, order=[], factors={})] * len(rows)
  ip, fp, ap = ac.kernel_params(rows, jit)
  aug = PairedAugmenter(torch.from_numpy(imgs).cuda(), 36, 36, True)
  rc, out = _launch(aug, ip, fp, ap)
  assert rc == 0
  got = out.cpu().numpy()
  for i, r in enumerate(rows):
    x0, y0 = r["xy"]
    a = imgs[r["src"]][y0:y0 + 36, x0:x0 + 36]
    a = a if r["m"] is None else ac.np_affine_bilinear(a, r["m"])
    want = np.transpose(a.astype(np.float32) / np.float32(255), (2, 0, 1))
    assert np.array_equal(got[i, :3], want), (r["name"], int((got[i, :3] != want).sum()))


@pytest.mark.parametrize("variant", ["cutout", "fluid_warp", "demean", "mixed"])
def test_affine_branches_bit_exact_vs_pil(variant):
  """The public draws with random_affine on top of the other branches of tf2: the cutout box lands on the AFFINED crop,
  fluid_warp rotates the whole image first and picks one of two crop sizes, demean normalises, and a batch mixes
  affined and plain rows."""
  from iic_amd.augment import PairedAugmenter
  imgs = ac.dataset(40, 40, seed=3)
  kw, norm, p = {}, None, 0.8
  if variant == "cutout":
    kw = dict(cutout=True, cutout_p=0.7, cutout_max_box=0.7)
  elif variant == "fluid_warp":
    kw = dict(fluid_warp=True, rot_val=25.0, rand_crop_szs_tf=[36, 28])
  elif variant == "demean":
    norm = ([0.43, 0.42, 0.39, 0.41], [0.27, 0.26, 0.28, 0.25])
    kw = dict(demean=True, data_mean=norm[0], data_std=norm[1])
  else:
    p = 0.5
  aug = PairedAugmenter(torch.from_numpy(imgs).cuda(), 36, 24, True, seed=6, random_affine=True, affine_p=p, **kw)
  idx = np.random.default_rng(2).integers(0, ac.N_IMAGES, 48)
  ip, fp, ap = aug.draw(idx, "jittered")
  affined = (ip[:, 11] & 2) != 0
  assert 0 < affined.sum() < 48 and np.isfinite(aug.last_affine[affined]).all()
  if variant == "cutout":
    assert ((ip[:, 19] != 0) & affined).sum() > 10
  if variant == "fluid_warp":
    assert ((ip[:, 11] & 1 != 0) & affined).sum() > 5 and len(set(ip[:, 10])) == 2
  got = aug.apply(ip, fp, ap).cpu().numpy()
  want = _oracle_from_params(imgs, aug, ip, fp, ap, angles=aug.last_angles, norm=norm)
  _assert_equal(got, want, variant)
  assert aug.jittered(idx).shape == (48, 4, 24, 24)          # draw + apply in one call: the training batch


def test_identity_and_plain_rows_equal_iic_augment():
  """Rows through the affine path with the identity matrix, and rows without the switch in an affine launch, give the
  bits iic_augment gives for the same parameters (rotation and cutout included)."""
  from iic_amd.augment import PairedAugmenter
  imgs = ac.dataset(40, 48, seed=4)
  dev_imgs = torch.from_numpy(imgs).cuda()
  for kw in (dict(cutout=True, cutout_p=0.7, cutout_max_box=0.7), dict(fluid_warp=True, rot_val=25.0,
                                                                        rand_crop_szs_tf=[36, 28])):
    aug = PairedAugmenter(dev_imgs, 36, 40, True, seed=8, **kw)
    ip, fp = aug.draw(np.arange(48) % 8, "jittered")
    base = aug.apply(ip, fp)                                   # iic_augment
    ap = np.tile(np.asarray(ac.IDENTITY), (48, 1))
    ip_id = ip.copy()
    ip_id[:, 11] |= 2
    rc, out = _launch(aug, ip_id, fp, ap)                      # every row through the affine stages
    assert rc == 0 and torch.equal(out, base)
    ip_mix = ip.copy()
    ip_mix[::3, 11] |= 2
    rc, out = _launch(aug, ip_mix, fp, ap)                     # two thirds of the rows take iic_augment's path
    assert rc == 0 and torch.equal(out, base)
    rc, out = _launch(aug, ip, fp, np.full((48, 6), 7.5))      # no row has the switch: the matrices are not read
    assert rc == 0 and torch.equal(out, base)


def test_refusals_come_before_any_launch():
  from iic_amd.augment import PairedAugmenter
  imgs = ac.dataset(40, 40, seed=5)
  aug = PairedAugmenter(torch.from_numpy(imgs).cuda(), 36, 24, True)
  rows = ac.case_list(36, 40, 40, seed=1)[:4]
  ip, fp, ap = ac.kernel_params(rows, ac.jitter_rows(np.random.default_rng(0), 4))
  out = torch.full((4, 4, 24, 24), -7.0, device="cuda")
  rc, out = _launch(aug, ip, fp, ap, out=out, null_aparams=True)
  assert rc == IIC_ERR_ARG and bool((out == -7.0).all())
  # planes beyond the LDS limit: crop 200 -> 96 fits iic_augment (84 KB) but not the affine's two crop planes (234 KB)
  big = PairedAugmenter(torch.zeros((2, 200, 200, 3), dtype=torch.uint8, device="cuda"), 200, 96, True)
  ipb, fpb = big.draw([0, 1], "plain")
  big.apply(ipb, fpb)                                          # iic_augment serves the shape
  ipb[:, 11] = 2
  out = torch.full((2, 4, 96, 96), -7.0, device="cuda")
  rc, out = _launch(big, ipb, fpb, np.tile(np.asarray(ac.IDENTITY), (2, 1)), out=out)
  assert rc == IIC_ERR_UNSUPPORTED and bool((out == -7.0).all())
  from iic_amd._lib import IICLibraryError
  with pytest.raises(IICLibraryError):
    big.apply(ipb, fpb, np.tile(np.asarray(ac.IDENTITY), (2, 1)))


def test_train_loader_yields_the_semisup_batches():
  """Model 698's training batches: one PairedAugmenter(random_affine, cutout).jittered(idx) call per batch."""
  from iic_amd.augment import PairedAugmenter
  from iic_amd.semisup import train_loader
  imgs = ac.dataset(40, 40, seed=6)
  aug = PairedAugmenter(torch.from_numpy(imgs).cuda(), 36, 24, True, seed=2, random_affine=True, affine_p=0.5,
                        cutout=True, cutout_p=0.5, cutout_max_box=0.7)
  targets = torch.arange(8, device="cuda") + 100
  twin = PairedAugmenter(torch.from_numpy(imgs).cuda(), 36, 24, True, seed=2, random_affine=True, affine_p=0.5,
                         cutout=True, cutout_p=0.5, cutout_max_box=0.7)
  perm = np.random.RandomState(3).permutation(8)
  sizes = []
  for b, (x, t) in enumerate(train_loader(aug, targets, 3, seed=3)):
    idx = perm[3 * b:3 * b + 3]
    assert torch.equal(t.cpu(), torch.as_tensor(idx) + 100)
    assert torch.equal(x, twin.jittered(idx)) and x.shape == (len(idx), 4, 24, 24)
    sizes.append(len(idx))
  assert sizes == [3, 3, 2]
