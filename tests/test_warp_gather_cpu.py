"""The gather-form backward of the general affine warp, proved without a GPU on the host emulation of
tests/warp_gather_cases.py: the search box finds exactly the contributors of a full scatter (at three slacks), every
matrix of the reference's range fits the cap, the fixed-order float32 sum is the exact adjoint on lattice inputs and inside
its accumulation bound on random ones, and the library's host-side query draws the line where the emulation draws it."""
import ctypes

import numpy as np
import pytest
import torch

from tests import iid_stage_cases as sc
from tests import warp_gather_cases as wc


def _ids(shape):
  return "x".join(map(str, shape))


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_box_finds_exactly_the_contributors_of_the_full_scatter(shape):
  """Membership is decided by the forward's taps; the box must not lose one -- not with the kernel's slack of 1/64, not
  with none, not with a whole pixel (boxes of up to the cap + 2 then, so the cap is not applied here)."""
  N, K, H, W = shape
  dout = wc.random_dout((N, 1, H, W))
  for c in wc.served_cases(shape):
    S = wc.scatter_members(c.M, H, W, c.sx, c.sy)
    for slack in (wc.SLACK, 0.0, 1e-3, 1.0):
      e = wc.emulate(dout, c.M, c.sx, c.sy, slack=slack, clamp_cap=False)
      assert np.array_equal(e["members"], S), (shape, c.name, slack, int((e["members"] != S).sum()))
      assert e["count"] == int(S.sum(2).max())


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_served_boxes_are_within_the_cap(shape):
  """Every served case, the reference-range ones among them: the largest box of any pixel, before any cut, is at most
  IIC_WARP_GATHER_CAP positions each way -- what the range condition of include/iic_hip.h promises."""
  N, K, H, W = shape
  dout = wc.random_dout((N, 1, H, W))
  n_ref = 0
  for c in wc.served_cases(shape):
    assert wc.supported(c.M), c.name
    e = wc.emulate(dout, c.M, c.sx, c.sy, clamp_cap=False)
    assert e["width"] <= wc.CAP and e["height"] <= wc.CAP, (shape, c.name, e["width"], e["height"])
    n_ref += c.ref_range
  assert n_ref == 8


def test_reference_range_at_its_corners_and_20_to_9_is_served():
  """The condition, not a sample: rotation +-30 deg, shear +-10 deg, scale 0.8 / 1.2 at the corners of the range and on a
  grid inside it, with and without the flip, both conventions, at 9 x 20, 20 x 9 and 90 x 200."""
  from iic_amd import seg_losses
  thetas = []
  for a in np.radians(np.linspace(-30.0, 30.0, 13)):
    for sh in np.radians((-10.0, 0.0, 10.0)):
      for s in (0.8, 1.0, 1.2):
        m = np.array([[np.cos(a) * s, -np.sin(a + sh) * s, 0.], [np.sin(a) * s, np.cos(a + sh) * s, 0.], [0., 0., 1.]],
                     dtype=np.float32)
        inv = np.linalg.inv(m).astype(np.float32)[:2, :]
        thetas += [inv, inv * np.array([-1.0, 1.0, 1.0], dtype=np.float32)]
  th = torch.from_numpy(np.stack(thetas))
  worst = 0.0
  for H, W in ((9, 20), (20, 9), (90, 200), (200, 90), (128, 128)):
    for ac in (False, True):
      seg_losses.ALIGN_CORNERS[0] = ac
      try:
        M = seg_losses._pixel_matrices(th, H, W)
      finally:
        seg_losses.ALIGN_CORNERS[0] = False
      ex, ey, ok = wc.extents(M)
      assert ok.all(), (H, W, ac, float(ex.max()), float(ey.max()))
      worst = max(worst, float(ex.max()), float(ey.max()))
  assert 2.0 * worst + 1.0 < wc.CAP - 1          # a position to spare


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_emulation_is_the_exact_adjoint_on_lattice_inputs(shape):
  inp = sc.warp_inputs(shape)
  n = 0
  for c in wc.served_cases(shape):
    if not c.exact:
      continue
    e = wc.emulate(inp["dout"], c.M, c.sx, c.sy)
    ref = sc.warp_bwd_ref(inp["dout"], c.M, c.sx, c.sy)
    assert torch.equal(e["dx"].double(), ref), (shape, c.name)
    n += 1
  assert n >= len(sc.warp_matrices(shape)) + 4


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_emulation_within_float32_accumulation_error_of_the_float64_adjoint(shape):
  dout = wc.random_dout(shape)
  for c in wc.served_cases(shape):
    e = wc.emulate(dout, c.M, c.sx, c.sy)
    ref = sc.warp_bwd_ref(dout, c.M, c.sx, c.sy)
    tol = wc.accumulation_bound(dout, c.M, c.sx, c.sy, e["counts"])
    err = (e["dx"].double() - ref).abs()
    assert bool((err <= tol).all()), (shape, c.name, float((err - tol).max()))


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_non_finite_dout_lands_on_the_pixels_its_output_pixel_taps(shape):
  """One NaN and one +inf in dout: dx is non-finite exactly at the source pixels the scatter says those output pixels
  tap (a zero weight times inf is NaN), in that sample and channel only."""
  N, K, H, W = shape
  dout = wc.random_dout(shape).clone()
  spots = [(0, 0, H // 2, W // 2, float("nan")), (N - 1, K - 1, H - 1, 0, float("inf"))]
  for n, k, y, x, val in spots:
    dout[n, k, y, x] = val
  for c in wc.served_cases(shape):
    S = wc.scatter_members(c.M, H, W, c.sx, c.sy)
    want = np.zeros((N, K, H * W), dtype=bool)
    for n, k, y, x, _ in spots:
      want[n, k] |= S[n, :, y * W + x]
    got = ~np.isfinite(wc.emulate(dout, c.M, c.sx, c.sy)["dx"].numpy().reshape(N, K, H * W))
    assert np.array_equal(got, want), (shape, c.name)


def _query(M):
  from iic_amd import _lib
  M = M.contiguous()
  return _lib.lib().iic_affine_warp_gather_supported(M.data_ptr(), M.shape[0])


@pytest.mark.parametrize("shape", wc.SHAPES, ids=_ids)
def test_refused_matrices_are_refused_and_the_library_query_agrees(shape):
  """iic_affine_warp_gather_supported is host code: it runs here.  It must answer what the emulation's condition
  answers on every case, refuse the two refused ones, and refuse non-finite entries and void arguments."""
  assert len(wc.refused_cases(shape)) == 2
  for c in wc.cases(shape):
    assert wc.supported(c.M) == c.served, c.name
    assert _query(c.M) == (1 if c.served else 0), c.name
  N = shape[0]
  for bad in (float("nan"), float("inf"), -float("inf")):
    for col in range(6):
      M = torch.tensor([[1, 0, 0, 0, 1, 0]] * N, dtype=torch.float32)
      M[N - 1, col] = bad
      assert _query(M) == 0, (bad, col)
      assert not wc.supported(M)
  from iic_amd import _lib
  M = torch.tensor([[1, 0, 0, 0, 1, 0]], dtype=torch.float32)
  assert _lib.lib().iic_affine_warp_gather_supported(None, 1) == 0
  assert _lib.lib().iic_affine_warp_gather_supported(M.data_ptr(), 0) == 0
  assert _query(M) == 1


def test_launch_refuses_before_it_touches_the_device():
  """The refusal of iic_affine_warp_bwd_gather comes from the host copy of the matrices: with a refused batch it answers
  IIC_ERR_UNSUPPORTED without a device (the pointers below are never dereferenced), and IIC_ERR_ARG for void arguments."""
  from iic_amd import _lib
  L = _lib.lib()
  c = wc.refused_cases((2, 1, 20, 9))[0]
  buf = ctypes.create_string_buffer(64)
  p = ctypes.addressof(buf)
  assert L.iic_affine_warp_bwd_gather(p, p, c.M.data_ptr(), p, 2, 1, 20, 9, 0, 0, None) == -3
  assert L.iic_affine_warp_bwd_gather(p, p, None, p, 2, 1, 20, 9, 0, 0, None) == -1
  assert L.iic_affine_warp_bwd_gather(p, p, c.M.data_ptr(), p, 2, 0, 20, 9, 0, 0, None) == -1
