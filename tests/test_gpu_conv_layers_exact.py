"""Every conv layer the architectures build (tests/conv_layer_cases.py), bit for bit on the integer lattice, and the
closure test that keeps that table and iic_amd/archs the same list.

The bodies are those of tests/test_gpu_conv_exact.py (forward with both BatchNorm statistics and the untouched PT border,
backward-data over all parity classes, its eight epilogue forms, the weight gradient for three split-K factors with both
read paths and accumulation, the fused BatchNorm-backward reduction), run at the geometries that file does not have: the
25-tap 5 x 5 layers of ClusterNet6c, the 33 .. 3 pixel planes of ClusterNet5g at input 64 and 32, SegmentationNet10a c3,
c4, c6 and every COCO layer -- at N = 1 (M below one tile), at a batch that leaves a few rows after whole 256-row tiles,
and at the smallest batch that runs the bench batch's kernel form (tests/test_conv_layers_cpu.py proves which).

Nothing is skipped: what the library serves is a literal of the table, asserted here and on the CPU.  A parity class
the weights-direct kernels refuse (the one-tap class of the 64 -> 128 stride-2 layers) is asserted refused by the return
code of iic_conv_igemm_frag and runs where the product runs it, on the first-generation kernel through ops.conv_igemm.
The references of a case are computed once and shared by the runs of that case.
"""
import ctypes
import types

import pytest
import torch

from tests import conv_layer_cases as lc
from tests import test_gpu_conv_exact as ex

pytestmark = pytest.mark.gpu

IIC_ERR_UNSUPPORTED = -3      # include/iic_hip.h
CASES = lc.cases()
IDS = [lc.case_id(e, N) for e, N, _, _, _ in CASES]


class LayerShape(ex.Shape):
  """ex.Shape whose inputs and float64 references are kept for as long as the same shape is asked again (one shape at a
  time: the 100 x 100 layers' references are hundreds of megabytes).  Shared, never modified."""
  _owner, _memo = [None], {}

  def _kept(self, key, make):
    if LayerShape._owner[0] != repr(self):
      LayerShape._memo.clear()
      LayerShape._owner[0] = repr(self)
    if key not in LayerShape._memo:
      LayerShape._memo[key] = make()
    return LayerShape._memo[key]

  def x(self):
    return self._kept("x", lambda: ex.Shape.x(self))

  def w(self):
    return self._kept("w", lambda: ex.Shape.w(self))

  def dy(self):
    return self._kept("dy", lambda: ex.Shape.dy(self))

  def like_x(self, salt, density=ex.HALF):
    return self._kept(("like_x", salt, density), lambda: ex.Shape.like_x(self, salt, density))

  def ref_forward(self, x, w):
    assert x is self.x() and w is self.w()
    return self._kept("y", lambda: ex.Shape.ref_forward(self, x, w))

  def ref_backward_data(self, dy, w):
    assert dy is self.dy() and w is self.w()
    return self._kept("dx", lambda: ex.Shape.ref_backward_data(self, dy, w))

  def ref_backward_weight(self, x, dy):
    assert x is self.x() and dy is self.dy()
    return self._kept("dw", lambda: ex.Shape.ref_backward_weight(self, x, dy))


def _shape(entry, N, dens):
  name, cin, cout, K, s, p, d, H, W, P, _ = entry
  return LayerShape(cin, cout, K, s, p, N, H, W, d=d, P=P, dens=dens)


def _bench_form_batch(entry, N):
  """The third batch of a layer, tens to hundreds of images, is there for the weights-direct kernels' bench form: the
  tests that walk many forms take fewer of them there (the eight epilogues on the weights-direct operand only; the fused
  reduction with everything and with nothing), which keeps every case within a few seconds."""
  return entry[0] in lc.BENCH_FORM and N == lc.BENCH_FORM[entry[0]][0] and N > 2


def _assert_served(entry, N, served):
  """The library's answer per geometry equals the table's literal; returns the geometries and the operand the
  weights-direct runs take (`frag` where every geometry is served, else the product's own handle)."""
  from iic_amd import ops
  gs = lc.geoms_of(entry, N)
  got = tuple(int(ops.frag_supported(g)) for g in gs)
  assert got == served["frag"], "%s: iic_conv_igemm_frag_supported says %r, the table %r" % (entry[0], got, served["frag"])
  return gs, ("frag" if all(got[1:]) else "product")


def _assert_refused(sh, g):
  """iic_conv_igemm_frag answers IIC_ERR_UNSUPPORTED for a geometry it does not serve and launches nothing."""
  from iic_amd import ops
  from iic_amd._lib import lib, ptr, stream_ptr
  wf = ops.weight_prep_frag(sh.w().to(ex.dev()), True)
  dyp = ops.pt_from_nchw(sh.dy().to(ex.dev()), sh.P)
  dx = torch.zeros((sh.N, sh.H + 2 * sh.P, sh.W + 2 * sh.P, sh.cin), dtype=torch.bfloat16, device=ex.dev())
  rc = lib().iic_conv_igemm_frag(ctypes.byref(g), ptr(dyp), ptr(wf), ptr(dx), None, None, None, 0, stream_ptr())
  torch.cuda.synchronize()
  assert rc == IIC_ERR_UNSUPPORTED, rc
  assert float(dx.float().abs().max()) == 0.0, "a refused launch wrote its output"


@pytest.mark.parametrize("entry,N,dens,edens,served", CASES, ids=IDS)
def test_layer_forward_and_statistics_exact(entry, N, dens, edens, served):
  _assert_served(entry, N, served)
  assert served["frag"][0] == 1
  sh = _shape(entry, N, dens)
  for operand in ("rows", "frag"):
    ex._forward(sh, operand)


@pytest.mark.parametrize("entry,N,dens,edens,served", CASES, ids=IDS)
def test_layer_backward_data_exact(entry, N, dens, edens, served):
  """All parity classes; for the 1 x 1 stride-2 shortcuts ex._backward_data also asserts that the pixels no class covers
  are never written."""
  from iic_amd import geom
  gs, direct = _assert_served(entry, N, served)
  sh = _shape(entry, N, dens)
  for g, ok in zip(gs[1:], served["frag"][1:]):
    if not ok:
      _assert_refused(sh, g)
  assert geom.bwd_data_covers_all(sh.spec) == (not (sh.K == 1 and sh.s == 2))
  for operand in ("rows", direct):
    ex._backward_data(sh, operand)


EPILOGUE = [c for c in CASES if not (c[0][3] == 1 and c[0][4] == 2)]      # (1x1 stride 2: pixels no launch stores)


@pytest.mark.parametrize("entry,N,dens,edens,served", EPILOGUE, ids=[lc.case_id(c[0], c[1]) for c in EPILOGUE])
def test_layer_backward_data_epilogues_exact(entry, N, dens, edens, served):
  from iic_amd import geom
  _, direct = _assert_served(entry, N, served)
  sh = _shape(entry, N, edens)
  assert geom.bwd_data_covers_all(sh.spec)
  for operand in ((direct,) if _bench_form_batch(entry, N) else ("rows", direct)):
    ex._backward_data_epilogues(sh, operand)


@pytest.mark.parametrize("entry,N,dens,edens,served", CASES, ids=IDS)
def test_layer_weight_gradient_exact_for_any_split(entry, N, dens, edens, served):
  sh = _shape(entry, N, dens)
  for use_tr in (False, True):
    ex._backward_weight(sh, use_tr, splits=(None, 1, "large"))


RED = [c for c in CASES if any(c[4]["red"])]
assert {c[0][0] for c in CASES} - {c[0][0] for c in RED} == {e[0] for e in lc.ENTRIES if e[3] == 1 or e[1:3] == (64, 64)}


@pytest.mark.parametrize("entry,N,dens,edens,served", RED, ids=[lc.case_id(c[0], c[1]) for c in RED])
def test_layer_fused_bn_backward_reduction_exact(entry, N, dens, edens, served):
  """iic_conv_igemm_frag_red on every parity class ops.red_supported serves (the 64 -> 64 layers and the 1 x 1
  shortcuts have none: the table says so, tests/test_conv_layers_cpu.py holds the library to it), with and without the
  second sum and the mask."""
  from iic_amd import ops
  gs, _ = _assert_served(entry, N, served)
  sh = _shape(entry, N, dens)
  pw = ops.PreppedWeights(sh.w().to(ex.dev()))
  got = tuple(int(ops.red_supported(g, pw[1])) for g in gs[1:])
  assert got == served["red"], "%s: iic_conv_igemm_red_supported says %r, the table %r" % (entry[0], got, served["red"])
  forms = ((True, True), (False, False)) if _bench_form_batch(entry, N) else ((False, True), (True, False), (True, True), (False, False))
  for has2, masked in forms:
    ex._fused_reduction(sh, has2, masked)


# ----------------------------------------------------------------------------------------------------------------------
# no conv geometry without an exact case
# ----------------------------------------------------------------------------------------------------------------------
def _builds():
  """(prefix of the table's names, constructor, input tensor shape) of every listed configuration.  The clustering nets
  run at batch 2; the segmentation nets at their published size and batch 1 (their planes follow from the input)."""
  from iic_amd import archs
  cfg = lambda **kw: types.SimpleNamespace(batchnorm_track=True, num_sub_heads=1, **kw)
  out = []
  for sz in (96, 64, 32):
    out.append(("5g/%d " % sz, lambda sz=sz: archs.ClusterNet5g(cfg(in_channels=2, input_sz=sz, output_k=10)), (2, 2, sz, sz)))
  for sz in (24, 64):
    out.append(("6c/%d " % sz, lambda sz=sz: archs.ClusterNet6c(cfg(in_channels=1, input_sz=sz, output_k=10)), (2, 1, sz, sz)))
  for name, sz in (("potsdam ", 200), ("coco ", 128)):
    out.append((name, lambda sz=sz: archs.SegmentationNet10a(cfg(in_channels=4, input_sz=sz, output_k=3)), (1, 4, sz, sz)))
  return out


def test_every_conv_geometry_the_architectures_build_has_an_exact_case(monkeypatch):
  """One forward and backward of every architecture in every listed configuration, with _ConvHolder.geoms -- the one
  place the architectures make a fwd_geom / bwd_data_geoms pair -- recording (spec, H, W, pad_in, pad_out).  Every
  recorded geometry must be an entry of tests/conv_layer_cases.py, batch aside, and every entry must have been recorded:
  a layer added to an architecture, or an input size admitted, without its exact cases fails here, and so does an entry
  the product no longer builds.  (The first layers run their own kernels and never ask for a geometry.)"""
  from iic_amd.archs import cluster
  seen = {}
  original = cluster._ConvHolder.geoms

  def recording(self, N, H, W):
    s = self.spec
    seen.setdefault(prefix[0], set()).add((s.cin, s.cout, s.K, s.s, s.p, s.d, H, W, self.pad_in, self.pad_out))
    return original(self, N, H, W)

  monkeypatch.setattr(cluster._ConvHolder, "geoms", recording)
  prefix = [None]
  torch.manual_seed(0)
  for name, build, shape in _builds():
    prefix[0] = name
    net = build().to(ex.dev()).train()
    out = net(torch.randn(*shape, device=ex.dev()))
    sum(o.sum() for o in out).backward()
    torch.cuda.synchronize()
    del net, out
  want = {}
  for e in lc.ENTRIES:
    name = next(p for p, _, _ in _builds() if e[0].startswith(p))
    cin, cout, K, s, p, d, H, W, P = lc.geometry(e)
    want.setdefault(name, set()).add((cin, cout, K, s, p, d, H, W, P, P))
  assert set(seen) == set(want)
  for name in want:
    extra, missing = seen[name] - want[name], want[name] - seen[name]
    assert not extra, "%s builds conv geometries without an exact case in tests/conv_layer_cases.py: %r" % (name, sorted(extra))
    assert not missing, "tests/conv_layer_cases.py lists geometries that %s does not build: %r" % (name, sorted(missing))
