"""tests/conv_layer_cases.py held to the product without a GPU: the table against the dispatch table of
tests/test_conv_dispatch_cpu.py, the exactness preconditions of every case on its float64 reference alone, what the
library serves, the launch plan of every test batch (host code of the instrumented library), and the exact comparison
shown to see two defects of the 25-tap layers that the net-level checks let through.

Launch plans.  For a layer of TABLE at least one test batch must run the (kernel, ms, wn, pad, block-tiled) form of the
bench batch in the forward and in every backward-data class, and one the weight-gradient form of WTABLE; N = 1 often runs
another form (128-row tiles for a launch that fills less than half the chip), which is extra coverage.  For the layers
TABLE does not list (ClusterNet5g at input 64 and 32, ClusterNet6c at 64) the plan of every test batch is a literal
here, so a change of dispatch shows.
"""
import ctypes

import numpy as np
import pytest
import torch

from iic_amd import geom
from tests import conv_layer_cases as lc
from tests.lattice import (F32_EXACT_BOUND, assert_bf16_exact_range, assert_exact, exact_mismatch, lattice, record,
                           tolerance_accepts)
from tests.test_conv_dispatch_cpu import FIELDS, L, TABLE, WFIELDS, WTABLE      # noqa: F401  (L: the fixture)
from tests.test_gpu_conv_exact import Shape

WFORM = ("kernel", "cot", "bmk", "nbuf", "ntab", "band", "bw", "bh")
CASES = lc.cases()
IDS = [lc.case_id(e, N) for e, N, _, _, _ in CASES]


def _conv_form(L, g):
  out = (ctypes.c_int * len(FIELDS))()
  L.iic_debug_conv_plan(ctypes.byref(g), out)
  p = dict(zip(FIELDS, out))
  return (p["kernel"], p["ms"], p["wn"], p["pad"], int(p["bw"] > 0))


def _wgrad_form(L, g):
  out = (ctypes.c_int * len(WFIELDS))()
  L.iic_debug_wgrad_plan(ctypes.byref(g), 1, out)
  p = dict(zip(WFIELDS, out))
  return tuple(p[f] for f in WFORM)


def _forms(L, entry, N):
  gs = lc.geoms_of(entry, N)
  return [_conv_form(L, g) for g in gs], _wgrad_form(L, gs[0])


def _table_key(layer):
  cin, cout, K, s, p, d, N, H, P = layer
  return (cin, cout, K, s, p, d, H, H, P)


# ---- the table itself ------------------------------------------------------------------------------------------------
def test_every_layer_of_the_dispatch_table_is_an_entry_with_its_bench_batch():
  by_geometry = {lc.geometry(e): e for e in lc.ENTRIES}
  for name, layer, _ in TABLE:
    e = by_geometry.get(_table_key(layer))
    assert e is not None, "TABLE layer %r has no entry in tests/conv_layer_cases.py" % name
    assert e[10] == layer[6], (name, e)


def test_every_entry_has_the_two_batches_the_tile_tails_need():
  for e, batches, _ in lc.LAYERS:
    Ns = [N for N, _, _ in batches]
    assert Ns[0] == 1 and Ns == sorted(set(Ns)), e[0]
    rows = lc.spec_of(e).out_size(e[7]) * lc.spec_of(e).out_size(e[8])
    if e[7] < 62:
      tail = (Ns[1] * rows) % 256
      best = min(((N * rows) % 256 or 999) for N in range(2, 41) if N * rows > 256)
      assert Ns[1] * rows > 256 and (tail > 0 or best == 999), (e[0], Ns)      # (999: every N gives whole tiles)
      assert 0 < tail <= 24 or tail == best % 999, (e[0], Ns, tail, best)
    # the epilogue density is the rule of tests/test_gpu_conv_exact.py
    for _, _, edens in batches:
      assert edens == ((0.125 if e[2] * e[3] * e[3] >= 2304 else 0.25), 0.5), e[0]


# ---- what the library serves -----------------------------------------------------------------------------------------
def test_what_the_library_serves_is_what_the_table_says(L):
  """iic_conv_igemm_frag_supported / iic_conv_igemm_red_supported of every geometry of every case, against the table's
  literals: the GPU tests take each geometry to the kernel the table names and skip nothing."""
  for e, N, _, _, served in CASES:
    gs = lc.geoms_of(e, N)
    assert len(gs) == len(served["frag"]) == len(served["red"]) + 1, (e[0], N)
    frag = tuple(L.iic_conv_igemm_frag_supported(ctypes.byref(g)) for g in gs)
    red = tuple(L.iic_conv_igemm_red_supported(ctypes.byref(g)) for g in gs[1:])
    assert frag == served["frag"] and red == served["red"], (e[0], N, frag, red)
    for g in gs:      # the first-generation kernel (operand `rows`) takes every one of them
      assert g.Cin % 64 == 0 and g.Cout % 64 == 0 and 1 <= g.ntaps <= 25
      assert 0 < L.iic_conv_lds_bytes(ctypes.byref(g), 0) <= 160 * 1024, (e[0], N)
    assert _wgrad_form(L, gs[0])[0] != 0, (e[0], N)      # and a weight-gradient kernel


# ---- launch plans ----------------------------------------------------------------------------------------------------
def test_a_test_batch_reaches_the_kernel_form_of_the_bench_batch(L):
  by_geometry = {lc.geometry(e): (e, b) for e, b, _ in lc.LAYERS}
  for (name, layer, want), wwant in zip(TABLE, WTABLE):
    e, batches = by_geometry[_table_key(layer)]
    bench_conv, bench_w = _forms(L, e, e[10])
    assert [f for f in bench_conv] == [w[:5] for w in want], name            # TABLE itself, at the bench batch
    assert bench_w == tuple(wwant[:8]), name                                   # WTABLE: kernel, cot, bmk, nbuf, ntab, band, bw, bh
    got = {N: _forms(L, e, N) for N, _, _ in batches}
    for i in range(len(bench_conv)):
      assert any(f[0][i] == bench_conv[i] for f in got.values()), (name, "geometry %d" % i, bench_conv[i], got)
    assert any(f[1] == bench_w for f in got.values()), (name, bench_w, got)
    # one batch reaches all of them together; where that took a third batch the table says so, and no smaller N does
    whole = [N for N, f in got.items() if f == (bench_conv, bench_w)]
    assert whole, (name, got)
    if e[0] in lc.BENCH_FORM:
      first = lc.BENCH_FORM[e[0]][0]
      assert whole == [first] == [batches[-1][0]], (name, whole)
      assert got[1][0] != bench_conv, name
      assert all(_forms(L, e, N) != (bench_conv, bench_w) for N in range(1, first)), name
    else:
      assert len(batches) <= 2, name
  assert set(lc.BENCH_FORM) <= {e[0] for e in lc.ENTRIES}
  assert all(len(b) == 3 or e[7] >= 62 for e, b, _ in lc.LAYERS if e[0] in lc.BENCH_FORM)


# (kernel, ms, wn, pad, block-tiled): 1 = the persistent 64 -> 64 kernel, 3 = conv_igemm_bd_kernel, 0 = the first generation
P64, NO, B2, B4, B2P, W1 = (1, 0, 0, 0, 0), (0, 0, 0, 0, 0), (3, 2, 2, 0, 0), (3, 4, 2, 0, 0), (3, 2, 2, 1, 0), (3, 2, 1, 0, 0)
# (kernel, cot, bmk, nbuf, ntab, band, bw, bh): 4 / 3 = the planar kernels, 1 = the register-staged kernel
WPL2, WPL, WPL_64 = (4, 64, 128, 2, 8, 0, 0, 0), (3, 128, 128, 2, 8, 0, 0, 0), (3, 128, 64, 2, 8, 0, 0, 0)
WPL_4, WREG = (3, 128, 128, 2, 4, 0, 0, 0), (1, 128, 128, 1, 0, 0, 0, 0)
PLANS = {
    ("5g/64 layer1 3x3 64->64", 1): ([P64, P64], WPL2),
    ("5g/64 layer1 3x3 64->64", 4): ([P64, P64], WPL2),
    ("5g/64 layer2.0 3x3 s2 64->128", 1): ([B2, NO, W1, W1, W1], WPL_64),
    ("5g/64 layer2.0 3x3 s2 64->128", 8): ([B2, NO, W1, W1, W1], WPL_64),
    ("5g/64 layer2.0 1x1 s2 64->128", 1): ([B4, NO], WREG),
    ("5g/64 layer2.0 1x1 s2 64->128", 8): ([B4, NO], WREG),
    ("5g/64 layer2 3x3 128->128", 1): ([B2P, B2P], WPL),
    ("5g/64 layer2 3x3 128->128", 8): ([B2P, B2P], WPL),
    ("5g/64 layer3.0 3x3 s2 128->256", 1): ([B2, B4, B2P, B2P, B2P], WPL_4),
    ("5g/64 layer3.0 3x3 s2 128->256", 16): ([B2, B4, B2P, B2P, B2P], WPL_64),
    ("5g/64 layer3.0 1x1 s2 128->256", 1): ([B4, B4], WREG),
    ("5g/64 layer3.0 1x1 s2 128->256", 16): ([B4, B4], WREG),
    ("5g/64 layer3 3x3 256->256", 1): ([B2P, B2P], WPL),
    ("5g/64 layer3 3x3 256->256", 16): ([B2P, B2P], WPL),
    ("5g/64 layer4.0 3x3 s2 256->512", 1): ([B2, B4, B2P, B2P, B2P], WPL),
    ("5g/64 layer4.0 3x3 s2 256->512", 11): ([B2, B4, B2P, B2P, B2], WPL_64),
    ("5g/64 layer4.0 1x1 s2 256->512", 1): ([B4, B4], WREG),
    ("5g/64 layer4.0 1x1 s2 256->512", 11): ([B4, B4], WREG),
    ("5g/64 layer4 3x3 512->512", 1): ([B2P, B2P], WPL),
    ("5g/64 layer4 3x3 512->512", 11): ([B2P, B2P], WPL),
    ("5g/32 layer1 3x3 64->64", 1): ([P64, P64], WPL2),
    ("5g/32 layer1 3x3 64->64", 8): ([P64, P64], WPL2),
    ("5g/32 layer2.0 3x3 s2 64->128", 1): ([B2, NO, W1, W1, W1], WPL_4),
    ("5g/32 layer2.0 3x3 s2 64->128", 16): ([B2, NO, W1, W1, W1], WPL_64),
    ("5g/32 layer2.0 1x1 s2 64->128", 1): ([B4, NO], WREG),
    ("5g/32 layer2.0 1x1 s2 64->128", 16): ([B4, NO], WREG),
    ("5g/32 layer2 3x3 128->128", 1): ([B2P, B2P], WPL),
    ("5g/32 layer2 3x3 128->128", 16): ([B2P, B2P], WPL),
    ("5g/32 layer3.0 3x3 s2 128->256", 1): ([B2, B4, B2P, B2P, B2P], WPL),
    ("5g/32 layer3.0 3x3 s2 128->256", 11): ([B2, B4, B2P, B2P, B2], WPL_64),
    ("5g/32 layer3.0 1x1 s2 128->256", 1): ([B4, B4], WREG),
    ("5g/32 layer3.0 1x1 s2 128->256", 11): ([B4, B4], WREG),
    ("5g/32 layer3 3x3 256->256", 1): ([B2P, B2P], WPL),
    ("5g/32 layer3 3x3 256->256", 11): ([B2P, B2P], WPL),
    ("5g/32 layer4.0 3x3 s2 256->512", 1): ([B2, B4, B2P, B2P, B2P], WPL),
    ("5g/32 layer4.0 3x3 s2 256->512", 29): ([B2, B4, B2, B2, B2], WPL_64),
    ("5g/32 layer4.0 1x1 s2 256->512", 1): ([B4, B4], WREG),
    ("5g/32 layer4.0 1x1 s2 256->512", 29): ([B4, B4], WREG),
    ("5g/32 layer4 3x3 512->512", 1): ([B2P, B2P], WPL),
    ("5g/32 layer4 3x3 512->512", 29): ([B2, B2], WPL_4),
    ("6c/64 5x5 64->128", 1): ([B2P, W1], WREG),
    ("6c/64 5x5 64->128", 2): ([B2P, W1], WREG),
    ("6c/64 5x5 128->256", 1): ([B2P, B2P], WREG),
    ("6c/64 5x5 128->256", 2): ([B2P, B2P], WREG),
    ("6c/64 5x5 256->512", 1): ([B2P, B2P], WREG),
    ("6c/64 5x5 256->512", 5): ([B2P, B2P], WREG),
}


def test_plans_of_the_layers_the_dispatch_table_does_not_list(L):
  listed = {_table_key(layer) for _, layer, _ in TABLE}
  unlisted = [(e, N) for e, N, _, _, _ in CASES if lc.geometry(e) not in listed]
  assert {(e[0], N) for e, N in unlisted} == set(PLANS)
  for e, N in unlisted:
    assert _forms(L, e, N) == PLANS[(e[0], N)], (e[0], N, _forms(L, e, N))


def test_the_5x5_weight_gradient_runs_its_25_taps_in_3_batches(L):
  for e, N, _, _, _ in CASES:
    if e[3] == 5:
      out = (ctypes.c_int * len(WFIELDS))()
      L.iic_debug_wgrad_plan(ctypes.byref(lc.geoms_of(e, N)[0]), 1, out)
      p = dict(zip(WFIELDS, out))
      assert (p["kernel"], p["gz"], p["threads"]) == (1, 3, 768), (e[0], N, p)


# ---- preconditions, on the reference alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry,N,dens,edens,served", CASES, ids=IDS)
def test_exactness_preconditions_hold_on_the_float64_reference(entry, N, dens, edens, served):
  """What tests/test_gpu_conv_layers_exact.py asserts before it launches, on the same inputs: max |ref| <= 255 for
  forward and backward-data (and for the fused reduction's stored gradient), per-channel sum of squares < 2^24,
  |dW| < 2^24, 2 max and max + 2 within 255 at the epilogue density."""
  name, cin, cout, K, s, p, d, H, W, P, _ = entry
  sh = Shape(cin, cout, K, s, p, N, H, W, d=d, P=P, dens=dens)
  x, w, dy = sh.x(), sh.w(), sh.dy()
  y = sh.ref_forward(x, w)
  top_y = assert_bf16_exact_range(y, "forward %s" % name)
  ssq = float((y * y).sum((0, 2, 3)).max())
  assert ssq < F32_EXACT_BOUND, "per-channel sum of squares %g >= 2^24" % ssq
  del y
  dx = sh.ref_backward_data(dy, w)
  top_dx = assert_bf16_exact_range(dx, "backward-data %s" % name)
  if any(served["red"]):
    g = (dx + sh.like_x(11).double()) * (sh.like_x(12) > 0).double()
    assert_bf16_exact_range(g, "fused reduction %s" % name)
    assert float(g.abs().sum((0, 2, 3)).max()) < F32_EXACT_BOUND
  del dx
  top_dw = float(sh.ref_backward_weight(x, dy).abs().max())
  assert top_dw < F32_EXACT_BOUND
  se = Shape(cin, cout, K, s, p, N, H, W, d=d, P=P, dens=edens)
  top_e = float(se.ref_backward_data(se.dy(), se.w()).abs().max())
  assert 2 * top_e <= 255 and top_e + 2 <= 255, "epilogue sums leave the bf16-exact range (max |ref| = %g)" % top_e
  record(kind="layer preconditions", layer=name, N=N, dens=list(dens), max_y=top_y, max_dx=top_dx, max_dw=top_dw,
         max_sum_sq=ssq, epilogue_dens=list(edens), max_dx_epilogue=top_e)


# ---- the comparison sees what it is for ------------------------------------------------------------------------------
C5 = lc.BY_NAME["6c/24 5x5 256->512"][0]      # 3 x 3 plane, 25 taps, every output pixel a border pixel
C5_N = 29                                      # M = 261: one 256-row tile and five rows


def _c5_inputs():
  name, cin, cout, K, s, p, d, H, W, P, _ = C5
  rng = np.random.default_rng(5)
  return (lattice(rng, (C5_N, cin, H, W)), lattice(rng, (cout, cin, K, K)), lattice(rng, (C5_N, cout, H, W)))


def _rows(w):
  co, ci, kh, kw = w.shape
  return w.double().permute(2, 3, 0, 1).reshape(kh * kw, co, ci).numpy()


def test_exact_comparison_rejects_one_channel_of_one_tap_dropped_at_a_corner_pixel():
  """Defect 1 on ClusterNet6c's 256 -> 512 layer: at the corner pixel (0, 0) of image 0, one input channel of one of the
  9 taps that fall inside the 3 x 3 plane is left out -- one term of 2304.  Whether 1e-2 * max |ref| accepts it is
  recorded (it does: one unit against a maximum above 100)."""
  name, cin, cout, K, s, p, d, H, W, P, _ = C5
  x, w, _ = _c5_inputs()
  y = torch.nn.functional.conv2d(x.double(), w.double(), padding=p)
  top = assert_bf16_exact_range(y, "forward")
  g = geom.fwd_geom(lc.spec_of(C5), C5_N, H, W, P, P)
  assert g.ntaps == 25 and geom.gemm_rows(g) == 261
  xp = geom.to_pt(x.double().numpy(), P)
  wr = _rows(w)
  out = geom.emulate_igemm(g, xp, wr)
  assert exact_mismatch(geom.from_pt(out, P), y) is None
  xf = xp.reshape(-1, g.Cin)
  pin, pout = int(geom._pin(g, 0)), int(geom._pout(g, 0))
  term = None
  for t in range(g.ntaps):
    src = xf[pin + g.tap_off[t]]
    for ci in np.flatnonzero(src):
      co = np.flatnonzero(wr[g.tap_w[t]][:, ci])
      if len(co):
        term = (t, int(ci), int(co[0]))
        break
    if term:
      break
  assert term, "no non-zero term at the corner pixel: the inputs are degenerate"
  t, ci, co = term
  kh, kw = divmod(int(g.tap_w[t]), K)
  assert kh >= p and kw >= p, "a tap outside the plane cannot carry a non-zero term at the corner"
  bad = out.copy()
  bad.reshape(-1, g.Cout)[pout, co] -= xf[pin + g.tap_off[t], ci] * wr[g.tap_w[t], co, ci]
  got = geom.from_pt(bad, P)
  msg = exact_mismatch(got, y)
  assert msg is not None and msg.startswith("1 of ") and "(0, %d, 0, 0)" % co in msg, msg
  accepted = tolerance_accepts(got, y)
  record(kind="seeded defect", defect="corner tap, one channel", max_ref=top, tolerance_accepts=accepted)
  assert accepted == (1.0 <= 1e-2 * top)


def test_exact_comparison_rejects_a_tap_of_the_second_batch_counted_twice_in_one_split():
  """Defect 2: the register-staged weight-gradient kernel walks the 25 taps in 3 batches of 9 (grid z) and the batch in
  splits of K-tiles (grid y).  Here the batch of 29 images is cut into 3 splits of images; in the middle split one tap of
  the second batch (taps 9 .. 17) is added twice.  Whether 1e-2 * max |ref| accepts it is recorded."""
  name, cin, cout, K, s, p, d, H, W, P, _ = C5
  x, _, dy = _c5_inputs()
  dw = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, K, K), dy.double(), padding=p)
  top = float(dw.abs().max())
  assert top < F32_EXACT_BOUND
  g = geom.fwd_geom(lc.spec_of(C5), C5_N, H, W, P, P)
  xp = geom.to_pt(x.double().numpy(), P)
  parts = []
  for images in np.array_split(np.arange(C5_N), 3):      # emulate_wgrad is linear in dy: a split = the other images' dy zeroed
    dys = torch.zeros_like(dy)
    dys[images] = dy[images]
    parts.append(geom.emulate_wgrad(g, xp, geom.to_pt(dys.double().numpy(), P), K * K))
  to_oihw = lambda a: np.transpose(a, (1, 2, 0)).reshape(cout, cin, K, K)
  assert exact_mismatch(to_oihw(sum(parts)), dw) is None
  tap = 12
  assert 9 <= tap < 18
  bad = sum(parts)
  bad[tap] += parts[1][tap]
  msg = exact_mismatch(to_oihw(bad), dw)
  assert msg is not None, "the exact comparison must reject a tap counted twice"
  differing = int(msg.split(" of ")[0])
  assert 0 < differing <= cout * cin and ", 2, 2):" in msg, msg      # tap 12 = (kh, kw) = (2, 2), nothing else
  accepted = tolerance_accepts(to_oihw(bad), dw)
  record(kind="seeded defect", defect="tap 12 twice in split 1 of 3", max_ref=top, elements=differing,
         tolerance_accepts=accepted)
  # and the smallest form of it, one element of that tap off by the contribution of one image, passes 1e-2 * max only
  # when that contribution is small next to the largest element; the exact comparison rejects it whatever its size
  one = sum(parts)
  co, ci = (int(v[0]) for v in np.nonzero(parts[1][tap]))
  one[tap, co, ci] += np.sign(parts[1][tap, co, ci])
  msg = exact_mismatch(to_oihw(one), dw)
  assert msg is not None and msg.startswith("1 of "), msg
  record(kind="seeded defect", defect="one unit in one element of tap 12", max_ref=top,
         tolerance_accepts=tolerance_accepts(to_oihw(one), dw))
