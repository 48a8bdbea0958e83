"""The float64 brackets of tests/test_gpu_conv_f64.py, proven without a GPU (tests/parity.py: conv_acc_bound,
bf16_bracket, bf16_bracket_epilogue; tests/conv_f64_cases.py: the draws, the statistic bounds, the emulations).

Three things are held here.

  1. The decisive-share CONDITION, from the float64 reference alone: on every `pos` case at least 0.85 of the brackets
     hold one bf16 value (measured 0.907 at 4608 terms to 0.999 at 64), on `mixed` the floors of
     conv_f64_cases.mixed_decisive_floor at <= 576 terms (measured 0.96 / 0.975 at 64 / 128 terms, 0.544-0.559 at 576,
     0.23 at 1152, 0 at 4608 -- hence both draws).

  2. CORRECT emulations stay inside: plain fp32 F.conv2d / conv2d_input / conv2d_weight, and a chunked-K fp32
     accumulation folded in three different orders, each followed by one round-to-nearest-even store -- every element of
     forward, backward-data with each epilogue, and the weight gradient (also accumulated onto a previous dW), and every
     statistic cell, on all eight shape / draw pairs.

  3. SEEDED DEFECTS that the suite's older criteria accept -- 1e-2 * max |ref| (3e-3 for the weight gradient, 2e-3
     scale for the statistics) of tests/test_gpu_kernels.py and, run on lattice operands, the exact comparison of
     tests/test_gpu_conv_exact.py -- are rejected on a named case.  Shares of elements outside, as measured here:
       1. truncating bf16 store                          pos 64->64: 0.49 outside      (mixed: 0.28)
       2. one of two K-halves rounded to bf16 before     pos 64->64: 0.12, pos 512->512: 0.083 outside
          the fold; the weight gradient's version        pos 64->64, one of 5 partials: 0.92 of dW outside its bound
       3. lowest mantissa bit of x cleared               mixed 1x1 stride 2 (64 terms): 0.63, mixed 64->64 (576): 0.52
       4. per-channel sums from the rounded outputs      pos 1x1 stride 2 (64 terms, 147 pixels): 0.945 of the 128
                                                         channels miss the S1 bound, 0.977 the S2 bound (error 1.5e-4
                                                         relative rms, bound 1.26e-5)
       5. fp32 accumulator cut to 10 mantissa bits       pos 64->64 (fp32 store, bound alone): 0.9999 outside
     Every defect is rejected on its named case: no fallback was needed.
"""
import numpy as np
import pytest
import torch

from tests import conv_f64_cases as cc
from tests.lattice import exact_mismatch, lattice
from tests.parity import (BF16_MAX, U32, assert_in_bracket, assert_within, bf16_bracket, bf16_rne, bf16_spacing,
                          conv_acc_bound, outside_share)
from tests.test_gpu_kernels import CONV_CASES

C64 = cc.of((64, 64, 3, 1, 1, 5, 13))
C512 = cc.of((512, 512, 3, 1, 1, 6, 7))
C1X1 = cc.of((64, 128, 1, 2, 0, 3, 13))
C128 = cc.of((128, 128, 3, 1, 1, 20, 25))
PROOF = [C64, C512, C1X1, C128]
assert all(c in [cc.of(t) for t in CONV_CASES] for c in PROOF)


def _report(**kw):
  print("FIGURES " + " ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in kw.items()))


# ---- the helper itself ---------------------------------------------------------------------------------------------
def test_bf16_rne_rounds_once_to_nearest_even():
  rng = np.random.default_rng(0)
  v = torch.from_numpy(rng.standard_normal(200000) * np.exp2(rng.integers(-30, 30, 200000))).float()
  assert torch.equal(bf16_rne(v.double()), v.to(torch.bfloat16).double())          # float32-exact inputs: torch agrees
  # ties go to even; a value just above a tie that float32 would first round ONTO the tie still goes up
  one, ulp = 1.0, 2.0 ** -7
  assert float(bf16_rne(torch.tensor(one + ulp / 2))) == one and float(bf16_rne(torch.tensor(one + 3 * ulp / 2))) == one + 2 * ulp
  x = one + ulp / 2 + 2.0 ** -40
  assert float(bf16_rne(torch.tensor(x, dtype=torch.float64))) == one + ulp
  assert float(torch.tensor(x, dtype=torch.float64).float().to(torch.bfloat16)) == one, "the double rounding this avoids"
  edge = torch.tensor([BF16_MAX, BF16_MAX * (1 + 2.0 ** -10), BF16_MAX * (1 + 2.0 ** -8), -3.4e38, float("inf"), 2.0 ** -133, 2.0 ** -135],
                      dtype=torch.float64)
  want = torch.tensor([BF16_MAX, BF16_MAX, float("inf"), float("-inf"), float("inf"), 2.0 ** -133, 0.0], dtype=torch.float64)
  assert torch.equal(bf16_rne(edge), want)
  assert bool(torch.isnan(bf16_rne(torch.tensor(float("nan")))))
  assert float(bf16_spacing(torch.tensor(1.5))) == 2.0 ** -7 and float(bf16_spacing(torch.tensor(0.0))) == 2.0 ** -133


def test_assert_in_bracket_reports_and_records():
  from tests import parity
  ref = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
  lo, hi = bf16_bracket(ref, 1e-6 * ref)
  assert torch.equal(lo, hi)
  fam = "selftest"
  parity.WORST.pop(fam, None)
  assert_in_bracket(ref.float(), lo, hi, "ok", fam, ref=ref, b=1e-6 * ref)
  assert parity.WORST[fam]["decisive"] == 1.0 and parity.WORST[fam]["ratio"] == 0.0
  bad = ref.clone()
  bad[1] += 2.0 ** -6
  with pytest.raises(AssertionError, match=r"1 of 3 elements outside .* first at \(1,\)"):
    assert_in_bracket(bad, lo, hi, "shifted", fam, ref=ref, b=1e-6 * ref)
  assert 0.9 < parity.WORST[fam]["ratio"] < 1.1
  with pytest.raises(AssertionError):
    assert_in_bracket(torch.tensor([1.0, float("nan"), 3.0]), lo, hi, "nan")
  parity.WORST.pop(fam, None)


# ---- 1. the condition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [cc.of(t) for t in CONV_CASES] + cc.LAYER_CASES, ids=repr)
def test_decisive_share_holds_from_the_reference_alone(case):
  """(cc.LAYER_CASES: the layer geometries of tests/conv_layer_cases.py.  The 5 x 5 layers reach 6400 and 12800 terms,
  where cc.pos_decisive_floor continues the expression 0.85 was derived from: 0.795 and 0.599.)"""
  for kind, bracket, terms in (("forward", cc.forward_bracket, case.terms_fwd),
                               ("backward-data", cc.backward_data_bracket, case.terms_bd)):
    for draw in cc.DRAWS:
      _, _, lo, hi = bracket(case, draw)
      share = cc.decisive_share(lo, hi)
      floor = cc.pos_decisive_floor(terms) if draw == "pos" else cc.mixed_decisive_floor(terms)
      _report(case=repr(case), kind=kind, draw=draw, terms=terms, decisive=share, floor=floor)
      if floor is not None:
        assert share >= floor, (kind, draw, terms, share, floor)


def test_floors_beyond_4608_terms_and_the_layer_cases_are_layers_of_the_table():
  assert cc.pos_decisive_floor(64) == cc.pos_decisive_floor(4608) == cc.POS_DECISIVE_FLOOR == 0.85
  assert abs(cc.pos_decisive_floor(6400) - (1 - 2 * 6400 / 65536.0 - 0.01)) < 1e-12 and 0.79 < cc.pos_decisive_floor(6400) < 0.80
  assert abs(cc.pos_decisive_floor(12800) - (1 - 2 * 12800 / 65536.0 - 0.01)) < 1e-12 and 0.59 < cc.pos_decisive_floor(12800) < 0.60
  assert sorted({t for c in cc.LAYER_CASES for t in (c.terms_fwd, c.terms_bd) if t > 4608}) == [6400, 12800]
  from tests import conv_layer_cases as lc
  table = {lc.geometry(e) for e in lc.ENTRIES}
  for c in cc.LAYER_CASES:
    assert (c.cin, c.cout, c.K, c.s, c.p, c.d, c.H, c.W, c.P) in table, c


# ---- 2. correct emulations stay inside ---------------------------------------------------------------------------------
def _orders(n):
  return [list(range(n)), list(range(n - 1, -1, -1)), list(range(1, n, 2)) + list(range(0, n, 2))]


def _accumulations(parts_fn, chunks):
  """Plain fp32 and a chunked-K accumulation in three orders: (name, fp32 accumulator)."""
  yield "fp32", parts_fn(1)[0]
  parts = parts_fn(chunks)
  for i, order in enumerate(_orders(len(parts))):
    yield "chunked/%d" % i, cc.fold(parts, order)


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("case", PROOF, ids=repr)
def test_correct_forward_emulations_stay_inside(case, draw):
  t = cc.inputs(case, draw)
  ref, b, lo, hi = cc.forward_bracket(case, draw)
  tol1, tol2 = cc.stat_bounds(ref, b, case.count)
  want = torch.stack([ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3))])
  for name, acc in _accumulations(lambda n: cc.forward_parts(case, t["x"], t["w"], n), min(8, case.cin // 16)):
    assert_within(acc, ref, b, "fp32 accumulator, %s" % name)                       # (the fp32 path's whole check)
    assert_in_bracket(cc.store_rne(acc), lo, hi, "forward, %s" % name)
    for st in (cc.stats_of(acc), cc.stats_of_fp32_sums(acc)):
      assert_within(st[0], want[0], tol1, "S1, %s" % name)
      assert_within(st[1], want[1], tol2, "S2, %s" % name)


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("case", PROOF, ids=repr)
def test_correct_backward_data_emulations_stay_inside_with_every_epilogue(case, draw):
  from iic_amd import geom
  t = cc.inputs(case, draw)
  ref, b, lo, hi = cc.backward_data_bracket(case, draw)
  for name, acc in _accumulations(lambda n: cc.backward_data_parts(case, t["dy"], t["w"], n), min(8, case.cout // 16)):
    tile = cc.store_rne(acc)
    assert_in_bracket(tile, lo, hi, "backward-data, %s" % name)
    if not geom.bwd_data_covers_all(case.spec):
      continue      # (1x1 stride 2: an epilogue runs only on the pixels its launch stores)
    for ename, kw, reads in cc.EPILOGUES:
      lo2, hi2 = cc.epilogue_bracket(lo, hi, t, reads, kw.get("premask", False))
      got = cc.epilogue_emulated(tile, t, reads, kw.get("premask", False))
      assert_in_bracket(got, lo2, hi2, "backward-data %s, %s" % (ename, name))
      if "act" in reads and kw.get("premask"):
        assert float(got[~(t["act"] > 0)].abs().max()) == 0.0 and 0.3 < float((t["act"] > 0).float().mean()) < 0.7


@pytest.mark.parametrize("draw", cc.DRAWS)
@pytest.mark.parametrize("case", PROOF, ids=repr)
def test_correct_weight_gradient_emulations_stay_inside(case, draw):
  t = cc.inputs(case, draw)
  nsplit = min(case.N, 5)
  ref, tol = cc.weight_gradient_bound(case, draw, nsplit)
  prev = cc.bf16(torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, tuple(ref.shape)).astype(np.float32)))
  refp, tolp = cc.weight_gradient_bound(case, draw, nsplit, prev=prev)
  for name, acc in _accumulations(lambda n: cc.backward_weight_parts(case, t["x"], t["dy"], n), nsplit):
    assert_within(acc, ref, tol, "weight gradient, %s" % name)
    assert_within(prev + acc, refp, tolp, "weight gradient onto a previous dW, %s" % name)


# ---- 3. seeded defects -------------------------------------------------------------------------------------------------
def _lattice_inputs(case, density=0.5):
  rng = np.random.default_rng(7)
  Ho, Wo = case.out_hw
  return (lattice(rng, (case.N, case.cin, case.H, case.W), density), lattice(rng, (case.cout, case.cin, case.K, case.K), density),
          lattice(rng, (case.N, case.cout, Ho, Wo), density))


def _lattice_accepts(case, pipeline, what):
  """The defect's pipeline on {-1, 0, +1} operands reproduces float64 exactly: tests/test_gpu_conv_exact.py cannot see it."""
  x, w, dy = _lattice_inputs(case)
  got, ref = pipeline(x, w, dy)
  assert float(ref.abs().max()) <= 255, "the lattice precondition of tests/lattice.py"
  msg = exact_mismatch(got, ref)
  assert msg is None, "%s: expected the lattice comparison to accept this defect: %s" % (what, msg)


def test_defect_1_truncating_store_is_rejected():
  def pipeline(x, w, dy):
    return cc.store_truncating(cc.forward_parts(C64, x, w, 1)[0]), cc.conv64(C64, x, w)
  _lattice_accepts(C64, pipeline, "truncating store")
  shares = {}
  for draw in cc.DRAWS:
    t = cc.inputs(C64, draw)
    ref, b, lo, hi = cc.forward_bracket(C64, draw)
    got, _ = pipeline(t["x"], t["w"], None)
    assert cc.old_accepts(got, ref), "1e-2 * max was expected to accept a truncating store"
    shares[draw] = outside_share(got, lo, hi)
  _report(defect=1, **shares)
  # truncation and RNE differ whenever the discarded part exceeds half a spacing: half of all values; all of those with
  # a one-value bracket are outside (decisive share >= 0.85 on pos), so 0.3 is far below what must show
  assert shares["pos"] >= 0.3, shares
  assert shares["mixed"] > 0.0, shares


@pytest.mark.parametrize("case", [C64, C512], ids=repr)
def test_defect_2_bf16_rounded_split_partial_is_rejected(case):
  def pipeline(x, w, dy):
    parts = cc.forward_parts(case, x, w, 2)
    parts[1] = cc.store_rne(parts[1])                   # half of the K range passes through bf16 before the fold
    return cc.store_rne(cc.fold(parts)), cc.conv64(case, x, w)
  if case is C64:
    _lattice_accepts(case, pipeline, "bf16 split partial")
  t = cc.inputs(case, "pos")
  ref, b, lo, hi = cc.forward_bracket(case, "pos")
  got, _ = pipeline(t["x"], t["w"], None)
  assert cc.old_accepts(got, ref), "1e-2 * max was expected to accept a bf16-rounded partial"
  share = outside_share(got, lo, hi)
  _report(defect=2, case=repr(case), pos=share)
  # the partial's rounding error is uniform within half ITS spacing, a quarter to a half of the total's: it moves the
  # total across a rounding boundary for roughly one element in eight; 0.03 is a quarter of that
  assert share >= 0.03, share


def test_defect_2_bf16_rounded_split_partial_of_the_weight_gradient_is_rejected():
  case = C64

  def pipeline(x, w, dy):
    parts = cc.backward_weight_parts(case, x, dy, case.N)
    parts[2] = cc.store_rne(parts[2])
    return cc.fold(parts), cc.wg64(case, x, dy)
  _lattice_accepts(case, pipeline, "bf16 split partial of the weight gradient")
  t = cc.inputs(case, "pos")
  ref, tol = cc.weight_gradient_bound(case, "pos", case.N)
  got, _ = pipeline(t["x"], None, t["dy"])
  assert cc.old_accepts(got, ref, 3e-3), "3e-3 * max was expected to accept a bf16-rounded partial"
  share = float(((got.double() - ref).abs() > tol).double().mean())
  _report(defect="2w", pos=share)
  # one partial of five carries up to 2^-9 of a fifth of |dW| = 4e-4 |dW|, eight times the bound of
  # (845 + 6) * 2^-24 = 5e-5 |dW|: all but the elements whose partial happens to round by < 1/8 spacing are outside
  assert share >= 0.5, share


@pytest.mark.parametrize("case,floor", [(C1X1, 0.1), (C64, 0.05)], ids=["1x1s2-64terms", "64to64-576terms"])
def test_defect_3_cleared_low_mantissa_bit_is_rejected_by_mixed(case, floor):
  def pipeline(x, w, dy):
    return cc.store_rne(cc.forward_parts(case, cc.clear_low_mantissa_bit(x), w, 1)[0]), cc.conv64(case, x, w)
  _lattice_accepts(case, pipeline, "cleared mantissa bit")        # +-1 and 0 have no low bit set
  t = cc.inputs(case, "mixed")
  assert 0.3 < float((cc.clear_low_mantissa_bit(t["x"]) != t["x"]).float().mean()) < 0.7
  ref, b, lo, hi = cc.forward_bracket(case, "mixed")
  got, _ = pipeline(t["x"], t["w"], None)
  assert cc.old_accepts(got, ref), "1e-2 * max was expected to accept a cleared mantissa bit"
  share = outside_share(got, lo, hi)
  _report(defect=3, case=repr(case), mixed=share)
  # half of the activations lose 2^-7 .. 2^-8 of their value: a random walk of rms ~2^-9 of the output's own rms,
  # against half a spacing of 2^-9 .. 2^-8 |y| -- a third or more of the decisive elements move; the floors are a
  # quarter of that third times the decisive share (0.96 / 0.55), rounded down
  assert share >= floor, share


def test_defect_4_statistics_from_the_rounded_tile_are_rejected():
  case, draw = C1X1, "pos"

  def pipeline(x, w, dy):
    return cc.stats_of(cc.store_rne(cc.forward_parts(case, x, w, 1)[0])), None
  x, w, _ = _lattice_inputs(case)
  y = cc.conv64(case, x, w)
  assert float(y.abs().max()) <= 255
  assert exact_mismatch(pipeline(x, w, None)[0], torch.stack([y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))])) is None
  t = cc.inputs(case, draw)
  ref, b, lo, hi = cc.forward_bracket(case, draw)
  assert case.terms_fwd == 64 and case.count == 147
  tol1, tol2 = cc.stat_bounds(ref, b, case.count)
  want = torch.stack([ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3))])
  st, _ = pipeline(t["x"], t["w"], None)
  assert cc.old_accepts_stats(st, ref, case.count), "the 2e-3 * scale criterion was expected to accept these sums"
  miss1 = float(((st[0] - want[0]).abs() > tol1).double().mean())
  miss2 = float(((st[1] - want[1]).abs() > tol2).double().mean())
  _report(defect=4, channels_missing_S1=miss1, channels_missing_S2=miss2, rel_bound=float((tol1 / want[0].abs()).max()),
          rel_err_rms=float(((st[0] - want[0]) / want[0]).pow(2).mean().sqrt()))
  assert float((tol1 / want[0].abs()).max()) < 1.4e-5          # (64 + 147) U32 = 1.26e-5
  # 147 independent rounding errors, each uniform within half a spacing (2^-10 .. 2^-9 of |y|, rms ~0.8e-3 |y|), sum to
  # ~0.8e-3 / sqrt(147) = 7e-5 relative or more (1.5e-4 rms measured), a normal variable of five to ten times the bound:
  # nearly every channel misses it
  assert miss1 >= 0.5, miss1
  # and the accumulators themselves pass
  ok = cc.stats_of(cc.forward_parts(case, t["x"], t["w"], 1)[0])
  assert_within(ok[0], want[0], tol1, "S1 from the accumulators")
  assert_within(ok[1], want[1], tol2, "S2 from the accumulators")


def test_defect_5_shortened_fp32_accumulator_is_rejected_on_the_fp32_path():
  case = C64

  def pipeline(x, w, dy):
    return cc.fold(cc.forward_parts(case, x, w, 3), on_acc=lambda a: cc.shorten_mantissa(a, 10)), cc.conv64(case, x, w)
  _lattice_accepts(case, pipeline, "10-bit accumulator")          # integers below 2^11 keep every bit
  t = cc.inputs(case, "pos")
  ref, A = cc.ref_forward(case, "pos")
  tol = conv_acc_bound(case.terms_fwd, A)
  got, _ = pipeline(t["x"], t["w"], None)
  assert cc.old_accepts(got, ref), "1e-2 * max was expected to accept a 10-bit accumulator"
  share = float(((got.double() - ref).abs() > tol).double().mean())
  _report(defect=5, pos=share)
  # three truncations of up to 2^-10 each against 576 * 2^-24 = 3.4e-5 relative: only sums that happen to be
  # representable in 10 bits survive
  assert share >= 0.9, share
  assert_within(cc.fold(cc.forward_parts(case, t["x"], t["w"], 3)), ref, tol, "the undamaged fold")


def test_overflow_and_non_finite_classes_of_the_reference():
  """The float64 reference that the GPU test's non-finite cases use classifies like the arithmetic rules: NaN where an
  inf meets a zero weight or a NaN pixel or infs of both signs meet, +-inf where infs of one sign meet non-zero weights."""
  case = cc.of((64, 128, 1, 2, 0, 3, 13))
  x, w = (v.clone() for v in (cc.inputs(case, "mixed")["x"], cc.inputs(case, "mixed")["w"]))
  x[0, 3, 2, 2], x[1, 5, 4, 6], x[2, 7, 0, 0] = float("inf"), float("-inf"), float("nan")
  w[9, 3, 0, 0] = 0.0
  y = cc.conv64(case, x, w)
  col = y[0, :, 1, 1]
  assert bool(torch.isnan(col[9])) and bool(torch.isinf(col[torch.arange(128) != 9]).all())
  assert bool((torch.sign(col[torch.arange(128) != 9]) == torch.sign(w[torch.arange(128) != 9, 3, 0, 0].double())).all())
  assert bool(torch.isnan(y[2, :, 0, 0]).all()) and bool(torch.isfinite(y[2, :, 1:, 1:]).all())
  assert U32 == 2.0 ** -24


def test_shapes_of_the_gpu_file_reach_their_kernel_families():
  """The launch plans (host code of the instrumented library, no device needed) of the shapes that
  tests/test_gpu_conv_f64.py picks for kernel families: block tiles in both directions at 1 x 33 x 82 and not at the next
  smaller images; the persistent 64 -> 64 kernel; the stride-1 persistent kernel only behind its switch at 49 tiles."""
  import ctypes
  import os
  from iic_amd import _lib, geom
  from tests.test_gpu_conv_f64 import BLOCK_TILED, CONV_BD, CONV_P64, CONV_PW, P64_FORCED, PADDED, PW_FORCED, SMALL64, SMALL128
  dbg = os.path.join(os.path.dirname(_lib.LIB_PATH), "libiic_hip_dbg.so")
  assert os.path.exists(dbg), "build it: make -C iic_amd/csrc dbg"
  L = ctypes.CDLL(dbg)
  L.iic_debug_conv_plan.restype = None

  def plans(case):
    gs = [geom.fwd_geom(case.spec, case.N, case.H, case.W, case.P, case.P)] + geom.bwd_data_geoms(case.spec, case.N, case.H, case.W, case.P, case.P)
    out = []
    for g in gs:
      p = (ctypes.c_int * 12)()
      L.iic_debug_conv_plan(ctypes.byref(g), p)
      out.append(dict(kernel=p[0], wn=p[2], bw=p[5], mtiles=p[7], grid=p[8]))
    return out
  f, b = plans(BLOCK_TILED)
  assert (f["kernel"], f["wn"], b["kernel"], b["wn"]) == (CONV_BD, 2, CONV_BD, 1) and f["bw"] > 0 and b["bw"] > 0, (f, b)
  for H, W in ((32, 82), (33, 81)):
    f, b = plans(cc.Case(64, 128, 3, 1, 1, 1, H, W=W, P=3))
    assert not (f["bw"] > 0 and b["bw"] > 0), (H, W, f, b)
  assert all(p["kernel"] == CONV_P64 for p in plans(P64_FORCED) + plans(SMALL64))
  assert all(p["kernel"] == CONV_BD and p["bw"] == 0 for p in plans(PW_FORCED) + plans(SMALL128))
  try:
    L.iic_debug_enable_pw(2)
    L.iic_debug_pw_gx_cap(1)
    assert all((p["kernel"], p["mtiles"], p["grid"]) == (CONV_PW, 49, 8) for p in plans(PW_FORCED))
    L.iic_debug_p64_grid(2)
    assert all((p["kernel"], p["mtiles"], p["grid"]) == (CONV_P64, 19, 2) for p in plans(P64_FORCED))
  finally:
    L.iic_debug_enable_pw(1)
    L.iic_debug_pw_gx_cap(0)
    L.iic_debug_p64_grid(0)
  g = geom.fwd_geom(PADDED.spec, PADDED.N, PADDED.H, PADDED.W, PADDED.P, PADDED.P)
  assert g.MP > g.MY * g.MX and g.MP % 256 == 0
