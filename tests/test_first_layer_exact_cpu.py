"""The exact-arithmetic harness of tests/test_gpu_first_layer_exact.py, proven without a GPU.

A plain float64 restatement of the ClusterNet5g stem (patches, convolution, BatchNorm affine map, ReLU, the 2x2 / stride 2 /
padding 1 max-pool with first-maximum routing, the four sums, dW directly and as c1*G1 + c2*G2 + c3*G3) and of the three
products of the segmentation head is held against the float64 torch references of tests/lattice.py on the generators and
preconditions the GPU tests use -- so a precondition that fails, fails here first.  Then defects of the kinds a kernel can
have, each confined to ONE term, are seeded into the restatement: the exact comparison must reject every one, and the
criterion the older GPU test applies to that quantity is evaluated next to it.  What the older criterion says is
deterministic here and asserted as it came out; a defect it rejects as well stays in the file and is reported as such.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lattice as L
from tests.lattice import assert_exact, exact_mismatch, record


# ----------------------------------------------------------------------------------------------------------------------
# plain restatements
# ----------------------------------------------------------------------------------------------------------------------
def stem_plain(inp, defect=None):
  """The stem in numpy float64.  defect: None, or one of
     "tap"      -- input channel 0 of the centre tap dropped from the convolution at the last image column of one row of
                   one image (the recomputed y of every pass; the dW patch operand is staged separately);
     "tie"      -- ONE pool window whose positive maximum occurs twice routes its gradient to the last maximum;
     "stat"     -- the final pixel of the last row of the last image left out of sum y and sum y^2;
     "g3"       -- the row G3 excludes for tap (c, kh, kw) = (0, 0, 1), the image's last row, counted."""
  cin, H, W, N = inp["case"]
  x, w = inp["x"].double().numpy(), inp["w"].double().numpy().reshape(L.STEM_CO, cin * 9)
  sc, sh = (inp["coef"][i].double().numpy()[None, :, None, None] for i in (0, 1))
  c1, c2, c3 = (inp["bcoef"][i].double().numpy() for i in (0, 1, 2))
  dpool = inp["dpool"].double().numpy()
  xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
  patch = np.stack([xp[:, c, kh:kh + H, kw:kw + W] for c in range(cin) for kh in range(3) for kw in range(3)], 1)
  pf = patch
  if defect == "tap":
    rows = [(n, r) for n in range(N) for r in range(H) if patch[n, 4, r, W - 1] != 0]      # k = 4: (c, kh, kw) = (0, 1, 1)
    pf = patch.copy()
    pf[rows[0][0], 4, rows[0][1], W - 1] = 0.0
  y = np.einsum("ok,nkyx->noyx", w, pf)
  a = np.maximum(y * sc + sh, 0.0)
  Ho, Wo = H // 2 + 1, W // 2 + 1
  ap = np.full((N, L.STEM_CO, H + 2, W + 2), -1.0)      # -1: outside the image, below every activation
  ap[:, :, 1:H + 1, 1:W + 1] = a
  win = np.stack([ap[:, :, r::2, c::2] for r in (0, 1) for c in (0, 1)])      # scan order of the window
  best = win.max(0)
  am = win.argmax(0)                                     # first maximum
  if defect == "tie":
    last = 3 - win[::-1].argmax(0)
    cand = np.argwhere((last != am) & (best > 0) & (dpool != 0))
    am = am.copy()
    am[tuple(cand[0])] = last[tuple(cand[0])]
  gp = np.zeros_like(ap)
  for q, (r, c) in enumerate((r, c) for r in (0, 1) for c in (0, 1)):
    gp[:, :, r::2, c::2] += np.where((am == q) & (best > 0), dpool, 0.0)
  g = gp[:, :, 1:H + 1, 1:W + 1]
  ys = y
  if defect == "stat":
    ys = y.copy()
    ys[N - 1, :, H - 1, W - 1] = 0.0
  G1 = np.einsum("noyx,nkyx->ok", g, patch)
  G2 = np.einsum("noyx,nkyx->ok", y, patch)
  G3 = patch.sum((0, 2, 3))
  if defect == "g3":
    G3 = G3.copy()
    G3[1] += x[:, 0, H - 1, :].sum()
  dy = c1[None, :, None, None] * g + c2[None, :, None, None] * y + c3[None, :, None, None]
  t = torch.from_numpy
  return dict(y=t(y), pool=t(np.maximum(best, 0.0)), sum_y=t(ys.sum((0, 2, 3))), sum_yy=t((ys * ys).sum((0, 2, 3))),
              g=t(g.copy()), sum_g=t(g.sum((0, 2, 3))), sum_gy=t((g * y).sum((0, 2, 3))),
              dW=t(np.einsum("noyx,nkyx->ok", dy, patch).reshape(L.STEM_CO, cin, 3, 3)),
              dW_combined=t((c1[:, None] * G1 + c2[:, None] * G2 + c3[:, None] * G3[None]).reshape(L.STEM_CO, cin, 3, 3)))


def head_plain(inp, logits_rows=None, dw_skip=None, sentinel=7.0):
  """The head's three products on the window matrix F [M][C] (the feature map inside a ring of zeros): logits = F W^T,
  dF = dlog W, dW = dlog^T F.  logits_rows: only that many rows are written, the rest keep `sentinel`; dw_skip: that row
  is left out of dW."""
  C, k, N, Hf = inp["case"]
  M = N * (Hf + 2) * (Hf + 2)
  Fm = np.pad(inp["f"].double().numpy(), ((0, 0), (0, 0), (1, 1), (1, 1))).transpose(0, 2, 3, 1).reshape(M, C)
  w = inp["w"].double().numpy().reshape(k, C)
  dlog = inp["dlog"].double().numpy().transpose(0, 2, 3, 1).reshape(M, k)
  logits = np.full((M, k), sentinel)
  n = M if logits_rows is None else logits_rows
  logits[:n] = Fm[:n] @ w.T
  keep = np.ones(M, bool)
  if dw_skip is not None:
    keep[dw_skip] = False
  dF = (dlog @ w).reshape(N, Hf + 2, Hf + 2, C)[:, 1:-1, 1:-1].transpose(0, 3, 1, 2)
  t = torch.from_numpy
  return dict(logits=t(logits), dx=t(np.ascontiguousarray(dF)), dW=t(dlog[keep].T @ Fm[keep]), Fm=Fm)


# ----------------------------------------------------------------------------------------------------------------------
# the criteria of the older GPU tests (tests/test_gpu_kernels.py, test_gpu_vgg.py, test_gpu_seg_net.py)
# ----------------------------------------------------------------------------------------------------------------------
def old_stem_mean(sum_y, ref_sum_y, cnt):
  return torch.allclose((sum_y / cnt).float(), (ref_sum_y / cnt).float(), atol=1e-4)


def old_stem_sqmean(sum_yy, ref_sum_yy, cnt):
  return torch.allclose((sum_yy / cnt).float(), (ref_sum_yy / cnt).float(), rtol=1e-4, atol=1e-4)


def old_stem_pool(pool, ref_pool):
  return float((pool - ref_pool).abs().max()) <= 1e-2 * float(ref_pool.abs().max())


def old_stem_dw(dW, ref_dW):
  return float((dW - ref_dW).abs().max()) <= 4e-3 * float(ref_dW.abs().max())


def old_firstconv_y(y, ref_y):
  return float((y - ref_y).abs().max()) <= 1e-2 * float(ref_y.abs().max())


def old_head_forward(logits, ref_logits, N, Hw, k, S=24):
  """test_seg_head_forward_backward sees the logits through softmax and the bilinear up-sampling, at 2e-5."""
  def up(l):
    p = F.softmax(l.reshape(N, Hw, Hw, k).permute(0, 3, 1, 2), dim=1)
    return F.interpolate(p, size=S, mode="bilinear", align_corners=False)
  return float((up(logits) - up(ref_logits)).abs().max()) <= 2e-5


def old_head_dw(dW, ref_dW):
  return torch.allclose(dW.float(), ref_dW.float(), rtol=1e-3, atol=1e-4 * float(ref_dW.abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# the generators, the preconditions and the references, on the CPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.STEM_CASES + [(1, 4, 256, 2), (3, 4, 254, 2), (1, 4, 204, 2), (5, 4, 186, 2)])
def test_stem_reference_preconditions_and_plain_restatement(case):
  inp = L.stem_inputs(case)
  ref = L.stem_reference(inp)             # asserts the preconditions
  got = stem_plain(inp)
  for key in ("y", "pool", "sum_y", "sum_yy", "g", "sum_g", "sum_gy", "dW"):
    assert_exact(got[key], ref[key], "plain stem %s" % key)
  assert_exact(got["dW_combined"], ref["dW"], "c1*G1 + c2*G2 + c3*G3")
  fig = ref["figures"]
  if case in L.STEM_CASES[:8]:      # the figures a CPU run of these cases gave when they were chosen
    assert fig["max_y"] <= 16 and fig["max_pool"] <= 32 and fig["sum_yy"] <= 3.5e5 and fig["max_dy"] <= 17
    assert fig["max_dW"] <= 1.5e4
  record(**fig)


@pytest.mark.parametrize("case", L.FIRSTCONV_CASES)
def test_firstconv_reference_preconditions(case):
  record(**L.firstconv_reference(L.firstconv_inputs(case))["figures"])


@pytest.mark.parametrize("case", L.SEG_HEAD_CASES + L.SEG_CHAIN_CASES)
def test_seg_head_reference_preconditions_and_plain_restatement(case):
  C, k, N, Hf = case
  inp = L.seg_head_inputs(case)
  ref = L.seg_head_reference(inp)
  got = head_plain(inp)
  for key in ("logits", "dx", "dW"):
    assert_exact(got[key], ref[key], "plain head %s" % key)
  assert ref["figures"]["max_logit"] <= 512 and ref["figures"]["max_dx"] <= 32
  record(**ref["figures"])


def test_seg_head_cases_cover_what_the_issue_asks():
  for C in (256, 512):
    assert sorted(set(c[1] for c in L.SEG_HEAD_CASES if c[0] == C)) == L.SEG_KS
  for small in (True, False):      # the k <= 16 and the k > 16 weight-gradient kernels
    assert set(c[2:] for c in L.SEG_HEAD_CASES if (c[1] <= 16) == small) == set(L.SEG_SHAPES)
  assert [N * (Hf + 2) ** 2 for N, Hf in L.SEG_SHAPES] == [300, 1083, 1024]


@pytest.mark.parametrize("shape", L.GEMM_SHAPES + [L.SPLITK_CASE])
def test_gemm_reference_preconditions(shape):
  inp = L.gemm_inputs(shape)
  m = max(float(L.gemm_reference(inp, b, a).abs().max()) for b in (False, True) for a in (False, True))
  assert m <= 4610
  record(shape=list(shape), max_C=m)


def test_stem_width_limits_follow_the_launch_arithmetic():
  """Largest served width per entry point and Cin (csrc/stem.hip: stem_check, stem_bwd_lds, stem_bwd_fits;
  csrc/stem_bwd2.hip: iic_stem_bwd2_supported).  The closed forms, for W a multiple of 16 and static s_cf = 1280 bytes:
  mode 0: 512 W; modes 1 / 2: 768 W + 1024 + 16 Cin (W + 10)."""
  assert L.stem_bwd_lds(5, 192, 1) == 512 * 192 + 256 * 192 + 1024 + 80 * 202 == 164640      # the issue's ~165 KB
  assert L.stem_bwd_lds(2, 96, 2) == 78144                                                    # tests/test_gpu_kernels.py
  assert L.stem_bwd_lds(1, 256, 0) + L.STEM_BWD_STATIC == 132352 <= L.LDS_BYTES
  assert L.stem_bwd_lds(5, 186, 1) + L.STEM_BWD_STATIC == 162848 <= L.LDS_BYTES < L.stem_bwd_lds(5, 188, 1) + 1280
  for entry in ("stats", "apply_pool", "bwd_reduce"):
    assert [L.stem_max_width(entry, c) for c in range(1, 6)] == [256] * 5
  assert [L.stem_max_width("bwd_wgrad", c) for c in range(1, 6)] == [204, 196, 192, 192, 186]
  assert [L.stem_max_width("bwd_fused", c) for c in range(1, 6)] == [254, 254, 254, 192, 186]
  assert [L.stem_max_width("bwd_fused", c, bwd2=False) for c in range(1, 6)] == [204, 196, 192, 192, 186]


# ----------------------------------------------------------------------------------------------------------------------
# seeded defects
# ----------------------------------------------------------------------------------------------------------------------
FLAGSHIP = (2, 96, 96, 2)
RAGGED = (4, 6, 34, 2)


def _verdicts(name, exact_rejects, old):
  """Every defect must be rejected by the exact comparison; `old` maps the older criterion's name to (accepted,
  expected)."""
  record(defect=name, exact_rejects=exact_rejects, old_accepts={k: v[0] for k, v in old.items()})
  assert exact_rejects, name
  for crit, (accepted, expected) in old.items():
    assert accepted == expected, "%s / %s: accepted = %s" % (name, crit, accepted)


def test_defect_one_channel_of_one_tap_dropped_at_the_last_column():
  inp = L.stem_inputs(FLAGSHIP)
  ref, bad = L.stem_reference(inp), stem_plain(inp, "tap")
  cnt = FLAGSHIP[3] * FLAGSHIP[1] * FLAGSHIP[2]
  assert int((bad["y"] != ref["y"]).any((1, 2, 3)).sum()) == 1 and int((bad["y"] != ref["y"]).any((0, 1, 2)).sum()) == 1
  for key in ("sum_y", "sum_yy", "pool", "dW"):
    assert exact_mismatch(bad[key], ref[key]) is not None, key
  _verdicts("tap", True, {
    "mean, atol 1e-4": (old_stem_mean(bad["sum_y"], ref["sum_y"], cnt), True),
    "second moment, rtol 1e-4 atol 1e-4": (old_stem_sqmean(bad["sum_yy"], ref["sum_yy"], cnt), True),
    "pool, 1e-2 of max": (old_stem_pool(bad["pool"], ref["pool"]), False),
    "dW, 4e-3 of max": (old_stem_dw(bad["dW"], ref["dW"]), True),
    "first conv output, 1e-2 of max": (old_firstconv_y(bad["y"], ref["y"]), False)})


def test_defect_pool_tie_routed_to_the_last_maximum():
  inp = L.stem_inputs(FLAGSHIP)
  ref, bad = L.stem_reference(inp), stem_plain(inp, "tie")
  assert int((bad["g"] != ref["g"]).sum()) == 2        # one gradient value moved inside one window
  assert exact_mismatch(bad["sum_g"], ref["sum_g"]) is None and exact_mismatch(bad["sum_gy"], ref["sum_gy"]) is None
  for key in ("dW", "dW_combined"):
    assert exact_mismatch(bad[key], ref["dW"]) is not None
  _verdicts("tie", True, {"dW, 4e-3 of max": (old_stem_dw(bad["dW"], ref["dW"]), True)})


def test_defect_last_pixel_of_the_ragged_segment_left_out_of_the_statistics():
  inp = L.stem_inputs(RAGGED)
  ref, bad = L.stem_reference(inp), stem_plain(inp, "stat")
  cnt = RAGGED[3] * RAGGED[1] * RAGGED[2]
  assert RAGGED[2] % 32 == 2
  rej = exact_mismatch(bad["sum_y"], ref["sum_y"]) is not None and exact_mismatch(bad["sum_yy"], ref["sum_yy"]) is not None
  _verdicts("stat", rej, {
    "mean, atol 1e-4": (old_stem_mean(bad["sum_y"], ref["sum_y"], cnt), False),
    "second moment, rtol 1e-4 atol 1e-4": (old_stem_sqmean(bad["sum_yy"], ref["sum_yy"], cnt), False)})
  # at the flagship shape one pixel is 1 / 18432 of the count: still above the mean's 1e-4 in some channel
  inp = L.stem_inputs(FLAGSHIP)
  ref, bad = L.stem_reference(inp), stem_plain(inp, "stat")
  cnt = FLAGSHIP[3] * FLAGSHIP[1] * FLAGSHIP[2]
  rej = exact_mismatch(bad["sum_y"], ref["sum_y"]) is not None and exact_mismatch(bad["sum_yy"], ref["sum_yy"]) is not None
  _verdicts("stat, flagship", rej, {"mean, atol 1e-4": (old_stem_mean(bad["sum_y"], ref["sum_y"], cnt), False)})


def test_defect_excluded_row_counted_in_g3():
  inp = L.stem_inputs(FLAGSHIP)
  ref, bad = L.stem_reference(inp), stem_plain(inp, "g3")
  assert exact_mismatch(bad["dW"], ref["dW"]) is None              # the direct form has no G3
  diff = (bad["dW_combined"] - ref["dW"]) != 0
  assert bool(diff.any()) and bool((diff.reshape(64, -1)[:, [0] + list(range(2, 18))] == 0).all())      # tap k = 1 only
  _verdicts("g3", exact_mismatch(bad["dW_combined"], ref["dW"]) is not None,
            {"dW, 4e-3 of max": (old_stem_dw(bad["dW_combined"], ref["dW"]), True)})


def test_defect_last_row_of_a_ragged_chunk_dropped_from_the_head():
  """Logits: M = 300 -- the last row of the ragged second 256-row workgroup is not written (the buffer keeps what it
  held).  That row is a corner of the window's ring, where the true logits are all zero, and softmax maps any constant
  row to the same uniform distribution: the older forward criterion cannot see it.  dW: M = 1083 -- the ring rows
  contribute nothing, so the defect drops the last row of the ragged second 1024-row chunk that carries features."""
  case = (512, 24, 3, 8)
  inp = L.seg_head_inputs(case)
  ref = L.seg_head_reference(inp)
  bad = head_plain(inp, logits_rows=299)
  _verdicts("head logits", exact_mismatch(bad["logits"], ref["logits"]) is not None,
            {"softmax + bilinear, 2e-5": (old_head_forward(bad["logits"], ref["logits"], 3, 10, 24), True)})
  case = (512, 24, 3, 17)
  inp = L.seg_head_inputs(case)
  ref = L.seg_head_reference(inp)
  Fm = head_plain(inp)["Fm"]
  row = max(m for m in range(1024, 1083) if np.abs(Fm[m]).sum() > 0)
  bad = head_plain(inp, dw_skip=row)
  assert int(((bad["dW"] - ref["dW"]).abs() > 1).sum()) == 0       # one unit at most per element
  _verdicts("head dW", exact_mismatch(bad["dW"], ref["dW"]) is not None,
            {"rtol 1e-3, atol 1e-4 of max": (old_head_dw(bad["dW"], ref["dW"]), False)})
