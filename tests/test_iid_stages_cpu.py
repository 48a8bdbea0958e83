"""CPU proof of tests/iid_stage_cases.py and of the bounds of tests/parity.py that tests/test_gpu_iid_stages.py holds the
loss kernels to: the float64 references against independent ones (F.conv2d autograd on the oracle's joint, F.grid_sample,
oracle/iid_oracle.py), every precondition of every GPU case, seeded defects that the exact comparison must reject (with
the older criterion's verdict next to it), a CPU emulation of the bf16 three-term split inside its derived bound, and
seeded fp32 intermediates of the k x k stage outside theirs.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import iid_oracle
from tests import iid_stage_cases as sc
from tests.lattice import exact_mismatch, record
from tests.parity import SPLIT_D, fma_acc_bound_each, split_joint_bound, stage_bound, stage_n

REL = 1e-12


def close(got, ref, what, rel=REL):
  err = float((got - ref).abs().max())
  assert err <= rel * max(float(ref.abs().max()), 1e-300), (what, err)


# ---- the references against independent ones -------------------------------------------------------------------------------
def _theta(flips):
  t = torch.zeros((flips.shape[0], 2, 3), dtype=torch.float64)
  t[:, 0, 0] = 1.0 - 2.0 * flips[:, 0].double()
  t[:, 1, 1] = 1.0 - 2.0 * flips[:, 1].double()
  return t


@pytest.mark.parametrize("case", sc.SEG_CASES)
def test_seg_references_match_conv2d_autograd_on_the_oracle_joint(case):
  bn, k, h, w, T = case
  inp = sc.seg_inputs(case)
  ref = sc.seg_exact_reference(case)
  x1 = inp["x1"].double().requires_grad_(True)
  x2 = inp["x2"].double().requires_grad_(True)
  pij = iid_oracle._seg_joint(x1, x2, _theta(inp["flips"]), inp["mask"].double(), T)      # [k][k][2T+1][2T+1]
  close(pij.detach().permute(2, 3, 0, 1), ref["R"], "joint")
  G = sc.seg_G(inp["dR1u"], inp["dR2u"], inp["glu"], inp["gnlu"], T, k)
  (pij.permute(2, 3, 0, 1) * G).sum().backward()
  close(x1.grad, ref["du0"], "dx1")
  close(x2.grad, ref["du1"], "dx2")
  # collapsed: the same matrix at every shift
  Gc = sc.seg_G(inp["dR1c"], inp["dR2c"], inp["glc"], inp["gnlc"], T, k)
  x1.grad = x2.grad = None
  pij = iid_oracle._seg_joint(x1, x2, _theta(inp["flips"]), inp["mask"].double(), T)
  (pij.permute(2, 3, 0, 1) * Gc).sum().backward()
  close(x1.grad, ref["dc0"], "dx1 collapsed")
  close(x2.grad, ref["dc1"], "dx2 collapsed")


@pytest.mark.parametrize("shape", sc.WARP_SHAPES)
def test_warp_reference_matches_grid_sample(shape):
  N, K, H, W = shape
  inp = sc.warp_inputs(shape)
  rng = np.random.default_rng(3)
  extra = [("rotation", torch.from_numpy(rng.normal(0, 0.6, (N, 6)).astype(np.float32)) +
            torch.tensor([1.0, 0, 0, 0, 1.0, 0]), 0, 0)]
  extra.append(("rotation_shifted", extra[0][1], 2, -1))
  for name, M, sx, sy in sc.warp_matrices(shape) + extra:
    x = inp["x"].double().requires_grad_(True)
    grid = F.affine_grid(sc.pixel_to_theta(M, H, W), [N, K, H, W], align_corners=False)
    want = sc.shifted(F.grid_sample(x, grid, padding_mode="zeros", align_corners=False), sy, sx)
    (want + 0.0 * x.sum()).backward(inp["dout"].double())      # (a shift that empties the window cuts the graph)
    got = sc.warp_fwd_ref(inp["x"], M, sx, sy)
    assert float((got - want.detach()).abs().max()) <= 1e-9, name
    assert float((sc.warp_bwd_ref(inp["dout"], M, sx, sy) - x.grad).abs().max()) <= 1e-9, name


@pytest.mark.parametrize("case", sc.IID_CASES)
def test_clustering_references_match_the_oracle(case):
  H, bn, k = case
  inp = sc.iid_f64_inputs(case)
  R = sc.iid_joint_ref(inp["z"], inp["zt"])
  for h in range(H):
    z, zt = inp["z"][h].numpy(), inp["zt"][h].numpy()
    close(R[h], torch.from_numpy(iid_oracle.raw_joint_np(z, zt)), "raw joint")
    if k == 1:
      continue      # one class: the loss is identically 0 and so is the oracle's gradient
    st = sc.stage_ref(R[h][None, None].float(), 1.5, 0)
    Rh = R[h].float().double().numpy()
    loss, loss_nl, dR = iid_oracle.loss_and_grad_from_raw_np(Rh, 1.5, 0.5, -2.0)
    G = 0.5 * st["dR1"] - 2.0 * st["dR2"]
    close(G[0], torch.from_numpy(dR), "dR", 1e-10)
    dz, dzt = sc.iid_grad_ref(inp["z"][h][None], inp["zt"][h][None], torch.from_numpy(dR)[None])
    close(dz[0], torch.from_numpy(inp["zt"][h].double().numpy() @ dR.T), "dz")
    close(dzt[0], torch.from_numpy(inp["z"][h].double().numpy() @ dR), "dz'")


@pytest.mark.parametrize("case", sc.STAGE_CASES)
@pytest.mark.parametrize("kind", sc.STAGE_DRAWS)
def test_stage_reference_is_pinned_to_the_oracle(case, kind):
  """H = 1 slices, normaliser not detached: oracle/iid_oracle.py's closed form at 1e-12 relative."""
  H, k, nparts = case
  part = sc.stage_partials(case, kind)
  for lamb in sc.STAGE_LAMBS:
    st = sc.stage_ref(part, lamb, 0)
    for h in range(min(H, 2)):
      R = part[:, h].double().sum(0).numpy()
      loss, loss_nl, dR1 = iid_oracle.loss_and_grad_from_raw_np(R, lamb, 1.0, 0.0)
      _, _, dR2 = iid_oracle.loss_and_grad_from_raw_np(R, lamb, 0.0, 1.0)
      M = float(st["M1"][h])
      assert abs(float(st["loss1"][h]) - loss) <= REL * M and abs(float(st["loss2"][h]) - loss_nl) <= REL * M
      for got, want in ((st["dR1"][h], dR1), (st["dR2"][h], dR2)):
        assert float((got - torch.from_numpy(want)).abs().max()) <= REL * float(st["mag1"][h].max())


# ---- preconditions of every GPU case ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.SEG_CASES)
def test_seg_exact_preconditions(case):
  bn, k, h, w, T = case
  assert h != w
  inp = sc.seg_inputs(case)
  fl = set(map(tuple, inp["flips"].tolist()))
  assert bn < 4 or fl == {(0, 0), (1, 0), (0, 1), (1, 1)}
  assert set(inp["mask"].unique().tolist()) == set(sc.MASK_VALUES) or inp["mask"].numel() < 30
  for name in ("c", "u"):      # not symmetric
    assert k == 1 or not torch.equal(inp["dR1" + name], inp["dR1" + name].transpose(1, 2))
  record(**sc.seg_exact_reference(case)["figures"])      # the references assert the lattice preconditions


@pytest.mark.parametrize("case", sc.IID_CASES)
def test_clustering_exact_preconditions(case):
  inp = sc.iid_inputs(case)
  assert case[2] == 1 or not torch.equal(inp["dR1"], inp["dR1"].transpose(1, 2))
  record(**sc.iid_exact_reference(case)["figures"])
  for layout in sc.IID_LAYOUTS:
    sc.iid_layout(case, layout)


@pytest.mark.parametrize("shape", sc.WARP_SHAPES)
def test_warp_exact_preconditions(shape):
  N, K, H, W = shape
  inp = sc.warp_inputs(shape)
  seen_quarter = False
  for name, M, sx, sy in sc.warp_matrices(shape):
    out = sc.warp_fwd_ref(inp["x"], M, sx, sy)
    sc.assert_lattice(out, 16, name)
    sc.assert_lattice(sc.warp_fwd_ref(inp["x"].abs(), M.abs() * 0 + M, sx, sy), 16, name)
    sc.assert_lattice(sc.warp_bwd_ref(inp["dout"], M, sx, sy), 4, name)
    sc.assert_lattice(sc.warp_bwd_ref(inp["dout"].abs(), M, sx, sy), 4, name)
    if name.startswith("outside"):
      assert float(out.abs().max()) == 0.0
    seen_quarter |= name.startswith("half_xy")
  assert seen_quarter
  assert N * H * W == 1 or shape != sc.WARP_SHAPES[3] or (N * H * W > 256 and N * H * W % 256 != 0)


@pytest.mark.parametrize("case", sc.STAGE_CASES)
@pytest.mark.parametrize("kind", sc.STAGE_DRAWS)
def test_stage_clamp_gap_and_branches(case, kind):
  """No P and no marginal within 1e-6 relative of EPS (the branch taken does not hang on the last bit); the sparse draw
  clamps entries, the dead draw a marginal as well."""
  H, k, nparts = case
  part = sc.stage_partials(case, kind)
  assert bool((part >= 0).all())
  st = sc.stage_ref(part, 1.0, 0)
  for t in (st["P"], st["pi"], st["pj"]):
    assert sc.clamp_gap(t) > 1e-6
    assert bool(((t == 0) | (t > 1e3 * sc.EPS)).all()), "a clamped entry that is no exact zero"
  clamped_P = int((st["P"] < sc.EPS).sum())
  clamped_m = int((st["pi"] < sc.EPS).sum())
  assert (clamped_P > 0) == (kind != "dense" and (k > 2 or kind == "dead")) or k <= 3
  assert clamped_m == (H if kind == "dead" else 0)
  assert all(torch.isfinite(st[n]).all() for n in ("loss1", "loss2", "dR1", "dR2"))
  if H > 1:
    assert not torch.equal(part[:, 0], part[:, 1])


# ---- seeded defects ------------------------------------------------------------------------------------------------------------
def restated_joint(inp, T, defect=None):
  """The joint once more, term by term, with one seeded defect."""
  x1, x2, m, flips = inp["x1"].double(), inp["x2"].double(), inp["mask"].double()[:, None], inp["flips"]
  bn, k, h, w = x1.shape
  if defect == "flip_wrong_view":
    x1 = sc.flip_samples(x1, flips)
  else:
    x2 = sc.flip_samples(x2, flips)
  x2m = x2 * m * (m if defect == "mask_squared" else 1.0)
  if defect == "last_row_split":      # the rows of the last of bn h splits
    x2m = x2m.clone()
    x2m[bn - 1, :, h - 1] = 0
  nq = 2 * T + 1
  R = torch.zeros((nq, nq, k, k), dtype=torch.float64)
  for p in range(nq):
    for q in range(nq):
      ty, tx = (q - T, p - T) if defect == "axes_swapped" else (p - T, q - T)
      a = sc.shifted(x1, ty, tx) * m if defect == "mask_unshifted" else sc.shifted(x1 * m, ty, tx)
      if defect == "halo_column" and q == nq - 1 and p == T and T > 0:      # one row of one shift: the staged row ends one
        a = a.clone()                                                          # column early (the first row where that shows)
        live = (a[:, :, :, w - 1 - T].sum(1) * x2m[:, :, :, w - 1 - T].sum(1)).nonzero()[0]
        a[int(live[0]), :, int(live[1]), w - 1 - T] = 0
      R[p, q] = torch.einsum("nihw,njhw->ij", a, x2m)
  if defect == "third_tile":
    R[:, :, 32:, :] = 0
  return R


JOINT_DEFECTS = ["axes_swapped", "flip_wrong_view", "mask_unshifted", "mask_squared", "halo_column", "last_row_split",
                 "third_tile"]


@pytest.mark.parametrize("defect", JOINT_DEFECTS)
def test_exact_comparison_rejects_seeded_joint_defects(defect):
  case = (2, 33, 3, 12, 1) if defect == "third_tile" else (4, 15, 5, 13, 3)
  inp, ref = sc.seg_inputs(case), sc.seg_exact_reference(case)["R"]
  assert exact_mismatch(restated_joint(inp, case[4]), ref) is None
  bad = restated_joint(inp, case[4], defect)
  assert exact_mismatch(bad, ref) is not None
  older = float((bad - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
  record(defect=defect, case=list(case), exact_rejects=True, older_criterion_accepts=older)
  # the same defect on full-mantissa maps, where only the older criterion (2e-5 max) is available
  f = sc.seg_f64_inputs(case)
  good = restated_joint(f, case[4])
  bad = restated_joint(f, case[4], defect)
  record(defect=defect, draws="softmax", older_criterion_accepts=float((bad - good).abs().max()) <= 2e-5 * float(good.abs().max()),
         max_ratio=float((bad - good).abs().max() / good.abs().max()))


def test_exact_comparison_rejects_a_flipped_shift_sign_in_the_second_gradient():
  case = (4, 15, 5, 13, 3)
  bn, k, h, w, T = case
  inp, ref = sc.seg_inputs(case), sc.seg_exact_reference(case)
  x1m, x2m = sc.seg_maps(inp["x1"], inp["x2"], inp["mask"], inp["flips"])
  G = sc.seg_G(inp["dR1u"], inp["dR2u"], inp["glu"], inp["gnlu"], T, k)
  bad = torch.zeros_like(x1m)
  for p in range(2 * T + 1):
    for q in range(2 * T + 1):
      bad += torch.einsum("ij,nihw->njhw", G[p, q], sc.shifted(x1m, -(p - T), -(q - T)))      # the defect: - t for + t
  bad = sc.flip_samples(bad * inp["mask"].double()[:, None], inp["flips"])
  assert exact_mismatch(bad, ref["du1"]) is not None
  record(defect="shift_sign_which1", exact_rejects=True,
         older_criterion_accepts=float((bad - ref["du1"]).norm() / ref["du1"].norm()) <= 2e-5)
  # with the collapsed loss's symmetric matrix summed over a symmetric shift range the two signs agree on an image
  # without a mask -- the end-to-end tests' blind spot; the per-shift matrices above are what tells them apart


def test_exact_comparison_rejects_a_transposed_G_in_the_clustering_gradient():
  case = (2, 17, 31)
  inp, ref = sc.iid_inputs(case), sc.iid_exact_reference(case)
  G = sc.iid_G(inp, True)
  bad = torch.einsum("hab,hnb->hna", G, inp["z"].double())      # which = 1 reading G[a][b] for G[b][a]
  assert exact_mismatch(bad, ref["dzt", True]) is not None
  Gs = 0.5 * (G + G.transpose(1, 2))      # what the k x k stage produces: the defect is invisible end to end
  assert exact_mismatch(torch.einsum("hab,hnb->hna", Gs, inp["z"].double()), sc.iid_grad_ref(inp["z"], inp["zt"], Gs)[1]) is None
  record(defect="G_transposed_which1", exact_rejects=True, older_criterion_accepts=False, symmetric_G_hides_it=True)


def test_exact_comparison_rejects_an_omitted_zero_fill_of_the_sparse_shift():
  shape = sc.WARP_SHAPES[0]
  N, K, H, W = shape
  inp = sc.warp_inputs(shape)
  rejected = 0
  for name, M, sx, sy in sc.warp_matrices(shape):
    if (sx, sy) == (0, 0):
      continue
    ref = sc.warp_fwd_ref(inp["x"], M, sx, sy)
    # the defect: sample at M (o + s) wherever that lands, without the test on o + s itself
    Ms = M.double().clone()
    Ms[:, 2] += Ms[:, 0] * sx + Ms[:, 1] * sy
    Ms[:, 5] += Ms[:, 3] * sx + Ms[:, 4] * sy
    bad = sc.warp_fwd_ref(inp["x"], Ms, 0, 0)
    if exact_mismatch(bad, ref) is not None:
      rejected += 1
    record(defect="zero_fill_omitted", matrix=name, exact_rejects=exact_mismatch(bad, ref) is not None,
           older_criterion_accepts=float((bad - ref).abs().max()) <= 2e-5)
  assert rejected >= 2      # every shift that moves an inside source position out of the shifted window


# ---- the bf16 three-term split ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.SEG_BF16)
def test_emulated_split_contraction_stays_inside_its_bound_and_five_products_leave_it(case):
  bn, k, h, w, T = case
  f = sc.seg_f64_inputs(case)
  x1m, x2m = sc.seg_maps(f["x1"], f["x2"], f["mask"], f["flips"])
  for t in (x1m, x2m):      # the split is complete: x = h + m + l exactly, |m| <= 2^-8 |x|, |l| <= 2^-16 |x|
    hh, mm, ll = sc.split3(t.float())
    assert torch.equal(hh.double() + mm.double() + ll.double(), t.float().double())
    assert bool((mm.abs().double() <= 2.0 ** -8 * t.abs()).all()) and bool((ll.abs().double() <= 2.0 ** -16 * t.abs()).all())
  assert torch.equal(x1m.float().double(), x1m)      # mask in {0, 1/2, 1}: the masked maps are fp32 numbers
  ref = sc.seg_joint_ref(x1m, x2m, T)      # operands >= 0: the joint is its own magnitude sum A
  terms = sc.seg_terms(case)[:, :, None, None]
  bound = split_joint_bound(terms, ref)
  six = sc.split_joint_emulated(x1m.float(), x2m.float(), T).double()
  worst = float(((six - ref).abs() / bound.clamp_min(1e-300)).max())
  assert bool(((six - ref).abs() <= bound).all()), worst
  five = sc.split_joint_emulated(x1m.float(), x2m.float(), T, sc.SIX[1:]).double()
  out = int((~((five - ref).abs() <= bound)).sum())
  record(case=list(case), split_six_worst_ratio=worst, five_products_outside=out, d=SPLIT_D)
  # m m' is 2^-16 of a product at most and enters with both signs; the accumulation term of the bound is 6 terms 2^-24.
  # Only an entry with a handful of pixel products can tell the two apart: the shifts that leave a corner of the image
  # overlapping.  (2, 2, 4, 8, 10) has them; the other three cases' smallest overlap is 88 pixels or more and the
  # five-product variant stays inside their bound -- recorded above, not asserted.
  if float(terms[terms > 0].min()) <= 8:
    assert out > 0, "dropping m m' stays inside the bound"
  assert bool((fma_acc_bound_each(terms, ref) <= bound).all())


# ---- seeded fp32 intermediates of the k x k stage ------------------------------------------------------------------------------------
def _log32(t):
  return torch.log(t.float()).double()


@pytest.mark.parametrize("case", sc.STAGE_CASES)
@pytest.mark.parametrize("kind", sc.STAGE_DRAWS)
def test_fp32_intermediates_leave_the_stage_bound(case, kind):
  """A float `logf` and a float accumulator of the k k-term sums each leave the bound on at least one output.  The reference
  itself, recomputed in another summation order (the partials summed last), stays inside."""
  H, k, nparts = case
  part = sc.stage_partials(case, kind)
  st = sc.stage_ref(part, 1.5, 0)
  n = stage_n(k, nparts)

  def outside(v):
    cnt = 0
    for name, mag in (("loss1", "M1"), ("loss2", "M2"), ("dR1", "mag1"), ("dR2", "mag2")):
      err = (v[name].float().double() - st[name]).abs()
      cnt += int((~(err <= stage_bound(st[name], st[mag], k, nparts))).sum())
    return cnt
  assert outside(st) == 0
  perm = sc.stage_ref(part.flip(0), 1.5, 0)
  assert outside(perm) == 0
  res = dict(case=list(case), kind=kind, n=n, log32_outside=outside(sc.stage_ref(part, 1.5, 0, log=_log32)),
             sum32_outside=outside(sc.stage_ref(part, 1.5, 0, sum32=True)))
  record(**res)
  assert res["log32_outside"] > 0 and res["sum32_outside"] > 0, res
