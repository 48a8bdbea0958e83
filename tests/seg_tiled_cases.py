"""Cases, seeds and seeded defects for the tiled segmentation-loss kernels (csrc/seg_loss_tiled.hip: beyond 48 classes and
256-pixel rows), shared by tests/test_seg_tiled_cpu.py (which proves them without a GPU) and tests/test_gpu_seg_tiled.py
(which holds the kernels to them).  A helper module, not a test file.

Generators, references and preconditions are those of tests/iid_stage_cases.py: dyadic-lattice inputs on which every
product and every partial sum is exact in fp32 in any order, so the kernels must reproduce the float64 reference exactly.
The cases are the smallest shapes at which a window edge or a class-block edge can go wrong; the decompositions restated
here in float64 (windowed_joint, blocked_joint) exist to show that the exact comparison catches such an edge going wrong,
not to check the kernels."""
import functools

import torch

from tests import iid_stage_cases as sc

# (bn, k, h, w, T)
WINDOWS_ALIGNED = [(2, 3, 3, 260, 1), (1, 16, 2, 264, 10),      # a T = 10 halo across column 256, 8 columns beyond it
                   (2, 5, 2, 516, 2),                           # three windows
                   (1, 24, 2, 320, 3), (1, 3, 2, 260, 10)]
WINDOWS_UNALIGNED = [(2, 4, 3, 257, 2), (1, 17, 2, 301, 1)]      # w % 4 != 0
CLASS_BLOCKS = [(2, 49, 3, 8, 1),                               # a fourth tile holding one class
                (2, 64, 2, 12, 2), (1, 97, 2, 16, 1), (2, 50, 2, 9, 1), (1, 49, 2, 8, 10)]
BOTH = [(1, 49, 2, 260, 1), (1, 80, 2, 272, 2)]
CASES = WINDOWS_ALIGNED + WINDOWS_UNALIGNED + CLASS_BLOCKS + BOTH
F64_CASES = [(1, 16, 2, 264, 10), (2, 5, 2, 516, 2), (2, 64, 2, 12, 2), (1, 97, 2, 16, 1), (1, 49, 2, 260, 1)]
# shapes today's kernels serve too (tests/iid_stage_cases.py SEG_STREAM): the tiled entries must give their bits
SHARED = [(2, 48, 2, 136, 1), (2, 16, 3, 132, 2)]
# the shapes tools/seg_tiled_perf.py times (LAB.md S18): --input_sz 320 / 512 and k_A = 3 gt_k
WORKLOAD = [(8, 45, 320, 320, 10), (4, 24, 512, 512, 10), (16, 81, 128, 128, 10), (8, 96, 200, 200, 5)]
GRADS = ("dc0", "dc1", "du0", "du1")
MAX_SEED = 16


@functools.lru_cache(maxsize=None)
def case_seed(case):
  """The lowest seed at which all four gradient references of the case are non-zero (the upstream gradients are drawn
  from {1, -2, 1/2, 0}: with both drawn as 0 a collapsed gradient is all zero and its check is vacuous)."""
  for seed in range(MAX_SEED):
    ref = sc.seg_exact_reference(case, seed)
    if all(bool(ref[g].abs().max() > 0) for g in GRADS):
      return seed
  raise AssertionError("%s: no seed below %d gives four non-zero gradient references" % (case, MAX_SEED))


def inputs(case):
  return sc.seg_inputs(case, case_seed(case))


def reference(case):
  ref = sc.seg_exact_reference(case, case_seed(case))
  for g in GRADS:
    assert bool(ref[g].abs().max() > 0), (case, g)
  return ref


# ---- the decompositions, restated in float64, and the defects the exact comparison must reject ---------------------------
def windows(w, ws):
  """[(x0, width)] of the column windows of a row of w pixels at window pitch ws."""
  return [(x0, min(ws, w - x0)) for x0 in range(0, w, ws)]


def _cols(t, lo, hi):
  """t with every column outside [lo, hi) zeroed."""
  out = torch.zeros_like(t)
  lo, hi = max(lo, 0), min(hi, t.shape[-1])
  if lo < hi:
    out[..., lo:hi] = t[..., lo:hi]
  return out


def windowed_joint(x1m, x2m, T, ws, defect=None):
  """The joint as a sum over column windows: x2m on [x0, x0 + n), x1m on [x0 - T, x0 + n + T).
  defect "no_halo": x1m on [x0, x0 + n) only; "off_by_one": every window but the first starts one column late."""
  R = None
  for x0, n in windows(x1m.shape[-1], ws):
    lo = x0 + 1 if (defect == "off_by_one" and x0 > 0) else x0
    halo = 0 if defect == "no_halo" else T
    r = sc.seg_joint_ref(_cols(x1m, lo - halo, x0 + n + halo), _cols(x2m, lo, x0 + n), T)
    R = r if R is None else R + r
  return R


def blocked_joint(x1m, x2m, T, bs, defect=None):
  """The joint assembled from (i block, j block) pairs of bs classes: block (bi, bj) contracts classes [i0, i0 + bs) of
  x1m with classes [j0, j0 + bs) of x2m.  defect "transposed": an off-diagonal block reads x1m at j0 and x2m at i0."""
  k = x1m.shape[1]
  nq = 2 * T + 1
  R = torch.zeros((nq, nq, k, k), dtype=torch.float64)
  for i0 in range(0, k, bs):
    for j0 in range(0, k, bs):
      a0, b0 = (j0, i0) if defect == "transposed" else (i0, j0)
      ni, nj = min(bs, k - i0), min(bs, k - j0)
      shape = (x1m.shape[0], bs) + tuple(x1m.shape[2:])      # a block as the kernel stages it: bs classes, zero past k
      a, b = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
      na, nb_ = min(bs, k - a0), min(bs, k - b0)
      a[:, :na] = x1m[:, a0:a0 + na]
      b[:, :nb_] = x2m[:, b0:b0 + nb_]
      R[:, :, i0:i0 + ni, j0:j0 + nj] = sc.seg_joint_ref(a, b, T)[:, :, :ni, :nj]
  return R
