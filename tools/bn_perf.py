"""A/B timing of the BatchNorm backward passes at the north-star layer shapes (660 images/view):
first-generation (row-per-block) vs second-generation (pixel walkers) kernels.
GB/s = algorithmic bytes: reduce reads dout + y, apply reads dout + y and writes dy (bf16).

--frozen: the one-pass backward of a BatchNorm on running statistics (iic_bn_bwd_frozen: reads dout + y, writes dy)
against its yardstick, the two-pass composition of the batch-statistics kernels with bcoef = (scale, 0, 0)
(iic_bn_bwd_reduce + iic_bn_bwd_finalize + iic_bn_bwd_apply: five tensor streams), at 660 x {48x48x64, 24x24x128,
12x12x256, 6x6x512}, P = 1.  The two are timed alternately, --rounds times --iters launches each; median and
[min, max] over the rounds go to stdout and to --out."""
import argparse, ctypes, os, sys
import torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
os.environ.setdefault("IIC_HIP_LIB", "dbg")      # the iic_debug_* switches live in libiic_hip_dbg.so only (make -C iic_amd/csrc dbg)
from iic_amd import ops, _lib   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=660)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--blocks", type=int, nargs="*", default=[1024])
ap.add_argument("--frozen", action="store_true")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=None)
a = ap.parse_args()
L = ctypes.CDLL(_lib.LIB_PATH)
d = torch.device("cuda:0")
shapes = [(49, 64), (25, 128), (13, 256), (7, 512)]


def timeit(fn):
  fn(); torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(a.iters):
    fn()
  e1.record(); torch.cuda.synchronize()
  return e0.elapsed_time(e1) / a.iters * 1e3     # us


def frozen_case():
  import statistics
  lines = ["# iic_bn_bwd_frozen (one pass) vs iic_bn_bwd_reduce + iic_bn_bwd_finalize + iic_bn_bwd_apply with bcoef = (scale, 0, 0)",
           "# N = %d, P = 1, %d rounds x %d launches, alternating; us per backward: median [min, max]; TB/s of the one pass = 3 streams"
           % (a.n, a.rounds, a.iters)]
  for (H, C) in [(48, 64), (24, 128), (12, 256), (6, 512)]:
    N, P = a.n, 1
    shape = (N, H + 2, H + 2, C)
    dout, y, y2 = (torch.randn(shape, device=d).to(torch.bfloat16) for _ in range(3))
    act = torch.relu(torch.randn(shape, device=d)).to(torch.bfloat16)
    dy, dy2 = (torch.zeros(shape, dtype=torch.bfloat16, device=d) for _ in range(2))
    coef, coef2 = torch.randn(5, C, device=d), torch.randn(5, C, device=d)
    coef[3], coef2[3] = coef[3].abs() + 0.5, coef2[3].abs() + 0.5
    gamma = torch.ones(C, device=d)
    bc, bc2 = torch.zeros(3, C, device=d), torch.zeros(3, C, device=d)      # (scale, 0, 0)
    bc[0], bc2[0] = coef[0], coef2[0]
    sums, sums2 = ops.new_stats(C, d), ops.new_stats(C, d)
    nbytes = N * H * H * C * 2
    for mode, aa, mc, two in (("none", None, None, False), ("from_y", None, coef, False), ("act", act, None, False),
                              ("none+bn2", None, None, True)):
      k2 = dict(y2=y2, coef2=coef2, dy2=dy2, sums2=sums2) if two else {}

      def one_pass():
        ops.bn_bwd_frozen(dout, aa, y, coef, dy, sums, N, H, H, P, C, mask_coef=mc, **k2)

      def two_pass():
        ops.bn_bwd_reduce(dout, aa, y, sums, N, H, H, P, C, mask_coef=mc, y2=y2 if two else None, sums2=sums2 if two else None)
        ops.bn_bwd_finalize(sums, gamma, coef, C, N * H * H)          # (dgamma, dbeta; re-zeroes the sums)
        if two:
          ops.bn_bwd_finalize(sums2, gamma, coef2, C, N * H * H)
        ops.bn_bwd_apply(dout, aa, y, bc, dy, N, H, H, P, C, mask_coef=mc, y2=y2 if two else None,
                         bcoef2=bc2 if two else None, dy2=dy2 if two else None)
      t1, t2 = [], []
      for _ in range(a.rounds):
        t1.append(timeit(one_pass))
        t2.append(timeit(two_pass))
      m1, m2 = statistics.median(t1), statistics.median(t2)
      streams = 3 + (1 if aa is not None else 0) + (2 if two else 0)
      lines.append("H=%2d C=%3d %-9s one-pass %7.1f [%7.1f, %7.1f] us %5.2f TB/s | two-pass %7.1f [%7.1f, %7.1f] us | ratio %.3f"
                   % (H, C, mode, m1, min(t1), max(t1), streams * nbytes / m1 / 1e6, m2, min(t2), max(t2), m1 / m2))
      print(lines[-1], flush=True)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if a.frozen:
  frozen_case()
  sys.exit(0)

tot = {}
for (H, C) in shapes:
  N, P = a.n, 1
  shape = (N, H + 2, H + 2, C)
  dout = torch.randn(shape, device=d).to(torch.bfloat16)
  y = torch.randn(shape, device=d).to(torch.bfloat16)
  act = torch.relu(torch.randn(shape, device=d)).to(torch.bfloat16)
  dy = torch.zeros(shape, dtype=torch.bfloat16, device=d)
  coef = torch.randn(4, C, device=d)
  bcoef = torch.randn(3, C, device=d)
  sums = ops.new_stats(C, d)
  nbytes = N * H * H * C * 2
  for label, gen, blocks in [("v1", 0, 0)] + [("v2/%d" % b, 2, b) for b in a.blocks]:
    L.iic_debug_bn_v2(gen, blocks)
    for mode, aa, mc in (("act", act, None), ("from_y", None, coef)):
      t_r = timeit(lambda: ops.bn_bwd_reduce(dout, aa, y, sums, N, H, H, P, C, mask_coef=mc))
      t_a = timeit(lambda: ops.bn_bwd_apply(dout, aa, y, bcoef, dy, N, H, H, P, C, mask_coef=mc))
      rb = (3 if aa is not None else 2) * nbytes
      ab = (4 if aa is not None else 3) * nbytes
      print("H=%2d C=%3d %-8s %-6s reduce %7.1f us %5.2f TB/s | apply %7.1f us %5.2f TB/s"
            % (H, C, label, mode, t_r, rb / t_r / 1e6, t_a, ab / t_a / 1e6))
      tot[(label, "r")] = tot.get((label, "r"), 0) + t_r
      tot[(label, "a")] = tot.get((label, "a"), 0) + t_a
L.iic_debug_bn_v2(1, 1024)
print({k: round(v, 1) for k, v in tot.items()})
