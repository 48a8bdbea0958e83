"""Times one Lloyd iteration of iic_amd.kmeans (csrc/kmeans.hip) against the composition a user would write today on the
same device, in one process:

  hip  : iic_kmeans_assign (norms, X.C^T on the fp32 MFMA pipe, arg-min, one-hot sums, fixed-order reduce) + iic_kmeans_update
  torch: (X * X).sum(1), (C * C).sum(1), X @ C.T, min over the n x k matrix, index_add_ of the rows, bincount, the division

Both sides restore the centroids before every iteration (a k x d copy), so that every iteration does the same work.  Before
anything is timed the two sides' labels are compared (they may differ on rows whose two best scores are an fp32 rounding
apart).  After a warm-up the rounds alternate between the two sides; each round puts device events around `--iters`
back-to-back iterations; reported: median and min..max per iteration over the rounds, and the X bytes per second of the
hip side (n * d * 4 bytes over the median).

Then a whole default fit (k-means++, n_init=10) at the shapes named by --fit, wall clock around fit() + synchronise, next to
one Lloyd iteration of the float64 numpy arithmetic on the host and, where scikit-learn is installed, its whole fit.

    python tools/kmeans_perf.py [--shapes 13000x512x10 70000x4608x10 1000000x512x27] [--fit 13000x512x10 70000x4608x10]
                                [--rounds 9] [--iters 5] [--sklearn_max 10000000] [--out FILE]

Needs a GPU; there is no CPU fall-back."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from iic_amd import kmeans   # noqa: E402


def make_data(n, d, k, dev, seed=0):
  g = torch.Generator(device=dev)
  g.manual_seed(seed)
  centres = torch.randn((k, d), device=dev, generator=g) * 1.5
  which = torch.randint(0, k, (n,), device=dev, generator=g)
  X = torch.randn((n, d), device=dev, generator=g)
  X += centres[which]
  C0 = X[torch.randperm(n, device=dev, generator=g)[:k]].contiguous()
  return X, C0


def torch_iter(X, C):
  k = C.shape[0]
  xn = (X * X).sum(1)
  cn = (C * C).sum(1)
  S = cn[None, :] - 2.0 * (X @ C.t())
  best, labels = S.min(1)
  mind = (best + xn).clamp_min_(0)
  sums = torch.zeros_like(C).index_add_(0, labels, X)
  counts = torch.bincount(labels, minlength=k)
  C.copy_(sums / counts.clamp_min(1)[:, None].to(sums.dtype))
  return labels, mind


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", nargs="*", default=["13000x512x10", "70000x4608x10", "1000000x512x27"])
  ap.add_argument("--fit", nargs="*", default=["13000x512x10", "70000x4608x10"])
  ap.add_argument("--rounds", type=int, default=9)
  ap.add_argument("--iters", type=int, default=5)
  ap.add_argument("--sklearn_max", type=int, default=10 ** 7, help="largest n * d scikit-learn's fit is timed at")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  assert args.rounds >= 7
  dev = torch.device("cuda:0")
  lines = []

  def say(s):
    print(s)
    sys.stdout.flush()
    lines.append(s)

  say("device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
  for shape in args.shapes:
    n, d, k = (int(v) for v in shape.split("x"))
    X, C0 = make_data(n, d, k, dev)
    buf = kmeans._Buffers(X, k)
    state = torch.zeros((kmeans.STATE_BYTES,), dtype=torch.uint8, device=dev)
    Ch, Ct = C0.clone(), C0.clone()

    def hip_iter():
      Ch.copy_(C0)
      state.zero_()
      kmeans._assign(X, Ch, buf, state=state)
      kmeans._update(Ch, buf, state, force=1)

    def torch_side():
      Ct.copy_(C0)
      return torch_iter(X, Ct)

    hip_iter()
    lt, _ = torch_side()
    torch.cuda.synchronize()
    differ = int((buf.labels.long() != lt).sum())
    cdiff = float((Ch - Ct).abs().max())
    say("%s: labels that differ between the sides %d of %d, max |centre difference| %.3g" % (shape, differ, n, cdiff))
    for _ in range(3):
      hip_iter()
      torch_side()
    torch.cuda.synchronize()
    times = {"hip": [], "torch": []}
    for _ in range(args.rounds):
      for name, fn in (("hip", hip_iter), ("torch", torch_side)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
          fn()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) / args.iters)
    for name in ("hip", "torch"):
      t = np.array(times[name])
      say("%s %-5s: median %.4f ms (min %.4f .. max %.4f) per iteration over %d rounds of %d"
          % (shape, name, np.median(t), t.min(), t.max(), args.rounds, args.iters))
    mh, mt = np.median(times["hip"]), np.median(times["torch"])
    say("%s: torch / hip = %.2f; X bytes / hip time = %.0f GB/s (X is read twice by the kernel)"
        % (shape, mt / mh, n * d * 4 / (mh * 1e-3) / 1e9))
    del X, buf
    torch.cuda.empty_cache()

  for shape in args.fit:
    n, d, k = (int(v) for v in shape.split("x"))
    X, _ = make_data(n, d, k, dev)
    km = kmeans.KMeans(k)
    km.fit(X)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    km = kmeans.KMeans(k).fit(X)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    say("%s: default fit (k-means++, n_init=10) %.3f s on the device, inertia %.6g, n_iter of the best run %d"
        % (shape, t1 - t0, km.inertia_, km.n_iter_))
    Xh = X.cpu().numpy().astype(np.float64)
    Ch = km.cluster_centers_.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    S = (Ch * Ch).sum(1)[None, :] - 2.0 * (Xh @ Ch.T)
    labels = np.argmin(S, axis=1)
    sums = np.zeros_like(Ch)
    np.add.at(sums, labels, Xh)
    t1 = time.perf_counter()
    say("%s: ONE Lloyd iteration of the float64 numpy arithmetic on the host %.3f s (labels equal to the fit's: %s)"
        % (shape, t1 - t0, bool((labels == km.labels_.cpu().numpy()).all())))
    if n * d > args.sklearn_max:
      say("%s: scikit-learn's fit skipped above --sklearn_max = %d values" % (shape, args.sklearn_max))
      del X
      torch.cuda.empty_cache()
      continue
    try:
      from sklearn.cluster import KMeans as SkKMeans
    except ImportError:
      say("%s: scikit-learn is not installed here" % shape)
    else:
      t0 = time.perf_counter()
      sk = SkKMeans(n_clusters=k, n_init=10, random_state=0).fit(Xh.astype(np.float32))
      t1 = time.perf_counter()
      say("%s: scikit-learn KMeans(n_init=10) on the host %.3f s, inertia %.6g" % (shape, t1 - t0, sk.inertia_))
    del X
    torch.cuda.empty_cache()
  if args.out:
    with open(args.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
