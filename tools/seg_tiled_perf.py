"""Microbenchmark of the tiled segmentation-loss kernels (csrc/seg_loss_tiled.hip; no network):
  python tools/seg_tiled_perf.py [reps] [--out FILE]
prints, per shape, ms per launch of iic_seg_tiled_joint_raw and of each iic_seg_tiled_grad (collapsed, as the published
loss runs it), the fp32-MFMA rate and the time per useful GFLOP, counting 2 bn h w k^2 (2T+1)^2 per pass.  The shared
shape (60, 45, 128, 128, 10) is timed on the tiled entries and on today's streaming kernels in the same run, alternating.
Timing as tools/seg_kernel_perf.py: device events around `reps` launches after a warm-up launch of the same shape."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from iic_amd._lib import check, lib, ptr, stream_ptr

WORKLOAD = [(8, 45, 320, 320, 10), (4, 24, 512, 512, 10), (16, 81, 128, 128, 10), (8, 96, 200, 200, 5)]
SHARED = (60, 45, 128, 128, 10)
PEAK_TF = 157.3      # fp32 MFMA (tools/seg_kernel_perf.py)


def entries(shape, tiled):
  """{name: launch} for the joint and the two collapsed gradients of a shape, on the tiled or the resident entries."""
  bn, k, h, w, T = shape
  dev = torch.device("cuda:0")
  g = torch.Generator().manual_seed(0)
  x1 = torch.softmax(torch.randn(bn, k, h, w, generator=g), 1).to(dev)
  x2 = torch.softmax(torch.randn(bn, k, h, w, generator=g), 1).to(dev)
  mask = (torch.rand(bn, h, w, generator=g) < 0.8).float().to(dev)
  flips = torch.tensor([[i & 1, 0] for i in range(bn)], dtype=torch.int32).to(dev)
  L = lib()
  nq = 2 * T + 1
  ns = L.iic_seg_tiled_joint_nsplit(bn, h, w, k, T) if tiled else L.iic_seg_joint_nsplit(bn, h, k, T)
  part = torch.empty((ns, nq * nq, k, k), device=dev)
  dR1, dR2 = torch.randn(1, k, k, generator=g).to(dev), torch.randn(1, k, k, generator=g).to(dev)
  g1, g2 = torch.randn(1, generator=g).to(dev), torch.randn(1, generator=g).to(dev)
  wsb = L.iic_seg_tiled_grad_workspace_bytes(k, T, 1) if tiled else L.iic_seg_grad_workspace_bytes(k, T)
  ws = torch.empty(wsb // 4, device=dev)
  out = torch.empty_like(x1)
  jfn = L.iic_seg_tiled_joint_raw if tiled else L.iic_seg_joint_raw
  gfn = L.iic_seg_tiled_grad if tiled else L.iic_seg_grad

  def joint():
    check(jfn(ptr(x1), ptr(x2), ptr(mask), ptr(flips), ptr(part), bn, k, h, w, T, ns, stream_ptr()), "joint")

  def grad(wh):
    src = x2 if wh == 0 else x1
    check(gfn(ptr(src), ptr(mask), ptr(flips), ptr(dR1), ptr(dR2), ptr(g1), ptr(g2), ptr(out), bn, k, h, w, T, wh, 1,
              ptr(ws), stream_ptr()), "grad")
  return {"joint": joint, "grad dx1": lambda: grad(0), "grad dx2": lambda: grad(1)}, ns


def time_ms(fn, reps):
  fn(); torch.cuda.synchronize()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    fn()
  e1.record(); torch.cuda.synchronize()
  return e0.elapsed_time(e1) / reps


def main():
  args = sys.argv[1:]
  out = None
  if "--out" in args:
    i = args.index("--out")
    out = open(args[i + 1], "w")
    del args[i:i + 2]
  reps = int(args[0]) if args else 3
  assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"

  def emit(line):
    print(line, flush=True)
    if out:
      out.write(line + "\n")
      out.flush()

  def report(tag, shape, name, ms):
    bn, k, h, w, T = shape
    gflop = 2.0 * bn * h * w * k * k * (2 * T + 1) ** 2 / 1e9
    emit("%-8s %-22s %-9s %9.3f ms  %6.2f TF/s (%.3f of %.1f)  %8.3f us/GFLOP" % (
      tag, shape, name, ms, gflop / ms, gflop / ms / PEAK_TF, PEAK_TF, 1e3 * ms / gflop))

  emit("# reps %d; useful FLOP = 2 bn h w k^2 (2T+1)^2 per pass; collapsed gradients" % reps)
  for shape in WORKLOAD:
    fns, ns = entries(shape, True)
    emit("# %s: tiled nsplit %d" % (shape, ns))
    for name, fn in fns.items():
      report("tiled", shape, name, time_ms(fn, reps))
  tiled, nt = entries(SHARED, True)
  resident, nr = entries(SHARED, False)
  emit("# %s: tiled nsplit %d, resident nsplit %d; alternating, two rounds" % (SHARED, nt, nr))
  for rnd in range(2):
    for name in tiled:
      report("tiled", SHARED, name, time_ms(tiled[name], reps))
      report("resident", SHARED, name, time_ms(resident[name], reps))
  # the k > 32 head's weight gradient dW[k][C] = dlog^T F: fixed-order partials + fold against the atomic split-K GEMM
  for (n, hw, k) in ((75, 102, 45), (8, 162, 81)):
    M, C = n * hw * hw, 512
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    dlog, Fm = torch.randn(M, k, generator=g).to(dev), torch.randn(M, C, generator=g).to(dev)
    L = lib()
    nch = L.iic_seg_head_wgrad_chunks(M)
    part, dW = torch.empty((nch, k * C), device=dev), torch.zeros((k, C), device=dev)
    splitk = max(1, min(512, M // 2048))

    def fixed():
      check(L.iic_seg_window_wgrad(ptr(dlog), ptr(Fm), ptr(part), M, C, k, stream_ptr()), "wgrad")
      check(L.iic_colsum_f32(ptr(part), ptr(dW), nch, k * C, 0, stream_ptr()), "colsum")

    def atomic():
      dW.zero_()
      check(L.iic_gemm_f32_splitk(ptr(dlog), 1, k, ptr(Fm), C, 1, ptr(dW), C, k, C, M, splitk, stream_ptr()), "splitk")
    for rnd in range(2):
      emit("head dW   M %d C %d k %d: partials + fold %8.3f ms, atomic split-K %8.3f ms" % (
        M, C, k, time_ms(fixed, reps), time_ms(atomic, reps)))
  if out:
    out.close()


if __name__ == "__main__":
  main()
