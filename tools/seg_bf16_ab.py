"""Segmentation joint: exact-fp32 MFMA (16x16x4 f32) against the three-term bf16 split on v_mfma_f32_16x16x32_bf16
(iic_debug_seg_bf16 0 against 2, round 6) at the BASELINE shapes -- ms per launch, and the difference of the partial
joints summed in float64.  The gradient has no bf16 kernel: profiles/r06_seg_bf16_ab.txt is the record of the one that was
measured (0.5-0.84x) and retired."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("IIC_HIP_LIB", "dbg")      # the iic_debug_* switches live in libiic_hip_dbg.so only (make -C iic_amd/csrc dbg)
import torch  # noqa: E402

from iic_amd import _lib  # noqa: E402
from iic_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402

CFG = {"coco3 k15 T10": (120, 15, 128, 128, 10, 0.6), "potsdam3 k24 T10": (75, 24, 200, 200, 10, 1.0),
       "coco3 head B k3 T10": (120, 3, 128, 128, 10, 0.6), "potsdam k24 T5": (75, 24, 200, 200, 5, 1.0)}


def run(which, reps=5):
  bn, k, h, w, T, dens = CFG[which]
  dev = torch.device("cuda:0")
  g = torch.Generator().manual_seed(0)
  x1 = torch.softmax(2 * torch.randn(bn, k, h, w, generator=g), 1).to(dev)
  x2 = torch.softmax(2 * torch.randn(bn, k, h, w, generator=g), 1).to(dev)
  mask = (torch.rand(bn, h, w, generator=g) < dens).float().to(dev)
  flips = torch.tensor([[i & 1, 0] for i in range(bn)], dtype=torch.int32).to(dev)
  L = lib()
  D = ctypes.CDLL(_lib.LIB_PATH)
  nq = 2 * T + 1
  H = nq * nq
  ns = L.iic_seg_joint_nsplit(bn, h, k, T)
  flops = 2.0 * bn * h * w * H * k * k
  res = {}
  try:
    for mode in (0, 2):
      D.iic_debug_seg_bf16(mode)
      part = torch.empty((ns, H, k, k), device=dev)

      def joint():
        check(L.iic_seg_joint_raw(ptr(x1), ptr(x2), ptr(mask), ptr(flips), ptr(part), bn, k, h, w, T, ns, stream_ptr()), "j")

      joint(); torch.cuda.synchronize()
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      for _ in range(reps):
        joint()
      e1.record(); torch.cuda.synchronize()
      res[mode] = (e0.elapsed_time(e1) / reps, part.double().sum(0).clone())
  finally:
    D.iic_debug_seg_bf16(1)
  a, b = res[0], res[2]
  dj = float((a[1] - b[1]).abs().max() / a[1].abs().max())
  print("%-22s joint %7.3f -> %7.3f ms (%.2fx) | fp32 MFMA %5.1f TF/s -> %6.1f TF/s effective | bf16-split vs fp32-MFMA: "
        "max rel %.2e" % (which, a[0], b[0], a[0] / b[0], flops / a[0] / 1e9, flops / b[0] / 1e9, dj))


if __name__ == "__main__":
  for name in CFG:
    run(name)
