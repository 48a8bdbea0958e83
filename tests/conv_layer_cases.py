"""Every conv layer the architectures build on the bf16 MFMA path, with the batches the exact and bracket tests give it.
A plain module, not a test file: tests/test_conv_layers_cpu.py (preconditions, launch plans, no GPU),
tests/test_gpu_conv_layers_exact.py (the kernels, bit for bit, and the closure test that ties this table to
iic_amd/archs) and tests/conv_f64_cases.py (the bracket subset) read it.

LAYERS holds (entry, batches, served).

  entry    (name, cin, cout, K, stride, pad, dilation, H, W, PT border, bench batch): nn.Conv2d(cin, cout, K, stride,
           pad, dilation) on an H x W plane.  Bench batch: the N of TABLE in tests/test_conv_dispatch_cpu.py where the
           layer is listed there, else the published batch of BASELINE.md (ClusterNet5g at 64 and 32), else None
           (ClusterNet6c at input 64: the constructor admits it, no published config uses it).
  batches  (N, density, epilogue density) per test batch; density = (activation / output gradient, weight) of
           tests/lattice.py.  Every layer has N = 1 (M = Ho Wo rows: 9, 25, 36, 81 ... below a 64-row tile wherever the
           plane allows) and, up to 49 x 49, the smallest N in 2 .. 40 whose N Ho Wo rows are a whole number of 256-row
           tiles and a tail of 1 .. 24 rows (8 x 8 has no such N: the smallest tail, 64 rows; 16 x 16 and 32 x 32 give
           whole tiles at every N: N = 2).  The 62 .. 200 pixel planes of SegmentationNet10a keep N = 1.  A third batch
           (for COCO c5 / c6 a second) is the smallest N that reaches the bench batch's kernel form where no other batch
           does (BENCH_FORM below says which plan fields differ at N = 1).
           Densities: 1/2, 1/2 unless the preconditions (max |ref| <= 255, per-channel sum of squares < 2^24) need less,
           which only the bench-form batches do: their statistics run over 10^5 pixels.  The epilogue density is the
           rule of tests/test_gpu_conv_exact.py (1/8 once cout K K >= 2304, else 1/4) at every batch.
  served   frag: per geometry (forward, then every backward-data parity class) whether the weights-direct kernels serve it
           (iic_conv_igemm_frag_supported); red: per backward-data class whether its launch can carry the fused
           BatchNorm-backward reduction (iic_conv_igemm_red_supported).  Literals: tests/test_conv_layers_cpu.py holds the
           library to them, the GPU tests skip nothing.

The first layers (stem, first conv) have their own kernels and files (tests/test_gpu_first_layer_exact.py).
"""
H2, Q4, E8 = 0.5, 0.25, 0.125
HH, QH, EH, EQ = (H2, H2), (Q4, H2), (E8, H2), (E8, Q4)

# what the library serves, by the layer's role
L1 = dict(frag=(1, 1), red=(0,))                        # 64 -> 64 3x3: the persistent kernel (no fused reduction)
S1 = dict(frag=(1, 1), red=(1,))                        # every other stride-1 layer
S2_64 = dict(frag=(1, 0, 1, 1, 1), red=(0, 1, 1, 1))    # 3x3 stride 2, 64 -> 128: the one-tap class writes 64 channels
S2 = dict(frag=(1, 1, 1, 1, 1), red=(0, 1, 1, 1))       # 3x3 stride 2: the one-tap class is a gather (no reduction)
D_64 = dict(frag=(1, 0), red=(0,))                      # 1x1 stride 2, 64 -> 128
D = dict(frag=(1, 1), red=(0,))                         # 1x1 stride 2

LAYERS = [
    # ---- ClusterNet5g, input 96 (STL10 script default): planes 49 / 25 / 13 / 7 ----
    (("5g/96 layer1 3x3 64->64", 64, 64, 3, 1, 1, 1, 49, 49, 1, 660), [(1, HH, QH), (8, HH, QH)], L1),
    (("5g/96 layer2.0 3x3 s2 64->128", 64, 128, 3, 2, 1, 1, 49, 49, 1, 660), [(1, HH, QH), (7, HH, QH), (105, HH, QH)], S2_64),
    (("5g/96 layer2.0 1x1 s2 64->128", 64, 128, 1, 2, 0, 1, 49, 49, 1, 660), [(1, HH, QH), (7, HH, QH)], D_64),
    (("5g/96 layer2 3x3 128->128", 128, 128, 3, 1, 1, 1, 25, 25, 1, 660), [(1, HH, QH), (7, HH, QH), (524, EQ, QH)], S1),
    (("5g/96 layer3.0 3x3 s2 128->256", 128, 256, 3, 2, 1, 1, 25, 25, 1, 660), [(1, HH, EH), (38, HH, EH), (456, QH, EH)], S2),
    (("5g/96 layer3.0 1x1 s2 128->256", 128, 256, 1, 2, 0, 1, 25, 25, 1, 660), [(1, HH, QH), (38, HH, QH)], D),
    (("5g/96 layer3 3x3 256->256", 256, 256, 3, 1, 1, 1, 13, 13, 1, 660), [(1, HH, EH), (38, HH, EH), (194, QH, EH)], S1),
    (("5g/96 layer4.0 3x3 s2 256->512", 256, 512, 3, 2, 1, 1, 13, 13, 1, 660), [(1, HH, EH), (16, HH, EH), (335, HH, EH)], S2),
    (("5g/96 layer4.0 1x1 s2 256->512", 256, 512, 1, 2, 0, 1, 13, 13, 1, 660), [(1, HH, QH), (16, HH, QH)], D),
    (("5g/96 layer4 3x3 512->512", 512, 512, 3, 1, 1, 1, 7, 7, 1, 660), [(1, HH, EH), (16, HH, EH), (335, HH, EH)], S1),
    # ---- ClusterNet5g, input 64 (STL10 64 x 64, batch 700): planes 33 / 17 / 9 / 5 ----
    (("5g/64 layer1 3x3 64->64", 64, 64, 3, 1, 1, 1, 33, 33, 1, 700), [(1, HH, QH), (4, HH, QH)], L1),
    (("5g/64 layer2.0 3x3 s2 64->128", 64, 128, 3, 2, 1, 1, 33, 33, 1, 700), [(1, HH, QH), (8, HH, QH)], S2_64),
    (("5g/64 layer2.0 1x1 s2 64->128", 64, 128, 1, 2, 0, 1, 33, 33, 1, 700), [(1, HH, QH), (8, HH, QH)], D_64),
    (("5g/64 layer2 3x3 128->128", 128, 128, 3, 1, 1, 1, 17, 17, 1, 700), [(1, HH, QH), (8, HH, QH)], S1),
    (("5g/64 layer3.0 3x3 s2 128->256", 128, 256, 3, 2, 1, 1, 17, 17, 1, 700), [(1, HH, EH), (16, HH, EH)], S2),
    (("5g/64 layer3.0 1x1 s2 128->256", 128, 256, 1, 2, 0, 1, 17, 17, 1, 700), [(1, HH, QH), (16, HH, QH)], D),
    (("5g/64 layer3 3x3 256->256", 256, 256, 3, 1, 1, 1, 9, 9, 1, 700), [(1, HH, EH), (16, HH, EH)], S1),
    (("5g/64 layer4.0 3x3 s2 256->512", 256, 512, 3, 2, 1, 1, 9, 9, 1, 700), [(1, HH, EH), (11, HH, EH)], S2),
    (("5g/64 layer4.0 1x1 s2 256->512", 256, 512, 1, 2, 0, 1, 9, 9, 1, 700), [(1, HH, QH), (11, HH, QH)], D),
    (("5g/64 layer4 3x3 512->512", 512, 512, 3, 1, 1, 1, 5, 5, 1, 700), [(1, HH, EH), (11, HH, EH)], S1),
    # ---- ClusterNet5g, input 32 (CIFAR 32 x 32, batch 660): planes 17 / 9 / 5 / 3 ----
    (("5g/32 layer1 3x3 64->64", 64, 64, 3, 1, 1, 1, 17, 17, 1, 660), [(1, HH, QH), (8, HH, QH)], L1),
    (("5g/32 layer2.0 3x3 s2 64->128", 64, 128, 3, 2, 1, 1, 17, 17, 1, 660), [(1, HH, QH), (16, HH, QH)], S2_64),
    (("5g/32 layer2.0 1x1 s2 64->128", 64, 128, 1, 2, 0, 1, 17, 17, 1, 660), [(1, HH, QH), (16, HH, QH)], D_64),
    (("5g/32 layer2 3x3 128->128", 128, 128, 3, 1, 1, 1, 9, 9, 1, 660), [(1, HH, QH), (16, HH, QH)], S1),
    (("5g/32 layer3.0 3x3 s2 128->256", 128, 256, 3, 2, 1, 1, 9, 9, 1, 660), [(1, HH, EH), (11, HH, EH)], S2),
    (("5g/32 layer3.0 1x1 s2 128->256", 128, 256, 1, 2, 0, 1, 9, 9, 1, 660), [(1, HH, QH), (11, HH, QH)], D),
    (("5g/32 layer3 3x3 256->256", 256, 256, 3, 1, 1, 1, 5, 5, 1, 660), [(1, HH, EH), (11, HH, EH)], S1),
    (("5g/32 layer4.0 3x3 s2 256->512", 256, 512, 3, 2, 1, 1, 5, 5, 1, 660), [(1, HH, EH), (29, HH, EH)], S2),
    (("5g/32 layer4.0 1x1 s2 256->512", 256, 512, 1, 2, 0, 1, 5, 5, 1, 660), [(1, HH, QH), (29, HH, QH)], D),
    (("5g/32 layer4 3x3 512->512", 512, 512, 3, 1, 1, 1, 3, 3, 1, 660), [(1, HH, EH), (29, HH, EH)], S1),
    # ---- ClusterNet6c, input 24 (MNIST, batch 700): 5x5 pad 2 on 12 / 6 / 3, PT border 2 ----
    (("6c/24 5x5 64->128", 64, 128, 5, 1, 2, 1, 12, 12, 2, 700), [(1, HH, EH), (9, HH, EH), (456, QH, EH)], S1),
    (("6c/24 5x5 128->256", 128, 256, 5, 1, 2, 1, 6, 6, 2, 700), [(1, HH, EH), (22, HH, EH)], S1),
    (("6c/24 5x5 256->512", 256, 512, 5, 1, 2, 1, 3, 3, 2, 700), [(1, HH, EH), (29, HH, EH)], S1),
    # ---- ClusterNet6c, input 64: 32 / 16 / 8 ----
    (("6c/64 5x5 64->128", 64, 128, 5, 1, 2, 1, 32, 32, 2, None), [(1, HH, EH), (2, HH, EH)], S1),
    (("6c/64 5x5 128->256", 128, 256, 5, 1, 2, 1, 16, 16, 2, None), [(1, HH, EH), (2, HH, EH)], S1),
    (("6c/64 5x5 256->512", 256, 512, 5, 1, 2, 1, 8, 8, 2, None), [(1, HH, EH), (5, HH, EH)], S1),
    # ---- SegmentationNet10a, Potsdam 200 x 200 (batch 75): PT border 3, c5 / c6 dilation 2 with padding 1 ----
    (("potsdam c2", 64, 128, 3, 1, 1, 1, 200, 200, 3, 75), [(1, HH, QH)], S1),
    (("potsdam c3", 128, 256, 3, 1, 1, 1, 100, 100, 3, 75), [(1, HH, EH), (32, EQ, EH)], S1),
    (("potsdam c4", 256, 256, 3, 1, 1, 1, 100, 100, 3, 75), [(1, HH, EH), (16, EQ, EH)], S1),
    (("potsdam c5", 256, 512, 3, 1, 1, 2, 100, 100, 3, 75), [(1, HH, EH)], S1),
    (("potsdam c6", 512, 512, 3, 1, 1, 2, 98, 98, 3, 75), [(1, HH, EH)], S1),
    # ---- SegmentationNet10a, COCO-Stuff 128 x 128 (batch 120) ----
    (("coco c2", 64, 128, 3, 1, 1, 1, 128, 128, 3, 120), [(1, HH, QH)], S1),
    (("coco c3", 128, 256, 3, 1, 1, 1, 64, 64, 3, 120), [(1, HH, EH), (80, EQ, EH)], S1),
    (("coco c4", 256, 256, 3, 1, 1, 1, 64, 64, 3, 120), [(1, HH, EH), (40, EQ, EH)], S1),
    (("coco c5", 256, 512, 3, 1, 1, 2, 64, 64, 3, 120), [(1, HH, EH), (9, QH, EH)], S1),
    (("coco c6", 512, 512, 3, 1, 1, 2, 62, 62, 3, 120), [(1, HH, EH), (2, HH, EH)], S1),
]

# Layers of TABLE whose N = 1 and tail batches run another form than the bench batch: the smallest N that reaches the
# bench form (the third batch above), and the (kernel, ms, wn, pad, block-tiled) plans that differ, as "geometry: N = 1
# -> bench".  Kernels: 2 = conv_igemm_pw_kernel, 3 = conv_igemm_bd_kernel.  Small launches take 128-row tiles (ms 2)
# where the bench batch takes 256-row tiles (ms 4), and the stride-1 persistent kernel wants >= 1280 tiles.
BENCH_FORM = {
    "5g/96 layer2.0 3x3 s2 64->128": (105, "forward: (3, 2, 2, 0, 0) -> (3, 4, 2, 0, 0)"),
    "5g/96 layer2 3x3 128->128": (524, "forward, backward-data: (3, 2, 2, 1, 0) -> (2, 4, 2, 1, 0)"),
    "5g/96 layer3.0 3x3 s2 128->256": (456, "forward: (3, 2, 2, 0, 0) -> (3, 4, 2, 0, 0); classes 1-3: (3, 2, 2, 1, 0) -> (3, 4, 2, 1, 0)"),
    "5g/96 layer3 3x3 256->256": (194, "forward, backward-data: (3, 2, 2, 1, 0) -> (3, 4, 2, 1, 0)"),
    "5g/96 layer4.0 3x3 s2 256->512": (335, "forward: (3, 2, 2, 0, 0) -> (3, 4, 2, 0, 0)"),
    "5g/96 layer4 3x3 512->512": (335, "forward, backward-data: (3, 2, 2, 1, 0) -> (3, 4, 2, 1, 0)"),
    "6c/24 5x5 64->128": (456, "forward: (3, 2, 2, 1, 0) -> (3, 4, 2, 1, 0)"),
    "potsdam c3": (32, "forward, backward-data: (3, 4, 2, 0, 1) -> (2, 4, 2, 0, 0)"),
    "potsdam c4": (16, "forward, backward-data: (3, 4, 2, 0, 1) -> (2, 4, 2, 0, 0)"),
    "coco c3": (80, "forward, backward-data: (3, 2, 2, 1, 0) -> (2, 4, 2, 1, 0)"),
    "coco c4": (40, "forward, backward-data: (3, 2, 2, 1, 0) -> (2, 4, 2, 1, 0)"),
    "coco c5": (9, "backward-data: (3, 2, 2, 0, 0) -> (3, 4, 2, 0, 0)"),
    "coco c6": (2, "backward-data: (3, 2, 2, 0, 0) -> (3, 4, 2, 0, 1)"),
}

ENTRIES = [e for e, _, _ in LAYERS]
BY_NAME = {e[0]: (e, b, s) for e, b, s in LAYERS}
assert len(BY_NAME) == len(LAYERS)


def geometry(entry):
  """(cin, cout, K, stride, pad, dilation, H, W, PT border): what identifies a layer, batch aside."""
  return tuple(entry[1:10])


assert len({geometry(e) for e in ENTRIES}) == len(ENTRIES), "two entries with one geometry"


def spec_of(entry):
  from iic_amd import geom
  return geom.ConvSpec(*entry[1:7])


def geoms_of(entry, N):
  """The forward geometry, then every backward-data parity class, as the architectures make them (_ConvHolder.geoms)."""
  from iic_amd import geom
  H, W, P = entry[7:10]
  return [geom.fwd_geom(spec_of(entry), N, H, W, P, P)] + geom.bwd_data_geoms(spec_of(entry), N, H, W, P, P)


def cases():
  """(entry, N, density, epilogue density, served) of every entry and batch."""
  return [(e, N, dens, edens, served) for e, batches, served in LAYERS for N, dens, edens in batches]


def case_id(entry, N):
  return "%s-n%d" % (entry[0].replace(" ", "_"), N)
