"""iic_amd -- MI355X-native (gfx950) hot path of Invariant Information Clustering.

Host-side mirror of the reference's operator interface for the training hot path
(SURVEY.md §8b): ``IID_loss``, ``sobel_process`` and the ``ClusterNet5g*`` architectures,
implemented on hand-written HIP kernels behind the C ABI of ``libiic_hip.so``
(include/iic_hip.h).  ``iic_amd.install.install()`` registers them under the reference's
module names so its training scripts import them unchanged.

Submodules: losses, seg_losses, transforms, archs, optim, dist, install, geom, ops, branches, pool, augment, seg_augment, seg_ragged, seg_prescale, linear, semisup, seg_baselines, _lib.
``linear`` holds every fully-connected layer (exact fp32, and bf16 MFMA over one or two PT activations); the heads of
archs, semisup and the baselines call it.
"""
import importlib

_LAZY = {
  "IID_loss": ("losses", "IID_loss"),
  "IID_loss_heads": ("losses", "IID_loss_heads"),
  "sobel_process": ("transforms", "sobel_process"),
  "Adam": ("optim", "Adam"),
  "SupHead5": ("semisup", "SupHead5"),
  "TenCropEvaluator": ("semisup", "TenCropEvaluator"),
  "SegPairedAugmenter": ("seg_augment", "SegPairedAugmenter"),
  "SegRaggedAugmenter": ("seg_ragged", "SegRaggedAugmenter"),
  "prescale_dataset": ("seg_prescale", "prescale_dataset"),
  "seg_paired_dataloaders": ("seg_augment", "seg_paired_dataloaders"),
  "SegTestPreparer": ("seg_augment", "SegTestPreparer"),
  "seg_mapping_dataloader": ("seg_augment", "seg_mapping_dataloader"),
}


def __getattr__(name):
  # lazy so that `import iic_amd` works on a box without a GPU (CPU test tier)
  if name in _LAZY:
    mod, attr = _LAZY[name]
    return getattr(importlib.import_module("." + mod, __name__), attr)
  raise AttributeError("module %r has no attribute %r" % (__name__, name))
