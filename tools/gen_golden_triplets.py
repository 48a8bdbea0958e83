"""Generates tests/golden/triplets_state_keys.json by CONSTRUCTING the reference's own TripletsNet5g / TripletsNet6c
(code/archs/cluster/baselines/triplets.py:11-77) and listing their state_dict: names and shapes only -- no reference
text, no weights.  Run where the reference tree exists (IIC_REFERENCE):

    python tools/gen_golden_triplets.py

Import recipe: ``xrange`` for Python 3, the reference's archs/cluster directory on sys.path for
its implicit-relative imports (``from residual import ...``), and package shims ``code``, ``code.archs``,
``code.archs.cluster`` whose __path__ points into the reference, because baselines/triplets.py imports its trunks as
``code.archs.cluster.net5g``.  The shim named ``code`` shadows the standard library's module of that name: this runs
in a process of its own and imports neither pdb nor doctest.

The reference's two classes never store ``batchnorm_track`` ("no saving of configs") although the initialisers they
inherit assert on it (residual.py:80, vgg.py:49): their constructors raise AttributeError as published.  The tool
supplies the attribute on the classes before constructing them; nothing else is touched.
"""
import builtins
import importlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("IIC_REFERENCE", "/root/reference")

# (name in the fixture, class, config)
CONFIGS = [
  ("TripletsNet5g/in2_sz32_k10", "TripletsNet5g", dict(in_channels=2, input_sz=32, batchnorm_track=True, output_k=10)),
  ("TripletsNet5g/in2_sz64_k70_notrack", "TripletsNet5g", dict(in_channels=2, input_sz=64, batchnorm_track=False,
                                                               output_k=70)),
  ("TripletsNet6c/in1_sz24_k10", "TripletsNet6c", dict(in_channels=1, input_sz=24, batchnorm_track=True, output_k=10)),
  ("TripletsNet6c/in1_sz64_k25_notrack", "TripletsNet6c", dict(in_channels=1, input_sz=64, batchnorm_track=False,
                                                               output_k=25)),
]


def reference_module():
  builtins.xrange = range
  sys.path.insert(0, os.path.join(REF, "code", "archs", "cluster"))
  for name in ("code", "code.archs", "code.archs.cluster"):
    pkg = types.ModuleType(name)
    pkg.__path__ = [os.path.join(REF, *name.split("."))]
    sys.modules[name] = pkg
  spec = importlib.util.spec_from_file_location(
    "ref_triplets_archs", os.path.join(REF, "code", "archs", "cluster", "baselines", "triplets.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def main():
  import importlib.util  # noqa: F401
  mod = reference_module()
  out = {}
  for key, cls_name, cfg in CONFIGS:
    cls = getattr(mod, cls_name)
    cls.batchnorm_track = cfg["batchnorm_track"]
    net = cls(types.SimpleNamespace(**cfg))
    out[key] = {"class": cls_name, "config": cfg,
                "state": [[n, list(t.shape), str(t.dtype)] for n, t in net.state_dict().items()]}
  path = os.path.join(ROOT, "tests", "golden", "triplets_state_keys.json")
  with open(path, "w") as f:      # one line per net
    f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(out.items()))
            + "\n}\n")
  print("wrote %s: %s" % (path, ", ".join("%s (%d entries)" % (k, len(v["state"])) for k, v in out.items())))


if __name__ == "__main__":
  main()
