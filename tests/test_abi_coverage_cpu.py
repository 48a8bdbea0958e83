"""No export without a test: every iic_* entry point of include/iic_hip.h must be reached by name from a GPU test file.

A symbol counts as covered when tests/test_gpu_*.py mention it, or mention a function of iic_amd/*.py /
iic_amd/archs/*.py whose body calls lib().<symbol> (the wrappers the tests go through).  The allow-list holds pure
host-side queries only -- nothing that launches a kernel may be on it."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# symbol -> why no GPU test has to name it.  Host-side queries: they return a number and enqueue nothing.
ALLOWED = {
  "iic_version": "query: library version (checked at load by build() and test_library_loaded_and_probe_tr16)",
  "iic_stat_bytes": "query: size of a statistics accumulator (every ops.new_stats call)",
  "iic_iid_nsplit": "query: recommended sample-split count of the IID joint",
  "iic_iid_workspace_bytes": "query: scratch size of the IID loss",
  "iic_seg_joint_nsplit": "query: recommended row-split count of the segmentation joint",
  "iic_seg_grad_workspace_bytes": "query: scratch size of the segmentation gradient",
  "iic_conv_lds_bytes": "query: LDS footprint of a geometry",
  "iic_conv_wgrad_nsplit": "query: default split-K factor of the weight gradient",
  "iic_conv_igemm_frag_supported": "query: can the weights-direct kernels serve a geometry",
  "iic_conv_igemm_red_supported": "query: can a launch carry the fused BatchNorm-backward reduction",
  "iic_weight_prep_multi_blocks": "query: workgroups one job of iic_weight_prep_multi owns",
  "iic_stem_wgrad_partial_floats": "query: scratch size of the stem weight gradient",
  "iic_firstconv_wgrad_partial_floats": "query: scratch size of the first-layer weight gradient",
  "iic_gemm_f32_ws_floats": "query: workspace size of the K-split GEMM",
  "iic_seg_head_supported": "query: can the fused segmentation head serve (C, k)",
  "iic_seg_head_wgrad_chunks": "query: number of partial matrices of the fused head's weight gradient",
}
QUERY_NAME = re.compile(r"^iic_version$|_nsplit$|_supported$|_bytes$|_floats$|_blocks$|_chunks$")


def header_text():
  """include/iic_hip.h without its comments."""
  text = open(os.path.join(ROOT, "include", "iic_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
  return re.sub(r"//[^\n]*", " ", text)


def exported_symbols():
  return sorted(set(re.findall(r"\b(?:int|long)\s+(iic_\w+)\s*\(", header_text())))


def _called_symbols(fn):
  """Names X of every `<handle>.iic_X` attribute inside the function: `lib().iic_X`, or `L.iic_X` with L = lib() -- in
  the package only the library handle has attributes of that name."""
  return set(node.attr for node in ast.walk(fn) if isinstance(node, ast.Attribute) and node.attr.startswith("iic_"))


def _units():
  """The package's named units and what each refers to: {unit: (symbols its body calls, identifiers its body uses)}.  A
  unit is a module-level function, or a CLASS for the methods inside it -- `forward`, `backward`, `step` or `apply` name
  nothing, the autograd Function or optimiser class they belong to does."""
  units = {}
  files = glob.glob(os.path.join(ROOT, "iic_amd", "*.py")) + glob.glob(os.path.join(ROOT, "iic_amd", "archs", "*.py"))

  def visit(node, owner):
    for child in ast.iter_child_nodes(node):
      if isinstance(child, ast.ClassDef):
        visit(child, owner or child.name)
      elif isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)):
        name = owner or child.name
        syms, ids = units.setdefault(name, (set(), set()))
        syms |= _called_symbols(child)
        for n in ast.walk(child):
          if isinstance(n, ast.Name):
            ids.add(n.id)
          elif isinstance(n, ast.Attribute):
            ids.add(n.attr)
      else:
        visit(child, owner)
  for path in files:
    visit(ast.parse(open(path).read(), path), None)
  return units


def wrappers(depth=2):
  """symbol -> names of the package units that reach lib().<symbol>: the units whose body calls it, and (up to `depth`
  levels up) the units that refer to those by name -- IID_loss for the autograd Function whose forward launches the
  kernels, for instance."""
  units = _units()
  table = {}
  for name, (syms, _) in units.items():
    for sym in syms:
      table.setdefault(sym, set()).add(name)
  for sym, names in table.items():
    frontier = set(names)
    for _ in range(depth):
      frontier = set(u for u, (_, ids) in units.items() if ids & frontier) - names
      names |= frontier
  return table


def gpu_test_text():
  return "\n".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))))


def _mentions(text, name):
  return re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(name), text) is not None


def test_header_parse_matches_the_binding_table():
  from iic_amd import _lib
  assert exported_symbols() == sorted(_lib.EXPORTED_SYMBOLS)


def test_allow_list_holds_queries_only():
  syms = set(exported_symbols())
  for name, why in ALLOWED.items():
    assert name in syms, "%s is on the allow-list but not exported" % name
    assert QUERY_NAME.search(name), "%s does not look like a host-side query: launches may not be on the allow-list" % name
    assert why.startswith("query: ")
  # a query never takes a stream: its prototype has no `void* stream` parameter
  text = header_text()
  for name in ALLOWED:
    proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert proto and "stream" not in proto.group(1), "%s takes a stream: it launches" % name


def test_every_exported_kernel_is_named_by_a_gpu_test():
  text = gpu_test_text()
  wr = wrappers()
  uncovered = []
  for sym in exported_symbols():
    if sym in ALLOWED:
      continue
    if _mentions(text, sym) or any(_mentions(text, fn) for fn in wr.get(sym, ())):
      continue
    uncovered.append(sym)
  assert not uncovered, "exported entry points that no tests/test_gpu_*.py reaches by name:\n  " + "\n  ".join(uncovered)
