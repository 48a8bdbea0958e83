"""Compare the product library's device code of two source trees kernel by kernel (no GPU needed).

  python tools/isa_diff.py OLD_CSRC NEW_CSRC [--rename 'REGEX=REPL' ...]

Compiles every SRCS file of each iic_amd/csrc directory with the Makefile's product flags plus
--offload-device-only -S, keys each kernel by its demangled name without the parameter list, and reports
kernels only in one tree, kernels whose instruction text differs (labels and comments normalised away) and,
for those, the register / LDS / scratch counts on both sides.  --rename rewrites an OLD key before matching
(a removed template argument, say); a rename to the empty string drops the kernel from the comparison.
Exit status 0 when every kernel present in both trees has identical instruction text."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COUNTS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def make_var(csrc, name):
  return subprocess.run(["make", "-s", "--no-print-directory", "-C", csrc, "--eval", "print-%: ; @echo $($*)",
                         "print-" + name], capture_output=True, text=True, check=True).stdout.split()


def compile_tree(csrc, out):
  flags, srcs = make_var(csrc, "CXXFLAGS"), make_var(csrc, "SRCS")
  def one(s):
    dst = os.path.join(out, s[:-4] + ".s")
    subprocess.run([HIPCC] + flags + ["--offload-device-only", "-S", s, "-o", dst], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    return dst
  with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
    return list(ex.map(one, srcs))


def kernels(asm_files):
  text = {}
  meta = {}
  for f in asm_files:
    s = open(f).read()
    for m in re.finditer(r"^(\S+):\s*; @\S+\n(.*?)^\.Lfunc_end\d+:", s, re.M | re.S):
      body = re.sub(r";.*", "", m.group(2))
      body = re.sub(r"\.LBB\d+_", ".LBB_", body)
      text[m.group(1)] = "\n".join(l.strip() for l in body.splitlines() if l.strip())
    for item in re.split(r"\n  - ", s.split("amdhsa.kernels:", 1)[-1])[1:]:
      sym = re.search(r"\.symbol:\s+(\S+)\.kd", item)
      if sym:
        meta[sym.group(1)] = {k: int(re.search(r"\n\s*%s:\s+(\d+)" % re.escape(k), "\n" + item).group(1))
                              for k in COUNTS if re.search(r"\n\s*%s:" % re.escape(k), "\n" + item)}
  names = [n for n in text if n in meta]
  dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True,
                       text=True).stdout.split("\n")
  out = {}
  for n, d in zip(names, dem):
    key = re.sub(r"^void ", "", d)
    key = key[:key.rfind("(")] if key.endswith(")") else key
    out[key] = (text[n].replace(n, "KERNEL"), meta[n])
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("old")
  ap.add_argument("new")
  ap.add_argument("--rename", action="append", default=[], help="REGEX=REPL applied to the OLD kernel keys")
  a = ap.parse_args()
  with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
    old, new = kernels(compile_tree(a.old, t0)), kernels(compile_tree(a.new, t1))
  print("kernels: old %d, new %d" % (len(old), len(new)))
  renamed = {}
  for k0, v in sorted(old.items()):
    k = k0
    for r in a.rename:
      pat, repl = r.split("=", 1)
      k = re.sub(pat, repl, k)
    if k:
      renamed[k] = v
    else:
      print("removed on purpose:", k0)
  gone = sorted(set(renamed) - set(new))
  added = sorted(set(new) - set(renamed))
  for k in gone:
    print("only in OLD:", k)
  for k in added:
    print("only in NEW:", k)
  changed = 0
  for k in sorted(set(renamed) & set(new)):
    if renamed[k][0] != new[k][0]:
      changed += 1
      print("differs:", k)
      for c in COUNTS:
        print("   %-28s %6s -> %s" % (c, renamed[k][1].get(c), new[k][1].get(c)))
  print("identical: %d, differ: %d" % (len(set(renamed) & set(new)) - changed, changed))
  return 1 if changed else 0


if __name__ == "__main__":
  sys.exit(main())
