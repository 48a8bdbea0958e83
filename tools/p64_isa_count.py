"""Instruction counts of conv_igemm_p64_kernel's K loop from the compiler's assembly (no GPU needed):

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -DIIC_DEBUG_HOOKS --cuda-device-only -S iic_amd/csrc/conv_igemm_p64.hip -o p64.s
  python tools/p64_isa_count.py p64.s

For every instantiation: MFMA, VALU and ds_read instructions between the first and the last MFMA of the tile loop, the
VALU mnemonics there, and the kernel's VGPRs, scratch bytes and occupancy as the assembler reports them."""
import collections
import re
import sys


def main():
  text = open(sys.argv[1]).read()
  verbose = "-v" in sys.argv
  for m in re.finditer(r"^(_Z21conv_igemm_p64_kernelILi(\d+)ELi(\d+)E(?:Lb(\d)E)?[^:\n]*):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
    name, abl, red, form, body = m.group(1), m.group(2), m.group(3), m.group(4), m.group(5)
    ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    mf = [i for i, x in enumerate(ins) if x.startswith("v_mfma")]
    region = ins[mf[0]:mf[-1] + 1]
    valu = [x for x in region if x.startswith("v_") and not x.startswith("v_mfma")]
    tail = text[m.end():]
    meta = {k: re.search(r"; %s: (\d+)" % k, tail).group(1) for k in ("NumVgprs", "ScratchSize", "Occupancy")}
    print("ABL %s RED %s FORM %s: MFMA %d  VALU %d  ds_read %d  ds_write %d  SALU %d | VGPR %s scratch %s B occupancy %s"
          % (abl, red, form, len(mf), len(valu), sum(x.startswith("ds_read") for x in region),
             sum(x.startswith("ds_write") for x in region), sum(x.startswith("s_") for x in region),
             meta["NumVgprs"], meta["ScratchSize"], meta["Occupancy"]))
    if verbose:
      print("   ", ", ".join("%d %s" % (n, k) for k, n in collections.Counter(valu).most_common()))


if __name__ == "__main__":
  main()
