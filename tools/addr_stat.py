#!/usr/bin/env python3
"""What the addresses of a kernel cost, statically: registers, spill code, kernel-argument loads and address arithmetic of one kernel
of a device assembly file (profiles/addr32_notes.md).

    hipcc --offload-arch=gfx950 <flags of pgdrive_amd/build.py> --cuda-device-only -S -gline-tables-only -o eng.s pgdrive_amd/csrc/pgd_engine.hip
    tools/addr_stat.py eng.s _Z6k_stepILb1ELb0ELb0ELb1ELi1ELb0EE [more symbol prefixes ...]

One line of counts per symbol prefix (the first kernel whose symbol starts with it).  No GPU needed."""
import re
import sys
from collections import Counter

VMEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")


def kernel_body(lines, prefix):
    i0 = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(";", 1)[0].rstrip().endswith(":"))
    body = []
    for l in lines[i0 + 1:]:
        t = l.split(";", 1)[0].strip()
        if t.startswith(".Lfunc_end"):
            break
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        body.append(t)
    return lines[i0].split(";", 1)[0].rstrip()[:-1], body


def descriptor(text, sym):
    m = re.search(r"- \.agpr_count:(?:(?!- \.agpr_count:).)*?\.name:\s+%s\n.*?\.wavefront_size:\s+\d+" % re.escape(sym), text, re.S)
    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(0)).group(1))
    return dict(vgpr=g("vgpr_count"), sgpr=g("sgpr_count"), sspill=g("sgpr_spill_count"), vspill=g("vgpr_spill_count"),
                scratch=g("private_segment_fixed_size"))


def stats(text, lines, prefix):
    sym, body = kernel_body(lines, prefix)
    ops = Counter(t.split()[0] for t in body)
    out = descriptor(text, sym)
    out["insts"] = len(body)
    out["v_writelane"] = ops["v_writelane_b32"]
    out["v_readlane"] = ops["v_readlane_b32"]
    out["s_nop"] = ops["s_nop"]
    out["s_nop_cycles"] = sum(int(t.split()[1], 0) + 1 for t in body if t.startswith("s_nop"))
    # the kernel-argument segment is addressed from the pair the kernel starts with (s[0:1] here, or where the compiler copied it)
    karg = [t for t in body if re.match(r"s_load_dword\w*\s+\S+,\s*s\[(0:1|\d+:\d+)\],\s*0x[0-9a-f]+", t)]
    kbase = Counter(re.search(r",\s*(s\[\d+:\d+\])", t).group(1) for t in karg)
    base = "s[0:1]" if "s[0:1]" in kbase else (kbase.most_common(1)[0][0] if kbase else "")
    offs = Counter()
    for t in karg:
        m = re.match(r"s_load_dword(\w*)\s+\S+,\s*(s\[\d+:\d+\]),\s*(0x[0-9a-f]+)", t)
        if m.group(2) == base:
            offs[m.group(3)] += 1
    out["karg_loads"] = sum(offs.values())
    out["karg_repeats"] = sum(n - 1 for n in offs.values())
    vm = [t for t in body if VMEM.match(t) and not t.startswith("scratch_")]
    out["vmem"] = len(vm)
    out["vmem_vaddr64"] = sum(1 for t in vm if re.search(r"v\[\d+:\d+\],\s*off\b|,\s*off\b", t) and t.startswith("global_"))
    for op in ("v_lshl_add_u64", "v_mad_u64_u32", "s_addc_u32", "v_addc_co_u32", "v_add_co_u32", "s_load_dword", "s_load_dwordx2",
               "s_load_dwordx4", "s_load_dwordx8", "s_load_dwordx16"):
        out[op] = ops[op]
    out["smem"] = sum(n for o, n in ops.items() if o.startswith("s_load") or o.startswith("s_buffer_load"))
    return sym, out


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    text = open(argv[1]).read()
    lines = text.split("\n")
    for prefix in argv[2:]:
        sym, out = stats(text, lines, prefix)
        print(sym[:60])
        print("  " + " ".join("%s=%d" % kv for kv in out.items()))


if __name__ == "__main__":
    main(sys.argv)
