#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel (no GPU needed).

    hipcc <the library's flags> -S --cuda-device-only -o A/protocol.s protocol.hip      (one build)
    hipcc ...                                         -o B/protocol.s protocol.hip      (the other)
    python tools/asm_compare.py A B protocol physics > asm_compare.json

Per kernel the instructions are compared one by one; directives, comments, labels and blank lines are left
aside and branch targets are replaced by their number within the kernel.  A kernel only one side has is
listed as "new" / "gone" with its register, scratch and LDS figures from the compiler's own comments and the
code object metadata.
"""
import json
import re
import subprocess
import sys

FIG = {"sgprs": r"; TotalNumSgprs: (\d+)", "vgprs": r"; NumVgprs: (\d+)", "agprs": r"; NumAgprs: (\d+)",
       "scratch_bytes": r"; ScratchSize: (\d+)", "lds_bytes": r"; LDSByteSize: (\d+)",
       "occupancy": r"; Occupancy: (\d+)"}


def demangle(names):
    out = None
    for tool in ("llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), text=True, capture_output=True,
                                 check=True).stdout.split("\n")
            break
        except (OSError, subprocess.CalledProcessError):
            continue
    if out is None:
        return {n: n for n in names}
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        m = re.match(r"(?:void )?(?:swarm::)?([\w:]+(?:<[^(]*>)?)\(", d)
        short[n] = m.group(1) if m else d
    return short


def kernels(path):
    """{mangled name: (instructions, figures)} of every kernel (.amdhsa_kernel) of an assembly file."""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    spills = {}
    for blk in re.split(r"^\s+- \.agpr_count:", text, flags=re.M)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm:
            spills[nm.group(1)] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                                   for k in ("sgpr_spill_count", "vgpr_spill_count")
                                   if re.search(r"\.%s:\s+(\d+)" % k, blk)}
    out = {}
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        body = m.group(1)
        tail = text[m.end():m.end() + 12000]
        labels, ins = {}, []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):
                lab = re.match(r"(\.L\w+):", line)
                if lab:
                    labels[lab.group(1)] = len(labels)
                continue
            ins.append(line)
        ins = [re.sub(r"\.L\w+", lambda q: "L%d" % labels.get(q.group(0), -1), i) for i in ins]
        fig = {k: int(re.search(p, tail).group(1)) for k, p in FIG.items() if re.search(p, tail)}
        fig.update({k.replace("_count", "s"): v for k, v in spills.get(name, {}).items()})
        out[name] = (ins, fig)
    return out


def main():
    a_dir, b_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    res, same, changed, new, gone, lib = {}, 0, [], [], [], {"same": 0, "different": 0}
    for f in files:
        a, b = kernels("%s/%s.s" % (a_dir, f)), kernels("%s/%s.s" % (b_dir, f))
        short = demangle(sorted(set(a) | set(b)))
        for name in sorted(set(a) | set(b), key=lambda q: short[q]):
            key = "%s:%s" % (f, short[name])
            if "rocprim" in name or "hipcub" in name:
                lib["same" if name in a and name in b and a[name][0] == b[name][0] else "different"] += 1
            elif name in a and name in b:
                if a[name][0] == b[name][0]:
                    res[key] = {"verdict": "same", "instructions": len(a[name][0])}
                    same += 1
                else:
                    res[key] = {"verdict": "changed", "parent": dict(instructions=len(a[name][0]), **a[name][1]),
                                "tree": dict(instructions=len(b[name][0]), **b[name][1])}
                    changed.append(key)
            elif name in b:
                res[key] = {"verdict": "new", "tree": dict(instructions=len(b[name][0]), **b[name][1])}
                new.append(key)
            else:
                res[key] = {"verdict": "gone", "parent": dict(instructions=len(a[name][0]), **a[name][1])}
                gone.append(key)
    json.dump({"what": "device assembly (hipcc -S --cuda-device-only, gfx950, the library's flags) of %s in the "
                       "parent commit and in this tree, compared per kernel instruction by instruction "
                       "(directives, comments, labels and blank lines aside; branch targets by their number "
                       "within the kernel)" % " and ".join(x + ".hip" for x in files),
               "kernels": res, "library_kernels_rocprim_hipcub": lib,
               "summary": {"same": same, "changed": changed, "new": new, "gone": gone}}, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
