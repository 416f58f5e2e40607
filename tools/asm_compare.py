#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel (no GPU needed).

    hipcc <the library's flags> -S --cuda-device-only -o A/protocol.s protocol.hip      (one build)
    hipcc ...                                         -o B/protocol.s protocol.hip      (the other)
    python tools/asm_compare.py A B protocol physics [--pair OLD=NEW ...] > asm_compare.json

Per kernel the instructions are compared one by one; directives, comments, labels and blank lines are left
aside and branch targets are replaced by their number within the kernel.  A kernel only one side has is
listed as "new" / "gone" with its register, scratch and LDS figures from the compiler's own comments and the
code object metadata.  --pair OLD=NEW (short names as the output prints them, repeatable) compares A's kernel
OLD with B's kernel NEW: a kernel that was renamed, or became a template's instantiation.  Verdicts: "same";
"same but kernel-argument offsets" -- equal once the immediate offset of every s_load_dword* (the scalar
loads that fetch kernel arguments) is masked, what one more or one fewer argument does to a kernel whose
code is otherwise untouched; "changed", with both sides' figures.
"""
import argparse
import json
import re
import subprocess
import sys

FIG = {"sgprs": r"; TotalNumSgprs: (\d+)", "vgprs": r"; NumVgprs: (\d+)", "agprs": r"; NumAgprs: (\d+)",
       "scratch_bytes": r"; ScratchSize: (\d+)", "lds_bytes": r"; LDSByteSize: (\d+)",
       "occupancy": r"; Occupancy: (\d+)"}
OFFSETS = "same but kernel-argument offsets"


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
        short[n] = re.sub(r"\bswarm::", "", m.group(1)) if m else d
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


def mask_offsets(ins):
    """The instructions with the immediate offset (the last operand) of every s_load_dword* masked."""
    return [re.sub(r"^(s_load_dword\w*\s+[^,]+,[^,]+,\s*)(?:offset:)?(?:0x[0-9a-fA-F]+|\d+)\b", r"\1OFF", i)
            for i in ins]


def verdict(a, b):
    """One kernel of each side, as kernels() gives them."""
    if a[0] == b[0]:
        return {"verdict": "same", "instructions": len(a[0])}
    return {"verdict": OFFSETS if mask_offsets(a[0]) == mask_offsets(b[0]) else "changed",
            "parent": dict(instructions=len(a[0]), **a[1]), "tree": dict(instructions=len(b[0]), **b[1])}


def compare(a_dir, b_dir, files, pairs=()):
    """The report: `pairs` are (old short name, new short name) of kernels to compare across the two sides."""
    res, lib = {}, {"same": 0, "different": 0}
    summary = {"same": 0, OFFSETS: [], "changed": [], "new": [], "gone": []}
    unused = set(pairs)

    def put(key, v):
        res[key] = v
        if v["verdict"] == "same":
            summary["same"] += 1
        else:
            summary[v["verdict"]].append(key)

    for f in files:
        a, b = kernels("%s/%s.s" % (a_dir, f)), kernels("%s/%s.s" % (b_dir, f))
        short = demangle(sorted(set(a) | set(b)))
        only_a = {short[n]: n for n in a if n not in b}
        only_b = {short[n]: n for n in b if n not in a}
        paired = set()
        for old, new in pairs:
            if old in only_a and new in only_b:
                put("%s:%s -> %s" % (f, old, new), verdict(a[only_a[old]], b[only_b[new]]))
                paired |= {only_a[old], only_b[new]}
                unused.discard((old, new))
        for name in sorted((set(a) | set(b)) - paired, key=lambda q: short[q]):
            key = "%s:%s" % (f, short[name])
            if "rocprim" in name or "hipcub" in name:
                lib["same" if name in a and name in b and a[name][0] == b[name][0] else "different"] += 1
            elif name in a and name in b:
                put(key, verdict(a[name], b[name]))
            elif name in b:
                put(key, {"verdict": "new", "tree": dict(instructions=len(b[name][0]), **b[name][1])})
            else:
                put(key, {"verdict": "gone", "parent": dict(instructions=len(a[name][0]), **a[name][1])})
    if unused:
        raise SystemExit("no such pair of kernels (one only the parent has, one only the tree has): " +
                         ", ".join("%s=%s" % p for p in sorted(unused)))
    return {"what": "device assembly (hipcc -S --cuda-device-only, gfx950, the library's flags) of %s in the "
                    "parent commit and in this tree, compared per kernel instruction by instruction "
                    "(directives, comments, labels and blank lines aside; branch targets by their number "
                    "within the kernel; 'A -> B': the parent's kernel A against the tree's B)"
                    % " and ".join(x + ".hip" for x in files),
            "kernels": res, "library_kernels_rocprim_hipcub": lib, "summary": summary}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a_dir")
    ap.add_argument("b_dir")
    ap.add_argument("files", nargs="+", help="source names without extension: A/NAME.s against B/NAME.s")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    pairs = []
    for p in a.pair:
        old, sep, new = p.partition("=")
        if not (old and sep and new):
            ap.error("--pair takes OLD=NEW")
        pairs.append((old, new))
    json.dump(compare(a.a_dir, a.b_dir, a.files, pairs), sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
