"""tools/asm_compare.py on synthetic assembly (no GPU, no compiler): its verdicts and --pair.

The tool is the evidence that a refactored kernel kept its instructions, so what it calls equal matters.  Tiny
assembly texts in the compiler's layout (body between `name:` and `.Lfunc_end`, `.amdhsa_kernel`, the figures
in comments) are written for a parent and a tree and compared:
  same                               equal instructions; labels may be numbered differently
  same but kernel-argument offsets   only the immediate offset of s_load_dword* differs
  changed                            anything else -- another destination register of an s_load, another
                                     offset on a vector load, one more instruction -- with both sides' figures
  new / gone                         a kernel one side has, unless --pair OLD=NEW names the two
No reference counterpart (the reference has no device code).
"""
import importlib.util
import json
import os
import sys

import pytest

from conftest import ROOT

spec = importlib.util.spec_from_file_location("asm_compare", os.path.join(ROOT, "tools", "asm_compare.py"))
asm_compare = importlib.util.module_from_spec(spec)
spec.loader.exec_module(asm_compare)

OFFSETS = "same but kernel-argument offsets"
BODY = ["s_load_dwordx2 s[4:5], s[0:1], 0x0",
        "s_load_dword s6, s[0:1], 0x58",
        "s_waitcnt lgkmcnt(0)",
        "v_add_u32_e32 v1, s6, v0",
        "s_cbranch_scc1 .LBB%d_2",
        "global_load_dword v2, v1, s[4:5] offset:16",
        ".LBB%d_2:",
        "s_endpgm"]


def body(fn, edit=None):
    """BODY with its labels numbered for function fn and `edit` = {line index: replacement} applied."""
    lines = [(edit or {}).get(q, line) for q, line in enumerate(BODY)]
    return [line % fn if "%d" in line else line for line in lines]


def write_asm(path, kernels):
    """kernels: [(name, instruction lines, vgprs)] in the layout hipcc -S gives a kernel."""
    out = []
    for q, (name, ins, vgprs) in enumerate(kernels):
        out += ["\t.text", "\t.globl\t" + name, name + ":                ; @" + name, "; %bb.0:"]
        out += [line if line.endswith(":") else "\t" + line + "    ; a comment" for line in ins]
        out += [".Lfunc_end%d:" % q, "\t.section\t.rodata,\"a\",@progbits", "\t.amdhsa_kernel " + name,
                "\t\t.amdhsa_next_free_vgpr %d" % vgprs, "\t.end_amdhsa_kernel", "\t.text",
                "; NumVgprs: %d" % vgprs, "; ScratchSize: 0", "; Occupancy: 8", "; LDSByteSize: 16 bytes/workgroup", ""]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(out))


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("asm_compare")
    a, b = str(root / "parent"), str(root / "tree")
    write_asm(a + "/proto.s", [("k_keep", body(0), 10),
                               ("k_plain", body(1), 12),
                               ("k_copy", body(2), 14),
                               ("k_reg", body(3), 10),
                               ("k_vec", body(4), 10)])
    write_asm(b + "/proto.s", [("k_tmpl_copy", body(0) + ["s_nop 0"], 15),                # one more instruction
                               ("k_keep", body(1), 10),                                   # other label numbers
                               ("k_tmpl_plain", body(2, {1: "s_load_dword s6, s[0:1], 0x60"}), 12),
                               ("k_reg", body(3, {1: "s_load_dword s7, s[0:1], 0x58"}), 10),
                               ("k_vec", body(4, {5: "global_load_dword v2, v1, s[4:5] offset:24"}), 10)])
    return a, b


PAIRS = [("k_plain", "k_tmpl_plain"), ("k_copy", "k_tmpl_copy")]


def test_verdicts_with_pairs(dirs):
    rep = asm_compare.compare(dirs[0], dirs[1], ["proto"], PAIRS)
    k = rep["kernels"]
    assert k["proto:k_keep"] == {"verdict": "same", "instructions": 7}
    assert k["proto:k_plain -> k_tmpl_plain"]["verdict"] == OFFSETS
    assert k["proto:k_plain -> k_tmpl_plain"]["parent"] == k["proto:k_plain -> k_tmpl_plain"]["tree"]
    copy = k["proto:k_copy -> k_tmpl_copy"]
    assert copy["verdict"] == "changed"
    assert copy["parent"] == {"instructions": 7, "vgprs": 14, "scratch_bytes": 0, "lds_bytes": 16, "occupancy": 8}
    assert copy["tree"] == {"instructions": 8, "vgprs": 15, "scratch_bytes": 0, "lds_bytes": 16, "occupancy": 8}
    # only the offset of a scalar load is masked: its registers and a vector load's offset are not
    assert k["proto:k_reg"]["verdict"] == "changed" and k["proto:k_vec"]["verdict"] == "changed"
    assert rep["summary"] == {"same": 1, OFFSETS: ["proto:k_plain -> k_tmpl_plain"],
                              "changed": ["proto:k_copy -> k_tmpl_copy", "proto:k_reg", "proto:k_vec"],
                              "new": [], "gone": []}
    assert len(k) == 5


def test_without_pairs_renamed_kernels_are_new_and_gone(dirs):
    rep = asm_compare.compare(dirs[0], dirs[1], ["proto"])
    assert rep["summary"]["new"] == ["proto:k_tmpl_copy", "proto:k_tmpl_plain"]
    assert rep["summary"]["gone"] == ["proto:k_copy", "proto:k_plain"]
    assert rep["summary"]["same"] == 1 and rep["summary"][OFFSETS] == []
    assert rep["kernels"]["proto:k_tmpl_copy"] == {
        "verdict": "new", "tree": {"instructions": 8, "vgprs": 15, "scratch_bytes": 0, "lds_bytes": 16, "occupancy": 8}}


def test_a_pair_that_names_no_such_kernels_is_an_error(dirs):
    with pytest.raises(SystemExit, match="k_plain=k_keep"):  # k_keep is on both sides: not a renamed kernel
        asm_compare.compare(dirs[0], dirs[1], ["proto"], [("k_plain", "k_keep")])


def test_command_line(dirs, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["asm_compare.py", dirs[0], dirs[1], "proto", "--pair", "k_plain=k_tmpl_plain",
                                      "--pair", "k_copy=k_tmpl_copy"])
    asm_compare.main()
    assert json.loads(capsys.readouterr().out) == asm_compare.compare(dirs[0], dirs[1], ["proto"], PAIRS)
    monkeypatch.setattr(sys, "argv", ["asm_compare.py", dirs[0], dirs[1], "proto", "--pair", "k_plain"])
    with pytest.raises(SystemExit):
        asm_compare.main()
