"""Compare the shipped gfx950 device code of two builds of the library, function by function.

For a refactor that must not change any kernel: every function symbol of OLD.so and NEW.so is disassembled
(tools/isa_hazards.code_objects) and its instruction stream compared -- mnemonic and the full operand text, a
branch by its symbol-relative target.  Load addresses and encodings are ignored, so a function that merely moved
inside its code object, or into another one, compares equal -- including to the end of one: the s_nop padding after a
function's last instruction (alignment of the next function; ~256 of them after the last function of a code object)
is no part of it and is dropped.  The kernel metadata is compared too: VGPR, AGPR and
SGPR counts, LDS bytes, scratch bytes, max flat workgroup size.  Symbols on one side only are listed.

Usage: python tools/isa_diff.py OLD.so NEW.so      (exit 1 on any difference)
Test: tests/test_isa_diff.py (synthetic listings).
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_hazards import _FUNC, _INSN, LLVM, code_objects  # noqa: E402

META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
             "max_flat_workgroup_size")
_META = re.compile(r"^(\s*)(- )?\.(\w+):\s*(.*?)\s*$")


def streams(asm_text):
    """{function: [(mnemonic, operands)]} of an llvm-objdump -d listing; a branch's operand is its target as
    'symbol+0xoffset' (the annotation objdump prints), every other instruction's its operand text as printed.  Trailing
    's_nop 0' padding is dropped."""
    funcs, cur = {}, None
    for line in asm_text.splitlines():
        m = _FUNC.match(line)
        if m:
            cur = funcs.setdefault(m.group(2), [])
            continue
        m = _INSN.match(line) if cur is not None else None
        if not m:
            continue
        mn, rest, _addr, tfun, toff = m.groups()
        if tfun and (mn.startswith("s_cbranch") or mn == "s_branch"):
            rest = "%s+0x%s" % (tfun, toff)
        cur.append((mn, rest))
    for ins in funcs.values():
        while ins and ins[-1] == ("s_nop", "0"):
            ins.pop()
    return funcs


def metadata(notes_text):
    """{kernel name: {key: value}} (META_KEYS) from llvm-readelf --notes output (the amdhsa.kernels list)."""
    out, cur, item_col = {}, None, None
    in_kernels = False
    for line in notes_text.splitlines():
        if line.strip() == "amdhsa.kernels:":
            in_kernels, item_col = True, None
            continue
        m = _META.match(line)
        if not in_kernels or not m:
            if in_kernels and line.strip() and not line.startswith(" "):
                in_kernels = False
            continue
        col = len(m.group(1)) + (2 if m.group(2) else 0)
        if m.group(2) and (item_col is None or col == item_col):
            item_col = col
            cur = {}
        if cur is None or col != item_col:
            continue  # a nested list (.args) or a shallower key
        key, val = m.group(3), m.group(4)
        if key == "name":
            out[val] = cur
        elif key in META_KEYS:
            cur[key] = int(val)
    return out


def load(so_path):
    """(streams, metadata) over every gfx950 code object bundled in the library."""
    funcs, meta = {}, {}
    with tempfile.TemporaryDirectory() as td:
        for i, co in enumerate(code_objects(so_path)):
            path = os.path.join(td, "co%d.elf" % i)
            with open(path, "wb") as fh:
                fh.write(co)
            run = lambda *cmd: subprocess.run(cmd, capture_output=True, text=True, check=True).stdout  # noqa: E731
            for name, ins in streams(run(os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", path)).items():
                if name in funcs:
                    raise RuntimeError("%s: function %s in two code objects" % (so_path, name))
                funcs[name] = ins
            meta.update(metadata(run(os.path.join(LLVM, "llvm-readelf"), "--notes", path)))
    return funcs, meta


def diff(old, new):
    """Report lines for every difference between two (streams, metadata) pairs; empty when identical."""
    (of, om), (nf, nm) = old, new
    rep = []
    for name in sorted(set(of) - set(nf)):
        rep.append("only in OLD: %s" % name)
    for name in sorted(set(nf) - set(of)):
        rep.append("only in NEW: %s" % name)
    for name in sorted(set(of) & set(nf)):
        a, b = of[name], nf[name]
        if a != b:
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            show = lambda s: "%s %s" % s[k] if k < len(s) else "<end>"  # noqa: E731
            rep.append("code differs: %s (%d vs %d instructions; first at #%d: '%s' vs '%s')"
                       % (name, len(a), len(b), k, show(a), show(b)))
    for name in sorted(set(om) - set(nm)):
        rep.append("metadata only in OLD: %s" % name)
    for name in sorted(set(nm) - set(om)):
        rep.append("metadata only in NEW: %s" % name)
    for name in sorted(set(om) & set(nm)):
        for key in META_KEYS:
            if om[name].get(key) != nm[name].get(key):
                rep.append("metadata differs: %s .%s %s vs %s" % (name, key, om[name].get(key), nm[name].get(key)))
    return rep


def main():
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    old, new = load(sys.argv[1]), load(sys.argv[2])
    rep = diff(old, new)
    print("OLD: %d functions, %d kernels with metadata; NEW: %d functions, %d kernels with metadata"
          % (len(old[0]), len(old[1]), len(new[0]), len(new[1])))
    for line in rep:
        print(line)
    print("%d instructions compared; %s" % (sum(len(v) for k, v in old[0].items() if k in new[0]),
                                           "%d differences" % len(rep) if rep else "identical"))
    return 1 if rep else 0


if __name__ == "__main__":
    sys.exit(main())
