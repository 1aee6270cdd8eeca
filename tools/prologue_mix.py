"""Instruction mix of a rollout kernel's prologue (hipcc -S listing): everything one wave executes once between the
env-tile loop's barrier and the step loop -- the theta' gather (ParamSrc via MlpPair::load / MlpLane::load), the norm,
the loop invariants.

    python tools/prologue_mix.py /tmp/fdr_rollout_pair.s rollout_pair_kernelILi17ELi6ELb0ELi0 v_pk_fma_f32

Region: from the first s_barrier of the kernel to the head of the step loop (step_loop.py's choice of loop).  Where the
region holds more than one long chain of blocks between scalar branches (a loader instantiated twice, say), a wave
executes one of them: the chains of 200 instructions or more are then listed too.

    python tools/prologue_mix.py --so dfd-starter_amd/fdr/libfdr.so rollout_pair_kernelILi17ELi6ELb0ELi0E

prints where the step loop of the built library starts, modulo 64 bytes (fdr_rollout_pair.hip places it 8 bytes past a
64-byte boundary: DESIGN.md 3.0 p14).
"""
import os
import re
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_loop import body_of, loops  # noqa: E402

F64 = ("v_cvt_f64_f32", "v_mul_f64", "v_add_f64", "v_fma_f64", "v_fmac_f64")


def is_ins(x):
    return not x.startswith((".", ";")) and not x.endswith(":")


def mix(ins):
    c = Counter(x.split()[0] for x in ins)
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    cnd = sum(v for k, v in c.items() if k.startswith("v_cndmask"))
    f64 = sum(v for k, v in c.items() if k.startswith(F64))
    gl = sum(v for k, v in c.items() if k.startswith("global_load"))
    glx4 = sum(v for k, v in c.items() if k.startswith("global_load_dwordx4"))
    scr = sum(v for k, v in c.items() if k.startswith("scratch_"))
    return c, "instrs %d: VALU %d (v_cndmask %d, f64 %d), global loads %d (dwordx4 %d), s_waitcnt %d, scratch %d" % (
        len(ins), valu, cnd, f64, gl, glx4, c.get("s_waitcnt", 0), scr)


def main(path, pat, marker):
    name, body = body_of(path, pat)
    cand = [(sum(marker in body[j] for j in range(a, b)), a, b) for a, b in loops(body)]
    top = max(n for n, _, _ in cand)
    _, a, _ = min((c for c in cand if 2 * c[0] > top), key=lambda c: c[2] - c[1])
    start = next(i for i, x in enumerate(body) if x.startswith("s_barrier"))
    region = body[start + 1:a]
    ins = [x for x in region if is_ins(x)]
    c, line = mix(ins)
    print("%s: prologue %s" % (name[:50], line))
    for k in ("v_cndmask_b32_e32", "v_cndmask_b32_e64", "v_cvt_f64_f32_e32", "v_mul_f64", "v_add_f64", "v_fma_f64", "v_fmac_f64",
              "v_sub_f32_e32", "v_add_f32_e32", "v_mul_f32_e32", "v_pk_mul_f32", "v_pk_add_f32"):
        n = sum(v for kk, v in c.items() if kk.startswith(k))
        if n:
            print("   %-22s %d" % (k, n))
    # chains of blocks between scalar branches, largest first
    chains, cur = [], []
    for x in region:
        if is_ins(x):
            cur.append(x)
            if re.match(r"s_(cbranch|branch)", x):
                chains.append(cur)
                cur = []
    chains.append(cur)
    big = sorted((ch for ch in chains if len(ch) >= 200), key=len, reverse=True)
    if len(big) > 1:
        for ch in big:
            print("   chain: %s" % mix(ch)[1])


def placement(so, pat):
    import isa_hazards as ih
    import isa_mix
    text = isa_mix.disasm(so)
    funcs = ih.functions(text)
    name = [n for n in funcs if pat in n][0]
    insns = funcs[name]
    lines, on = {}, False  # mnemonics from the raw listing, as isa_mix.main does
    for line in text.splitlines():
        m = ih._FUNC.match(line)
        if m:
            on = m.group(2) == name
            continue
        if on:
            mm = ih._INSN.match(line)
            if mm:
                lines[int(mm.group(3), 16)] = line.split("//")[0].strip()
    lo, hi = isa_mix.hot_loop(insns, lines)
    a, b = insns[lo].addr, insns[hi].addr
    print("%s: step loop 0x%x..0x%x, %d instructions, head = %d mod 64 (%d mod 8), %d 64-byte lines" % (
        name[:50], a, b, hi - lo + 1, a % 64, a % 8, b // 64 - a // 64 + 1))
    return a


if __name__ == "__main__":
    if sys.argv[1] == "--so":
        placement(sys.argv[2], sys.argv[3])
    else:
        main(sys.argv[1], sys.argv[2], sys.argv[3])
