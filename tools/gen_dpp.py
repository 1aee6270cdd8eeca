"""Generate dfd-starter_amd/csrc/fdr_dpp_gen.h: multi-accumulator DPP-broadcast FMA blocks.

Each block is ONE inline-asm statement (hipcc cannot reorder inside it) whose FMAs rotate over
NACC independent accumulators, so a wave always has NACC independent v_fmac_f32_dpp in flight
instead of one dependent chain.  Operand k of the block reads x[k] through row_newbcast.
"""
import os

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfd-starter_amd", "csrc",
                   "fdr_dpp_gen.h")


def block(name, nx, n_per_x, nacc, init=False):
    """acc[a] += sum_{q<nx} sum_{c<n_per_x} w[q*n_per_x + c] * bcast(X[q], c); FMA i -> acc[i % nacc].
    init: the accumulators are outputs only -- the first product of each is a v_mul_f32_dpp (no
    zeroing movs); early-clobber, since the inputs are still read after the first writes."""
    outs = [('"=&v"(a%d)' if init else '"+v"(a%d)') % a for a in range(nacc)]
    ins = ['"v"(X%d)' % q for q in range(nx)] + ['"v"(w[%d])' % i for i in range(nx * n_per_x)]
    lines = ['"s_nop 1\\n\\t"']
    i = 0
    for c in range(n_per_x):
        for q in range(nx):
            a = i % nacc
            op = "v_mul_f32_dpp %%%d, %%%d, %%%d" if (init and i < nacc) else "v_fmac_f32_dpp %%%d, %%%d, %%%d"
            lines.append(('"' + op + ' row_newbcast:%d row_mask:0xf bank_mask:0xf\\n\\t"')
                         % (a, nacc + q, nacc + nx + q * n_per_x + c, c))
            i += 1
    sig = ", ".join(["float& a%d" % a for a in range(nacc)] + ["float X%d" % q for q in range(nx)] +
                    ["const float* w"])
    return ("__device__ __forceinline__ void %s(%s) {\n  asm volatile(\n      %s\n      : %s\n      : %s);\n}\n"
            % (name, sig, "\n      ".join(lines), ", ".join(outs), ", ".join(ins)))


def lanes_block(name, lanes):
    """acc += sum_m w[m] * bcast(X, lanes[m]): dpp_fma_tail's sibling for inputs that sit in the given lanes of the row."""
    lines = ['"s_nop 1\\n\\t"']
    for m, lane in enumerate(lanes):
        lines.append('"v_fmac_f32_dpp %%0, %%1, %%%d row_newbcast:%d row_mask:0xf bank_mask:0xf\\n\\t"' % (2 + m, lane))
    ins = ['"v"(X0)'] + ['"v"(w[%d])' % m for m in range(len(lanes))]
    return ("__device__ __forceinline__ void %s(float& a0, float X0, const float* w) {\n  asm volatile(\n      %s\n"
            "      : \"+v\"(a0)\n      : %s);\n}\n" % (name, "\n      ".join(lines), ", ".join(ins)))


# ---- the pair kernel's 12-output head: products, then a reduce-scatter over the 16-lane row ----------------------
# Every thread of a row forms its own partial of all 12 outputs in registers R[0..11] (6 packed accumulators); four
# levels of DPP adds leave output head_rs12_out(l) = 3 (l / 4) + min(l % 4, 2), summed over the row, in R[0] of lane l
# (lane 4q + 3 repeats lane 4q + 2).  Which output a thread keeps in which register differs per lane -- the weights
# are loaded in that order -- so every lane runs the same instructions:
#   level 1  partner l ^ 15 (row_mirror)       R[i] += R'[i + 6], i < 6
#   level 2  partner l ^ 7  (row_half_mirror)  R[i] += R'[i + 3], i < 3
#   level 3  partner l ^ 2  (quad_perm)        R[0] += R'[2]; R[1] += R'[1]  (lanes 4q + 0/1 keep two outputs, 2/3 one)
#   level 4  partner l ^ 1  (quad_perm)        R[0] += R'[1] in lanes 4q + 0/1: the two exchange their second output;
#                                              R[0] += R'[0] in lanes 4q + 2/3: the two all-reduce their one output.
# Level 4 takes two instructions (a lane select of the register to hand over, then the add): with one add
# f = X[k] + X'[m] over the two level-3 results, k != m would need the three outputs of a quad in both columns k and m
# of three lanes each, which the four lanes' three registers cannot hold, and k == m uses one result only.
# Order: every DPP / permlane source is written >= 2 wait states before it is read; an s_nop 1 ahead of level 4 and
# one ahead of the cross-row swap.
HEAD_RS12_LEVELS = [
    ("row_mirror", 15, [(3, 9), (4, 10), (5, 11), (0, 6), (1, 7), (2, 8)]),  # (register kept, partner's register)
    ("row_half_mirror", 7, [(2, 5), (1, 4), (0, 3)]),
    ("quad_perm:[2,3,0,1]", 2, [(0, 2), (1, 1)]),
]
HEAD_RS12_LAST = ("quad_perm:[1,0,3,2]", 1)
HEAD_RS12_BASE = 232  # the partials' registers v232 .. v243 (of the bases tried, the one that left the kernel at 245 VGPRs, no scratch)


def head_rs12_out(l):
    return 3 * (l // 4) + min(l % 4, 2)


def head_rs12_slots():
    """slot[l][r]: the output whose partial lane l keeps in register r -- derived backwards from the levels."""
    need = [[None] * 12 for _ in range(16)]

    def put(tab, l, r, o):
        assert tab[l][r] in (None, o), (l, r, o, tab[l][r])
        tab[l][r] = o

    for l in range(16):  # what level 4 reads
        put(need, l, 0, head_rs12_out(l))
        if l % 4 < 2:
            put(need, l ^ 1, 1, head_rs12_out(l))
        else:
            assert head_rs12_out(l ^ 1) == head_rs12_out(l)
    for _, x, adds in reversed(HEAD_RS12_LEVELS):
        before = [[None] * 12 for _ in range(16)]
        for _ in range(2):  # an idle add's output is fixed by its partner's: second pass
            for l in range(16):
                for d, s in adds:
                    o = need[l][d] if need[l][d] is not None else before[l][d]
                    if o is not None:
                        put(before, l, d, o)
                        put(before, l ^ x, s, o)
        need = before
    for l in range(16):
        assert sorted(need[l]) == list(range(12)), (l, need[l])
    return need


def head_rs12_slot_closed(l, r):
    """the same table in closed form (emitted as head_rs12_slot for the loader)"""
    lp = l ^ (0, 7, 15, 8)[r // 3]
    return 3 * (lp // 4) + (0x486864 >> (2 * (3 * (lp % 4) + r % 3)) & 3)


def head_rs12_text():
    slots = head_rs12_slots()
    assert all(slots[l][r] == head_rs12_slot_closed(l, r) for l in range(16) for r in range(12))
    t = ["// ---- pair kernel head, 12 outputs: products and reduce-scatter (see tools/gen_dpp.py) ----\n",
         "typedef float dpp_f2 __attribute__((ext_vector_type(2)));\n",
         "// output whose partial lane l of a row keeps in register r\n",
         "constexpr unsigned char kHeadRs12Slot[16][12] = {\n"]
    for l in range(16):
        t.append("    {%s},\n" % ", ".join(str(o) for o in slots[l]))
    t.append("};\n")
    t.append("__host__ __device__ constexpr int head_rs12_out(int l) { return 3 * (l >> 2) + ((l & 3) < 2 ? (l & 3) : 2); }\n")
    t.append("__host__ __device__ constexpr int head_rs12_slot(int l, int r) {\n"
             "  const int lp = l ^ (r < 3 ? 0 : (r < 6 ? 7 : (r < 9 ? 15 : 8)));\n"
             "  return 3 * (lp >> 2) + ((0x486864 >> (2 * (3 * (lp & 3) + r % 3))) & 3);\n}\n")
    t.append("constexpr bool head_rs12_table_ok() {\n  for (int l = 0; l < 16; ++l)\n    for (int r = 0; r < 12; ++r)\n"
             "      if (kHeadRs12Slot[l][r] != head_rs12_slot(l, r)) return false;\n  return true;\n}\n"
             "static_assert(head_rs12_table_ok(), \"head_rs12_slot != kHeadRs12Slot\");\n")
    # One asm statement (nothing is scheduled or padded inside it).  The 12 partials live in fixed registers
    # v[BASE .. BASE + 11], named as pairs by the packed products and singly by the DPP adds -- an asm operand has no
    # way to name the halves of a register pair, and tied scalar operands made the compiler copy five of them between
    # the two steps.  Products: R[2j], R[2j + 1] = w[j] * h.x + w[6 + j] * h.y, the level-1 DPP sources first.
    base = HEAD_RS12_BASE  # operands: %0 u, %1 v, %2-%13 w[0..11], %14 h, %15 the lane mask
    R = lambda k: "v%d" % (base + k)
    P = lambda j: "v[%d:%d]" % (base + 2 * j, base + 2 * j + 1)
    lines = []
    for j in range(6):
        lines.append('"v_pk_mul_f32 %s, %%%d, %%14 op_sel_hi:[1,0]\\n\\t"' % (P(j), 2 + j))
    for j in (3, 4, 5, 0, 1, 2):
        lines.append('"v_pk_fma_f32 %s, %%%d, %%14, %s op_sel:[0,1,0] op_sel_hi:[1,1,1]\\n\\t"' % (P(j), 8 + j, P(j)))
    flat = [(ctrl, d, s) for ctrl, _, adds in HEAD_RS12_LEVELS for d, s in adds]
    for n, (ctrl, d, s) in enumerate(flat):
        dst = R(d)
        lines.append('"v_add_f32_dpp %s, %s, %s %s row_mask:0xf bank_mask:0xf bound_ctrl:1\\n\\t"' % (dst, R(s), R(d), ctrl))
    ctrl = HEAD_RS12_LAST[0]
    # level 4: the partner's register this lane adds is R[1] in lanes 4q + 0/1 and R[0] in lanes 4q + 2/3 -- selected
    # into R[2] (free since level 3) by a lane mask held in an SGPR pair, then one add
    lines.append('"v_cndmask_b32_e64 %s, %s, %s, %%15\\n\\t"' % (R(2), R(1), R(0)))
    lines.append('"s_nop 1\\n\\t"')
    # the add twice, into R[1] and R[0]: the two copies the cross-row swap needs (no v_mov), then the swap -- R[0] = the
    # even row's sum and R[1] = the odd row's, in both rows of the half
    for d in (1, 0):
        lines.append('"v_add_f32_dpp %s, %s, %s %s row_mask:0xf bank_mask:0xf bound_ctrl:1\\n\\t"' % (R(d), R(2), R(0), ctrl))
    lines.append('"s_nop 1\\n\\t"')
    lines.append('"v_permlane16_swap_b32 %s, %s\\n\\t"' % (R(0), R(1)))
    ins = ", ".join(['"v"(w[%d])' % k for k in range(12)] + ['"v"(h)', '"s"(0xccccccccccccccccull)'])
    clob = ", ".join('"v%d"' % (base + k) for k in range(2, 12))  # R[0], R[1] are the result operands
    t.append("// u / v = the even / odd row's sum of output head_rs12_out(l) over w[j] * h.x + w[6 + j] * h.y (w[j]: the outputs of\n"
             "// registers 2j, 2j + 1), in both rows of the half\n"
             "__device__ __forceinline__ void dpp_head_rs12(float& u, float& v, const dpp_f2* w, dpp_f2 h) {\n"
             "  asm volatile(\n      %s\n      : \"=&{v%d}\"(u), \"=&{v%d}\"(v)\n      : %s\n      : %s);\n}\n"
             % ("\n      ".join(lines), base, base + 1, ins, clob))
    return "".join(t)


def main():
    parts = ["// GENERATED by tools/gen_dpp.py -- do not edit.\n#pragma once\n\nnamespace fdr {\n\n"]
    # the pair-kernel head: one chain of 32 (the accumulator is no DPP source: no wait states)
    parts.append(block("dpp_dot_32x1", 2, 16, 1, init=True))
    # 16 inputs of the caller's own row, 4 chains (one-lane kernels' head)
    parts.append(block("dpp_dot_16x4", 1, 16, 4, init=True))
    # short tails: n inputs (lane 0..n-1 of the row) from one register, 1 accumulator
    for n in range(1, 16):
        parts.append(block("dpp_fma_tail%d" % n, 1, n, 1))
    # K a of the 12-output head: the 6 actions sit in lanes 0, 1, 2, 4, 5, 6 of the row
    parts.append(lanes_block("dpp_fma_tail6_q3", [l for l in range(8) if head_rs12_out(l) < 6 and l % 4 < 3]))
    parts.append(head_rs12_text())
    parts.append("}  // namespace fdr\n")
    with open(OUT, "w") as f:
        f.write("".join(parts))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
