"""The pair kernel's 12-output head (fdr_dpp_gen.h: kHeadRs12Slot, dpp_head_rs12), simulated in numpy from the generated
text itself.

16 threads of a DPP row each hold their own partial of all 12 outputs in registers R[0..11], in the per-thread order of
kHeadRs12Slot; the generated instructions (12 packed products, 12 DPP adds over row_mirror / row_half_mirror / two
quad_perms, one lane select; the last add twice, for the two operands of the cross-row swap) must leave output
3 (l / 4) + min(l % 4, 2) -- means in lanes 0, 1, 2, 4, 5, 6, the std pre-activations 8 lanes up -- summed over the 16
threads, in R[0] of lane l.  Integer-valued partials: the sums are
exact, so the comparison is equality.  Also: every W3 element belongs to exactly one (thread, register) of the half,
every DPP source is at least 2 wait states old (the rule tools/isa_hazards.py checks in the built code), and the header
is what tools/gen_dpp.py generates.
"""
import os
import re

import numpy as np

import tools.gen_dpp as gen

HEADER = gen.OUT
PARTNER = {"row_mirror": 15, "row_half_mirror": 7, "quad_perm:[2,3,0,1]": 2, "quad_perm:[1,0,3,2]": 1}
N_OUT, N_LANES, HIDDEN = 12, 16, 64


def header_text():
    with open(HEADER) as f:
        return f.read()


def slot_table(text):
    body = re.search(r"kHeadRs12Slot\[16\]\[12\] = \{(.*?)\};", text, re.S).group(1)
    rows = re.findall(r"\{([0-9, ]+)\}", body)
    return np.array([[int(x) for x in r.split(",")] for r in rows])


def head_asm(text):
    """the instructions of dpp_head_rs12, with the operand numbers of its constraints resolved: (lines, base)"""
    fn = text[text.index("void dpp_head_rs12("):]
    fn = fn[:fn.index("\n}\n")]
    lines = re.findall(r'"(v_\w+|s_nop) ?(.*?)\\n\\t"', fn)
    base = int(re.search(r'"=&\{v(\d+)\}"\(u\)', fn).group(1))
    assert '"=&{v%d}"(v)' % (base + 1) in fn
    return lines, base


def out_of(lane):
    return 3 * (lane // 4) + min(lane % 4, 2)


def test_slot_table_is_the_generators_and_a_permutation_per_lane():
    tab = slot_table(header_text())
    assert tab.shape == (N_LANES, N_OUT)
    assert np.array_equal(tab, np.array(gen.head_rs12_slots()))
    for lane in range(N_LANES):
        assert sorted(tab[lane]) == list(range(N_OUT))
        for r in range(N_OUT):
            assert gen.head_rs12_slot_closed(lane, r) == tab[lane][r]


def test_header_is_up_to_date(tmp_path, monkeypatch):
    monkeypatch.setattr(gen, "OUT", str(tmp_path / "fdr_dpp_gen.h"))
    gen.main()
    assert (tmp_path / "fdr_dpp_gen.h").read_text() == header_text()


def test_every_w3_element_has_one_owner_in_the_half():
    tab = slot_table(header_text())
    owners = np.zeros((N_OUT, HIDDEN), int)
    for t in range(32):                                  # thread t of the half: layer-2 units 8 (t/4) + t%4, + 4
        ua = 8 * (t // 4) + t % 4
        for r in range(N_OUT):
            owners[tab[t % 16][r], ua] += 1              # against h2.x
            owners[tab[t % 16][r], ua + 4] += 1          # against h2.y
    assert np.all(owners == 1)


def simulate(partials, tab):
    """run the generated instructions on 16 lanes; partials[l][o]: lane l's partial of output o, given as the
    (w . h) products the packed instructions form: w[j] * h.x + w[6 + j] * h.y with h = (1, 1)"""
    lines, base = head_asm(header_text())
    reg = {}                                             # register number -> 16 lane values
    age = {}                                             # register number -> wait states since its last VALU write
    wx = partials // 2                                   # split every partial over the two products
    wy = partials - wx
    n_dpp = 0
    swapped = False

    def tick(n=1):
        for k in age:
            age[k] += n

    for mn, ops in lines:
        if mn == "s_nop":
            tick(int(ops) + 1)
            continue
        if mn in ("v_pk_mul_f32", "v_pk_fma_f32"):
            m = re.match(r"v\[(\d+):(\d+)\], %(\d+), %14", ops)     # %0 u, %1 v, %2-%13 w[0..11], %14 h, %15 mask
            lo, hi, w = int(m.group(1)), int(m.group(2)), int(m.group(3))
            assert hi == lo + 1 and lo % 2 == 0
            for e, v in enumerate((lo, hi)):
                r = v - base
                if mn == "v_pk_mul_f32":                 # w[0..5], against h.x
                    assert 2 <= w <= 7 and r // 2 == w - 2 and "op_sel_hi:[1,0]" in ops
                    val = np.array([wx[l][tab[l][r]] for l in range(N_LANES)], float)
                else:                                    # w[6..11], against h.y
                    assert 8 <= w <= 13 and r // 2 == w - 8 and "op_sel:[0,1,0]" in ops
                    val = reg[v] + np.array([wy[l][tab[l][r]] for l in range(N_LANES)], float)
                reg[v] = val
            tick()
            age[lo] = age[hi] = 0
        elif mn == "v_add_f32_dpp":
            m = re.match(r"v(\d+), v(\d+), v(\d+) (\S+) row_mask:0xf bank_mask:0xf bound_ctrl:1", ops)
            d, s, o, ctrl = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
            assert age[s] >= 2, "DPP source v%d written %d wait states before" % (s, age[s])
            x = PARTNER[ctrl]
            val = reg[s][[l ^ x for l in range(N_LANES)]] + reg[o]
            reg[d] = val
            tick()
            age[d] = 0
            n_dpp += 1
        elif mn == "v_cndmask_b32_e64":
            m = re.match(r"v(\d+), v(\d+), v(\d+), %15", ops)
            d, a, b = int(m.group(1)), int(m.group(2)), int(m.group(3))
            mask = np.array([(0xCCCC >> l) & 1 for l in range(N_LANES)], bool)   # "s"(0xcccc...): lanes 4q + 2, 3
            reg[d] = np.where(mask, reg[b], reg[a])
            tick()
            age[d] = 0
        elif mn == "v_permlane16_swap_b32":                # the cross-row combine: both operands hold the row's result
            a, b = [int(x) for x in re.match(r"v(\d+), v(\d+)", ops).groups()]
            assert (a, b) == (base, base + 1) and age[a] >= 2 and age[b] >= 2
            assert np.array_equal(reg[a], reg[b])
            swapped = True
        else:
            raise AssertionError("unexpected instruction %s" % mn)
    assert '"s"(0xccccccccccccccccull)' in header_text() and swapped
    return reg[base], n_dpp


def test_reduce_scatter_leaves_every_output_in_its_lane():
    tab = slot_table(header_text())
    rng = np.random.RandomState(12)
    for _ in range(4):
        partials = rng.randint(-1000, 1000, size=(N_LANES, N_OUT))
        res, n_dpp = simulate(partials, tab)
        total = partials.sum(axis=0)
        for lane in range(N_LANES):
            assert res[lane] == total[out_of(lane)], lane
        assert n_dpp == 13                                 # 12 of the reduce-scatter, the last one twice
    means = [l for l in range(N_LANES) if out_of(l) < 6 and l % 4 < 3]
    assert means == [0, 1, 2, 4, 5, 6]
    assert [out_of(l) for l in means] == list(range(6))                      # lane -> dim = l - l / 4
    assert [out_of(l + 8) for l in means] == list(range(6, 12))              # its std pre-activation 8 lanes up


def test_k_a_sibling_reads_the_mean_lanes():
    fn = header_text()
    fn = fn[fn.index("void dpp_fma_tail6_q3("):]
    fn = fn[:fn.index("\n}\n")]
    got = [(int(w), int(l)) for w, l in re.findall(r"v_fmac_f32_dpp %0, %1, %(\d+) row_newbcast:(\d+)", fn)]
    assert got == [(2 + m, l) for m, l in enumerate([0, 1, 2, 4, 5, 6])]
    assert os.path.exists(HEADER)
