"""tools/isa_diff.py on synthetic listings: what counts as a difference between two builds' device code.

The tool is the acceptance check of refactors that must not change a kernel: it has to ignore where a function
was loaded and how it was encoded, and to catch a changed operand, a changed register count and a lost symbol.
"""
import tools.isa_diff as idf

_BODY = ["s_load_dwordx2 s[2:3], s[0:1], 0x0",
         "v_add_f32_e32 v4, v1, v2",
         "v_add_f32_dpp v0, v4, v0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf",
         "s_cbranch_scc1 65533 @+0x4",
         "s_endpgm"]


def _listing(funcs, base=0x1000, enc="00000000"):
    """llvm-objdump -d style text of {name: [instruction text]}; '@+0x..' marks a branch target inside the function."""
    out, addr = [], base
    for name, lines in funcs.items():
        out.append("%016x <%s>:" % (addr, name))
        for ln in lines:
            ann = ""
            if " @+" in ln:
                ln, off = ln.split(" @+")
                ann = " <%s+%s>" % (name, off)
            out.append("\t%s // %012X: %s%s" % (ln, addr, enc, ann))
            addr += 4
        out.append("")
    return "\n".join(out) + "\n"


def _notes(kernels):
    """llvm-readelf --notes style text of {name: vgpr_count}."""
    out = ["amdhsa.kernels:"]
    for name, vgprs in kernels.items():
        out += ["  - .agpr_count:     0",
                "    .args:",
                "      - .offset:         0",
                "        .size:           272",
                "        .value_kind:     by_value",
                "    .group_segment_fixed_size: 18816",
                "    .max_flat_workgroup_size: 256",
                "    .name:           %s" % name,
                "    .private_segment_fixed_size: 24",
                "    .sgpr_count:     60",
                "    .symbol:         %s.kd" % name,
                "    .vgpr_count:     %d" % vgprs,
                "    .wavefront_size: 64"]
    out += ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "amdhsa.version:", "  - 1", "  - 2"]
    return "\n".join(out) + "\n"


def _build(funcs, vgprs=128, **kw):
    return idf.streams(_listing(funcs, **kw)), idf.metadata(_notes({name: vgprs for name in funcs}))


def test_parsers_read_streams_and_metadata():
    funcs, meta = _build({"k": _BODY})
    assert [mn for mn, _ in funcs["k"]] == ["s_load_dwordx2", "v_add_f32_e32", "v_add_f32_dpp", "s_cbranch_scc1",
                                           "s_endpgm"]
    assert funcs["k"][2][1].endswith("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")  # modifiers are compared too
    assert funcs["k"][3] == ("s_cbranch_scc1", "k+0x4")
    assert meta == {"k": {"agpr_count": 0, "group_segment_fixed_size": 18816, "max_flat_workgroup_size": 256,
                          "private_segment_fixed_size": 24, "sgpr_count": 60, "vgpr_count": 128}}


def test_a_shifted_load_address_and_another_encoding_are_no_difference():
    old = _build({"k": _BODY, "k2": _BODY})
    new = _build({"k2": _BODY, "k": _BODY}, base=0x7f000, enc="D1FE0000 AABBCCDD")  # other order, address, encoding
    assert idf.diff(old, new) == []


def test_padding_after_the_last_instruction_is_no_difference():
    # the function that ends a code object carries that object's end padding; one in the middle only its alignment
    old = _build({"k": _BODY + ["s_nop 0"] * 3, "k2": _BODY})
    new = _build({"k2": _BODY, "k": _BODY + ["s_nop 0"] * 260})
    assert idf.diff(old, new) == []
    # an s_nop inside the function still counts
    body = _BODY[:2] + ["s_nop 0"] + _BODY[2:]
    assert len(idf.diff(_build({"k": _BODY}), _build({"k": body}))) == 1


def test_one_changed_operand_is_a_difference():
    body = list(_BODY)
    body[1] = "v_add_f32_e32 v4, v1, v3"
    rep = idf.diff(_build({"k": _BODY, "k2": _BODY}), _build({"k": body, "k2": _BODY}))
    assert len(rep) == 1 and rep[0].startswith("code differs: k ") and "#1" in rep[0]
    # a DPP modifier is part of the operand text
    body = list(_BODY)
    body[2] = body[2].replace("quad_perm:[2,3,0,1]", "quad_perm:[1,0,3,2]")
    assert len(idf.diff(_build({"k": _BODY}), _build({"k": body}))) == 1
    # and a branch to another place in the function
    body = list(_BODY)
    body[3] = "s_cbranch_scc1 65533 @+0x8"
    assert len(idf.diff(_build({"k": _BODY}), _build({"k": body}))) == 1


def test_a_changed_vgpr_count_is_a_difference():
    rep = idf.diff(_build({"k": _BODY}, vgprs=128), _build({"k": _BODY}, vgprs=127))
    assert rep == ["metadata differs: k .vgpr_count 128 vs 127"]


def test_a_missing_symbol_is_a_difference():
    rep = idf.diff(_build({"k": _BODY, "k2": _BODY}), _build({"k": _BODY}))
    assert "only in OLD: k2" in rep and "metadata only in OLD: k2" in rep
    rep = idf.diff(_build({"k": _BODY}), _build({"k": _BODY, "k3": _BODY}))
    assert "only in NEW: k3" in rep
