"""The eBPF ISA pinned to a judge that neither implementation wrote.

tests/_isa_model.py is a plain interpreter over Python ints, written from
the instruction-set rules.  VECTORS pins the model itself: every expected
value below was worked out by hand from the rule named beside it, none
comes from the model, the oracle or the device.  The matrices
(_isa_programs.py) then compare oracle/interp.c with the model bit for bit,
r0 and every unit byte, over every register pair, the immediates I and the
boundary operands B x B.  test_gpu_isa_model.py runs the same on the
device.
"""
import numpy as np
import pytest

import _isa_model as model
import _isa_programs as P

M64 = (1 << 64) - 1
X = 0x123456789ABCDEF0
E8 = 0xEEEEEEEEEEEEEEEE

# (instruction, a, b or immediate, expected r0) -- see _isa_programs.vector_program
VECTORS = [
    # ALU32 results are zero-extended to 64 bits
    ("add32", 0x00000001FFFFFFFF, 1, 0x0),
    ("sub32", 0, 1, 0x00000000FFFFFFFF),
    ("mov32", 0, 0x1234567890ABCDEF, 0x0000000090ABCDEF),
    ("mul32", 0xFFFFFFFF, 0xFFFFFFFF, 0x1),
    ("neg32", 1, None, 0x00000000FFFFFFFF),
    ("neg32", 0xFFFFFFFF00000000, None, 0x0),
    ("lsh32", 0x80000001, 1, 0x2),
    # ALU64 wraps at 64 bits
    ("add64", M64, 1, 0x0),
    ("sub64", 0, 1, 0xFFFFFFFFFFFFFFFF),
    ("mul64", 0x100000000, 0x100000000, 0x0),
    ("neg64", 1, None, 0xFFFFFFFFFFFFFFFF),
    ("neg64", 1 << 63, None, 0x8000000000000000),
    # 64-bit immediates are sign-extended; ALU32 uses the low 32 bits
    ("mov32i", 0, -1, 0x00000000FFFFFFFF),
    ("mov64i", 0, -1, 0xFFFFFFFFFFFFFFFF),
    ("add64i", 0, -1, 0xFFFFFFFFFFFFFFFF),
    ("or64i", 0, -0x80000000, 0xFFFFFFFF80000000),
    ("and32i", M64, -0x80000000, 0x0000000080000000),
    ("xor64i", 0, 0x7FFFFFFF, 0x000000007FFFFFFF),
    ("mul64i", 2, -1, 0xFFFFFFFFFFFFFFFE),
    # unsigned division by zero gives 0
    ("div32", 0xFFFFFFFF00000007, 0, 0x0),
    ("div32i", 0xFFFFFFFF00000007, 0, 0x0),
    ("div64", 7, 0, 0x0),
    ("div64i", 7, 0, 0x0),
    ("div32", 0x0000000100000009, 0x0000000700000002, 0x4),
    # div imm -1 divides by 2^64-1 (2^32-1 for ALU32): unsigned
    ("div64i", M64, -1, 0x1),
    ("div64i", M64 - 1, -1, 0x0),
    ("div32i", 0xFFFFFFFE, -1, 0x0),
    ("div32i", 0xFFFFFFFF, -1, 0x1),
    # modulo by zero leaves dst unchanged; ALU32 truncates it
    ("mod32", 0xFFFFFFFF00000007, 0, 0x7),
    ("mod32i", 0xFFFFFFFF00000007, 0, 0x7),
    ("mod64", 0xFFFFFFFF00000007, 0, 0xFFFFFFFF00000007),
    ("mod64i", 0xFFFFFFFF00000007, 0, 0xFFFFFFFF00000007),
    ("mod64i", 5, -1, 0x5),
    ("mod32", 0x0000000500000009, 0x0000000300000004, 0x1),
    # shift counts are masked with 63 (ALU64) and 31 (ALU32)
    ("lsh64", X, 64, X),
    ("lsh64", 1, 65, 0x2),
    ("lsh64i", 1, 63, 0x8000000000000000),
    ("rsh64", 1 << 63, 63, 0x1),
    ("rsh64i", 1 << 63, 63, 0x1),
    ("lsh32", 1, 33, 0x2),
    ("lsh32i", 1, 33, 0x2),
    ("lsh32i", 0xFFFFFFFF, 31, 0x0000000080000000),
    ("rsh32", 0xAABBCCDD11223344, 32, 0x0000000011223344),
    ("rsh32i", 0x80000000, 63, 0x1),
    ("rsh32", 0x80000000, 63, 0x1),
    # arsh shifts the operand as a signed value of its own width
    ("arsh32", 0x80000000, 31, 0x00000000FFFFFFFF),
    ("arsh32", 0x80000000, 63, 0x00000000FFFFFFFF),
    ("arsh32i", 0x80000000, 33, 0x00000000C0000000),
    ("arsh32", 0xFFFFFFFF7FFFFFFF, 4, 0x0000000007FFFFFF),
    ("arsh64", 1 << 63, 63, 0xFFFFFFFFFFFFFFFF),
    ("arsh64", 0x0000000080000000, 31, 0x1),
    ("arsh64i", 1 << 63, 64, 0x8000000000000000),
    # le16 / le32 truncate, le64 is a no-op; be swaps at its width and zero-extends
    ("le16", 0x1122334455667788, None, 0x7788),
    ("le32", 0x1122334455667788, None, 0x55667788),
    ("le64", 0x1122334455667788, None, 0x1122334455667788),
    ("be16", 0x1122334455667788, None, 0x8877),
    ("be32", 0x1122334455667788, None, 0x88776655),
    ("be64", 0x1122334455667788, None, 0x8877665544332211),
    # lddw loads all 64 bits, no extension
    ("lddw", 0x0000000080000000, None, 0x0000000080000000),
    ("lddw", 0xFFFFFFFF80000000, None, 0xFFFFFFFF80000000),
    # JMP32 compares the low halves, signed or unsigned; JMP all 64 bits
    ("jsgt32", 0x80000000, 0, 0),
    ("jsgt", 0x80000000, 0, 1),
    ("jeq32", 0x0000000100000005, 0x0000000200000005, 1),
    ("jeq", 0x0000000100000005, 0x0000000200000005, 0),
    ("jne32", 0xAAAAAAAA00000001, 0xBBBBBBBB00000001, 0),
    ("jne", 0xAAAAAAAA00000001, 0xBBBBBBBB00000001, 1),
    ("jslt", M64, 0, 1),
    ("jlt", M64, 0, 0),
    ("jslt32", 0x00000000FFFFFFFF, 0, 1),
    ("jsle32", 0x7FFFFFFF, 0x80000000, 0),
    ("jle32", 0x7FFFFFFF, 0x80000000, 1),
    ("jsge32i", 0xFFFFFFFF, 0, 0),
    ("jge32i", 0xFFFFFFFF, 0, 1),
    ("jsgt32i", 0xFFFFFFFF7FFFFFFF, 0x7FFFFFFF, 0),
    ("jsge32i", 0xFFFFFFFF7FFFFFFF, 0x7FFFFFFF, 1),
    ("jsgti", 0xFFFFFFFF7FFFFFFF, 0x7FFFFFFF, 0),
    ("jsle32i", 0x80000000, -1, 1),
    ("jslt32i", 0x80000000, -0x80000000, 0),
    # jump immediates are sign-extended: jgt r, -1 compares against 2^64-1
    ("jgti", M64 - 1, -1, 0),
    ("jgei", M64, -1, 1),
    ("jgt32i", 0xFFFFFFFE, -1, 0),
    ("jlt32i", 0xFFFFFFFE, -1, 1),
    ("jslti", 1 << 63, -0x80000000, 1),
    ("jeqi", 0xFFFFFFFF80000000, -0x80000000, 1),
    ("jeq32i", 0x0000000080000000, -0x80000000, 1),
    # jset tests dst & src
    ("jset32i", 0xFFFFFFFF00000000, -1, 0),
    ("jseti", 0xFFFFFFFF00000000, -1, 1),
    ("jset", 0x10, 0x0F, 0),
    ("jset32", 0x0000000100000000, 0x0000000100000000, 0),
    # ja jumps over the next instruction
    ("ja", 0, None, 1),
    # LDX zero-extends
    ("ldx1", 0xFFEEDDCCBBAA9988, None, 0x88),
    ("ldx2", 0xFFEEDDCCBBAA9988, None, 0x9988),
    ("ldx4", 0xFFEEDDCCBBAA9988, None, 0xBBAA9988),
    ("ldx8", 0xFFEEDDCCBBAA9988, None, 0xFFEEDDCCBBAA9988),
    # st of 8 bytes stores the sign-extended immediate; narrower stores truncate
    ("st8i", E8, -5, 0xFFFFFFFFFFFFFFFB),
    ("st8i", E8, 0x7FFFFFFF, 0x000000007FFFFFFF),
    ("st4i", E8, -5, 0xEEEEEEEEFFFFFFFB),
    ("st2i", E8, 0x7FFFFFFF, 0xEEEEEEEEEEEEFFFF),
    ("st1i", E8, -1, 0xEEEEEEEEEEEEEEFF),
    ("stx4", E8, 0x1122334455667788, 0xEEEEEEEE55667788),
    ("stx2", E8, 0x1122334455667788, 0xEEEEEEEEEEEE7788),
    ("stx1", E8, 0x1122334455667788, 0xEEEEEEEEEEEEEE88),
    ("stx8", E8, 0x1122334455667788, 0x1122334455667788),
]


def vector_id(v):
    return f"{v[0]}-{v[1]:#x}-{'none' if v[2] is None else hex(v[2])}"


def test_vector_table_size():
    assert len(VECTORS) >= 40 and len(set(map(vector_id, VECTORS))) == len(VECTORS)


@pytest.mark.parametrize("vec", VECTORS, ids=vector_id)
def test_hand_vector_model(vec):
    insn, a, b, want = vec
    code, mem = P.vector_program(insn, a, b)
    assert model.Model(code).run(mem) == want


@pytest.mark.parametrize("vec", VECTORS, ids=vector_id)
def test_hand_vector_oracle(fresh_oracle, vec):
    insn, a, b, want = vec
    code, mem = P.vector_program(insn, a, b)
    vm = fresh_oracle.OracleVM()
    vm.load(code)
    assert vm.exec(mem) == (0, want)


def test_to_signed():
    assert model.to_signed(0x80000000, 32) == -(1 << 31)
    assert model.to_signed(0x7FFFFFFF, 32) == (1 << 31) - 1
    assert model.to_signed(0xFFFFFFFF00000001, 32) == 1
    assert model.to_signed(M64, 64) == -1


def test_model_refuses_what_it_cannot_judge():
    """A pointer-dependent read, an unwritten stack byte and an instruction
    outside the scope are faults of the model, not values."""
    from bpftime_amd.isa import Asm
    with pytest.raises(model.ModelFault):
        model.Model(Asm().ldx(8, 0, 10, -8).exit().assemble()).run(bytearray(8))
    with pytest.raises(model.ModelFault):
        model.Model(Asm().ldx(8, 0, 1, 1).exit().assemble()).run(bytearray(8))
    with pytest.raises(model.ModelFault):
        model.Model(Asm().call(1).exit().assemble())


# ---------------------------------------------------------------------------
# matrices: oracle against model
# ---------------------------------------------------------------------------
PAIRS = P.operand_pairs(seed=11)


def check_oracle(po, prog, units, key):
    m_r0, m_units = P.model_reference(prog, units, key)
    o_r0, o_units = P.oracle_reference(po, prog, units, key)
    np.testing.assert_array_equal(o_r0, m_r0, err_msg=prog.name)
    bad = np.argwhere(o_units != m_units)
    assert bad.size == 0, f"{prog.name}: unit {bad[0][0]} byte {bad[0][1]} " \
        f"(operands {units[bad[0][0], :16].view(np.uint64)}): oracle {o_units[tuple(bad[0])]:#x}, " \
        f"model {m_units[tuple(bad[0])]:#x}"


def alu_cases():
    for op in P.ALU:
        for w32 in (False, True):
            for form in ("R",) if op == "neg" else ("R", "I"):
                yield pytest.param(op, w32, form, id=f"{op}{32 if w32 else 64}{form.lower()}")


def jump_cases():
    for op in P.JMP:
        for w32 in (False, True):
            for form in ("R", "I"):
                yield pytest.param(op, w32, form, id=f"{op}{32 if w32 else ''}{form.lower()}")


@pytest.mark.parametrize("op,w32,form", alu_cases())
def test_alu_matrix(fresh_oracle, op, w32, form):
    prog = P.alu_program(op, w32, form)
    check_oracle(fresh_oracle, prog, P.make_units(PAIRS, prog.stride), "pairs")


@pytest.mark.parametrize("op,w32,form", jump_cases())
def test_jump_matrix(fresh_oracle, op, w32, form):
    prog = P.jump_program(op, w32, form)
    check_oracle(fresh_oracle, prog, P.make_units(PAIRS, prog.stride), "pairs")


@pytest.mark.parametrize("layout", P.LAYOUTS)
def test_endian_lddw_lea_matrix(fresh_oracle, layout):
    for prog in (P.endian_lddw_program(layout), P.lea_program(layout)):
        check_oracle(fresh_oracle, prog, P.make_units(PAIRS, prog.stride), "pairs")


@pytest.mark.parametrize("op,w32,form", [("sub", False, "R"), ("arsh", True, "I"), ("mod", True, "R")])
def test_alu_matrix_staged_layout(fresh_oracle, op, w32, form):
    """The other instruction order and pointer registers of the "staged"
    layout (the device tests use it to reach the staged handlers)."""
    prog = P.alu_program(op, w32, form, "staged")
    check_oracle(fresh_oracle, prog, P.make_units(P.boundary_pairs(), prog.stride), "bxb")


@pytest.mark.parametrize("length", [48, 96])
@pytest.mark.parametrize("mode", ["slot", "other"])
def test_memory_program(fresh_oracle, length, mode):
    prog = P.memory_program(length, mode)
    check_oracle(fresh_oracle, prog, P.memory_units(256, length), "mem256")


def test_walk_covers_every_register_pair():
    """The generator itself: every (dst, src) pair, dst == src included,
    with the pointer in a third register, in both layouts."""
    from bpftime_amd import isa
    for layout in P.LAYOUTS:
        prog = P.alu_program("sub", False, "R", layout)
        ins = isa.decode(prog.code)
        seen = set()
        for pc, handler in prog.sites:
            d = ins[pc]
            assert handler == "A64_SUB_R" and d.code == 0x1f
            st = ins[pc + 1]                         # the store of dst through the pointer
            assert st.code == 0x7b and st.src == d.dst and st.dst not in (d.dst, d.src)
            seen.add((d.dst, d.src))
        assert seen == {(d, s) for d in range(10) for s in range(10)}
