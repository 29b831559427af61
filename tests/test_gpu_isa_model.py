"""The device interpreter against the ISA model (tests/_isa_model.py), with
the oracle as the third party: all three must agree bit for bit, on r0 and
on every unit byte, over the matrices of _isa_programs.py -- every
(dst, src) register pair, dst == src included, the immediates I, the
boundary operands B x B -- and over the hand vectors of test_isa_model.py
through the single-unit path.

Each matrix runs in the variants the runtime can select: the default plan,
BPFTIME_AMD_NO_ASM_DIVERGENCE (lane groups in the C++ loop),
BPFTIME_AMD_NO_FUSE (no superinstructions), BPFTIME_AMD_NO_STAGING (no
staged unit bytes) and EBPF_BATCH_ORDERED (one lane, unit after unit).
VM.fast_handler proves which handler every instruction under test got:
the asm tier's for everything but div / mod, which must stay on the C++
single step ("SLOW") until a change of tier is made on purpose.

Unit orders.  Interleaved: neighbouring lanes hold different operands, so
conditional jumps split the waves.  Wave-uniform (every pair 64 times):
each wave takes a jump with all of its lanes or with none, the two
uniform outcomes of the asm tier's jump handlers.  Batches of 1 and 65
units put a single lane into a wave of its own, where the inactive lanes
must not count as "not taken".
"""
import numpy as np
import pytest

import _isa_programs as P
from test_isa_model import VECTORS, vector_id

pytestmark = pytest.mark.gpu

VARIANTS = ["default", "no_asm_divergence", "no_fuse", "no_staging", "ordered"]
SWITCHES = {"no_asm_divergence": "BPFTIME_AMD_NO_ASM_DIVERGENCE", "no_fuse": "BPFTIME_AMD_NO_FUSE",
            "no_staging": "BPFTIME_AMD_NO_STAGING"}
PAIRS = P.operand_pairs(seed=11)
BXB = P.boundary_pairs()
# where the 1- and 65-unit batches start in the wave-uniform order (pairs
# (0, 1)/(0, 2), (0x80000000, 0x80000001)/(.., 0xFFFFFFFF), (2^63, 2^64-1)/(2^63, ...))
EDGE_WAVES = (1, 10 * len(P.B) + 11, 16 * len(P.B) + 17)
STAGED_ALU = ("add", "mul", "lsh", "mod", "neg")
UNIFORM_ALU = ("add", "mul", "lsh", "mod")       # one op per family
STAGED_JMP = ("jeq", "jset", "jsgt", "jlt")


@pytest.fixture(params=VARIANTS)
def variant(request, monkeypatch):
    for env in SWITCHES.values():
        monkeypatch.delenv(env, raising=False)
    if request.param in SWITCHES:
        monkeypatch.setenv(SWITCHES[request.param], "1")
    return request.param


class DeviceProg:
    """A program loaded once on the device, its handlers checked, run over
    any number of unit sets and compared with the model and the oracle."""

    def __init__(self, po, dev, prog, variant):
        self.po, self.dev, self.prog, self.variant = po, dev, prog, variant
        self.flags = dev.BATCH_SYNC | (dev.BATCH_ORDERED if variant == "ordered" else 0)
        self.vm = dev.VM()
        self.vm.load(prog.code)
        got = [(pc, want, self.vm.fast_handler(dev.CTX_RAW, pc)) for pc, want in prog.sites]
        wrong = [g for g in got if g[1] != g[2]]
        assert not wrong, f"{prog.name}: (pc, wanted handler, got) {wrong[:4]}"
        assert self.vm.info()["fused_rmw"] == 0, prog.name
        if prog.static_sites:
            assert self.vm.fast_specialized(dev.CTX_RAW) == prog.static_sites, prog.name

    def check(self, units, key):
        prog, dev = self.prog, self.dev
        n = units.shape[0]
        m_r0, m_units = P.model_reference(prog, units, key)
        o_r0, o_units = P.oracle_reference(self.po, prog, units, key)
        d = dev.DeviceBuffer.from_array(units)
        dr = dev.DeviceBuffer(8 * n)
        try:
            failed = self.vm.exec_batch(dev.CTX_RAW, d, n, prog.stride, fixed_len=prog.stride, rets=dr,
                                        flags=self.flags)
            d_r0 = dr.download(np.uint64)
            d_units = d.download().reshape(n, prog.stride)
        finally:
            d.free()
            dr.free()
        what = f"{prog.name} [{self.variant}, {key}]"
        assert failed == 0, what
        stage = self.vm.last_launch()["stage"]
        if self.variant == "default":
            assert (stage > 0) == prog.staged, (what, stage)
        elif self.variant == "no_staging":
            assert stage == 0, (what, stage)
        for name, r0, after in (("model", m_r0, m_units), ("oracle", o_r0, o_units)):
            bad = np.argwhere(d_units != after)
            assert bad.size == 0, f"{what}: unit {bad[0][0]} byte {bad[0][1]} " \
                f"(operands {units[bad[0][0], :16].view(np.uint64)}): device {d_units[tuple(bad[0])]:#x}, " \
                f"{name} {after[tuple(bad[0])]:#x}"
            np.testing.assert_array_equal(d_r0, r0, err_msg=f"{what} r0 against the {name}")

    def check_orders(self, pairs_units, uniform):
        """The interleaved order, and (not in the one-lane ordered mode,
        where the order of lanes means nothing) the wave-uniform order with
        its 1- and 65-unit batches."""
        self.check(*pairs_units)
        if self.variant == "ordered" or not uniform:
            return
        units = P.make_units(P.wave_uniform(BXB), self.prog.stride)
        self.check(units, "uniform")
        for w in EDGE_WAVES:
            self.check(units[64 * w:64 * w + 65], f"uniform-{w}-65")
            self.check(units[64 * w + 64:64 * w + 65], f"uniform-{w}-1")


def pairs_units(prog, variant):
    """The interleaved unit set: B x B and the random pairs; B x B alone in
    the ordered mode (one lane runs the batch) and for the staged layout."""
    if variant == "ordered" or prog.staged:
        return P.make_units(BXB, prog.stride), "bxb"
    return P.make_units(PAIRS, prog.stride), "pairs"


def test_hand_vectors_single_unit(fresh_oracle, fresh_runtime):
    """The hand-derived vectors through ebpf_exec: the single-unit path."""
    dev = fresh_runtime
    wrong = []
    for vec in VECTORS:
        insn, a, b, want = vec
        code, mem = P.vector_program(insn, a, b)
        vm = dev.VM()
        vm.load(code)
        got = vm.exec(mem)
        if got != (0, want):
            wrong.append((vector_id(vec), got, hex(want)))
        vm.close()
    assert not wrong, wrong


@pytest.mark.parametrize("op", P.ALU)
def test_alu_matrix(fresh_oracle, fresh_runtime, variant, op):
    po, dev = fresh_oracle, fresh_runtime
    for w32 in (False, True):
        for form in ("R",) if op == "neg" else ("R", "I"):
            for layout in P.LAYOUTS if op in STAGED_ALU else ("global",):
                prog = P.alu_program(op, w32, form, layout)
                dp = DeviceProg(po, dev, prog, variant)
                uniform = op in UNIFORM_ALU and form == "R" and layout == "global" and not w32
                dp.check_orders(pairs_units(prog, variant), uniform)


@pytest.mark.parametrize("op", P.JMP)
def test_jump_matrix(fresh_oracle, fresh_runtime, variant, op):
    po, dev = fresh_oracle, fresh_runtime
    for w32 in (False, True):
        for form in ("R", "I"):
            for layout in P.LAYOUTS if op in STAGED_JMP else ("global",):
                prog = P.jump_program(op, w32, form, layout)
                dp = DeviceProg(po, dev, prog, variant)
                dp.check_orders(pairs_units(prog, variant), True)


@pytest.mark.parametrize("layout", P.LAYOUTS)
def test_endian_lddw_lea_matrix(fresh_oracle, fresh_runtime, variant, layout):
    """le / be / lddw over every register, and the `mov; add imm` pairs the
    loader fuses into LEA at link time (run as two dispatches under
    BPFTIME_AMD_NO_FUSE; the pair's halves keep their load-time handlers)."""
    po, dev = fresh_oracle, fresh_runtime
    for prog in (P.endian_lddw_program(layout), P.lea_program(layout)):
        dp = DeviceProg(po, dev, prog, variant)
        dp.check_orders(pairs_units(prog, variant), False)


@pytest.mark.parametrize("length", [48, 96])
@pytest.mark.parametrize("mode", ["slot", "other"])
def test_memory_program(fresh_oracle, fresh_runtime, variant, length, mode):
    po, dev = fresh_oracle, fresh_runtime
    prog = P.memory_program(length, mode)
    dp = DeviceProg(po, dev, prog, variant)
    units = P.memory_units(256, length)
    dp.check(units, "mem256")
    dp.check(units[:65], "mem65")
    dp.check(units[7:8], "mem1")
