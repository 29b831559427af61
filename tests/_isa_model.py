"""A plain eBPF reference interpreter over Python integers -- TEST JUDGE ONLY.

Written from the instruction-set rules (RFC 9669, "BPF Instruction Set
Architecture"; the kernel's Documentation/bpf/standardization/
instruction-set.rst), not from oracle/interp.c or csrc/interp.hip: the
oracle and the device were written by the same hands, and this model is the
third opinion both are compared with (test_isa_model.py,
test_gpu_isa_model.py).  The hand-derived vectors in test_isa_model.py pin
the model itself.

Registers are unbounded Python ints masked explicitly; every rule is one
small function with the rule it encodes named in its comment.

Scope: ALU / ALU64 add sub mul div mod or and xor mov lsh rsh arsh neg
(register and immediate forms), le / be at 16 / 32 / 64, lddw with src 0,
JMP / JMP32 (every condition, register and immediate, and ja), LDX / ST /
STX of 1 / 2 / 4 / 8 bytes, exit.  Helpers, maps and atomics are not
modelled (an instruction outside the scope raises ModelFault).

Entry state, as OracleVM.run_raw / ebpf_exec give it: r1 = the unit, r2 =
its length, r10 = the top of a 512-byte stack, everything else 0.  The
addresses are synthetic (UNIT_BASE, STACK_BASE), so a program whose result
depends on a pointer's value cannot be compared: test programs keep
pointers in dedicated registers and never let one reach r0 or the unit.
Reading a stack byte that was never written is a fault too (no
implementation defines its value).
"""
import struct

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1

UNIT_BASE = 0x0000_1000_0000_0000
STACK_BASE = 0x0000_2000_0000_0000
STACK_SIZE = 512
STEP_LIMIT = 1 << 20


class ModelFault(Exception):
    pass


# --------------------------------------------------------------------------
# integer helpers
# --------------------------------------------------------------------------
MASK = {8: 0xFF, 16: 0xFFFF, 32: M32, 64: M64}


def mask(bits):
    return MASK[bits]


def to_signed(v, bits):
    """The two's-complement value of the low `bits` bits of v."""
    v &= MASK[bits]
    return v - (1 << bits) if v >> (bits - 1) else v


def to_unsigned(v, bits):
    return v & mask(bits)


def imm_operand(imm32, bits):
    # rule: a 32-bit immediate is sign-extended to 64 bits; ALU32 and JMP32
    # then use its low 32 bits
    return to_unsigned(to_signed(imm32, 32), 64) & mask(bits)


# --------------------------------------------------------------------------
# ALU rules: a, b are already reduced to the operation's width (`bits`)
# --------------------------------------------------------------------------
def rule_add(a, b, bits):
    # rule: dst += src, wrapping at the width
    return (a + b) & mask(bits)


def rule_sub(a, b, bits):
    # rule: dst -= src, wrapping at the width
    return (a - b) & mask(bits)


def rule_mul(a, b, bits):
    # rule: dst *= src, the low `bits` bits of the product
    return (a * b) & mask(bits)


def rule_div(a, b, bits):
    # rule: unsigned division; division by zero gives 0
    return 0 if b == 0 else a // b


def rule_mod(a, b, bits):
    # rule: unsigned modulo; modulo by zero leaves dst unchanged (for ALU32
    # that is dst truncated to 32 bits: `a` is already the low half)
    return a if b == 0 else a % b


def rule_or(a, b, bits):
    # rule: dst |= src
    return a | b


def rule_and(a, b, bits):
    # rule: dst &= src
    return a & b


def rule_xor(a, b, bits):
    # rule: dst ^= src
    return a ^ b


def rule_mov(a, b, bits):
    # rule: dst = src
    return b


def shift_count(b, bits):
    # rule: shift counts are masked with 63 for ALU64 and 31 for ALU32
    return b & (bits - 1)


def rule_lsh(a, b, bits):
    # rule: dst <<= (src & mask), bits shifted past the width are lost
    return (a << shift_count(b, bits)) & mask(bits)


def rule_rsh(a, b, bits):
    # rule: logical shift right, zeros come in from the top
    return a >> shift_count(b, bits)


def rule_arsh(a, b, bits):
    # rule: arsh shifts the operand as a signed value of its own width
    return to_unsigned(to_signed(a, bits) >> shift_count(b, bits), bits)


def rule_neg(a, b, bits):
    # rule: dst = -dst in two's complement at the width
    return (-a) & mask(bits)


ALU_RULES = {
    0x00: rule_add, 0x10: rule_sub, 0x20: rule_mul, 0x30: rule_div, 0x40: rule_or, 0x50: rule_and,
    0x60: rule_lsh, 0x70: rule_rsh, 0x80: rule_neg, 0x90: rule_mod, 0xA0: rule_xor, 0xB0: rule_mov,
    0xC0: rule_arsh,
}


def alu(rule, bits, dst, src):
    """One ALU / ALU64 instruction: the new 64-bit value of dst."""
    # rule: ALU32 works on the low halves of both operands ...
    m = MASK[bits]
    r = rule(dst & m, src & m, bits)
    # rule: ... and ALU32 results are zero-extended to 64 bits
    return r & m


def byteswap(v, bits):
    return int.from_bytes((v & mask(bits)).to_bytes(bits // 8, "little"), "big")


def rule_le(v, bits):
    # rule: on a little-endian host le16 / le32 truncate (zero-extend the
    # low bits), le64 is a no-op
    return v & mask(bits)


def rule_be(v, bits):
    # rule: be byte-swaps the low `bits` bits and zero-extends
    return byteswap(v, bits)


# --------------------------------------------------------------------------
# jump rules: a, b are already reduced to the compare's width
# --------------------------------------------------------------------------
def cond_jeq(a, b, bits):
    # rule: jeq, dst == src
    return a == b


def cond_jne(a, b, bits):
    # rule: jne, dst != src
    return a != b


def cond_jgt(a, b, bits):
    # rule: jgt, unsigned >
    return a > b


def cond_jge(a, b, bits):
    # rule: jge, unsigned >=
    return a >= b


def cond_jlt(a, b, bits):
    # rule: jlt, unsigned <
    return a < b


def cond_jle(a, b, bits):
    # rule: jle, unsigned <=
    return a <= b


def cond_jset(a, b, bits):
    # rule: jset tests dst & src
    return (a & b) != 0


def cond_jsgt(a, b, bits):
    # rule: jsgt, signed > at the compare's width
    return to_signed(a, bits) > to_signed(b, bits)


def cond_jsge(a, b, bits):
    # rule: jsge, signed >=
    return to_signed(a, bits) >= to_signed(b, bits)


def cond_jslt(a, b, bits):
    # rule: jslt, signed <
    return to_signed(a, bits) < to_signed(b, bits)


def cond_jsle(a, b, bits):
    # rule: jsle, signed <=
    return to_signed(a, bits) <= to_signed(b, bits)


JMP_RULES = {
    0x10: cond_jeq, 0x20: cond_jgt, 0x30: cond_jge, 0x40: cond_jset, 0x50: cond_jne, 0x60: cond_jsgt,
    0x70: cond_jsge, 0xA0: cond_jlt, 0xB0: cond_jle, 0xC0: cond_jslt, 0xD0: cond_jsle,
}


def jump_taken(rule, bits, dst, src):
    # rule: JMP32 compares the low halves (signed or unsigned), JMP all 64 bits
    m = MASK[bits]
    return rule(dst & m, src & m, bits)


# --------------------------------------------------------------------------
# memory rules
# --------------------------------------------------------------------------
SIZE_OF = {0x00: 4, 0x08: 2, 0x10: 1, 0x18: 8}  # the size field of LDX / ST / STX


def store_value(v, size):
    # rule: a store writes the low `size` bytes, little-endian (narrower
    # stores truncate)
    return (v & mask(8 * size)).to_bytes(size, "little")


def st_imm_value(imm32, size):
    # rule: st of 8 bytes stores the sign-extended immediate; narrower
    # stores truncate it
    return store_value(imm_operand(imm32, 64), size)


def load_value(raw):
    # rule: LDX zero-extends the loaded bytes
    return int.from_bytes(raw, "little")


class Memory:
    """The unit's bytes and the 512-byte stack at synthetic addresses."""

    def __init__(self, unit, length):
        self.unit = unit
        self.length = length
        self.stack = bytearray(STACK_SIZE)
        self.written = bytearray(STACK_SIZE)

    def _where(self, addr, size):
        if UNIT_BASE <= addr and addr + size <= UNIT_BASE + self.length:
            return self.unit, addr - UNIT_BASE, False
        if STACK_BASE <= addr and addr + size <= STACK_BASE + STACK_SIZE:
            return self.stack, addr - STACK_BASE, True
        raise ModelFault(f"access of {size} bytes at {addr:#x} outside the unit and the stack")

    def load(self, addr, size):
        buf, at, stk = self._where(addr, size)
        if stk and not all(self.written[at:at + size]):
            raise ModelFault(f"read of unwritten stack bytes at r10{at - STACK_SIZE:+d}")
        return load_value(buf[at:at + size])

    def store(self, addr, raw):
        buf, at, stk = self._where(addr, len(raw))
        buf[at:at + len(raw)] = raw
        if stk:
            self.written[at:at + len(raw)] = b"\1" * len(raw)


# --------------------------------------------------------------------------
# the interpreter
# --------------------------------------------------------------------------
CLS_LD, CLS_LDX, CLS_ST, CLS_STX, CLS_ALU, CLS_JMP, CLS_JMP32, CLS_ALU64 = range(8)
K_ALU, K_END, K_LDDW, K_JA, K_JCC, K_LDX, K_ST, K_STX, K_EXIT = range(9)


def decode(code):
    """Bytes -> one tuple per 8-byte slot (None for the second lddw slot)."""
    if len(code) % 8:
        raise ModelFault("code length is not a multiple of 8")
    raw = [struct.unpack_from("<BBhi", code, i) for i in range(0, len(code), 8)]
    out = []
    i = 0
    while i < len(raw):
        op, regs, off, imm = raw[i]
        dst, src, cls = regs & 15, regs >> 4, op & 7
        use_reg = bool(op & 0x08)
        if dst > 10 or src > 10:
            raise ModelFault(f"bad register at {i}")
        if cls in (CLS_ALU, CLS_ALU64):
            bits = 64 if cls == CLS_ALU64 else 32
            o = op & 0xF0
            if o == 0xD0:
                if cls != CLS_ALU or imm not in (16, 32, 64):
                    raise ModelFault(f"bad byte swap at {i}")
                out.append((K_END, rule_be if use_reg else rule_le, imm, dst, 0, 0, 0))
            elif o in ALU_RULES:
                if o == 0x80 and use_reg:
                    raise ModelFault(f"neg with a source register at {i}")
                out.append((K_ALU, ALU_RULES[o], bits, dst, use_reg, src, imm_operand(imm, bits)))
            else:
                raise ModelFault(f"unknown ALU opcode {op:#x} at {i}")
        elif cls in (CLS_JMP, CLS_JMP32):
            bits = 64 if cls == CLS_JMP else 32
            o = op & 0xF0
            if op == 0x95:
                out.append((K_EXIT, None, 0, 0, 0, 0, 0))
            elif op == 0x05:
                out.append((K_JA, None, 0, 0, 0, 0, off))
            elif o in JMP_RULES:
                out.append((K_JCC, JMP_RULES[o], bits, dst, use_reg, src, (imm_operand(imm, bits), off)))
            else:
                raise ModelFault(f"jump opcode {op:#x} at {i} is outside the model")
        elif cls == CLS_LDX and (op & 0xE0) == 0x60:
            out.append((K_LDX, None, SIZE_OF[op & 0x18], dst, 0, src, off))
        elif cls == CLS_STX and (op & 0xE0) == 0x60:
            out.append((K_STX, None, SIZE_OF[op & 0x18], dst, 0, src, off))
        elif cls == CLS_ST and (op & 0xE0) == 0x60:
            out.append((K_ST, None, SIZE_OF[op & 0x18], dst, 0, 0, (st_imm_value(imm, SIZE_OF[op & 0x18]), off)))
        elif op == 0x18:
            if src != 0 or i + 1 >= len(raw) or raw[i + 1][0] != 0:
                raise ModelFault(f"lddw at {i} is outside the model")
            # rule: lddw (src 0) loads imm | next.imm << 32, no extension
            out.append((K_LDDW, None, 0, dst, 0, 0, (imm & M32) | ((raw[i + 1][3] & M32) << 32)))
            out.append(None)
            i += 1
        else:
            raise ModelFault(f"opcode {op:#x} at {i} is outside the model")
        i += 1
    return out


class Model:
    def __init__(self, code):
        self.prog = decode(code)

    def run(self, unit, length=None):
        """Runs the program on one unit (a bytearray, modified in place);
        returns r0."""
        length = len(unit) if length is None else length
        mem = Memory(unit, length)
        reg = [0] * 11
        reg[1] = UNIT_BASE
        reg[2] = length
        reg[10] = STACK_BASE + STACK_SIZE
        prog = self.prog
        n = len(prog)
        pc = 0
        for _ in range(STEP_LIMIT):
            if not 0 <= pc < n or prog[pc] is None:
                raise ModelFault(f"pc {pc} outside the program")
            kind, rule, w, dst, use_reg, src, x = prog[pc]
            pc += 1
            if kind == K_ALU:
                if dst == 10:
                    raise ModelFault("write of r10")
                reg[dst] = alu(rule, w, reg[dst], reg[src] if use_reg else x)
            elif kind == K_LDX:
                if dst == 10:
                    raise ModelFault("write of r10")
                reg[dst] = mem.load((reg[src] + x) & M64, w)
            elif kind == K_STX:
                mem.store((reg[dst] + x) & M64, store_value(reg[src], w))
            elif kind == K_ST:
                mem.store((reg[dst] + x[1]) & M64, x[0])
            elif kind == K_JCC:
                # rule: a taken jump continues at pc + 1 + off
                if jump_taken(rule, w, reg[dst], reg[src] if use_reg else x[0]):
                    pc += x[1]
            elif kind == K_JA:
                # rule: ja jumps by its 16-bit offset
                pc += x
            elif kind == K_END:
                reg[dst] = rule(reg[dst], w)
            elif kind == K_LDDW:
                reg[dst] = x
                pc += 1
            else:
                # rule: exit returns r0
                return reg[0]
        raise ModelFault("step limit")


def run_units(code, units, length):
    """The model over a (n, stride) uint8 array: (r0 per unit as a list of
    ints, the units after the run as a new array).  Equal units are run
    once."""
    import numpy as np
    m = Model(code)
    out = np.empty_like(units)
    rets = []
    seen = {}
    for i in range(units.shape[0]):
        key = units[i].tobytes()
        hit = seen.get(key)
        if hit is None:
            buf = bytearray(key)
            r0 = m.run(buf, length)
            hit = (r0, np.frombuffer(bytes(buf), dtype=np.uint8))
            seen[key] = hit
        rets.append(hit[0])
        out[i] = hit[1]
    return np.array(rets, dtype=np.uint64), out
