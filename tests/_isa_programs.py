"""Deterministic program and unit generators for the ISA model tests
(test_isa_model.py on the CPU, test_gpu_isa_model.py on the device).

Every generator returns a Prog: the code, the unit size, and the sites of
the instructions under test with the asm-tier handler each must get
(VM.fast_handler reports the handler chosen at load; what is fused or
staged at link time -- LEA, the staged LDXS* / STXS* / STS* forms -- keeps
its load-time name there).

Pointers never reach r0 or the unit: the unit pointer lives in one register
per step (reloaded from the stack slot r10-8, or r1 itself while r1 is
free), scalars in the others.

Layouts.  "global": the pointer is always reloaded from the stack, so the
loader knows nothing about it and every unit access runs the generic LDX* /
STX* / ST* handlers; nothing is staged.  "staged": the steps that do not
use r1 come first and address the unit through r1 itself, which the loader
knows to be the unit's slot: their operand loads and the stores below byte
64 are link-time staged slot accesses (LDXS* / STXS* / STS*), the stores
past the window generic ones with staging live; the steps that use r1
follow with the reloaded pointer.
"""
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from bpftime_amd import gen
from bpftime_amd.isa import Asm

M64 = (1 << 64) - 1

# operand set B: boundary values of the shift counts, the 32 / 64-bit signs,
# the halves, and a few mixed patterns
B = [0, 1, 2, 31, 32, 33, 63, 64, 65,
     0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000,
     (1 << 63) - 1, 1 << 63, (1 << 64) - 1,
     0x123456789ABCDEF0, 0xFFFFFFFF7FFFFFFF, 0x7FFFFFFF80000000, 0x8000000080000000,
     0x00000001FFFFFFFF, 0xAAAAAAAA55555555]
# immediate set I
I = [0, 1, -1, 31, 32, 33, 63, 64, 0x7FFFFFFF, -0x80000000]

ALU = ["add", "sub", "mul", "div", "mod", "or", "and", "xor", "mov", "lsh", "rsh", "arsh", "neg"]
JMP = ["jeq", "jne", "jgt", "jge", "jlt", "jle", "jset", "jsgt", "jsge", "jslt", "jsle"]
LAYOUTS = ["global", "staged"]
IN_BYTES = 16          # operands a, b at unit bytes 0..15
FILL = 0xEE            # what the output area holds before the run


@dataclass
class Prog:
    name: str
    code: bytes
    stride: int                                   # unit size = length passed to the VM
    sites: List[Tuple[int, str]] = field(default_factory=list)   # (pc, handler at load)
    static_sites: int = 0                         # accesses the loader types (fast_specialized)
    staged: bool = False                          # the default launch stages unit bytes


def random_pairs(n, seed):
    """Random operand pairs in the style of test_gpu_parity._operands: a
    third small (< 70), a third with the upper half set, a third raw."""
    r = gen.sm64(seed, np.arange(2 * n, dtype=np.uint64)).reshape(n, 2)
    small = (r % np.uint64(70)).astype(np.uint64)
    pick = (gen.sm64(seed + 1, np.arange(2 * n, dtype=np.uint64)) % np.uint64(3)).reshape(n, 2)
    r = np.where(pick == 0, small, r)
    r[pick == 1] = r[pick == 1] | np.uint64(0xFFFFFFFF00000000)
    return r


def boundary_pairs():
    """Every pair of B x B, b varying fastest: neighbouring units differ."""
    b = np.array(B, dtype=np.uint64)
    return np.stack([np.repeat(b, len(B)), np.tile(b, len(B))], axis=1)


def operand_pairs(seed, nrand=200):
    return np.concatenate([boundary_pairs(), random_pairs(nrand, seed)])


def make_units(pairs, stride):
    """(n, stride) uint8: the pair at bytes 0..15, FILL behind it."""
    n = pairs.shape[0]
    u = np.full((n, stride), FILL, dtype=np.uint8)
    u[:, :IN_BYTES] = np.ascontiguousarray(pairs, dtype=np.uint64).view(np.uint8).reshape(n, IN_BYTES)
    return u


def wave_uniform(pairs):
    """Every pair 64 times over: each wave holds one pair, so a conditional
    jump is taken by all of its lanes or by none."""
    return np.repeat(pairs, 64, axis=0)


# --------------------------------------------------------------------------
# the register walk
# --------------------------------------------------------------------------
def _ptr_reg(k, *busy):
    free = [r for r in range(10) if r not in busy]
    return free[k % len(free)]


class _Walk:
    """Emits the steps of a walk: per step the unit pointer in a register
    that is not one of the step's own, and an output slot."""

    def __init__(self, layout, out_size):
        assert layout in LAYOUTS
        self.layout = layout
        self.out_size = out_size
        self.a = Asm().stx(8, 10, -8, "r1")
        self.k = 0
        self.r1_free = layout == "staged"
        self.static_sites = 1                      # the stack store above
        self.sites = []

    @staticmethod
    def order(steps, layout, regs_of):
        if layout == "global":
            return list(steps)
        return [s for s in steps if 1 not in regs_of(s)] + [s for s in steps if 1 in regs_of(s)]

    def pointer(self, *busy):
        """The register holding the unit pointer for this step."""
        if self.r1_free and 1 not in busy:
            return 1
        self.r1_free = False
        p = _ptr_reg(self.k, *busy)
        self.a.ldx(8, p, 10, -8)
        self.static_sites += 1
        return p

    def load(self, size, dst, p, off):
        self.a.ldx(size, dst, p, off)
        if p == 1 and self.r1_free and off + size <= 64:
            self.static_sites += 1

    def out_off(self):
        return IN_BYTES + self.out_size * self.k

    def site(self, handler):
        self.sites.append((self.a.pc, handler))

    def store_out(self, p, src=None, imm=None):
        off = self.out_off()
        if src is not None:
            self.a.stx(self.out_size, p, off, f"r{src}")
        else:
            self.a.st(self.out_size, p, off, imm)
        if p == 1 and self.r1_free and off + self.out_size <= 64:
            self.static_sites += 1

    def finish(self, name):
        nout = self.k
        a = self.a
        a.ldx(8, 1, 10, -8).ldx(self.out_size, 0, 1, IN_BYTES).exit()
        self.static_sites += 1
        stride = (IN_BYTES + self.out_size * nout + 15) & ~15
        return Prog(name, a.assemble(), stride, self.sites, self.static_sites, self.layout == "staged")


def _alu_handler(op, w32, form):
    if op in ("div", "mod"):
        return "SLOW"                      # no asm handler: the C++ single step
    w = "32" if w32 else "64"
    if op == "neg":
        return f"A{w}_NEG"
    return f"A{w}_{op.upper()}_{form}"


def alu_program(op, w32, form, layout="global"):
    """form "R": every (dst, src) of r0..r9 x r0..r9, dst == src included
    (then both operands are b); form "I": every dst x every immediate of I.
    neg: every dst.  out[k] = dst after the instruction."""
    if op == "neg":
        steps = [(d, None) for d in range(10)]
    elif form == "R":
        steps = [(d, s) for d in range(10) for s in range(10)]
    else:
        steps = [(d, imm) for d in range(10) for imm in I]
    regs_of = (lambda st: (st[0], st[1])) if form == "R" and op != "neg" else (lambda st: (st[0],))
    w = _Walk(layout, 8)
    emit = w.a.alu32 if w32 else w.a.alu64
    for st in _Walk.order(steps, layout, regs_of):
        d, x = st
        busy = regs_of(st)
        p = w.pointer(*busy)
        w.load(8, d, p, 0)
        if form == "R" and op != "neg":
            w.load(8, x, p, 8)
        w.site(_alu_handler(op, w32, form))
        if op == "neg":
            w.a.neg32(d) if w32 else w.a.neg64(d)
        elif form == "R":
            emit(op, d, f"r{x}")
        else:
            emit(op, d, x)
        w.store_out(p, src=d)
        w.k += 1
    return w.finish(f"{op}{32 if w32 else 64}{'' if op == 'neg' else form.lower()}-{layout}")


def jump_program(op, w32, form, layout="global"):
    """The same walk for a conditional jump: out[k] (one byte) = 1 on the
    taken path, 0 on the other."""
    if form == "R":
        steps = [(d, s) for d in range(10) for s in range(10)]
        regs_of = lambda st: (st[0], st[1])      # noqa: E731
    else:
        steps = [(d, imm) for d in range(10) for imm in I]
        regs_of = lambda st: (st[0],)            # noqa: E731
    w = _Walk(layout, 1)
    emit = w.a.jmp32 if w32 else w.a.jmp
    handler = f"J{32 if w32 else 64}_{op[1:].upper()}_{form}"
    for st in _Walk.order(steps, layout, regs_of):
        d, x = st
        p = w.pointer(*regs_of(st))
        w.load(8, d, p, 0)
        if form == "R":
            w.load(8, x, p, 8)
        w.site(handler)
        emit(op, d, f"r{x}" if form == "R" else x, f"t{w.k}")
        w.store_out(p, imm=0)
        w.a.ja(f"j{w.k}")
        w.a.label(f"t{w.k}")
        w.store_out(p, imm=1)
        w.a.label(f"j{w.k}")
        w.k += 1
    return w.finish(f"{op}{32 if w32 else ''}{form.lower()}-{layout}")


LDDW_VALUES = [0, 1, 0x80000000, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF80000000, 0x7FFFFFFFFFFFFFFF,
               0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0]


def endian_lddw_program(layout="global"):
    """le / be at 16, 32, 64 over every dst, then lddw into every dst."""
    names = {("le", 16): "LE16", ("le", 32): "LE32", ("le", 64): "NOP",
             ("be", 16): "BE16", ("be", 32): "BE32", ("be", 64): "BE64"}
    steps = [(kind, bits, d) for kind in ("le", "be") for bits in (16, 32, 64) for d in range(10)]
    steps += [("lddw", 0, d) for d in range(10)]
    regs_of = lambda st: (st[2],)                # noqa: E731
    w = _Walk(layout, 8)
    for kind, bits, d in _Walk.order(steps, layout, regs_of):
        p = w.pointer(d)
        if kind == "lddw":
            w.site("LDDW")
            w.a.lddw(d, LDDW_VALUES[d])
        else:
            w.load(8, d, p, 8 if d & 1 else 0)
            w.site(names[(kind, bits)])
            (w.a.le if kind == "le" else w.a.be)(d, bits)
        w.store_out(p, src=d)
        w.k += 1
    return w.finish(f"endian-lddw-{layout}")


def lea_program(layout="global"):
    """`mov64 d, s; add64 / sub64 d, imm` over every (dst, src): the pair
    the loader fuses at link time into one LEA dispatch (two dispatches
    under BPFTIME_AMD_NO_FUSE).  The sites are the pair's two halves, which
    keep their load-time handlers."""
    steps = [(d, s) for d in range(10) for s in range(10)]
    regs_of = lambda st: (st[0], st[1])          # noqa: E731
    w = _Walk(layout, 8)
    for d, s in _Walk.order(steps, layout, regs_of):
        p = w.pointer(d, s)
        w.load(8, s, p, 0)
        imm = I[w.k % len(I)]
        sub = (w.k // len(I)) & 1
        w.site("A64_MOV_R")
        w.a.mov64(d, f"r{s}")
        w.site("A64_SUB_I" if sub else "A64_ADD_I")
        w.a.alu64("sub" if sub else "add", d, imm)
        w.store_out(p, src=d)
        w.k += 1
    return w.finish(f"lea-{layout}")


# --------------------------------------------------------------------------
# memory
# --------------------------------------------------------------------------
SIZES = (1, 2, 4, 8)
ST_IMMS = (-1, -5, 0x7FFFFFFF)


def memory_program(length, mode):
    """ldx / stx / st of every size at unit offsets 0, 1, 3, 7 and at the
    last legal byte, stores followed by loads of the other sizes over the
    same bytes, st immediates -1, -5 and 0x7FFFFFFF, and the same on the
    stack at negative offsets from r10 (aligned and not).  r0 folds every
    loaded value; the unit keeps every store.

    mode "slot": the unit pointer is a copy of r1, so the loader types
    every access below byte 64 as a slot access (staged at link time);
    "other": the pointer comes back from the stack and every access is
    generic."""
    a = Asm()
    p = 6
    if mode == "slot":
        a.mov64(p, "r1")
    else:
        a.stx(8, 10, -8, "r1").ldx(8, p, 10, -8)
    a.mov64(0, 0)

    def fold(r):
        a.alu64("mul", 0, 0x9E37).alu64("add", 0, f"r{r}")

    def offsets(sz):
        return sorted({0, 1, 3, 7, length - sz})

    for sz in SIZES:
        for off in offsets(sz):
            a.ldx(sz, 3, p, off)
            fold(3)
    for sz in SIZES:
        for off in offsets(sz):
            a.stx(sz, p, off, "r0")
            for sz2 in SIZES:
                if sz2 != sz:
                    a.ldx(sz2, 3, p, min(off, length - sz2))
                    fold(3)
    for imm in ST_IMMS:
        for sz in SIZES:
            for off in offsets(sz):
                a.st(sz, p, off, imm)
                a.ldx(8, 3, p, min(off, length - 8))
                fold(3)
    # the stack: [-16,-8) stx8, [-24,-16) st8, [-28,-24) st4, [-30,-28) st2,
    # -31 st1, -32 stx1; unaligned: [-47,-39) stx8, [-39,-37) stx2, [-37,-33) stx4
    a.stx(8, 10, -16, "r0").st(8, 10, -24, -5).st(4, 10, -28, -1).st(2, 10, -30, 0x7FFFFFFF)
    a.st(1, 10, -31, -5).stx(1, 10, -32, "r0")
    a.stx(8, 10, -47, "r0").stx(2, 10, -39, "r0").stx(4, 10, -37, "r0")
    for sz, off in [(1, -16), (2, -16), (4, -16), (8, -16), (8, -24), (4, -24), (4, -20), (8, -32), (4, -32),
                    (2, -30), (1, -31), (8, -47), (8, -41), (4, -45), (2, -43), (1, -34), (4, -37), (2, -39),
                    (8, -27), (4, -18)]:
        a.ldx(sz, 3, 10, off)
        fold(3)
    # the folded value back into the unit, then every size over it
    a.stx(8, p, 8, "r0")
    for sz in SIZES:
        a.ldx(sz, 3, p, 9)
        fold(3)
    a.exit()
    return Prog(f"memory-{length}-{mode}", a.assemble(), length, [], 0, mode == "slot")


def memory_units(n, length, seed=41):
    words = (n * length + 7) // 8
    return gen.sm64(seed, np.arange(words, dtype=np.uint64)).view(np.uint8)[:n * length].reshape(n, length).copy()


# --------------------------------------------------------------------------
# single-instruction programs for the hand vectors
# --------------------------------------------------------------------------
def vector_program(insn, a, b):
    """(code, memory) of the program that runs one hand vector; r0 is what
    the vector's expected value is compared with.  `insn` is
    <op>[32][i]: i = immediate form (b is the immediate); jumps give 1 when
    taken; ldx<N> loads from memory holding `a`; st<N>i / stx<N> store over
    memory holding `a` and give the 8 bytes back."""
    mem = bytearray((a & M64).to_bytes(8, "little") + ((b or 0) & M64).to_bytes(8, "little"))
    s = Asm()
    if insn == "ja":
        return s.mov64(0, 1).ja(1).mov64(0, 2).exit().assemble(), mem
    if insn == "lddw":
        return s.lddw(0, a).exit().assemble(), mem
    if insn.startswith("ldx"):
        return s.ldx(int(insn[3:]), 0, 1, 0).exit().assemble(), mem
    if insn.startswith("stx"):
        return s.ldx(8, 3, 1, 8).stx(int(insn[3:]), 1, 0, "r3").ldx(8, 0, 1, 0).exit().assemble(), mem
    if insn.startswith("st"):
        return s.st(int(insn[2:-1]), 1, 0, b).ldx(8, 0, 1, 0).exit().assemble(), mem
    if insn[:2] in ("le", "be") and insn[2:].isdigit():
        s.ldx(8, 0, 1, 0)
        (s.le if insn[:2] == "le" else s.be)(0, int(insn[2:]))
        return s.exit().assemble(), mem
    imm = insn.endswith("i")
    core = insn[:-1] if imm else insn
    w32 = core.endswith("32")
    op = core[:-2] if core[-2:] in ("32", "64") else core
    if op in JMP:
        s.ldx(8, 3, 1, 0).ldx(8, 4, 1, 8)
        (s.jmp32 if w32 else s.jmp)(op, 3, b if imm else "r4", "t")
        return s.mov64(0, 0).exit().label("t").mov64(0, 1).exit().assemble(), mem
    assert op in ALU, insn
    s.ldx(8, 0, 1, 0).ldx(8, 3, 1, 8)
    if op == "neg":
        s.neg32(0) if w32 else s.neg64(0)
    else:
        (s.alu32 if w32 else s.alu64)(op, 0, b if imm else "r3")
    return s.exit().assemble(), mem


# --------------------------------------------------------------------------
# references, computed once per (program, unit set) and shared
# --------------------------------------------------------------------------
_MODEL = {}
_ORACLE = {}


def _frozen(r0, units):
    r0.setflags(write=False)
    units.setflags(write=False)
    return r0, units


def model_reference(prog, units, key):
    """(r0 per unit, the units after the run) from the model; `key` names
    the unit set.  The arrays are shared and read-only."""
    from _isa_model import run_units
    k = (prog.name, key)
    if k not in _MODEL:
        _MODEL[k] = _frozen(*run_units(prog.code, units, prog.stride))
    return _MODEL[k]


def oracle_reference(po, prog, units, key):
    k = (prog.name, key)
    if k not in _ORACLE:
        vm = po.OracleVM()
        vm.load(prog.code)
        ou = units.copy()
        _ORACLE[k] = _frozen(vm.run_raw(ou, prog.stride), ou)
    return _ORACLE[k]
