"""Builders for the tests of the thread-ordered uprobe replay's two execution
tiers (tests/test_gpu_uprobe_asm.py): ragged per-thread records over five
functions, and the program pairs (eBPF bytes, the callable that restates them)
that tests/_uprobe*.py do not have."""
import numpy as np

from bpftime_amd import isa, programs
from bpftime_amd.isa import Asm

import _uprobe as um
import _uprobe_threads as ut

F0, F1, F2 = um.FUNCS
F3, F4 = 0x405500, 0x7F0000006600                       # two more attachable functions
FUNCS = (F0, F1, F2, F3, F4)
# common.hpp kUpSeqAsmThreads: up to this many recorded threads a dispatch that
# no environment variable steers runs its callbacks in the asm tier
ASM_THREADS = 65536
LDS_STACK = 64                                          # common.hpp kLdsStackMax
# (threads, ragged's calls range) of the many-wave cases: the cut-off from both sides
MANY_WAVES = [(4096, (1, 6)), (ASM_THREADS, (1, 3)), (ASM_THREADS + 1, (1, 3))]


def auto_tier(threads):
    return 1 if threads <= ASM_THREADS else 0


def ragged(threads, seed=5, funcs=FUNCS + (um.NOBODY,), calls=(1, 6)):
    """um.records' fields for `threads` recorded threads of calls[0] ..
    calls[1] - 1 calls each (1-5 by default; a fixed seed; the calls of all
    threads interleaved at random, so a lane's walk is ragged against its
    neighbours').  pid_tgid and strictly increasing clocks as ut.records has
    them."""
    rng = np.random.default_rng(seed + 7 * threads)
    calls = rng.integers(calls[0], calls[1], threads)
    owner = rng.permutation(np.repeat(np.arange(threads), calls))
    n = len(owner)
    r = um.records(n, seed=seed + threads, funcs=funcs)
    r["pid"] = np.array([(ut.tgid_of(t) << 32) | ut.tid_of(t) for t in owner], dtype=np.uint64)
    dur = (np.uint64(1) << rng.integers(0, 41, n).astype(np.uint64)) + rng.integers(0, 3, n).astype(np.uint64)
    gap = rng.integers(1, 5, n)
    clock = np.zeros((n, 2), dtype=np.uint64)
    now = 1000
    for i in range(n):
        clock[i] = (now, now + int(dur[i]))
        now += int(dur[i]) + int(gap[i])
    r["clock"], r["owner"] = clock, owner
    return r


def clock_seq(cnt_fd, at_fd, cnt, at):
    """c = cnt[tid] (0 when absent); cnt[tid] = c + 1; at[tid << 32 | c] =
    bpf_ktime_get_ns(): the clock every call of a thread saw, in the order the
    calls ran."""
    a = Asm()
    ut._tid_to_stack(a)
    a.mov64(2, "r10").add64(2, -4).ld_map_fd(1, cnt_fd).call(isa.BPF_FUNC_map_lookup_elem)
    ut._seq_count(a)
    a.mov64(1, "r7").add64(1, 1).stx(8, 10, -16, 1)
    a.mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, cnt_fd).call(isa.BPF_FUNC_map_update_elem)
    a.alu64("lsh", 6, 32).alu64("or", 6, "r7").stx(8, 10, -24, 6)
    a.call(isa.BPF_FUNC_ktime_get_ns).stx(8, 10, -32, 0)
    a.mov64(2, "r10").add64(2, -24).mov64(3, "r10").add64(3, -32).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, at_fd).call(isa.BPF_FUNC_map_update_elem)
    a.mov64(0, 0)

    def py(e):
        tid = e.pid_tgid & 0xFFFFFFFF
        c = cnt.get(tid, 0)
        cnt[tid] = c + 1
        at[(tid << 32) | c] = e.ktime
        return 0
    return a.exit().assemble(), py


def spin_then_count(jumps, map_fd, counts):
    """A bounded loop of `jumps` taken jumps, then counts[PT_REGS_PARM1] += 1:
    past the VM's step limit the callback fails before it counts."""
    a = Asm()
    a.mov64(9, "r1").mov64(0, 0).label("top").add64(0, 1).jmp("jlt", 0, jumps, "top")
    a.ldx(8, 0, 9, 8 * um.DI)
    code = programs._count_key_r0(a, map_fd).assemble()
    return code, lambda e: um._count(counts, int(e.regs[um.DI]))


def failing(e):
    raise um.Failed()


def deep_stack_count(map_fd, counts):
    """counts[PT_REGS_PARM1] += 1 by a program that keeps a word 2 * LDS_STACK
    bytes below its frame pointer: its stack does not fit the LDS stacks."""
    a = Asm()
    a.ldx(8, 0, 1, 8 * um.DI).stx(8, 10, -2 * LDS_STACK, 0).ldx(8, 0, 10, -2 * LDS_STACK)
    code = programs._count_key_r0(a, map_fd).assemble()
    return code, lambda e: um._count(counts, int(e.regs[um.DI]))


def replace_di_plus(k):
    """A replace program without 173: r0 = PT_REGS_PARM1 + k."""
    a = Asm()
    a.ldx(8, 0, 1, 8 * um.DI).add64(0, k)
    return a.exit().assemble(), lambda e: (int(e.regs[um.DI]) + k) & um.M64
