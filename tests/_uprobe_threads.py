"""Builders for the thread-ordered uprobe replay's tests: program pairs (the
eBPF bytes and the Python callable that restates them, as tests/_uprobe.py's)
and records with a chosen number of recorded threads.

um.Model.dispatch runs the calls one after another in record order, each
call's entry callbacks and then its return callbacks.  That is the per-thread
order's serial equivalent, and the parallel device run equals it for programs
that write per-thread keys only and touch shared words only by atomic adds:
every pair here is such a program, except the `plain` histogram variant, which
is for ORDERED dispatches.

The pairs restate the reference's funclatency
(example/tracing/funclatency/funclatency.bpf.c): the entry probe stores
starts[tid] = bpf_ktime_get_ns(), the return probe looks it up and adds one to
slot log2(now - start) of a histogram.  A callable's maps are Python
containers: `starts` / `cnt` / `order` dicts, `hist` a list of 32 ints."""
import numpy as np

from bpftime_amd import isa, programs
from bpftime_amd.isa import Asm

import _uprobe as um

M64 = um.M64
SLOTS = 32


def log2_slot(v):
    """The histogram slot of a u64 delta: floor(log2(v)) (0 for 0 and 1), at most 31."""
    return min(SLOTS - 1, max(v.bit_length() - 1, 0))


def _tid_to_stack(a):
    """*(u32 *)(fp - 4) = (u32)bpf_get_current_pid_tgid(); r6 = the whole value."""
    a.call(isa.BPF_FUNC_get_current_pid_tgid).mov64(6, "r0")
    return a.stx(4, 10, -4, 0)


def funclat_entry(starts_fd, starts, targ_tgid=0):
    """starts[tid] = bpf_ktime_get_ns(), for calls of process targ_tgid (0: every)."""
    a = Asm()
    _tid_to_stack(a)
    if targ_tgid:
        a.mov64(1, "r6").alu64("rsh", 1, 32).jmp("jne", 1, targ_tgid, "out")
    a.call(isa.BPF_FUNC_ktime_get_ns).stx(8, 10, -16, 0)
    a.mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, starts_fd).call(isa.BPF_FUNC_map_update_elem)
    a.label("out").mov64(0, 0)

    def py(e):
        if targ_tgid and e.pid_tgid >> 32 != targ_tgid:
            return 0
        starts[e.pid_tgid & 0xFFFFFFFF] = e.ktime
        return 0
    return a.exit().assemble(), py


def funclat_return(starts_fd, hist_fd, starts, hist, delete=False, plain=False):
    """hist[log2(bpf_ktime_get_ns() - starts[tid])] += 1 when starts[tid] is
    there.  The add is a 32-bit atomic add, or (plain, the reference's own
    source: ORDERED dispatches only) a load / add / store.  delete: starts[tid]
    is deleted afterwards, so a return without a start takes the miss path."""
    a = Asm()
    _tid_to_stack(a)
    a.mov64(2, "r10").add64(2, -4).ld_map_fd(1, starts_fd).call(isa.BPF_FUNC_map_lookup_elem)
    a.jmp("jeq", 0, 0, "out")
    a.ldx(8, 7, 0, 0)                                   # r7 = start
    a.call(isa.BPF_FUNC_ktime_get_ns).mov64(6, "r0").alu64("sub", 6, "r7")   # r6 = delta
    # r8 = floor(log2(r6)), loop-free: halve the range six times
    a.mov64(8, 0)
    for k, bits in enumerate((32, 16, 8, 4, 2, 1)):
        a.mov64(2, "r6").alu64("rsh", 2, bits).jmp("jeq", 2, 0, f"s{k}")
        a.mov64(6, "r2").add64(8, bits).label(f"s{k}")
    a.jmp("jle", 8, SLOTS - 1, "fits").mov64(8, SLOTS - 1).label("fits")
    a.st(4, 10, -8, 0)
    a.mov64(2, "r10").add64(2, -8).ld_map_fd(1, hist_fd).call(isa.BPF_FUNC_map_lookup_elem)
    a.jmp("jeq", 0, 0, "out")
    a.alu64("lsh", 8, 2).add64(0, "r8")
    if plain:
        a.ldx(4, 1, 0, 0).add64(1, 1).stx(4, 0, 0, 1)
    else:
        a.mov64(1, 1).atomic(4, isa.ATOMIC_ADD, 0, 0, 1)
    if delete:
        a.mov64(2, "r10").add64(2, -4).ld_map_fd(1, starts_fd).call(isa.BPF_FUNC_map_delete_elem)
    a.label("out").mov64(0, 0)

    def py(e):
        tid = e.pid_tgid & 0xFFFFFFFF
        if tid not in starts:
            return 0
        hist[log2_slot((e.ktime - starts[tid]) & M64)] += 1
        if delete:
            del starts[tid]
        return 0
    return a.exit().assemble(), py


def _seq_count(a):
    """r7 = the u64 the lookup in r0 found, 0 when it found none."""
    return a.mov64(7, 0).jmp("jeq", 0, 0, "none").ldx(8, 7, 0, 0).label("none")


def seq_entry(cnt_fd, order_fd, cnt, order):
    """c = cnt[tid] (0 when absent); cnt[tid] = c + 1; order[tid << 32 | c] =
    PT_REGS_PARM1: the calls of a thread, numbered in the order they ran."""
    a = Asm()
    a.mov64(9, "r1")
    _tid_to_stack(a)
    a.mov64(2, "r10").add64(2, -4).ld_map_fd(1, cnt_fd).call(isa.BPF_FUNC_map_lookup_elem)
    _seq_count(a)
    a.mov64(1, "r7").add64(1, 1).stx(8, 10, -16, 1)
    a.mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, cnt_fd).call(isa.BPF_FUNC_map_update_elem)
    a.alu64("lsh", 6, 32).alu64("or", 6, "r7").stx(8, 10, -24, 6)
    a.ldx(8, 1, 9, 8 * um.DI).stx(8, 10, -32, 1)
    a.mov64(2, "r10").add64(2, -24).mov64(3, "r10").add64(3, -32).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, order_fd).call(isa.BPF_FUNC_map_update_elem)
    a.mov64(0, 0)

    def py(e):
        tid = e.pid_tgid & 0xFFFFFFFF
        c = cnt.get(tid, 0)
        cnt[tid] = c + 1
        order[(tid << 32) | c] = int(e.regs[um.DI])
        return 0
    return a.exit().assemble(), py


def seq_return(cnt_fd, seen_fd, cnt, seen):
    """seen[tid << 32 | cnt[tid]] = the return registers' ax: a uretprobe that
    reads what seq_entry left for the same call (its number + 1)."""
    a = Asm()
    a.mov64(9, "r1")
    _tid_to_stack(a)
    a.mov64(2, "r10").add64(2, -4).ld_map_fd(1, cnt_fd).call(isa.BPF_FUNC_map_lookup_elem)
    _seq_count(a)
    a.alu64("lsh", 6, 32).alu64("or", 6, "r7").stx(8, 10, -24, 6)
    a.ldx(8, 1, 9, 8 * um.AX).stx(8, 10, -32, 1)
    a.mov64(2, "r10").add64(2, -24).mov64(3, "r10").add64(3, -32).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, seen_fd).call(isa.BPF_FUNC_map_update_elem)
    a.mov64(0, 0)

    def py(e):
        tid = e.pid_tgid & 0xFFFFFFFF
        seen[(tid << 32) | cnt.get(tid, 0)] = int(e.regs[um.AX])
        return 0
    return a.exit().assemble(), py


def di_count(map_fd, counts):
    """counts[PT_REGS_PARM1] += 1: reads the ctx a program before it may have written."""
    a = Asm()
    a.ldx(8, 0, 1, 8 * um.DI)
    return programs._count_key_r0(a, map_fd).assemble(), lambda e: um._count(counts, int(e.regs[um.DI]))


def replace_faulting_at(di_bad, value):
    """A replace program that reads address 0 when PT_REGS_PARM1 == di_bad (the
    launch's window check fails the unit; no access is made), else returns value."""
    a = Asm()
    a.ldx(8, 2, 1, 8 * um.DI).jmp("jne", 2, di_bad, "ok").mov64(3, 0).ldx(8, 0, 3, 0).label("ok").mov64(0, value)

    def py(e):
        if int(e.regs[um.DI]) == di_bad:
            raise um.Failed()
        return value
    return a.exit().assemble(), py


# ---- records ----------------------------------------------------------------------
def tid_of(t):
    return 100 + t


def tgid_of(t):
    return 1 + t % 3


def records(n, threads, seed=77, funcs=um.FUNCS + (um.NOBODY,)):
    """um.records' fields for n calls by min(threads, n) recorded threads.  The
    distribution is skewed: thread 0 owns about half the calls, and with more
    calls than threads every thread owns at least one (the upper half of the
    threads exactly one).  A thread's pid_tgid is tgid_of(t) << 32 | tid_of(t).
    The clocks increase strictly along the records, so inside every thread
    too; a call lasts 2^k + noise ns for k in 0..40 (every histogram slot, the
    clamp included)."""
    r = um.records(n, seed=seed + threads, funcs=funcs)
    rng = np.random.default_rng(seed + 31 * n + threads)
    threads = max(1, min(threads, n))
    owner = np.where(rng.random(n) < 0.5, 0, rng.integers(0, max(threads // 2, 1), n))
    if n >= threads:
        owner[rng.permutation(n)[:threads]] = np.arange(threads)
    r["pid"] = np.array([(tgid_of(t) << 32) | tid_of(t) for t in owner], dtype=np.uint64)
    dur = (np.uint64(1) << rng.integers(0, 41, n).astype(np.uint64)) + rng.integers(0, 3, n).astype(np.uint64)
    gap = rng.integers(1, 5, n)
    clock = np.zeros((n, 2), dtype=np.uint64)
    now = 1000
    for i in range(n):
        clock[i] = (now, now + int(dur[i]))
        now += int(dur[i]) + int(gap[i])
    r["clock"] = clock
    r["owner"] = owner
    return r


# ---- the oracle's maps as the callables' containers ----------------------------------
def oracle_dict(omap):
    return {int.from_bytes(k, "little"): int.from_bytes(v, "little") for k, v in omap.items().items()}


def oracle_hist(omap):
    return [int(x) for x in np.frombuffer(omap.lookup(b"\0\0\0\0"), dtype=np.uint32)]
