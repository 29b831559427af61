"""Case library for the syscall dispatch planner (csrc/syscall_dispatch.cpp
plan_for / first_map_conflict, csrc/loader.cpp map_effects): small tracepoint
programs over per-thread state, each with the plan the rule gives it and
whether the reference's result depends on the order of one thread's calls.

The rule (runtime.hpp first_map_conflict).  Two attachments conflict on a map
when one writes it (W: any store, update, delete, fetching or non-add atomic)
and the other touches it, or one adds to it and the other loads its values.  One
attachment conflicts with itself on a map when it writes it other than by a
bpf_map_update_elem with the constant flags BPF_NOEXIST and a constant value
(immediates stored on the stack right before the call), or both adds to it and
loads from its values.  Any conflict -> plan 1 (thread-ordered), else
plan 0 (program-major: a thread's records in parallel lanes).

Every program keys its state by tid (the low 32 bits of
bpf_get_current_pid_tgid): the reference defines no order across threads.
Evidence a program cannot leave in a map goes out through
bpf_override_return (sys_enter) or bpf_set_retval (sys_exit), i.e. out_rets.

Maps (all HASH u32 tid -> u64, made by `MAPS`): "a" and "b" hold the state,
"obs" collects what a sys_enter reader saw (an override would keep the
sys_exit programs from running).  `Case.prefill` names the maps that get one
entry per thread before the dispatch (`prefill_value`).
"""
from dataclasses import dataclass, field
from typing import Callable, List, Tuple

import numpy as np

from bpftime_amd import gen, isa
from bpftime_amd.isa import Asm

HASH = isa.BPF_MAP_TYPE_HASH
MAPS = [("a", HASH, 4, 8, 1024), ("b", HASH, 4, 8, 1024), ("obs", HASH, 4, 8, 1024)]
N_RECORDS = 4096
THREADS = (1, 8, 65, 200)
BPF_EXIST = 2
ARG0, ARG1, RET = 16, 24, 16  # ctx offsets: sys_enter args[0], args[1]; sys_exit ret


def records(threads: int) -> np.ndarray:
    """4096 128-B records from `threads` threads; a third of the calls are
    syscall 0 and a third syscall 1 (the per-syscall cases need both)."""
    recs = gen.syscall_records_timed(N_RECORDS, threads=threads)
    w = recs.view(np.int64).reshape(N_RECORDS, 16)
    w[0::3, 1] = w[0::3, 9] = 0
    w[1::3, 1] = w[1::3, 9] = 1
    return recs


def tids(recs: np.ndarray) -> np.ndarray:
    return np.unique(recs.view(np.uint64).reshape(len(recs), 16)[:, 11] & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def reverse_threads(recs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The same calls with each thread's calls in reverse order -> (records,
    src): position i of the result holds record src[i] of `recs`, so
    ``rets_of_original[src] = rets_of_reversed``."""
    pid = recs.view(np.uint64).reshape(len(recs), 16)[:, 11]
    src = np.arange(len(recs))
    for p in np.unique(pid):
        at = np.flatnonzero(pid == p)
        src[at] = at[::-1]
    return np.ascontiguousarray(recs[src]), src


def prefill_value(name: str, tid: int) -> int:
    return {"a": 3 * tid + 1, "b": 5 * tid + 2, "obs": 0}[name]


# ---- program pieces ---------------------------------------------------------

def _begin() -> Asm:
    """r6 = ctx; the u32 key (tid) at fp-4."""
    return Asm().mov64(6, "r1").call(isa.BPF_FUNC_get_current_pid_tgid).stx(4, 10, -4, "r0")


def _lookup(a: Asm, fd: int, miss: str) -> Asm:
    """r0 = &map[tid], or a jump to `miss`."""
    return (a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_lookup_elem)
            .jmp("jeq", 0, 0, miss))


def _end(a: Asm) -> bytes:
    return a.label("out").mov64(0, 0).exit().assemble()


def _update(a: Asm, fd: int, flags) -> Asm:
    """bpf_map_update_elem(map, &tid, fp-16, flags): flags an immediate or a register."""
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16)
    return a.mov64(4, flags).call(isa.BPF_FUNC_map_update_elem)


def _override(a: Asm, reg: str) -> Asm:
    return a.mov64(1, "r6").mov64(2, reg).call(isa.BPF_FUNC_override_return)


def s_add(fd: int) -> bytes:
    """cnt[tid] += (args[0] & 0xff) + 1, atomically."""
    a = _lookup(_begin(), fd, "out")
    a.ldx(8, 1, 6, ARG0).alu64("and", 1, 0xFF).add64(1, 1).atomic(8, isa.ATOMIC_ADD, 0, 0, "r1")
    return _end(a)


def s_init_add(fd: int) -> bytes:
    """bpf_map_lookup_or_try_init, then a counter add (syscount_exit's and
    syscall_agg's shape): a miss inserts a zero value with BPF_NOEXIST."""
    a = _begin()
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_lookup_elem).jmp("jne", 0, 0, "have")
    a.st(8, 10, -16, 0)
    _update(a, fd, isa.BPF_NOEXIST)
    _lookup(a, fd, "out")
    a.label("have").ldx(8, 1, 6, ARG0).alu64("and", 1, 0xFF).add64(1, 1).atomic(8, isa.ATOMIC_ADD, 0, 0, "r1")
    return _end(a)


def s_read(fd: int) -> bytes:
    """override_return(cnt[tid])."""
    a = _lookup(_begin(), fd, "out").ldx(8, 7, 0, 0)
    return _end(_override(a, "r7"))


def s_update(fd: int, flags=isa.BPF_ANY) -> bytes:
    """start[tid] = args[0] through bpf_map_update_elem (syscount_enter's
    shape with the argument for the clock); `flags` an immediate, or "var":
    args[1] & 1 at run time (BPF_ANY or BPF_NOEXIST, not a constant)."""
    a = _begin().ldx(8, 1, 6, ARG0).stx(8, 10, -16, "r1")
    if flags == "var":
        a.ldx(8, 8, 6, ARG1).alu64("and", 8, 1)
        flags = "r8"
    return _end(_update(a, fd, flags))


def s_update_joinflags(fd: int) -> bytes:
    """flags = args[1] & 1 ? BPF_NOEXIST : BPF_ANY the way compilers lower it:
    mov r4, 0; jeq +1; mov r4, 1; call -- the two paths meet AT the call, and
    the instruction before it says BPF_NOEXIST."""
    a = _begin().ldx(8, 1, 6, ARG0).stx(8, 10, -16, "r1").ldx(8, 8, 6, ARG1).alu64("and", 8, 1)
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16)
    a.mov64(4, isa.BPF_ANY).jmp("jeq", 8, 0, "call").mov64(4, isa.BPF_NOEXIST)
    a.label("call").call(isa.BPF_FUNC_map_update_elem)
    return _end(a)


def s_init_value(fd: int) -> bytes:
    """first[tid] = args[0] with BPF_NOEXIST (a first-seen record): the
    reference keeps the thread's FIRST call's value."""
    return s_update(fd, isa.BPF_NOEXIST)


def s_init_joinvalue(fd: int) -> bytes:
    """BPF_NOEXIST insert of 7 or, when args[1] is odd, 9: both stores are
    immediates, but the paths meet between them and the call."""
    a = _begin().ldx(8, 8, 6, ARG1).alu64("and", 8, 1)
    a.st(8, 10, -16, 7).jmp("jeq", 8, 0, "seven").st(8, 10, -16, 9).label("seven")
    return _end(_update(a, fd, isa.BPF_NOEXIST))


def s_store(fd: int) -> bytes:
    """*lookup(tid) = args[0]."""
    a = _lookup(_begin(), fd, "out").ldx(8, 3, 6, ARG0).stx(8, 0, 0, "r3")
    return _end(a)


def s_load_add(fd: int) -> bytes:
    """v = cnt[tid]; cnt[tid] += 1 (atomic); override_return(v): a per-thread
    rate limiter's shape.  In the reference a thread's calls see 0, 1, 2, ..."""
    a = _lookup(_begin(), fd, "out").ldx(8, 7, 0, 0).mov64(1, 1).atomic(8, isa.ATOMIC_ADD, 0, 0, "r1")
    return _end(_override(a, "r7"))


def s_fetch(fd: int) -> bytes:
    """old = fetch_add(&v, args[0] | 1); old2 = xchg(&v, args[1]);
    override_return(old + old2)."""
    a = _lookup(_begin(), fd, "out").mov64(9, "r0")
    a.ldx(8, 7, 6, ARG0).alu64("or", 7, 1).atomic(8, isa.ATOMIC_ADD | isa.ATOMIC_FETCH, 9, 0, "r7")
    a.ldx(8, 8, 6, ARG1).atomic(8, isa.ATOMIC_XCHG, 9, 0, "r8")
    a.alu64("add", 7, "r8")
    return _end(_override(a, "r7"))


def s_toggle(fd: int) -> bytes:
    """present ? delete : insert args[0]; override_return(present)."""
    a = _begin()
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_lookup_elem).jmp("jeq", 0, 0, "absent")
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_delete_elem)
    a.mov64(7, 1).ja("report")
    a.label("absent").ldx(8, 1, 6, ARG0).stx(8, 10, -16, "r1")
    _update(a, fd, isa.BPF_ANY)
    a.mov64(7, 0)
    a.label("report")
    return _end(_override(a, "r7"))


def p_read(fd: int, enter: bool, obs_fd: int) -> bytes:
    """The pair classes' reader.  sys_exit: set_retval(map[tid]).  sys_enter:
    obs[tid] += map[tid] (an override would stop the call's exit programs)."""
    a = _lookup(_begin(), fd, "out").ldx(8, 7, 0, 0)
    if enter:
        _lookup(a, obs_fd, "out").atomic(8, isa.ATOMIC_ADD, 0, 0, "r7")
    else:
        a.mov64(1, "r7").call(isa.BPF_FUNC_set_retval)
    return _end(a)


def p_add(fd: int, enter: bool) -> bytes:
    """map[tid] += (args[0] or ret) & 0xff, + 1."""
    a = _lookup(_begin(), fd, "out")
    a.ldx(8, 1, 6, ARG0 if enter else RET).alu64("and", 1, 0xFF).add64(1, 1).atomic(8, isa.ATOMIC_ADD, 0, 0, "r1")
    return _end(a)


def p_write(fd: int, enter: bool) -> bytes:
    """map[tid] = args[0] or ret, bpf_map_update_elem with BPF_ANY."""
    a = _begin().ldx(8, 1, 6, ARG0 if enter else RET).stx(8, 10, -16, "r1")
    return _end(_update(a, fd, isa.BPF_ANY))


def p_init(fd: int, value: int) -> bytes:
    """bpf_map_update_elem(map, &tid, &value, BPF_NOEXIST) of a constant: a
    write that does not conflict with itself (the first call's insert stays,
    and it is the same whichever call that is)."""
    a = _begin().st(8, 10, -16, value)
    return _end(_update(a, fd, isa.BPF_NOEXIST))


# ---- the cases --------------------------------------------------------------

@dataclass
class Case:
    id: str
    # fds {"a", "b", "obs"} -> [(code, sys_nr, enter)]
    build: Callable[[dict], List[Tuple[bytes, int, bool]]]
    plan: int              # what syscall_dispatch_plan() must answer
    sensitive: bool        # the reference's result changes when a thread's calls are reversed
    prefill: Tuple[str, ...] = field(default=("a", "b", "obs"))


def _self(id_, prog, plan, sensitive, prefill=("a",)):
    return Case(id_, lambda f: [(prog(f["a"]), -1, True)], plan, sensitive, prefill)


SELF = [
    _self("S-add", s_add, 0, False),
    _self("S-init-add", s_init_add, 0, False, prefill=()),
    _self("S-read", s_read, 0, False),
    _self("S-update", s_update, 1, True, prefill=()),
    _self("S-update-exist", lambda fd: s_update(fd, BPF_EXIST), 1, True),
    _self("S-update-varflags", lambda fd: s_update(fd, "var"), 1, True, prefill=()),
    _self("S-update-joinflags", s_update_joinflags, 1, True, prefill=()),
    _self("S-init-value", s_init_value, 1, True, prefill=()),
    _self("S-init-joinvalue", s_init_joinvalue, 1, True, prefill=()),
    _self("S-store", s_store, 1, True),
    _self("S-load-add", s_load_add, 1, True),
    _self("S-fetch", s_fetch, 1, True),
    _self("S-toggle", s_toggle, 1, True, prefill=()),
]

_KIND = {"read": lambda fd, enter, f: p_read(fd, enter, f["obs"]),
         "add": lambda fd, enter, f: p_add(fd, enter),
         "write": lambda fd, enter, f: p_write(fd, enter)}


def _pair_plan(e: str, x: str, same: bool) -> int:
    if "write" in (e, x):
        return 1  # BPF_ANY update: conflicts with itself, whatever the partner does
    if same and {e, x} == {"read", "add"}:
        return 1  # the reader sees the running sum
    return 0      # reads beside reads, adds beside adds, or disjoint maps


def _pair(e: str, x: str, same: bool) -> Case:
    build = lambda f: [(_KIND[e](f["a"], True, f), -1, True),
                       (_KIND[x](f["a" if same else "b"], False, f), -1, False)]
    plan = _pair_plan(e, x, same)
    # (for these classes the rule is tight: every conflict shows under reversal)
    return Case(f"P-{e}-{x}-{'same' if same else 'disjoint'}", build, plan, bool(plan))


PAIRS = [_pair(e, x, same) for same in (True, False) for e in _KIND for x in _KIND]

# NOEXIST inserts: free of the self rule, so these reach the pair rule's write
# arm on their own.  The order they depend on is enter-before-exit within one
# call, which reversing a thread's calls does not change: plan 1 without a
# difference under reversal (the model test cannot show these; the device
# parity test does: program-major runs every enter before every exit).
INIT_PAIRS = [
    Case("P-init-read-same", lambda f: [(p_init(f["a"], 7), -1, True), (p_read(f["a"], False, f["obs"]), -1, False)],
         1, False, prefill=("b", "obs")),
    Case("P-init-read-disjoint", lambda f: [(p_init(f["a"], 7), -1, True), (p_read(f["b"], False, f["obs"]), -1, False)],
         0, False, prefill=("b", "obs")),
    Case("P-read-init-same", lambda f: [(p_read(f["a"], True, f["obs"]), -1, True), (p_init(f["a"], 7), -1, False)],
         1, False, prefill=("b", "obs")),
    Case("P-read-init-disjoint", lambda f: [(p_read(f["b"], True, f["obs"]), -1, True), (p_init(f["a"], 7), -1, False)],
         0, False, prefill=("b", "obs")),
]

# sys_enter programs of different syscalls on the same per-thread key: each
# sees a disjoint set of records, and still they do not commute
PER_SYSCALL = [
    Case("N-init-init", lambda f: [(p_init(f["a"], 7), 0, True), (p_init(f["a"], 9), 1, True)],
         1, True, prefill=("b", "obs")),
    Case("N-add-read", lambda f: [(p_add(f["a"], True), 0, True), (p_read(f["a"], True, f["obs"]), 1, True)],
         1, True),
]

CASES = SELF + PAIRS + INIT_PAIRS + PER_SYSCALL
BY_ID = {c.id: c for c in CASES}
assert len(PAIRS) == 18 and len(BY_ID) == len(CASES)


def loop_then_add(fd: int, rounds: int = 110) -> bytes:
    """About 3 * rounds instructions of loop (rounds - 1 taken jumps: the asm
    tier counts those, the C++ tier every instruction), then cnt[tid] += 1:
    the step-limit cases.  A VM whose limit is below rounds - 1 never reaches
    the add in either tier."""
    a = _begin().mov64(7, rounds).mov64(8, 0)
    a.label("spin").add64(7, -1).alu64("xor", 8, "r7").jmp("jne", 7, 0, "spin")
    _lookup(a, fd, "out").mov64(1, 1).atomic(8, isa.ATOMIC_ADD, 0, 0, "r1")
    return _end(a)
