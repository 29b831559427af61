"""A Python model of the uprobe replay dispatch, restated from the reference's
frida attach implementation, and builders for the test programs and records.

Which attachments run at a function:
  * a function whose first attachment is an override / replace runs only that
    one and refuses later ones with -EEXIST (frida_uprobe_attach_impl.cpp:64-79);
  * otherwise its uprobes run at entry and its uretprobes at return, in attach
    order (frida_internal_attach_entry.cpp:221-239); an override attached after
    them never runs (the function is hooked as a listener, :128-165).
bpf_get_func_ip answers the function inside a uprobe / uretprobe and 0 inside an
override (frida_attach_entry.hpp:25-40); bpf_get_attach_cookie the attachment's
cookie or 0 (bpf_helper.cpp:684-695).  An override's 58 / 187 replaces the
call's return (:243-277); a replace always returns r0
(frida_uprobe_attach_impl.cpp:236-263); from a plain probe the two helpers
throw (base_attach_impl.hpp:76-105), which fails the callback.

The model runs the calls one after another, each call's entry callbacks and
then its return callbacks: the reference's order, not the device's
program-major one.  A program is a Python callable over an Env (the test
programs below come in pairs: the eBPF bytes and the callable that restates
them), so helpers 173 / 174 are plain attributes here.  The callables, not
the oracle interpreter, drive the model because the oracle's override state
and clock belong to its own syscall dispatch and cannot be set per callback;
instead run_bytes below executes a pair's eBPF bytes in the oracle
interpreter, with 173 / 174 / 58 / 187 / 14 / 5 registered as stubs over an
Env, and tests/test_uprobe_model.py holds every pair's two halves against
each other that way: the bytes are run by something other than the device."""
import ctypes as C

import numpy as np

from bpftime_amd import isa, programs
from bpftime_amd.isa import Asm

UPROBE, URETPROBE, OVERRIDE, UREPLACE = 6, 7, 1008, 1009
EEXIST = 17
M64 = (1 << 64) - 1
DI, AX, IP = 112 // 8, 80 // 8, 128 // 8                # words of struct pt_regs
FUNCS = (0x401000, 0x402200, 0x7F0000003300)            # three attachable functions
NOBODY = 0x404400                                       # ... and one nobody attaches to


class Failed(Exception):
    """The callback failed (the reference's helper threw)."""


class Env:
    def __init__(self, regs, func_ip, cookie, pid_tgid, ktime, stack, can_override):
        self.regs = regs                                # a copy: writes never reach the record
        self.func_ip, self.cookie, self.pid_tgid, self.ktime, self.stack = func_ip, cookie, pid_tgid, ktime, stack
        self.can_override = can_override
        self.overridden = None

    def override(self, value):                          # helpers 58 / 187
        if not self.can_override:
            raise Failed()
        self.overridden = value & M64


class Model:
    def __init__(self):
        self.att, self.replaced, self.next_id = [], {}, 1

    def attach(self, func, kind, prog, cookie=None):
        ovr = kind in (OVERRIDE, UREPLACE)
        if self.replaced.get(func):
            return -EEXIST
        self.replaced.setdefault(func, ovr)
        self.att.append(dict(id=self.next_id, func=func, kind=kind, prog=prog, cookie=cookie))
        self.next_id += 1
        return self.next_id - 1

    def detach(self, i):
        func = [a["func"] for a in self.att if a["id"] == i]
        self.att = [a for a in self.att if a["id"] != i]
        if func and not any(a["func"] == func[0] for a in self.att):
            self.replaced.pop(func[0], None)

    def running(self, func):
        """(entry callbacks, return callbacks) of a call of func."""
        at = [a for a in self.att if a["func"] == func]
        if not at:
            return [], []
        if self.replaced[func]:
            return at[:1], []
        return [a for a in at if a["kind"] == UPROBE], [a for a in at if a["kind"] == URETPROBE]

    def dispatch(self, func, enter=None, leave=None, pid_tgid=None, clock=None, stacks=None, out_state=None,
                 out_rets=None, default_pid=0, default_clock=0):
        """Runs every call in order; returns the failed callbacks.  out_state /
        out_rets: the caller's arrays, updated in place."""
        failed = 0
        for i, f in enumerate(func):
            ent, ret = self.running(int(f))
            for phase, cbs, regs in ((0, ent, enter), (1, ret, leave)):
                for a in cbs:
                    ovr = a["kind"] in (OVERRIDE, UREPLACE)
                    e = Env(np.array(regs[i], dtype=np.uint64), 0 if ovr else int(f), a["cookie"] or 0,
                            int(pid_tgid[i]) if pid_tgid is not None else default_pid,
                            int(clock[i][phase]) if clock is not None else default_clock,
                            None if stacks is None else list(stacks[i]), ovr)
                    try:
                        r0 = a["prog"](e)
                    except Failed:
                        failed += 1
                        continue
                    if a["kind"] == UREPLACE:
                        e.overridden = r0 & M64
                    if e.overridden is not None:
                        out_state[i] |= 1
                        out_rets[i] = np.uint64(e.overridden).astype(np.int64)
        return failed


# ---- programs: (eBPF bytes, the callable that restates them) -----------------------
def _count(counts, key):
    counts[key] = counts.get(key, 0) + 1
    return 0


def func_ip_count(map_fd, counts):
    return programs.func_ip_count(map_fd), lambda e: _count(counts, e.func_ip)


def cookie_tag(map_fd, counts):
    return programs.cookie_tag(map_fd), lambda e: _count(counts, e.cookie)


def count_by_helper(helper, map_fd, counts):
    """counts[helper()] += 1 for bpf_get_current_pid_tgid (14) / bpf_ktime_get_ns (5)."""
    a = Asm()
    a.call(helper)
    code = programs._count_key_r0(a, map_fd).assemble()
    attr = {isa.BPF_FUNC_get_current_pid_tgid: "pid_tgid", isa.BPF_FUNC_ktime_get_ns: "ktime"}[helper]
    return code, lambda e: _count(counts, getattr(e, attr))


def override_if_arg0(value, arg0):
    def py(e):
        if int(e.regs[DI]) == arg0 & M64:
            e.override(value)
        return 0
    return programs.override_if_arg0(value, arg0), py


def replace_with_arg0_plus(k):
    """A replace program: r0 = PT_REGS_PARM1 + k + bpf_get_func_ip (0 inside a replace)."""
    a = Asm()
    a.ldx(8, 6, 1, 8 * DI).call(isa.BPF_FUNC_get_func_ip).add64(0, "r6").add64(0, k)
    return a.exit().assemble(), lambda e: (int(e.regs[DI]) + k + e.func_ip) & M64


def override_func_ip_plus(k):
    """An override program: bpf_override_return(ctx, bpf_get_func_ip(ctx) + k), always."""
    a = Asm()
    a.mov64(6, "r1").call(isa.BPF_FUNC_get_func_ip).mov64(2, "r0").add64(2, k).mov64(1, "r6")
    a.call(isa.BPF_FUNC_override_return).mov64(0, 0)

    def py(e):
        e.override(e.func_ip + k)
        return 0
    return a.exit().assemble(), py


def ctx_writer(map_fd, counts):
    """Stores into its ctx (di, ax, ip), then counts by the di it reads back."""
    a = Asm()
    a.st(8, 1, 8 * DI, 77).st(8, 1, 8 * AX, -1).st(8, 1, 8 * IP, 0)
    a.ldx(8, 0, 1, 8 * DI)
    code = programs._count_key_r0(a, map_fd).assemble()

    def py(e):
        e.regs[DI], e.regs[AX], e.regs[IP] = 77, M64, 0
        return _count(counts, 77)
    return code, py


# ---- records ----------------------------------------------------------------------
def records(n, seed=1234, funcs=FUNCS + (NOBODY,), depth=6):
    """n recorded calls: pseudo-random functions, registers (di in 0..3), callers,
    clocks and stacks from a fixed seed."""
    rng = np.random.default_rng(seed + n)
    func = np.array([funcs[k] for k in rng.integers(0, len(funcs), n)], dtype=np.uint64)
    enter = rng.integers(0, 1 << 62, (n, 21), dtype=np.uint64)
    leave = rng.integers(0, 1 << 62, (n, 21), dtype=np.uint64)
    enter[:, DI] = rng.integers(0, 4, n, dtype=np.uint64)
    pid = (rng.integers(1, 5, n, dtype=np.uint64) << np.uint64(32)) | rng.integers(1, 9, n, dtype=np.uint64)
    clock = np.cumsum(rng.integers(1, 4, (n, 2), dtype=np.uint64).reshape(-1)).reshape(n, 2).astype(np.uint64)
    clock //= np.uint64(8)                              # repeated values: several calls per key
    depths = rng.integers(0, depth + 1, n, dtype=np.uint32)
    frames = rng.integers(1, 6, (n, depth), dtype=np.uint64) * np.uint64(0x1000)
    stacks = [list(int(x) for x in frames[i, :depths[i]]) for i in range(n)]
    return dict(func=func, enter=enter, leave=leave, pid=pid, clock=clock, depths=depths, frames=frames,
                stacks=stacks)


def hash_counts(m, keys):
    """{key: count} of a device HASH map of u64 -> u64 for the keys present."""
    out = {}
    for k in keys:
        v = m.lookup(int(k).to_bytes(8, "little"))
        if v is not None:
            out[int(k)] = int.from_bytes(v, "little")
    return out


# ---- the pairs' bytes in the oracle interpreter -------------------------------------
_HELPER = C.CFUNCTYPE(C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64)


def run_bytes(code, e):
    """Runs eBPF bytes once in the oracle interpreter (r1 = e.regs, r2 = 168)
    with the attachment's helpers answered from Env e.  Returns (rc, r0);
    e.regs holds what the program left there.  Map helpers are the oracle's:
    create an OracleMap at the fd the bytes name."""
    from oracle import pyoracle as po
    failed = []

    def retval(v):
        try:
            e.override(v)
        except Failed:
            failed.append(1)
        return 0
    stubs = {isa.BPF_FUNC_get_func_ip: lambda *a: e.func_ip, isa.BPF_FUNC_get_attach_cookie: lambda *a: e.cookie,
             isa.BPF_FUNC_get_current_pid_tgid: lambda *a: e.pid_tgid, isa.BPF_FUNC_ktime_get_ns: lambda *a: e.ktime,
             isa.BPF_FUNC_override_return: lambda a1, a2, *a: retval(a2),
             isa.BPF_FUNC_set_retval: lambda a1, *a: retval(a1)}
    vm = po.OracleVM()
    keep = []
    reg = po.lib().orc_vm_register
    reg.restype, reg.argtypes = C.c_int, [C.c_void_p, C.c_uint, C.c_char_p, _HELPER]
    for hid, fn in stubs.items():
        keep.append(_HELPER(fn))
        assert reg(vm.h, hid, b"stub%d" % hid, keep[-1]) == 0
    vm.load(code)
    mem = bytearray(np.ascontiguousarray(e.regs).tobytes())
    rc, r0 = vm.exec(mem)
    e.regs[:] = np.frombuffer(bytes(mem), dtype=np.uint64)
    return (-1 if failed else rc), r0
