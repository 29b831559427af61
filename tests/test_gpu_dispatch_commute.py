"""The syscall dispatch planner on the device against orc_sys_dispatch
(csrc/syscall_dispatch.cpp plan_for / first_map_conflict, csrc/loader.cpp
map_effects, csrc/vm_seq.cpp seq_dispatch).

For every case of tests/_dispatch_cases.py: the plan the rule gives it is the
plan syscall_dispatch_plan() answers, and a dispatch with NO plan flag leaves
every return, every map entry and the failed count as the oracle's
record-by-record run does.  A planner that keeps program-major for a set that
does not commute fails here: tests/test_dispatch_cases_model.py shows on the
oracle alone that each order-sensitive case differs when a thread's calls run
in another order (S-load-add: a thread's calls must return 0, 1, 2, ...,
which 512 parallel lanes of one thread cannot).

Shapes: 4096 128-B records over 1 thread (one lane), 8 (512 same-thread
records side by side in program-major), 65 (one lane in a second wave) and
200 (a partial fourth wave); S-update and S-load-add also in struct-of-arrays
form; the conflicting cases in both thread-ordered tiers.

Also: tail-calling programs (program-major only: run, or refused by name
before any launch), per-program step limits in both plans, the uprobe
replay's share of the rule, and the plans of the bench workloads.
"""
import errno
import struct

import ctypes as C
import numpy as np
import pytest

from bpftime_amd import gen, isa, programs
from bpftime_amd.isa import Asm

import _dispatch_cases as dc
import _uprobe as um
import _uprobe_threads as ut
from _helpers import make_maps

pytestmark = pytest.mark.gpu

TRACEPOINT, KPROBE = 5, 2
HASH, ARRAY, PROG_ARRAY = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_ARRAY, isa.BPF_MAP_TYPE_PROG_ARRAY
I32 = lambda v: struct.pack("<i", v)  # noqa: E731
_RECS = {}


def recs_of(threads):
    if threads not in _RECS:
        _RECS[threads] = dc.records(threads)
        _RECS[threads].setflags(write=False)
    return _RECS[threads]


def _attach(dev, o, code, nr, enter):
    i = dev.syscall_attach(dev.prog_create(code, "p", TRACEPOINT), nr, enter)
    assert o.attach(code, nr, enter) > 0
    return i


def _setup(po, dev, case, recs):
    om, dm = make_maps([m[1:] for m in dc.MAPS], po, dev)
    names = [m[0] for m in dc.MAPS]
    om, dm = dict(zip(names, om)), dict(zip(names, dm))
    for name in case.prefill:
        for tid in dc.tids(recs):
            k, v = struct.pack("<I", tid), struct.pack("<Q", dc.prefill_value(name, int(tid)))
            assert om[name].update(k, v) == 0 and dm[name].update(k, v) == 0
    o = po.OracleSyscallDispatch()
    for code, nr, enter in case.build({n: m.fd for n, m in dm.items()}):
        _attach(dev, o, code, nr, enter)
    return o, om, dm


def _dispatch(dev, recs, soa=False, flags=None):
    """-> (failed, out_rets) of a dispatch with no plan flag (or `flags`)."""
    n = len(recs)
    flags = dev.BATCH_SYNC if flags is None else flags
    out = dev.DeviceBuffer(8 * n)
    if soa:
        e, x, c = (dev.DeviceBuffer.from_array(a) for a in gen.syscall_records_soa(recs))
        failed = dev.syscall_dispatch_soa(x, n, enter=e, clock=c, out=out, flags=flags)
    else:
        d = dev.DeviceBuffer.from_array(recs)
        failed = dev.syscall_dispatch(d, n, record_size=dev.SYSCALL_RECORD_TIMED, out=out, flags=flags)
    return failed, out.download(np.int64)


def _parity(po, dev, case, threads, soa=False):
    recs = recs_of(threads)
    o, om, dm = _setup(po, dev, case, recs)
    assert dev.syscall_dispatch_plan() == case.plan
    failed, got = _dispatch(dev, recs, soa)
    want = o.dispatch(recs)
    assert failed == o.failed() == 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    for name in om:
        assert dm[name].hash_items() == om[name].items(), name
    return want, om


@pytest.mark.parametrize("threads", dc.THREADS)
@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.id)
def test_auto_plan_matches_oracle(fresh_oracle, fresh_runtime, case, threads):
    want, om = _parity(fresh_oracle, fresh_runtime, case, threads)
    if case.id == "S-load-add":
        # the reference's own answer: a thread's calls see its counter's
        # start, + 1, + 2, ...
        recs = recs_of(threads)
        w = recs.view(np.int64).reshape(len(recs), 16)
        live = ~np.isin(w[:, 1], [60, 231])
        for p in np.unique(w[:, 11]):
            at = np.flatnonzero((w[:, 11] == p) & live)
            assert (want[at] == dc.prefill_value("a", int(p) & 0xFFFFFFFF) + np.arange(len(at))).all()


@pytest.mark.parametrize("case", ["S-update", "S-load-add"])
def test_struct_of_arrays_records(fresh_oracle, fresh_runtime, case):
    _parity(fresh_oracle, fresh_runtime, dc.BY_ID[case], 65, soa=True)


@pytest.mark.parametrize("tier", ["asm", "cpp"])
@pytest.mark.parametrize("case", [c for c in dc.CASES if c.plan == 1], ids=lambda c: c.id)
def test_conflicting_cases_both_tiers(fresh_oracle, fresh_runtime, monkeypatch, case, tier):
    monkeypatch.setenv("BPFTIME_AMD_SEQ_ASM", "1" if tier == "asm" else "0")
    _parity(fresh_oracle, fresh_runtime, case, 65)
    # every case keeps its stack in the LDS stacks and so runs in the tier
    # asked for, but S-toggle: the loader does not bound its stack (private
    # stacks), and a forced asm tier falls back to the C++ tier for it
    asm = tier == "asm" and case.id != "S-toggle"
    assert fresh_runtime.last_seq_tier() == (1 if asm else 0)


# ---- the bench workloads keep their plans (bench_workloads.py's options) ----

def test_bench_workload_plans(fresh_runtime):
    dev = fresh_runtime
    att = lambda code, nr, enter: dev.syscall_attach(dev.prog_create(code, "p", TRACEPOINT), nr, enter)  # noqa: E731
    # syscount: syscount_exit alone, default .rodata
    data, ro = dev.Map(HASH, 4, 32, 8192), dev.Map(ARRAY, 4, programs.SYSCOUNT_RODATA, 1)
    ro.update(b"\0" * 4, programs.syscount_rodata())
    i = att(programs.syscount_exit(data.fd, ro.fd), -1, False)
    assert dev.syscall_dispatch_plan() == 0
    dev.syscall_detach(i)
    # syscall-agg: syscall_agg alone
    counts = dev.Map(HASH, 4, 32, 1024)
    i = att(programs.syscall_agg(counts.fd), -1, True)
    assert dev.syscall_dispatch_plan() == 0
    dev.syscall_detach(i)
    # syscount-latency: the pair with measure_latency
    start = dev.Map(HASH, 4, 8, 10240)
    ro.update(b"\0" * 4, programs.syscount_rodata(measure_latency=True))
    att(programs.syscount_enter(start.fd, ro.fd), -1, True)
    att(programs.syscount_exit(data.fd, ro.fd, start.fd), -1, False)
    assert dev.syscall_dispatch_plan() == 1


# ---- bpf_tail_call ----------------------------------------------------------

PA_FD, T0_FD, T1_FD = 700, 900, 901


def _tail_setup(po, dev):
    """A sys_enter caller tail_call(ctx, pa, 0) whose target adds to cnt[1];
    -> (caller code, (ocnt, dcnt), (oracle prog array, device prog array))."""
    (ocnt,), (dcnt,) = make_maps([(ARRAY, 4, 8, 4)], po, dev)
    pa_o = po.OracleMap(PROG_ARRAY, 4, 4, 4, fd=PA_FD)
    pa_d = dev.Map(PROG_ARRAY, 4, 4, 4, fd=PA_FD)
    code = programs.tail_target_count(dcnt.fd)
    assert po.prog_create(T0_FD, code) == T0_FD
    assert dev.prog_create(code, "target", TRACEPOINT, fd=T0_FD) == T0_FD
    assert pa_o.update(I32(0), I32(T0_FD)) == 0 and pa_d.update(I32(0), I32(T0_FD)) == 0
    caller = Asm().ld_map_fd(2, PA_FD).mov64(3, 0).call(isa.BPF_FUNC_tail_call).mov64(0, 0).exit().assemble()
    return caller, (ocnt, dcnt), (pa_o, pa_d)


def _tail_check(po, dev, o, maps, flags=None):
    recs = recs_of(65)
    failed, got = _dispatch(dev, recs, flags=flags)
    want = o.dispatch(recs)
    assert failed == o.failed() == 0
    assert (got == want).all()
    for om, dm in maps:
        for k in range(om.max_entries):
            assert dm.lookup(I32(k)) == om.lookup(I32(k))
    return want


def test_tail_caller_alone(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    caller, cnt, _ = _tail_setup(po, dev)
    o = po.OracleSyscallDispatch()
    _attach(dev, o, caller, -1, True)
    assert dev.syscall_dispatch_plan() == 0
    _tail_check(po, dev, o, [cnt])
    live = ~np.isin(recs_of(65).view(np.int64).reshape(dc.N_RECORDS, 16)[:, 1], [60, 231])
    assert struct.unpack("<Q", cnt[1].lookup(I32(1)))[0] == int(live.sum())  # the target ran once per call


def test_tail_caller_alone_ordered(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    caller, cnt, _ = _tail_setup(po, dev)
    o = po.OracleSyscallDispatch()
    _attach(dev, o, caller, -1, True)
    assert dev.syscall_dispatch_plan(dev.BATCH_ORDERED) == 0  # one ORDERED batch: the serial run
    _tail_check(po, dev, o, [cnt], flags=dev.BATCH_SYNC | dev.BATCH_ORDERED)
    assert struct.unpack("<Q", cnt[1].lookup(I32(1)))[0] > 0


def test_tail_caller_beside_map_free_override(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    caller, cnt, _ = _tail_setup(po, dev)
    o = po.OracleSyscallDispatch()
    _attach(dev, o, caller, -1, True)
    _attach(dev, o, programs.inject_enter(3, -1), -1, True)
    assert dev.syscall_dispatch_plan() == 0
    want = _tail_check(po, dev, o, [cnt])
    assert (want == -1).sum() > dc.N_RECORDS // 8


def _expect_tail_refusal(dev, call):
    with pytest.raises(dev.EbpfError, match="bpf_tail_call") as e:
        call()
    assert C.get_errno() == errno.EINVAL
    return e


def test_tail_caller_beside_conflicting_writer(fresh_oracle, fresh_runtime):
    """The target adds to cnt[1]; a second program stores into cnt: the set
    needs the thread-ordered plan, which runs no tail calls -- refused by name
    at plan time, nothing launched, the maps as they were."""
    po, dev = fresh_oracle, fresh_runtime
    caller, (ocnt, dcnt), _ = _tail_setup(po, dev)
    o = po.OracleSyscallDispatch()
    _attach(dev, o, caller, -1, True)
    writer = (Asm().ldx(8, 3, 1, dc.ARG0).ld_map_value(2, dcnt.fd, 8).stx(8, 2, 0, "r3").mov64(0, 0).exit().assemble())
    _attach(dev, o, writer, -1, True)
    recs = recs_of(65)
    _expect_tail_refusal(dev, dev.syscall_dispatch_plan)
    _expect_tail_refusal(dev, lambda: _dispatch(dev, recs))
    _expect_tail_refusal(dev, lambda: _dispatch(dev, recs, flags=dev.BATCH_SYNC | dev.DISPATCH_THREADS))
    _expect_tail_refusal(dev, lambda: _dispatch(dev, recs, flags=dev.BATCH_SYNC | dev.BATCH_ORDERED))
    for k in range(4):
        assert dcnt.lookup(I32(k)) == b"\0" * 8


def test_tail_effects_are_the_targets(fresh_oracle, fresh_runtime):
    """The caller's effects are its targets': beside a reader of the map a
    target adds to, the set is refused; once the slot names a target that
    touches no map, the same pair runs program-major and matches."""
    po, dev = fresh_oracle, fresh_runtime
    caller, (ocnt, dcnt), (pa_o, pa_d) = _tail_setup(po, dev)
    o = po.OracleSyscallDispatch()
    _attach(dev, o, caller, -1, True)
    reader = (Asm().mov64(6, "r1").ld_map_value(2, dcnt.fd, 8).ldx(8, 2, 2, 0).mov64(1, "r6")
              .call(isa.BPF_FUNC_override_return).mov64(0, 0).exit().assemble())
    _attach(dev, o, reader, -1, True)
    _expect_tail_refusal(dev, dev.syscall_dispatch_plan)
    idle = programs.tail_ref_kat_target()
    assert po.prog_create(T1_FD, idle) == T1_FD and dev.prog_create(idle, "idle", TRACEPOINT, fd=T1_FD) == T1_FD
    assert pa_o.update(I32(0), I32(T1_FD)) == 0 and pa_d.update(I32(0), I32(T1_FD)) == 0
    assert dev.syscall_dispatch_plan() == 0
    _tail_check(po, dev, o, [(ocnt, dcnt)])


# ---- per-program step limits ------------------------------------------------

@pytest.mark.parametrize("tier", ["asm", "cpp"])
def test_step_limit_is_per_program(fresh_oracle, fresh_runtime, monkeypatch, tier):
    """A (limit 1000) and B (limit 100) run the same ~330-instruction loop
    (109 taken jumps, what the asm tier counts) before their add: B fails on every record it runs on and leaves no map
    effect, A never fails, in both plans alike."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.setenv("BPFTIME_AMD_SEQ_ASM", "1" if tier == "asm" else "0")
    recs = recs_of(65)
    (oa, ob), (da, db) = make_maps([(HASH, 4, 8, 1024)] * 2, po, dev)
    for tid in dc.tids(recs):
        for m in (oa, ob, da, db):
            assert m.update(struct.pack("<I", tid), b"\0" * 8) == 0
    o = po.OracleSyscallDispatch()  # (the oracle has no limits: it runs A alone)
    monkeypatch.setenv("BPFTIME_AMD_STEP_LIMIT", "1000")
    dev.syscall_attach(dev.prog_create(dc.loop_then_add(da.fd), "A", TRACEPOINT), -1, True)
    assert o.attach(dc.loop_then_add(da.fd), -1, True) > 0
    monkeypatch.setenv("BPFTIME_AMD_STEP_LIMIT", "100")
    dev.syscall_attach(dev.prog_create(dc.loop_then_add(db.fd), "B", TRACEPOINT), 1, True)
    monkeypatch.delenv("BPFTIME_AMD_STEP_LIMIT")
    assert dev.syscall_dispatch_plan() == 0  # counter adds on disjoint maps
    w = recs.view(np.int64).reshape(len(recs), 16)
    b_records = int((w[:, 1] == 1).sum())
    assert b_records > 1000
    want = o.dispatch(recs)
    zero = {k: b"\0" * 8 for k in ob.items()}
    results = []
    for plan in (dev.DISPATCH_PROGRAMS, dev.DISPATCH_THREADS):
        for tid in dc.tids(recs):
            assert da.update(struct.pack("<I", tid), b"\0" * 8) == 0
        failed, got = _dispatch(dev, recs, flags=dev.BATCH_SYNC | plan)
        assert failed == b_records
        assert (got == want).all()
        assert da.hash_items() == oa.items()     # A ran to its end on every call
        assert db.hash_items() == zero           # B never reached its add
        results.append((failed, got.tobytes(), da.hash_items()))
    assert results[0] == results[1]


# ---- the uprobe replay shares the rule --------------------------------------

F0 = um.FUNCS[0]


def _ubuf(dev, a):
    return dev.DeviceBuffer.from_array(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def test_uprobe_self_conflict_is_refused_by_name(fresh_runtime):
    dev = fresh_runtime
    n, threads = 1031, 65
    r = ut.records(n, threads)
    ms, starts = dev.Map(HASH, 4, 8, 2 * threads + 8), {}
    code, py = ut.funclat_entry(ms.fd, starts)       # start[tid] = bpf_ktime_get_ns(): the S-update shape
    model = um.Model()
    fd = dev.prog_create(code, "entry", KPROBE)
    i = dev.uprobe_attach(fd, F0)
    assert model.attach(F0, um.UPROBE, py) > 0
    kw = lambda: dict(enter=_ubuf(dev, r["enter"]), leave=_ubuf(dev, r["leave"]), pid_tgid=_ubuf(dev, r["pid"]),  # noqa: E731
                      clock=_ubuf(dev, r["clock"]))
    with pytest.raises(dev.EbpfError, match=rf"program 'entry' \(prog fd {fd}, attachment {i}\) may not commute with "
                                            rf"itself on map fd {ms.fd}"):
        dev.uprobe_dispatch(_ubuf(dev, r["func"]), n, **kw())
    assert ms.count() == 0                            # refused before any launch
    got = dev.uprobe_dispatch(_ubuf(dev, r["func"]), n, flags=dev.BATCH_SYNC | dev.DISPATCH_THREADS, **kw())
    want = model.dispatch(r["func"], r["enter"], r["leave"], pid_tgid=r["pid"], clock=r["clock"])
    assert got == want == 0
    tids = sorted(set(int(p) & 0xFFFFFFFF for p in r["pid"]))
    have = {t: int.from_bytes(ms.lookup(struct.pack("<I", t)), "little") for t in tids if ms.lookup(struct.pack("<I", t))}
    assert have == starts and ms.count() == len(starts) > 0


def test_uprobe_init_add_is_still_accepted(fresh_runtime):
    dev = fresh_runtime
    n, threads = 1031, 65
    r = ut.records(n, threads)
    mc = dev.Map(HASH, 4, 8, 2 * threads + 8)
    fd = dev.prog_create(dc.s_init_add(mc.fd), "count", KPROBE)   # key tid; += (pt_regs word 2 & 0xff) + 1
    dev.uprobe_attach(fd, F0)
    assert dev.uprobe_dispatch_plan() == 0
    got = dev.uprobe_dispatch(_ubuf(dev, r["func"]), n, enter=_ubuf(dev, r["enter"]), leave=_ubuf(dev, r["leave"]),
                              pid_tgid=_ubuf(dev, r["pid"]), clock=_ubuf(dev, r["clock"]))
    assert got == 0
    want = {}
    for k in np.flatnonzero(r["func"] == F0):
        t = int(r["pid"][k]) & 0xFFFFFFFF
        want[t] = want.get(t, 0) + (int(r["enter"][k][dc.ARG0 // 8]) & 0xFF) + 1
    have = {struct.unpack("<I", k)[0]: struct.unpack("<Q", v)[0] for k, v in mc.hash_items().items()}
    assert have == want and want
