"""The event-list uprobe replay (bpftime_amd_uprobe_dispatch_events) on the
device against the model (tests/_uprobe_events.py EventModel), bit-exact: maps,
out_state, out_rets, failed callbacks, the records untouched.

The traces hold nested and recursive calls, a call entered before the
recording began and calls that never return; tests/test_uprobe_events_model.py
shows that on every shape with n >= 64 a replay that ignored the list (every
record's entry, then its return) would file different histograms and a
different `seen` map.

Shapes: (records, at most this many threads) as tests/test_gpu_uprobe_threads.py
has them -- lane, wave and block boundaries, ragged walks.  Hash maps hold 2 *
threads + 8 entries for per-thread keys and 2 * n + 8 for per-call keys, so no
insert races for a last slot."""
import os
import threading

import numpy as np
import pytest

from bpftime_amd import isa
from bpftime_amd import vm as dev

import _stacktrace as sm
import _uprobe as um
import _uprobe_events as ue
import _uprobe_threads as ut

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (64, 64), (65, 3), (65, 65), (257, 64), (257, 65), (1031, 1), (1031, 3), (1031, 65), (1031, 130)]
F0, F1, F2 = um.FUNCS
HASH, ARRAY, KPROBE = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_ARRAY, 2
THREADS = dev.BATCH_SYNC | dev.DISPATCH_THREADS
shapes = pytest.mark.parametrize("n,threads", SHAPES)


def buf(a):
    return dev.DeviceBuffer.from_array(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


class Bench:
    """Device and model side by side: attach a (code, callable) pair to both."""

    def __init__(self):
        self.model, self.n = ue.EventModel(), 0

    def attach(self, pair, func, kind=dev.UPROBE, cookie=None):
        self.n += 1
        fd = dev.prog_create(pair[0], f"p{self.n}", KPROBE)
        assert self.model.attach(func, kind, pair[1], cookie) > 0
        return dev.uprobe_attach(fd, func, kind, cookie)


def run_both(b, r, events, flags=THREADS, pid=True, outs=False):
    """Dispatches the event list on the device and in the model; compares the
    failure count, the records and (outs) out_state / out_rets, which it
    returns with the failure count."""
    n = len(r["func"])
    events = np.asarray(events, dtype=np.uint32)
    st_h, rets_h = np.full(n, 6, np.uint32), np.full(n, -5, np.int64)
    kw = {}
    if outs:
        kw["out_state"], kw["out_rets"] = buf(st_h), buf(rets_h)
    enter, leave = buf(r["enter"]), buf(r["leave"])
    got = dev.uprobe_dispatch_events(buf(r["func"]), n, buf(events), len(events), enter=enter, leave=leave,
                                     pid_tgid=buf(r["pid"]) if pid else None, clock=buf(r["clock"]), flags=flags, **kw)
    st_m, rets_m = st_h.copy(), rets_h.copy()
    me = (os.getpid() << 32) | threading.get_native_id()
    want = b.model.dispatch_events(events, r["func"], r["enter"], r["leave"], pid_tgid=r["pid"] if pid else None,
                                   clock=r["clock"], out_state=st_m, out_rets=rets_m, default_pid=me)
    assert got == want
    assert (enter.download(np.uint64).reshape(n, 21) == r["enter"]).all()
    assert (leave.download(np.uint64).reshape(n, 21) == r["leave"]).all()
    if outs:
        assert (kw["out_state"].download(np.uint32) == st_m).all()
        assert (kw["out_rets"].download(np.int64) == rets_m).all()
    return want, st_m, rets_m


def u32_map(m, keys):
    """{key: u64} of a device HASH of u32 -> u64 for the keys present."""
    out = {}
    for k in keys:
        v = m.lookup(int(k).to_bytes(4, "little"))
        if v is not None:
            out[int(k)] = int.from_bytes(v, "little")
    return out


def hist_of(m):
    return [int(x) for x in np.frombuffer(m.lookup(b"\0\0\0\0"), dtype=np.uint32)]


def tids(r):
    me = threading.get_native_id()
    return sorted(set(int(p) & 0xFFFFFFFF for p in r["pid"]) | {me})


def funclat(b, threads, func=F0, **kw):
    """The funclatency pair on `func`: (starts map, hist map, starts dict, hist list)."""
    ms, mh = dev.Map(HASH, 4, 8, 2 * threads + 8), dev.Map(ARRAY, 4, 4 * ut.SLOTS, 1)
    starts, hist = {}, [0] * ut.SLOTS
    b.attach(ut.funclat_entry(ms.fd, starts), func)
    b.attach(ut.funclat_return(ms.fd, mh.fd, starts, hist, **kw), func, dev.URETPROBE)
    return ms, mh, starts, hist


def check_funclat(r, ms, mh, starts, hist):
    assert hist_of(mh) == hist
    assert u32_map(ms, tids(r)) == starts and ms.count() == len(starts)


@pytest.mark.parametrize("variant", ["plain", "delete"])
@shapes
def test_funclatency_on_a_recursive_function(fresh_runtime, n, threads, variant):   # (a)
    b, r = Bench(), ue.traces(n, threads)
    fl = funclat(b, threads, delete=variant == "delete")
    assert dev.uprobe_dispatch_plan(dev.DISPATCH_THREADS) == 1
    assert run_both(b, r, r["events"])[0] == 0
    check_funclat(r, *fl)


def depth_pair(b, threads, funcs=(F0, F1)):
    md, mb = dev.Map(HASH, 4, 8, 2 * threads + 8), dev.Map(ARRAY, 4, 4 * ue.SLOTS, 1)
    depth, by = {}, [0] * ue.SLOTS
    for f in funcs:
        b.attach(ue.depth_entry(md.fd, mb.fd, depth, by), f)
        b.attach(ue.depth_return(md.fd, depth), f, dev.URETPROBE)
    return md, mb, depth, by


@shapes
def test_call_depth_across_two_functions(fresh_runtime, n, threads):   # (b)
    b, r = Bench(), ue.traces(n, threads)
    md, mb, depth, by = depth_pair(b, threads)
    assert run_both(b, r, r["events"])[0] == 0
    assert hist_of(mb) == by
    assert u32_map(md, tids(r)) == depth and md.count() == len(depth)
    if n >= 64:
        assert sum(by[1:]) > 0                           # calls that began inside another probed call


@shapes
def test_order_inside_threads(fresh_runtime, n, threads):             # (c)
    b, r = Bench(), ue.traces(n, threads)
    mc, mo, msn = dev.Map(HASH, 4, 8, 2 * threads + 8), dev.Map(HASH, 8, 8, 2 * n + 8), dev.Map(HASH, 8, 8, 2 * n + 8)
    cnt, order, seen = {}, {}, {}
    b.attach(ut.seq_entry(mc.fd, mo.fd, cnt, order), F1)
    b.attach(ut.seq_return(mc.fd, msn.fd, cnt, seen), F1, dev.URETPROBE)
    assert run_both(b, r, r["events"])[0] == 0
    assert u32_map(mc, tids(r)) == cnt and mc.count() == len(cnt)
    assert um.hash_counts(mo, order.keys()) == order and mo.count() == len(order)
    assert um.hash_counts(msn, seen.keys()) == seen and msn.count() == len(seen)


@shapes
def test_replace_inside_a_probed_function(fresh_runtime, n, threads):  # (d)
    b, r = Bench(), ue.traces(n, threads)
    b.attach(um.replace_with_arg0_plus(9), F1, dev.UREPLACE)
    fl = funclat(b, threads)
    failed, st, rets = run_both(b, r, r["events"], outs=True)
    assert failed == 0
    check_funclat(r, *fl)
    entered = set(int(w) >> 1 for w in r["events"] if not int(w) & 1)
    inner = [i for i in range(n) if r["func"][i] == F1 and i in entered]
    assert sorted(np.flatnonzero(st != 6)) == inner and sorted(np.flatnonzero(rets != -5)) == inner
    assert all(st[i] == 7 and rets[i] == int(r["enter"][i, um.DI]) + 9 for i in inner)


def lockstep(alternate):
    """64 threads in one wave, every call of F0.  Not alternate: a call each,
    all entries and then all returns, so the wave is at one phase in both
    steps.  Alternate: the odd threads begin with the return of a call entered
    before the recording, so at every step neighbouring lanes are at different
    phases."""
    t = 64
    n = t + (t // 2 if alternate else 0)
    r = ut.records(n, 1)
    r["func"] = np.full(n, F0, dtype=np.uint64)
    owner = np.concatenate([np.arange(t), np.arange(1, t, 2)])[:n]
    r["pid"] = np.array([(ut.tgid_of(x) << 32) | ut.tid_of(x) for x in owner], dtype=np.uint64)
    steps = [[ue.event(x, 0) for x in range(t)], [ue.event(x, 1) for x in range(t)]]
    if alternate:
        early = {x: t + x // 2 for x in range(1, t, 2)}   # thread -> its return-only record
        steps = [[ue.event(early[x], 1) if x & 1 else ue.event(x, 0) for x in range(t)],
                 [ue.event(x, 0) if x & 1 else ue.event(x, 1) for x in range(t)],
                 [ue.event(x, 1) for x in range(1, t, 2)]]
    events = [w for s in steps for w in s]
    clock = np.zeros((n, 2), dtype=np.uint64)
    for k, w in enumerate(events):
        clock[w >> 1, w & 1] = 1000 + 3 * k * k
    r["clock"] = clock
    return r, events


@pytest.mark.parametrize("alternate", [False, True], ids=["one-phase", "two-phases"])
def test_a_wave_in_lockstep(fresh_runtime, alternate):                # (e)
    b = Bench()
    r, events = lockstep(alternate)
    fl = funclat(b, 64)
    md, mb, depth, by = depth_pair(b, 64, funcs=(F0,))
    assert run_both(b, r, events)[0] == 0
    check_funclat(r, *fl)
    assert hist_of(mb) == by and u32_map(md, tids(r)) == depth
    assert sum(fl[3]) == 64


@shapes
def test_flat_list_is_the_call_dispatch(fresh_runtime, n, threads):   # (f)
    r = ut.records(n, threads)
    got, okeys, skeys = [], None, None
    for flat in (True, False):
        b = Bench()
        ms, mh, starts, hist = funclat(b, threads, delete=True)
        mc, mo, msn = (dev.Map(HASH, 4, 8, 2 * threads + 8), dev.Map(HASH, 8, 8, 2 * n + 8),
                       dev.Map(HASH, 8, 8, 2 * n + 8))
        cnt, order, seen = {}, {}, {}
        b.attach(ut.seq_entry(mc.fd, mo.fd, cnt, order), F1)
        b.attach(ut.seq_return(mc.fd, msn.fd, cnt, seen), F1, dev.URETPROBE)
        b.attach(um.replace_with_arg0_plus(3), F2, dev.UREPLACE)
        if flat:                                         # the event dispatch, against the model too
            failed, st, rets = run_both(b, r, ue.flat_events(n), outs=True)
            okeys, skeys = sorted(order), sorted(seen)
        else:                                            # the call dispatch on maps of its own
            st, rets = buf(np.full(n, 6, np.uint32)), buf(np.full(n, -5, np.int64))
            failed = dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), leave=buf(r["leave"]),
                                         pid_tgid=buf(r["pid"]), clock=buf(r["clock"]), out_state=st, out_rets=rets,
                                         flags=THREADS)
            st, rets = st.download(np.uint32), rets.download(np.int64)
        snap = (u32_map(ms, tids(r)), ms.count(), hist_of(mh), u32_map(mc, tids(r)), mc.count(),
                um.hash_counts(mo, okeys), mo.count(), um.hash_counts(msn, skeys), msn.count())
        if flat:
            assert snap == (starts, len(starts), hist, cnt, len(cnt), order, len(order), seen, len(seen))
        got.append((failed, list(st), list(rets)) + snap)
        dev.reset_runtime()
        dev.set_ncpu(64)
    assert got[0] == got[1]


@pytest.mark.parametrize("n,threads", [(1, 1), (65, 3), (257, 65)])
def test_ordered_is_the_serial_run(fresh_runtime, n, threads):        # (g)
    b, r = Bench(), ue.traces(n, threads)
    fl = funclat(b, threads, plain=True)
    assert dev.uprobe_dispatch_plan(dev.DISPATCH_THREADS | dev.BATCH_ORDERED) == 1
    assert run_both(b, r, r["events"], flags=THREADS | dev.BATCH_ORDERED)[0] == 0
    check_funclat(r, *fl)


@pytest.mark.parametrize("n,threads", [(65, 3), (1031, 65)])
def test_without_callers_one_thread_owns_every_event(fresh_runtime, n, threads):   # (h)
    b, r = Bench(), ue.traces(n, threads)
    fl = funclat(b, threads)
    md, mb, depth, by = depth_pair(b, threads)
    assert run_both(b, r, r["events"], pid=False)[0] == 0
    check_funclat(r, *fl)
    assert hist_of(mb) == by and u32_map(md, tids(r)) == depth and len(depth) == 1


@pytest.mark.parametrize("flags", [THREADS, THREADS | dev.BATCH_ORDERED], ids=["grouped", "ordered"])
def test_refusals_run_nothing(fresh_runtime, flags):                  # (i)
    n, threads = 257, 65
    b, r = Bench(), ue.traces(n, threads)
    ms, mh, starts, hist = funclat(b, threads, plain=True)
    b.attach(um.replace_with_arg0_plus(1), F1, dev.UREPLACE)
    st, rets = buf(np.full(n, 6, np.uint32)), buf(np.full(n, -5, np.int64))

    def refused(events, match, pid=True):
        with pytest.raises(dev.EbpfError, match=match):
            dev.uprobe_dispatch_events(buf(r["func"]), n, buf(events), len(events), enter=buf(r["enter"]),
                                       leave=buf(r["leave"]), pid_tgid=buf(r["pid"]) if pid else None,
                                       clock=buf(r["clock"]), out_state=st, out_rets=rets, flags=flags)
        assert ms.count() == 0 and sum(hist_of(mh)) == 0
        assert (st.download(np.uint32) == 6).all() and (rets.download(np.int64) == -5).all()
    ev = r["events"].copy()
    ev[len(ev) // 2] = ue.event(n, 1)                    # record index == count
    refused(ev, r"1 of the %d events name a record index >= count \(%d\)" % (len(ev), n))
    refused(ev, "1 of the %d events" % len(ev), pid=False)
    ev[0] = ev[-1] = ue.event((1 << 31) - 1, 0)          # the largest index a word holds
    refused(ev, "3 of the %d events" % len(ev))
    # a program that reads the recorded stacks: refused as by the thread-ordered plan
    stm = dev.Map(isa.BPF_MAP_TYPE_STACK_TRACE, 4, 8 * 6, 64)
    dev.uprobe_attach(dev.prog_create(sm.stackid_prog(stm.fd, sm.USER_STACK), "stk", KPROBE), F2, dev.UPROBE)
    refused(r["events"], "'stk' calls bpf_get_stackid / bpf_get_stack")


def test_absent_records_and_a_repeated_event(fresh_runtime):          # (j)
    n, threads = 257, 65
    b, r = Bench(), ue.traces(n, threads)
    b.attach(um.replace_with_arg0_plus(4), F1, dev.UREPLACE)
    md, mb, depth, by = depth_pair(b, threads, funcs=(F0,))
    gone = set(range(0, n, 3))                           # a third of the records appear in no event
    events = [int(w) for w in r["events"] if int(w) >> 1 not in gone]
    failed, st, rets = run_both(b, r, events, outs=True)
    assert failed == 0 and hist_of(mb) == by and u32_map(md, tids(r)) == depth
    assert all(st[i] == 6 and rets[i] == -5 for i in gone)
    assert (st == 7).sum() == len([w for w in events if not w & 1 and r["func"][w >> 1] == F1]) > 0
    # the same event twice runs twice
    dev.reset_runtime()
    dev.set_ncpu(64)
    b = Bench()
    md, mb, depth, by = depth_pair(b, threads, funcs=(F0,))
    i = int(np.flatnonzero(r["func"] == F0)[0])
    events = [ue.event(i, 0), ue.event(i, 0), ue.event(i, 1), ue.event(i, 0)]
    assert run_both(b, r, events)[0] == 0
    assert hist_of(mb) == by and by[:3] == [1, 2, 0]
    assert u32_map(md, tids(r)) == depth == {int(r["pid"][i]) & 0xFFFFFFFF: 2}
