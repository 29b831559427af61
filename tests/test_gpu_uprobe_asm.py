"""The thread-ordered uprobe replay's two execution tiers against each other
and against the model (tests/_uprobe.py Model, tests/_uprobe_events.py
EventModel), bit-exact.

Every case dispatches three times on fresh maps -- the tier left to the
library, BPFTIME_AMD_SEQ_ASM=1, BPFTIME_AMD_SEQ_ASM=0 -- asserts
last_seq_tier() after each, and holds every map entry, out_state, out_rets and
the failed callbacks of each run against the model's, hence against each
other's.

A block of the replay kernel is one wave, so the shapes are 1, 63, 64, 65 and
130 recorded threads of 1-5 calls each: a lone lane, a wave short of a lane, a
full wave, a wave and a lane, three blocks with a ragged last one; and, for
funclatency's pair beside tagging probes, 4,096, 65,536 and 65,537 threads:
many waves, and the automatic cut-off (ua.ASM_THREADS) from both sides.  Hash maps
hold at least twice their distinct keys and the counting programs insert 0,
look up and add (programs._count_key_r0), so no insert races for a last
slot."""
import os
import threading

import numpy as np
import pytest

from bpftime_amd import isa
from bpftime_amd import vm as dev

import _uprobe as um
import _uprobe_asm as ua
import _uprobe_events as ue
import _uprobe_threads as ut

pytestmark = pytest.mark.gpu
F0, F1, F2, F3, F4 = ua.FUNCS
HASH, ARRAY, KPROBE = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_ARRAY, 2
THREADS = dev.BATCH_SYNC | dev.DISPATCH_THREADS
ORDERED = THREADS | dev.BATCH_ORDERED
T_ALL = [1, 63, 64, 65, 130]
MODES = (None, "1", "0")                                 # BPFTIME_AMD_SEQ_ASM per run


def buf(a):
    return dev.DeviceBuffer.from_array(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


class Bench:
    """Device and model side by side: attach a (code, callable) pair to both."""

    def __init__(self, bulk=False):
        """bulk: snapshot() reads a hash map back whole (Map.hash_items), not
        key by key: for maps of many thousand entries."""
        self.model, self.n, self.snaps, self.bulk = ue.EventModel(), 0, [], bulk

    def attach(self, pair, func, kind=dev.UPROBE, cookie=None):
        self.n += 1
        fd = dev.prog_create(pair[0], f"p{self.n}", KPROBE)
        assert self.model.attach(func, kind, pair[1], cookie) > 0
        return dev.uprobe_attach(fd, func, kind, cookie)

    # a device map beside the model's container: snapshot() holds one against the other
    def _whole(self, m, d):
        ints = lambda kv: {int.from_bytes(k, "little"): int.from_bytes(v, "little") for k, v in kv.items()}  # noqa: E731
        self.snaps.append(lambda: (ints(m.hash_items()), m.count(), d, len(d)))
        return m, d

    def u32_hash(self, entries, keys):
        m, d = dev.Map(HASH, 4, 8, entries), {}
        if self.bulk:
            return self._whole(m, d)
        self.snaps.append(lambda: ({k: int.from_bytes(v, "little") for k in keys
                                    if (v := m.lookup(int(k).to_bytes(4, "little"))) is not None}, m.count(),
                                   d, len(d)))
        return m, d

    def u64_hash(self, entries):
        m, d = dev.Map(HASH, 8, 8, entries), {}
        if self.bulk:
            return self._whole(m, d)
        self.snaps.append(lambda: (um.hash_counts(m, d.keys()), m.count(), d, len(d)))
        return m, d

    def hist(self, slots):
        m, h = dev.Map(ARRAY, 4, 4 * slots, 1), [0] * slots
        self.snaps.append(lambda: ([int(x) for x in np.frombuffer(m.lookup(b"\0\0\0\0"), dtype=np.uint32)], None,
                                   h, None))
        return m, h

    def snapshot(self):
        """Every map's entries and entry count, checked against the model's
        containers; returned for the comparison between the runs."""
        out = []
        for s in self.snaps:
            got, got_n, want, want_n = s()
            assert got == want and got_n == want_n
            out.append((got, got_n))
        return out


def me():
    return (os.getpid() << 32) | threading.get_native_id()


def tids(r):
    return sorted(set(int(p) & 0xFFFFFFFF for p in r["pid"]) | {threading.get_native_id()})


def dispatch(b, r, events=None, flags=THREADS, pid=True, clock=True):
    """One dispatch (the call dispatch, or the event list) on the device and in
    the model: (failed, out_state, out_rets), each checked against the model's."""
    n = len(r["func"])
    st_h, rets_h = np.full(n, 6, np.uint32), np.full(n, -5, np.int64)
    st, rets = buf(st_h), buf(rets_h)
    kw = dict(enter=buf(r["enter"]), leave=buf(r["leave"]), pid_tgid=buf(r["pid"]) if pid else None,
              clock=buf(r["clock"]) if clock else None, out_state=st, out_rets=rets, flags=flags)
    st_m, rets_m = st_h.copy(), rets_h.copy()
    mk = dict(pid_tgid=r["pid"] if pid else None, clock=r["clock"] if clock else None, out_state=st_m,
              out_rets=rets_m, default_pid=me())
    if events is None:
        got = dev.uprobe_dispatch(buf(r["func"]), n, **kw)
        want = b.model.dispatch(r["func"], r["enter"], r["leave"], **mk)
    else:
        events = np.asarray(events, dtype=np.uint32)
        got = dev.uprobe_dispatch_events(buf(r["func"]), n, buf(events), len(events), **kw)
        want = b.model.dispatch_events(events, r["func"], r["enter"], r["leave"], **mk)
    st, rets = st.download(np.uint32), rets.download(np.int64)
    assert got == want and (st == st_m).all() and (rets == rets_m).all()
    return got, list(st), list(rets)


def three_ways(monkeypatch, setup, run, tiers, bulk=False):
    """setup(b) attaches to a fresh Bench on a fresh runtime; run(b) dispatches
    and returns what to compare; once per mode, the tier asserted after each."""
    seen = []
    for mode, tier in zip(MODES, tiers):
        dev.reset_runtime()
        dev.set_ncpu(64)
        if mode is None:
            monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
        else:
            monkeypatch.setenv("BPFTIME_AMD_SEQ_ASM", mode)
        b = Bench(bulk)
        setup(b)
        got = run(b)
        assert dev.last_seq_tier() == tier, f"BPFTIME_AMD_SEQ_ASM={mode}"
        seen.append((got, b.snapshot()))
    assert seen[0] == seen[1] == seen[2]
    return seen[0][0]


def funclat(b, r, func, **kw):
    (ms, starts), (mh, hist) = b.u32_hash(2 * len(tids(r)) + 8, tids(r)), b.hist(ut.SLOTS)
    b.attach(ut.funclat_entry(ms.fd, starts), func)
    b.attach(ut.funclat_return(ms.fd, mh.fd, starts, hist, **kw), func, dev.URETPROBE)
    return hist


@pytest.mark.parametrize("tag", ["di", "cookie"])
@pytest.mark.parametrize("events", [False, True], ids=["calls", "flat-events"])
@pytest.mark.parametrize("threads", T_ALL)
def test_per_thread_state_and_mixed_program_masks(fresh_runtime, monkeypatch, threads, events, tag):
    """funclatency's pair on F1 beside tagging uprobes on F2: the lanes of a
    wave need different program masks.  tag "di": the tags count
    PT_REGS_PARM1, and the map helpers leave the asm loop for the helper path.
    tag "cookie": they count bpf_get_attach_cookie / bpf_get_func_ip (174 /
    173) -- the loader marks a program that calls either for the scratch-stack
    kernels (loader.cpp task_trace_helper), so by the tier rule the whole
    dispatch stays in the C++ tier, BPFTIME_AMD_SEQ_ASM=1 included."""
    r = ua.ragged(threads)
    hists = []

    def setup(b):
        hists.append(funclat(b, r, F1))
        # (a uretprobe's PT_REGS_PARM1 is a random word of the return registers: a key per call)
        (mc, cookies), (mi, ips) = b.u64_hash(2 * len(r["func"]) + 16), b.u64_hash(16)
        if tag == "di":
            b.attach(ut.di_count(mc.fd, cookies), F2)
            b.attach(ut.di_count(mi.fd, ips), F2)
            b.attach(ut.di_count(mc.fd, cookies), F1, dev.URETPROBE)
        else:
            b.attach(um.cookie_tag(mc.fd, cookies), F2, cookie=0xC00C1E)
            b.attach(um.func_ip_count(mi.fd, ips), F2)
            b.attach(um.cookie_tag(mc.fd, cookies), F1, dev.URETPROBE, cookie=7)
    ev = ue.flat_events(len(r["func"])) if events else None
    tiers = [ua.auto_tier(threads), 1, 0] if tag == "di" else [0, 0, 0]
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r, ev), tiers)
    assert failed == 0 and sum(hists[0]) == int((r["func"] == F1).sum())


# Many waves, and the automatic cut-off from both sides: 4,096 threads of 1-5
# calls, then ua.ASM_THREADS (the last count the library puts in the asm tier)
# and ua.ASM_THREADS + 1 (the first it puts in the C++ tier; the last one-wave
# block holds one lane) of 1-2 calls each
MANY = ua.MANY_WAVES
_many = {}


def many_records(threads, calls):
    """ua.ragged for the many-wave cases, built once per shape (read-only)."""
    if threads not in _many:
        _many[threads] = ua.ragged(threads, calls=calls)
        assert len(np.unique(_many[threads]["pid"])) == threads
    return _many[threads]


@pytest.mark.parametrize("events", [False, True], ids=["calls", "flat-events"])
@pytest.mark.parametrize("threads,calls", MANY, ids=[str(t) for t, _ in MANY])
def test_many_waves_and_the_cut_off_from_both_sides(fresh_runtime, monkeypatch, threads, calls, events):
    """The "di" arm of test_per_thread_state_and_mixed_program_masks at 4,096,
    65,536 and 65,537 threads: funclatency's pair on F1 beside di_count tags
    on F2, by the call dispatch and by the flat event list, three ways.  Every
    wave inserts into starts[tid] at once; past the cut-off the forced asm
    tier is the contended regime.  The maps are read back whole."""
    r = many_records(threads, calls)
    hists = []

    def setup(b):
        hists.append(funclat(b, r, F1))
        (mc, cookies), (mi, ips) = b.u64_hash(2 * len(r["func"]) + 16), b.u64_hash(16)
        b.attach(ut.di_count(mc.fd, cookies), F2)
        b.attach(ut.di_count(mi.fd, ips), F2)
        b.attach(ut.di_count(mc.fd, cookies), F1, dev.URETPROBE)
    ev = ue.flat_events(len(r["func"])) if events else None
    tiers = [ua.auto_tier(threads), 1, 0]
    assert tiers[0] == (1 if threads <= 65536 else 0)
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r, ev), tiers, bulk=True)
    assert failed == 0 and sum(hists[0]) == int((r["func"] == F1).sum()) > threads // 8


def test_nested_calls_over_many_waves(fresh_runtime, monkeypatch):
    """test_mixed_phase_waves' nested event lists (entry / inner entry / inner
    return / return, recursion, up to four deep) at 4,096 threads against
    EventModel: thread 0 walks about half the events, the upper half of the
    threads one call each."""
    threads = 4096
    r = ue.traces(3 * threads, threads, max_depth=4)
    assert len(set(r["owner"])) == threads == len(np.unique(r["pid"])) and 2 <= ue.depth_profile(r) <= 4
    bys = []

    def setup(b):
        funclat(b, r, F1, delete=True)
        (md, depth), (mb, by) = b.u32_hash(2 * threads + 8, tids(r)), b.hist(ue.SLOTS)
        for f in (F0, F1):
            b.attach(ue.depth_entry(md.fd, mb.fd, depth, by), f)
            b.attach(ue.depth_return(md.fd, depth), f, dev.URETPROBE)
        bys.append(by)
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r, r["events"]), [1, 1, 0], bulk=True)
    assert failed == 0 and sum(bys[0][1:]) > 0           # calls that began inside another probed call


@pytest.mark.parametrize("threads", [64, 65, 130])
def test_mixed_phase_waves(fresh_runtime, monkeypatch, threads):
    """Nested event lists, chains up to four deep with recursion: at almost
    every step of the walk some lanes of a wave are at an entry and others at
    a return.  funclatency on F1, the call-depth pair on F0 and F1."""
    r = ue.traces(3 * threads, threads, max_depth=4)
    assert len(set(r["owner"])) == threads and 2 <= ue.depth_profile(r) <= 4
    bys = []

    def setup(b):
        funclat(b, r, F1, delete=True)
        (md, depth), (mb, by) = b.u32_hash(2 * threads + 8, tids(r)), b.hist(ue.SLOTS)
        for f in (F0, F1):
            b.attach(ue.depth_entry(md.fd, mb.fd, depth, by), f)
            b.attach(ue.depth_return(md.fd, depth), f, dev.URETPROBE)
        bys.append(by)
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r, r["events"]),
                              [ua.auto_tier(threads), 1, 0])
    assert failed == 0 and sum(bys[0][1:]) > 0           # calls that began inside another probed call


def test_mixed_phase_list_on_one_ordered_lane(fresh_runtime, monkeypatch):
    """THREADS | ORDERED: one lane walks the whole 65-thread list in list order
    (the `plain` histogram's load / add / store is exact there).  One thread:
    the library's own choice is the asm tier."""
    r = ue.traces(3 * 65, 65, max_depth=4)

    def setup(b):
        funclat(b, r, F1, plain=True)
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r, r["events"], flags=ORDERED), [1, 1, 0])
    assert failed == 0


@pytest.mark.parametrize("threads", T_ALL)
def test_override_replace_and_a_failing_plain_probe(fresh_runtime, monkeypatch, threads):
    """58 from an override on F3 when PT_REGS_PARM1 == 1, a replace on F4, and
    a plain uprobe on F2 that calls 58 when PT_REGS_PARM1 == 2: those units
    fail.  (None calls 173 / 174, which would keep the dispatch in the C++ tier.)"""
    r = ua.ragged(threads)
    counts = []

    def setup(b):
        b.attach(um.override_if_arg0(77, 1), F3, dev.UPROBE_OVERRIDE)
        b.attach(ua.replace_di_plus(9), F4, dev.UREPLACE)
        b.attach(um.override_if_arg0(-3, 2), F2)
        mc, c = b.u64_hash(16)
        b.attach(ut.di_count(mc.fd, c), F2)              # runs after the failing one, in every unit
        counts.append(c)
    failed, st, rets = three_ways(monkeypatch, setup, lambda b: dispatch(b, r), [ua.auto_tier(threads), 1, 0])
    f, di = r["func"], r["enter"][:, um.DI]
    assert failed == int(((f == F2) & (di == 2)).sum())
    assert sum(counts[0].values()) == int((f == F2).sum())
    for i in range(len(f)):
        want = (7, 77) if f[i] == F3 and di[i] == 1 else (7, int(di[i]) + 9) if f[i] == F4 else (6, -5)
        assert (st[i], rets[i]) == want
    if threads >= 63:
        assert failed > 0 and (f == F3).any() and (f == F4).any()


@pytest.mark.parametrize("threads", [1, 65])
def test_step_limit(fresh_runtime, monkeypatch, threads):
    """A limit of 200 steps: F1's callback loops 300 taken jumps and fails in
    every unit before it counts (FAST_STEPS in the asm tier), F0's loops 20 and
    counts.  The C++ loops count instructions and the asm tier taken jumps, so
    both callbacks stay far from the limit by either count: F0's runs about 70
    instructions, F1's 600."""
    monkeypatch.setenv("BPFTIME_AMD_STEP_LIMIT", "200")
    r = ua.ragged(threads)
    counts = []

    def setup(b):
        (m0, c0), (m1, c1) = b.u64_hash(16), b.u64_hash(16)
        b.attach(ua.spin_then_count(20, m0.fd, c0), F0)
        fd = dev.prog_create(ua.spin_then_count(300, m1.fd, c1)[0], "spin", KPROBE)
        assert b.model.attach(F1, dev.UPROBE, ua.failing) > 0
        dev.uprobe_attach(fd, F1, dev.UPROBE)
        counts.append((c0, c1))
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r), [ua.auto_tier(threads), 1, 0])
    f = r["func"]
    assert failed == int((f == F1).sum()) and (threads == 1 or failed > 0)
    assert sum(counts[0][0].values()) == int((f == F0).sum()) and not counts[0][1]


@pytest.mark.parametrize("threads", [1, 65])
def test_a_deep_stack_keeps_the_dispatch_in_the_cpp_tier(fresh_runtime, monkeypatch, threads):
    """One attached program with a 128-B stack: tier 0 under the library's own
    choice and under BPFTIME_AMD_SEQ_ASM=1, the same results."""
    r = ua.ragged(threads)

    def setup(b):
        funclat(b, r, F1)
        mc, c = b.u64_hash(16)
        b.attach(ua.deep_stack_count(mc.fd, c), F0)
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r), [0, 0, 0])
    assert failed == 0


@pytest.mark.parametrize("threads", [65, 130])
def test_caller_and_clock_from_the_records(fresh_runtime, monkeypatch, threads):
    """With pid_tgid and clock arrays, 14 and 5 return the recorded values: in
    the asm tier the two words beside the lane's ctx copy (CALL_REC)."""
    r = ua.ragged(threads)
    n = len(r["func"])

    def setup(b):
        (mp, pids), (mk, clocks) = b.u64_hash(2 * threads + 8), b.u64_hash(4 * n + 8)
        b.attach(um.count_by_helper(isa.BPF_FUNC_get_current_pid_tgid, mp.fd, pids), F0)
        b.attach(um.count_by_helper(isa.BPF_FUNC_ktime_get_ns, mk.fd, clocks), F0)
        b.attach(um.count_by_helper(isa.BPF_FUNC_ktime_get_ns, mk.fd, clocks), F0, dev.URETPROBE)
        (mc, cnt), (ma, at) = b.u32_hash(2 * threads + 8, tids(r)), b.u64_hash(2 * n + 8)
        b.attach(ua.clock_seq(mc.fd, ma.fd, cnt, at), F1, dev.URETPROBE)
    failed, _, _ = three_ways(monkeypatch, setup, lambda b: dispatch(b, r), [ua.auto_tier(threads), 1, 0])
    assert failed == 0


def test_caller_and_clock_without_arrays(fresh_runtime, monkeypatch):
    """Without the arrays one thread owns every call: 14 returns the
    dispatching thread's pid_tgid in both tiers; the device clock is non-zero
    and never runs backwards along the thread's calls."""
    r = ua.ragged(65)
    calls = int((r["func"] == F1).sum())
    for mode, tier in zip(MODES, (1, 1, 0)):
        dev.reset_runtime()
        dev.set_ncpu(64)
        if mode is None:
            monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
        else:
            monkeypatch.setenv("BPFTIME_AMD_SEQ_ASM", mode)
        b = Bench()
        mp, pids = b.u64_hash(16)
        b.attach(um.count_by_helper(isa.BPF_FUNC_get_current_pid_tgid, mp.fd, pids), F1)
        mc, ma = dev.Map(HASH, 4, 8, 16), dev.Map(HASH, 8, 8, 2 * calls + 8)
        b.attach(ua.clock_seq(mc.fd, ma.fd, {}, {}), F1)
        assert dispatch(b, r, pid=False, clock=False)[0] == 0
        assert dev.last_seq_tier() == tier
        b.snapshot()
        assert pids == {me(): calls}
        tid = me() & 0xFFFFFFFF
        assert int.from_bytes(mc.lookup(tid.to_bytes(4, "little")), "little") == calls and ma.count() == calls
        seen = [int.from_bytes(ma.lookup(((tid << 32) | c).to_bytes(8, "little")), "little") for c in range(calls)]
        assert seen[0] > 0 and all(x <= y for x, y in zip(seen, seen[1:]))
