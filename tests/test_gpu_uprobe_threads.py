"""The thread-ordered uprobe replay (BPFTIME_AMD_DISPATCH_THREADS) on the device
against the model (tests/_uprobe.py, programs and records from
tests/_uprobe_threads.py), bit-exact: maps, out_state, out_rets, failed
callbacks, the records untouched.

Shapes: records n in {1, 64, 65, 257, 1031} by 1, 3, 64, 65 (= the kernel's
64-lane block + 1: two blocks) and 130 recorded threads -- lane, wave and block
boundaries, and ragged walks (one thread owns about half the records, the upper
half of the threads one each).  Three attachable functions and one nobody
attaches to are mixed in the records.

Cases (a), (b) and (c) attach pairs that may not commute: without the plan
flag the dispatch refuses them."""
import os
import threading

import numpy as np
import pytest

from bpftime_amd import isa
from bpftime_amd import vm as dev

import _uprobe as um
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
        self.model, self.n = um.Model(), 0

    def attach(self, pair, func, kind=dev.UPROBE, cookie=None):
        self.n += 1
        fd = dev.prog_create(pair[0], f"p{self.n}", KPROBE)
        assert self.model.attach(func, kind, pair[1], cookie) > 0
        return dev.uprobe_attach(fd, func, kind, cookie)


def run_both(b, r, n, flags=THREADS, pid=True, outs=False, failed_replace=None):
    """Dispatches on the device and in the model; compares the failure count,
    the records and (outs) out_state / out_rets.  failed_replace: the records
    whose replace program fails -- the device stores 0 with bit 0 set (DESIGN.md,
    Uprobe replay), which the model, leaving a failed callback's record alone,
    is told here."""
    st_h, rets_h = np.full(n, 6, np.uint32), np.full(n, -5, np.int64)
    kw = {}
    if outs:
        kw["out_state"], kw["out_rets"] = buf(st_h), buf(rets_h)
    enter, leave = buf(r["enter"]), buf(r["leave"])
    got = dev.uprobe_dispatch(buf(r["func"]), n, enter=enter, leave=leave, pid_tgid=buf(r["pid"]) if pid else None,
                              clock=buf(r["clock"]), flags=flags, **kw)
    st_m, rets_m = st_h.copy(), rets_h.copy()
    me = (os.getpid() << 32) | threading.get_native_id()
    want = b.model.dispatch(r["func"], r["enter"], r["leave"], pid_tgid=r["pid"] if pid else None, clock=r["clock"],
                            out_state=st_m, out_rets=rets_m, default_pid=me)
    if failed_replace is not None:
        st_m[failed_replace] |= 1
        rets_m[failed_replace] = 0
    assert got == want
    assert (enter.download(np.uint64).reshape(n, 21) == r["enter"]).all()
    assert (leave.download(np.uint64).reshape(n, 21) == r["leave"]).all()
    if outs:
        assert (kw["out_state"].download(np.uint32) == st_m).all()
        assert (kw["out_rets"].download(np.int64) == rets_m).all()
    return want


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
    return sorted(set(int(p) & 0xFFFFFFFF for p in r["pid"]))


def funclat(b, threads, func=F0, **kw):
    """The funclatency pair on `func`: (starts map, hist map, starts dict, hist list)."""
    targ = kw.pop("targ_tgid", 0)
    ms, mh = dev.Map(HASH, 4, 8, 2 * threads + 8), dev.Map(ARRAY, 4, 4 * ut.SLOTS, 1)
    starts, hist = {}, [0] * ut.SLOTS
    b.attach(ut.funclat_entry(ms.fd, starts, targ_tgid=targ), func)
    b.attach(ut.funclat_return(ms.fd, mh.fd, starts, hist, **kw), func, dev.URETPROBE)
    return ms, mh, starts, hist


@pytest.mark.parametrize("variant", ["plain", "delete", "filter"])
@shapes
def test_funclatency_pair(fresh_runtime, n, threads, variant):       # (a)
    b, r = Bench(), ut.records(n, threads)
    kw = {"delete": {"delete": True}, "filter": {"targ_tgid": 2}}.get(variant, {})
    ms, mh, starts, hist = funclat(b, threads, **kw)
    with pytest.raises(dev.EbpfError, match="may not commute"):
        dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), leave=buf(r["leave"]), pid_tgid=buf(r["pid"]),
                            clock=buf(r["clock"]))
    assert ms.count() == 0 and sum(hist_of(mh)) == 0
    assert dev.uprobe_dispatch_plan(dev.DISPATCH_THREADS) == 1
    assert run_both(b, r, n) == 0
    assert hist_of(mh) == hist
    assert u32_map(ms, tids(r)) == starts and ms.count() == len(starts)
    if variant == "plain":
        assert sum(hist) == int((r["func"] == F0).sum())


@shapes
def test_order_inside_threads(fresh_runtime, n, threads):            # (b)
    b, r = Bench(), ut.records(n, threads)
    mc, mo, msn = dev.Map(HASH, 4, 8, 2 * threads + 8), dev.Map(HASH, 8, 8, 2 * n + 8), dev.Map(HASH, 8, 8, 2 * n + 8)
    cnt, order, seen = {}, {}, {}
    b.attach(ut.seq_entry(mc.fd, mo.fd, cnt, order), F1)
    b.attach(ut.seq_return(mc.fd, msn.fd, cnt, seen), F1, dev.URETPROBE)
    with pytest.raises(dev.EbpfError, match="may not commute"):
        dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), leave=buf(r["leave"]), pid_tgid=buf(r["pid"]))
    assert mc.count() == 0
    assert run_both(b, r, n) == 0
    assert u32_map(mc, tids(r)) == cnt and mc.count() == len(cnt)
    assert um.hash_counts(mo, order.keys()) == order and mo.count() == len(order)
    assert um.hash_counts(msn, seen.keys()) == seen and msn.count() == len(seen)
    assert len(order) == int((r["func"] == F1).sum())


@shapes
def test_pair_across_functions_shares_a_map(fresh_runtime, n, threads):   # (c)
    b, r = Bench(), ut.records(n, threads)
    m, c = dev.Map(HASH, 8, 8, 512), {}
    b.attach(um.func_ip_count(m.fd, c), F0)
    b.attach(um.cookie_tag(m.fd, c), F1, dev.URETPROBE)
    with pytest.raises(dev.EbpfError, match="may not commute on map fd"):
        dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), leave=buf(r["leave"]))
    assert m.count() == 0
    assert run_both(b, r, n) == 0
    assert um.hash_counts(m, [F0, F1, F2, 0]) == c and m.count() == len(c)


@shapes
def test_func_ip_and_cookies_per_attachment(fresh_runtime, n, threads):   # (d)
    b, r = Bench(), ut.records(n, threads)
    mk, mi = dev.Map(HASH, 8, 8, 512), dev.Map(HASH, 8, 8, 512)
    ck, ci = {}, {}
    b.attach(um.cookie_tag(mk.fd, ck), F2, cookie=11)
    b.attach(um.cookie_tag(mk.fd, ck), F2, cookie=0xABCDEF0123456789)
    b.attach(um.func_ip_count(mi.fd, ci), F2, dev.URETPROBE, cookie=5)
    b.attach(um.func_ip_count(mi.fd, ci), F0)
    assert run_both(b, r, n) == 0
    hits = int((r["func"] == F2).sum())
    assert um.hash_counts(mk, [0, 5, 11, 0xABCDEF0123456789]) == ck
    assert ck == ({11: hits, 0xABCDEF0123456789: hits} if hits else {})
    assert um.hash_counts(mi, [F0, F1, F2, 0]) == ci and mi.count() == len(ci)


@shapes
def test_override_replace_and_plain_in_one_dispatch(fresh_runtime, n, threads):   # (e)
    b, r = Bench(), ut.records(n, threads)
    m, c = dev.Map(HASH, 8, 8, 512), {}
    b.attach(um.override_if_arg0(-7, 2), F0, dev.UPROBE_OVERRIDE)
    b.attach(ut.replace_faulting_at(3, 5), F1, dev.UREPLACE)
    b.attach(um.override_if_arg0(1, 2), F2)              # a plain probe calling 58: its unit fails
    b.attach(um.func_ip_count(m.fd, c), F2, dev.URETPROBE)
    b.attach(um.override_func_ip_plus(1), F2, dev.UPROBE_OVERRIDE)   # late: never runs
    f, di = r["func"], r["enter"][:, um.DI]
    bad = (f == F1) & (di == 3)
    failed = run_both(b, r, n, outs=True, failed_replace=bad)
    assert failed == int(bad.sum()) + int(((f == F2) & (di == 2)).sum())
    assert um.hash_counts(m, [F0, F1, F2, 0]) == c


@shapes
def test_ctx_is_fresh_for_every_callback(fresh_runtime, n, threads):  # (f)
    b, r = Bench(), ut.records(n, threads)
    mw, mr, ml = dev.Map(HASH, 8, 8, 64), dev.Map(HASH, 8, 8, 64), dev.Map(HASH, 8, 8, 64)
    cw, cr, cl = {}, {}, {}
    b.attach(um.ctx_writer(mw.fd, cw), F0)
    b.attach(ut.di_count(mr.fd, cr), F0)                 # after the writer: the record's di, not 77
    b.attach(um.ctx_writer(ml.fd, cl), F0, dev.URETPROBE)
    assert run_both(b, r, n) == 0                        # (compares enter / leave afterwards)
    assert um.hash_counts(mw, [77]) == cw and um.hash_counts(ml, [77]) == cl
    assert um.hash_counts(mr, [0, 1, 2, 3, 77]) == cr and 77 not in cr


@pytest.mark.parametrize("pid", [True, False], ids=["recorded", "one-thread"])
@pytest.mark.parametrize("n,threads", [(1, 1), (65, 3), (257, 65)])
def test_ordered_is_the_serial_run(fresh_runtime, n, threads, pid):   # (g)
    b, r = Bench(), ut.records(n, threads)
    ms, mh, starts, hist = funclat(b, threads, plain=True)
    assert dev.uprobe_dispatch_plan(dev.DISPATCH_THREADS | dev.BATCH_ORDERED) == 1
    assert run_both(b, r, n, flags=THREADS | dev.BATCH_ORDERED, pid=pid) == 0
    assert hist_of(mh) == hist
    me = (os.getpid() << 32) | threading.get_native_id()
    assert u32_map(ms, tids(r) + [me & 0xFFFFFFFF]) == starts and ms.count() == len(starts)


def test_nothing_to_run(fresh_runtime):                  # (h)
    b = Bench()
    ms, mh, starts, hist = funclat(b, 8)
    r = ut.records(130, 5, funcs=(um.NOBODY, F1))
    assert run_both(b, r, 130) == 0
    assert ms.count() == 0 and sum(hist_of(mh)) == 0
    assert dev.uprobe_dispatch(None, 0, flags=THREADS) == 0
    # records without callers under the parallel plan: one thread owns them all
    r = ut.records(130, 5)
    assert run_both(b, r, 130, pid=False) == 0
    assert hist_of(mh) == hist and ms.count() == len(starts) == 1
