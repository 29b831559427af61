"""The uprobe replay dispatch on the device against the model (tests/_uprobe.py),
bit-exact: maps, out_state, out_rets, failed callbacks.  Record counts 1, 63,
64, 65 and 130 (the gather's wave boundaries); three attachable functions and
one nobody attaches to, assigned pseudo-randomly from a fixed seed."""
import os
import threading

import numpy as np
import pytest

from bpftime_amd import _lib, isa, programs
from bpftime_amd import vm as dev
from bpftime_amd.isa import Asm

import _stacktrace as sm
import _uprobe as um

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, 130]
KPROBE, TRACEPOINT = 2, 5
F0, F1, F2 = um.FUNCS
HASH = isa.BPF_MAP_TYPE_HASH


def buf(a):
    return dev.DeviceBuffer.from_array(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def hmap():
    return dev.Map(HASH, 8, 8, 512)


class Bench:
    """Device and model side by side: attach a (code, callable) pair to both."""

    def __init__(self):
        self.model, self.n = um.Model(), 0

    def attach(self, pair, func, kind=dev.UPROBE, cookie=None):
        self.n += 1
        fd = dev.prog_create(pair[0], f"p{self.n}", KPROBE)
        want = self.model.attach(func, kind, pair[1], cookie)
        assert want > 0
        return dev.uprobe_attach(fd, func, kind, cookie)


def run_both(b, r, n, flags=dev.BATCH_SYNC, pid=True, clock=True, outs=False, stacks=None, prefill=-5):
    st_h, rets_h = np.full(n, 6, np.uint32), np.full(n, prefill, np.int64)
    kw = {}
    if outs:
        kw["out_state"], kw["out_rets"] = buf(st_h), buf(rets_h)
    enter, leave = buf(r["enter"]), buf(r["leave"])
    got = dev.uprobe_dispatch(buf(r["func"]), n, enter=enter, leave=leave, pid_tgid=buf(r["pid"]) if pid else None,
                              clock=buf(r["clock"]) if clock else None, flags=flags, **kw, **(stacks or {}))
    st_m, rets_m = st_h.copy(), rets_h.copy()
    me = (os.getpid() << 32) | threading.get_native_id()
    want = b.model.dispatch(r["func"], r["enter"], r["leave"], pid_tgid=r["pid"] if pid else None,
                            clock=r["clock"] if clock else None, stacks=r["stacks"] if stacks else None,
                            out_state=st_m, out_rets=rets_m, default_pid=me)
    assert got == want
    # the records are never written
    assert (enter.download(np.uint64).reshape(n, 21) == r["enter"]).all()
    assert (leave.download(np.uint64).reshape(n, 21) == r["leave"]).all()
    if outs:
        assert (kw["out_state"].download(np.uint32) == st_m).all()
        assert (kw["out_rets"].download(np.int64) == rets_m).all()
    return st_m, rets_m


@pytest.mark.parametrize("n", COUNTS)
def test_func_ip_and_cookies(fresh_runtime, n):          # (a)
    b, r = Bench(), um.records(n)
    maps, counts = [hmap() for _ in range(4)], [{} for _ in range(4)]
    b.attach(um.func_ip_count(maps[0].fd, counts[0]), F0, cookie=11)
    b.attach(um.func_ip_count(maps[1].fd, counts[1]), F2)
    b.attach(um.cookie_tag(maps[2].fd, counts[2]), F0, dev.URETPROBE, cookie=0xABCDEF0123456789)
    b.attach(um.cookie_tag(maps[3].fd, counts[3]), F2, dev.URETPROBE)       # no cookie: 0
    run_both(b, r, n)
    keys = list(um.FUNCS) + [um.NOBODY, 0, 11, 0xABCDEF0123456789]
    for m, c in zip(maps, counts):
        assert um.hash_counts(m, keys) == c and m.count() == len(c)


def _sys_records(n):
    rng = np.random.default_rng(99 + n)
    rec = np.zeros((n, 12), dtype=np.uint64)
    rec[:, 1] = rec[:, 9] = rng.choice(np.array([0, 1, 60], dtype=np.uint64), n)   # read, write, exit
    rec[:, 11] = rng.integers(1, 4, n, dtype=np.uint64)
    return rec


@pytest.mark.parametrize("flags", [dev.DISPATCH_PROGRAMS, dev.BATCH_ORDERED], ids=["programs", "ordered"])
@pytest.mark.parametrize("n", COUNTS)
def test_cookie_in_syscall_dispatch(fresh_runtime, n, flags):   # (b)
    L = _lib.lib()
    rec = _sys_records(n)
    mc, mi, mn = hmap(), hmap(), hmap()
    tag = dev.prog_create(programs.cookie_tag(mc.fd), "tag", TRACEPOINT)
    ip = dev.prog_create(programs.func_ip_count(mi.fd), "ip", TRACEPOINT)
    plain = dev.prog_create(programs.cookie_tag(mn.fd), "plain", TRACEPOINT)
    # a cookie through BPF_PROG_ATTACH, one through BPF_LINK_CREATE, a link without
    assert L.bpftime_attach_perf_to_bpf_with_cookie(L.bpftime_amd_perf_event_syscall(-1, 0), tag, 0x51) > 0
    assert dev.link_create(ip, L.bpftime_amd_perf_event_syscall(-1, 1), 41, cookie=0x52) > 0
    lp = L.bpftime_attach_perf_to_bpf(L.bpftime_amd_perf_event_syscall(-1, -1), plain)
    assert lp > 0 and L.bpftime_amd_link_attached(lp) == 1
    assert dev.syscall_dispatch(buf(rec), n, flags=dev.BATCH_SYNC | flags) == 0
    nr = rec[:, 1]
    live = lambda c: {k: v for k, v in c.items() if v}  # noqa: E731
    assert um.hash_counts(mc, [0, 0x51, 0x52]) == live({0x51: int((nr == 0).sum())})
    assert um.hash_counts(mi, [0, 0x51, 0x52]) == live({0: int((nr == 1).sum())})      # func_ip: 0 here
    assert um.hash_counts(mn, [0, 0x51, 0x52]) == live({0: int((nr != 60).sum())})


@pytest.mark.parametrize("n", COUNTS)
def test_override_and_replace(fresh_runtime, n):         # (c)
    b, r = Bench(), um.records(n)
    m, c = hmap(), {}
    b.attach(um.override_if_arg0(-7, 2), F0, dev.UPROBE_OVERRIDE)
    b.attach(um.replace_with_arg0_plus(1000), F1, dev.UREPLACE)
    b.attach(um.func_ip_count(m.fd, c), F2)
    b.attach(um.override_func_ip_plus(1), F2, dev.UPROBE_OVERRIDE)          # late: never runs
    st, rets = run_both(b, r, n, outs=True)
    assert um.hash_counts(m, list(um.FUNCS) + [0]) == c
    f, di = r["func"], r["enter"][:, um.DI]
    assert (st == np.where(((f == F0) & (di == 2)) | (f == F1), 7, 6)).all()
    assert (rets == np.where((f == F0) & (di == 2), -7, np.where(f == F1, di.astype(np.int64) + 1000, -5))).all()


@pytest.mark.parametrize("n", COUNTS)
def test_override_func_ip_is_zero_everywhere(fresh_runtime, n):
    # every record matches (one function), and a function that matches none
    b, r = Bench(), um.records(n, funcs=(F1,))
    b.attach(um.override_func_ip_plus(9), F1, dev.UPROBE_OVERRIDE)
    b.attach(um.override_func_ip_plus(3), F0, dev.UPROBE_OVERRIDE)          # no record: launches nothing
    st, rets = run_both(b, r, n, outs=True)
    assert (st == 7).all() and (rets == 9).all()


@pytest.mark.parametrize("n", COUNTS)
def test_ctx_is_a_copy(fresh_runtime, n):                # (d)
    b, r = Bench(), um.records(n)
    m, c = hmap(), {}
    b.attach(um.ctx_writer(m.fd, c), F0)
    run_both(b, r, n)                                    # (compares enter / leave afterwards)
    assert um.hash_counts(m, [77]) == c


@pytest.mark.parametrize("recorded", [True, False], ids=["recorded", "default"])
@pytest.mark.parametrize("n", COUNTS)
def test_pid_and_clock(fresh_runtime, n, recorded):      # (e)
    b, r = Bench(), um.records(n)
    mp, mk, mx = hmap(), hmap(), hmap()
    cp, ck, cx = {}, {}, {}
    b.attach(um.count_by_helper(isa.BPF_FUNC_get_current_pid_tgid, mp.fd, cp), F0)
    if recorded:
        b.attach(um.count_by_helper(isa.BPF_FUNC_ktime_get_ns, mk.fd, ck), F1)
        b.attach(um.count_by_helper(isa.BPF_FUNC_ktime_get_ns, mx.fd, cx), F1, dev.URETPROBE)
        run_both(b, r, n)
        assert um.hash_counts(mp, set(int(x) for x in r["pid"])) == cp
        keys = set(int(x) for x in r["clock"].reshape(-1))
        assert um.hash_counts(mk, keys) == ck and um.hash_counts(mx, keys) == cx
    else:
        me = (os.getpid() << 32) | threading.get_native_id()
        dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]))
        hits = int((r["func"] == F0).sum())
        assert um.hash_counts(mp, [me]) == ({me: hits} if hits else {}) and mp.count() == (1 if hits else 0)


@pytest.mark.parametrize("layout", ["rows", "frame_major"])
@pytest.mark.parametrize("n", COUNTS)
def test_stackid_through_the_dispatch(fresh_runtime, n, layout):    # (f)
    r, D = um.records(n), 6
    stm, model = dev.Map(isa.BPF_MAP_TYPE_STACK_TRACE, 4, 8 * D, 64), sm.StackMap(4, 8 * D, 64)
    fd = dev.prog_create(sm.stackid_prog(stm.fd, sm.USER_STACK), "stk", KPROBE)
    dev.uprobe_attach(fd, F0, dev.UPROBE)
    frames = r["frames"].copy()
    for i in range(n):
        frames[i, r["depths"][i]:] = 0xBAD                 # past the depth: never read into a slot
    if layout == "rows":
        arr, us, fs = frames, 8 * D, 8
    else:
        arr, us, fs = frames.T, 8, 8 * n
    # ORDERED: which stack a contended slot keeps is an effect of the order
    assert dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), flags=dev.BATCH_SYNC | dev.BATCH_ORDERED,
                               stacks=buf(arr), stack_unit_stride=us, stack_frame_stride=fs,
                               stack_depths=buf(r["depths"]), stack_max_depth=D) == 0
    for i in range(n):
        if r["func"][i] == F0:
            sm.get_stackid(model, r["stacks"][i], sm.USER_STACK)
    for k in range(64):
        assert stm.stack_frames(k) == model.data.get(k), k


@pytest.mark.parametrize("n", COUNTS)
def test_conflicts_refused_and_single_ordered(fresh_runtime, n):    # (g)
    b, r = Bench(), um.records(n)
    m, c = hmap(), {}
    one = b.attach(um.func_ip_count(m.fd, c), F0)
    two = dev.uprobe_attach(dev.prog_create(programs.cookie_tag(m.fd), "second", KPROBE), F1, dev.URETPROBE)
    with pytest.raises(dev.EbpfError, match=rf"'p1' \(prog fd \d+, attachment {one}\) and 'second' \(prog fd \d+, "
                                            rf"attachment {two}\) may not commute on map fd {m.fd}"):
        dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), leave=buf(r["leave"]))
    assert m.count() == 0                                # refused before any launch
    dev.uprobe_detach(two)
    run_both(b, r, n, flags=dev.BATCH_SYNC | dev.BATCH_ORDERED)
    assert um.hash_counts(m, um.FUNCS) == c


@pytest.mark.parametrize("n", COUNTS)
def test_set_attach_on_plain_batches(fresh_runtime, n):  # (h)
    mu, mr = hmap(), hmap()
    v = dev.VM()
    v.load(programs.func_ip_count(mu.fd))
    w = dev.VM()
    w.load(programs.cookie_tag(mu.fd))
    v.set_attach(0x7F00DEADBEEF, 5)
    w.set_attach(0x7F00DEADBEEF, 5)
    regs = buf(um.records(n)["enter"])
    assert v.exec_batch(dev.CTX_UPROBE, regs, n, 168) == 0
    assert w.exec_batch(dev.CTX_UPROBE, regs, n, 168) == 0
    assert um.hash_counts(mu, [0, 5, 0x7F00DEADBEEF]) == {0x7F00DEADBEEF: n, 5: n}
    d = dev.VM()                                         # defaults: both 0
    d.load(programs.func_ip_count(mr.fd))
    assert d.exec_batch(dev.CTX_RAW, regs, n, 168, fixed_len=168) == 0
    assert um.hash_counts(mr, [0, 5, 0x7F00DEADBEEF]) == {0: n}
    with pytest.raises(dev.EbpfError, match="uprobe batch needs"):
        v.exec_batch(dev.CTX_UPROBE, regs, n, 160)


@pytest.mark.parametrize("n", COUNTS)
def test_retval_helpers_fail_a_plain_probe(fresh_runtime, n):   # (i)
    b, r = Bench(), um.records(n)
    b.attach(um.override_if_arg0(1, 2), F0)
    b.attach(um.override_if_arg0(1, 2 ** 40), F1, dev.URETPROBE)   # never equal: never calls the helper
    st, rets = run_both(b, r, n, outs=True)
    assert (st == 6).all() and (rets == -5).all()
    assert dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), leave=buf(r["leave"])) == \
        int(((r["func"] == F0) & (r["enter"][:, um.DI] == 2)).sum())


def test_failed_replace_reports_zero(fresh_runtime):
    """Decided here (Uprobe replay): a replace whose program fails
    its unit stores 0 with bit 0 set and is counted -- a failed exec reports
    r0 = 0 -- where the reference leaves that call's return alone.  The program
    reads address 0, which the launch's window check refuses (no access is
    made): the unit fails as any out-of-window load does."""
    n = 65
    r = um.records(n)
    a = Asm()
    code = a.ldx(8, 2, 1, 8 * um.DI).jmp("jne", 2, 3, "ok").mov64(3, 0).ldx(8, 0, 3, 0).label("ok") \
        .mov64(0, 5).exit().assemble()
    dev.uprobe_attach(dev.prog_create(code, "rep", KPROBE), F1, dev.UREPLACE)
    st, rets = buf(np.full(n, 6, np.uint32)), buf(np.full(n, -5, np.int64))
    hit, bad = r["func"] == F1, (r["func"] == F1) & (r["enter"][:, um.DI] == 3)
    assert dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), out_state=st, out_rets=rets) == int(bad.sum())
    assert bad.any() and (st.download(np.uint32) == np.where(hit, 7, 6)).all()
    assert (rets.download(np.int64) == np.where(bad, 0, np.where(hit, 5, -5))).all()
