"""The uprobe replay model (tests/_uprobe.py) against hand-written cases: what
the GPU tests compare the device with must itself say what the reference does.
No GPU."""
import numpy as np

import _uprobe as um

F, G = 0x1000, 0x2000


def _regs(n, di=0):
    r = np.zeros((n, 21), dtype=np.uint64)
    r[:, um.DI] = di
    return r


def _log(log, tag):
    def prog(e):
        log.append((tag, e.func_ip, e.cookie))
        return 0
    return prog


def test_attach_order():
    m, log = um.Model(), []
    m.attach(F, um.URETPROBE, _log(log, "r1"), cookie=5)
    m.attach(F, um.UPROBE, _log(log, "u1"))
    m.attach(G, um.UPROBE, _log(log, "g"))
    m.attach(F, um.UPROBE, _log(log, "u2"), cookie=9)
    m.attach(F, um.URETPROBE, _log(log, "r2"))
    assert m.dispatch([F, G, 0x3000], _regs(3), _regs(3)) == 0
    # per call: the uprobes in attach order, then the uretprobes; cookie absent: 0
    assert log == [("u1", F, 0), ("u2", F, 9), ("r1", F, 5), ("r2", F, 0), ("g", G, 0)]


def test_override_first_is_exclusive():
    m, log = um.Model(), []
    assert m.attach(F, um.OVERRIDE, um.override_if_arg0(-7, 3)[1]) == 1
    assert m.attach(F, um.UPROBE, _log(log, "u")) == -um.EEXIST
    assert m.attach(F, um.OVERRIDE, _log(log, "o")) == -um.EEXIST
    assert m.attach(G, um.UPROBE, _log(log, "g")) == 2           # another function is free
    st, rets = np.zeros(3, np.uint32), np.full(3, 111, np.int64)
    enter = _regs(3)
    enter[1, um.DI] = 3
    assert m.dispatch([F, F, G], enter, _regs(3), out_state=st, out_rets=rets) == 0
    assert list(st) == [0, 1, 0] and list(rets) == [111, -7, 111] and log == [("g", G, 0)]
    # the hook goes with its last attachment
    m.detach(1)
    assert m.attach(F, um.UPROBE, _log(log, "u")) == 3


def test_late_override_never_runs():
    m, log = um.Model(), []
    m.attach(F, um.UPROBE, _log(log, "u"))
    assert m.attach(F, um.OVERRIDE, um.override_func_ip_plus(1)[1]) == 2    # accepted, kept
    st, rets = np.zeros(1, np.uint32), np.full(1, 5, np.int64)
    assert m.dispatch([F], _regs(1), _regs(1), out_state=st, out_rets=rets) == 0
    assert log == [("u", F, 0)] and list(st) == [0] and list(rets) == [5]
    # ... not even once the uprobe is gone: the function stays hooked as a listener
    m.detach(1)
    assert m.dispatch([F], _regs(1), _regs(1), out_state=st, out_rets=rets) == 0
    assert list(st) == [0]


def test_replace_returns_r0_and_func_ip_is_zero():
    m = um.Model()
    m.attach(F, um.UREPLACE, um.replace_with_arg0_plus(10)[1])
    m.attach(G, um.OVERRIDE, um.override_func_ip_plus(4)[1])
    st, rets = np.zeros(3, np.uint32), np.full(3, -1, np.int64)
    assert m.dispatch([F, G, 0x3000], _regs(3, di=2), _regs(3), out_state=st, out_rets=rets) == 0
    assert list(st) == [1, 1, 0] and list(rets) == [12, 4, -1]


def test_retval_helpers_fail_a_plain_probe():
    m = um.Model()
    m.attach(F, um.UPROBE, um.override_if_arg0(1, 0)[1])
    m.attach(F, um.URETPROBE, um.override_if_arg0(1, 0)[1])
    st, rets = np.zeros(2, np.uint32), np.zeros(2, np.int64)
    enter, leave = _regs(2), _regs(2, di=9)
    enter[1, um.DI] = 1
    assert m.dispatch([F, F], enter, leave, out_state=st, out_rets=rets) == 1
    assert list(st) == [0, 0]


def test_ctx_is_a_copy_and_recorded_fields():
    m, c1, c2, c3 = um.Model(), {}, {}, {}
    m.attach(F, um.UPROBE, um.ctx_writer(0, c1)[1])
    m.attach(F, um.UPROBE, um.count_by_helper(14, 0, c2)[1])
    m.attach(F, um.URETPROBE, um.count_by_helper(5, 0, c3)[1])
    enter = _regs(2, di=1)
    before = enter.copy()
    assert m.dispatch([F, F], enter, _regs(2), pid_tgid=[7, 8], clock=[(1, 2), (3, 4)]) == 0
    assert (enter == before).all() and c1 == {77: 2} and c2 == {7: 1, 8: 1} and c3 == {2: 1, 4: 1}
    c2.clear()
    assert m.dispatch([F], enter, _regs(2), default_pid=42) == 0 and c2 == {42: 1}


def _env(di, func_ip=0x7F0000001234, cookie=0xC0FFEE, pid=0x500000007, ktime=991, ovr=True):
    regs = np.arange(21, dtype=np.uint64) + np.uint64(100)
    regs[um.DI] = di
    return um.Env(regs, func_ip, cookie, pid, ktime, None, ovr)


def _both(pair, fd, counts, fresh_oracle, **kw):
    """A pair's callable and its bytes (in the oracle interpreter, helper stubs
    over the same Env values) must leave the same r0, ctx, override and map."""
    from bpftime_amd import isa
    omap = fresh_oracle.OracleMap(isa.BPF_MAP_TYPE_HASH, 8, 8, 64, fd=fd) if fd else None
    for di in (0, 2, 3):
        ep, eb = _env(di, **kw), _env(di, **kw)
        try:
            want, bad = pair[1](ep), False
        except um.Failed:
            want, bad = None, True
        rc, r0 = um.run_bytes(pair[0], eb)
        assert (rc < 0) == bad
        if not bad:
            assert r0 == want & um.M64 and (eb.regs == ep.regs).all()
        assert eb.overridden == ep.overridden
    if omap:
        got = {int.from_bytes(k, "little"): int.from_bytes(v, "little") for k, v in omap.items().items()}
        assert got == counts and counts


def test_pairs_agree_in_the_oracle_interpreter(fresh_oracle):
    from bpftime_amd import isa
    for mk in (um.func_ip_count, um.cookie_tag, um.ctx_writer,
               lambda fd, c: um.count_by_helper(isa.BPF_FUNC_get_current_pid_tgid, fd, c),
               lambda fd, c: um.count_by_helper(isa.BPF_FUNC_ktime_get_ns, fd, c)):
        counts = {}
        _both(mk(9, counts), 9, counts, fresh_oracle)
        fresh_oracle.reset()
    for pair in (um.override_if_arg0(-7, 2), um.override_if_arg0(1 << 40, 3), um.replace_with_arg0_plus(1000),
                 um.override_func_ip_plus(4)):
        _both(pair, 0, None, fresh_oracle)
        _both(pair, 0, None, fresh_oracle, func_ip=0)
    # 58 / 187 with no return callback: the callback fails
    _both(um.override_if_arg0(1, 2), 0, None, fresh_oracle, ovr=False)
