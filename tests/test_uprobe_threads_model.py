"""The thread-ordered replay's program pairs (tests/_uprobe_threads.py): each
pair's eBPF bytes, run in the oracle interpreter over the oracle's maps, must
do what its Python callable does to its containers; and the reason the plan
exists -- a program-major replay of the funclatency pair differs from the
serial one as soon as a thread makes two calls.  No GPU."""
import numpy as np

from bpftime_amd import isa

import _uprobe as um
import _uprobe_threads as ut

HASH, ARRAY = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_ARRAY
A, B, C3 = 21, 22, 23                                   # map fds the bytes name


def _env(pid_tgid, ktime, di=0, ax=0):
    regs = np.arange(21, dtype=np.uint64) + np.uint64(100)
    regs[um.DI], regs[um.AX] = di, ax
    return um.Env(regs, 0x401000, 0, pid_tgid, ktime, None, False)


def _run_both(pair, *args):
    ep, eb = _env(*args), _env(*args)
    want = pair[1](ep)
    rc, r0 = um.run_bytes(pair[0], eb)
    assert rc == 0 and r0 == want and (eb.regs == ep.regs).all()


# (pid_tgid, clock) of calls by two threads of two processes; the durations
# reach slots 0, 1, 4, 31 (clamped) and 20
CALLS = [((1 << 32) | 100, 1000, 1001), ((2 << 32) | 101, 1002, 1005), ((1 << 32) | 100, 1010, 1010 + 17),
         ((2 << 32) | 101, 2000, 2000 + (1 << 40)), ((1 << 32) | 100, 1 << 41, (1 << 41) + (1 << 20) + 5)]


def test_log2_slot():
    assert [ut.log2_slot(v) for v in (0, 1, 2, 3, 4, 17, (1 << 31) - 1, 1 << 31, 1 << 40, um.M64)] == \
        [0, 0, 1, 1, 2, 4, 30, 31, 31, 31]


def _funclat(fresh_oracle, **kw):
    targ = kw.pop("targ_tgid", 0)
    starts, hist = {}, [0] * ut.SLOTS
    os_ = fresh_oracle.OracleMap(HASH, 4, 8, 16, fd=A)
    oh = fresh_oracle.OracleMap(ARRAY, 4, 4 * ut.SLOTS, 1, fd=B)
    ent = ut.funclat_entry(A, starts, targ_tgid=targ)
    ret = ut.funclat_return(A, B, starts, hist, **kw)
    # a return before any entry (the miss path), then the calls in order
    _run_both(ret, (1 << 32) | 100, 5)
    for pid, t0, t1 in CALLS:
        _run_both(ent, pid, t0)
        _run_both(ret, pid, t1)
        assert ut.oracle_dict(os_) == starts and ut.oracle_hist(oh) == hist
    return starts, hist


def test_funclat_pair(fresh_oracle):
    starts, hist = _funclat(fresh_oracle)
    want = [0] * ut.SLOTS
    for s in (0, 1, 4, 31, 20):
        want[s] += 1
    assert hist == want and starts == {100: 1 << 41, 101: 2000}


def test_funclat_pair_delete(fresh_oracle):
    starts, hist = _funclat(fresh_oracle, delete=True)
    assert sum(hist) == 5 and starts == {}


def test_funclat_pair_plain(fresh_oracle):
    assert sum(_funclat(fresh_oracle, plain=True)[1]) == 5


def test_funclat_pair_filter(fresh_oracle):
    starts, hist = _funclat(fresh_oracle, targ_tgid=2)
    assert sum(hist) == 2 and starts == {101: 2000}       # process 1's calls never start


def test_seq_pair(fresh_oracle):
    cnt, order, seen = {}, {}, {}
    oc = fresh_oracle.OracleMap(HASH, 4, 8, 16, fd=A)
    oo = fresh_oracle.OracleMap(HASH, 8, 8, 16, fd=B)
    osn = fresh_oracle.OracleMap(HASH, 8, 8, 16, fd=C3)
    ent, ret = ut.seq_entry(A, B, cnt, order), ut.seq_return(A, C3, cnt, seen)
    _run_both(ret, (1 << 32) | 100, 0, 0, 9)             # before any entry: number 0
    for k, (pid, t0, t1) in enumerate(CALLS):
        _run_both(ent, pid, t0, 50 + k, 0)
        _run_both(ret, pid, t1, 0, 70 + k)
    assert ut.oracle_dict(oc) == cnt == {100: 3, 101: 2}
    assert ut.oracle_dict(oo) == order == {(100 << 32): 50, (101 << 32): 51, (100 << 32) | 1: 52,
                                           (101 << 32) | 1: 53, (100 << 32) | 2: 54}
    assert ut.oracle_dict(osn) == seen and seen[(100 << 32) | 3] == 74 and seen[100 << 32] == 9


def test_di_count_and_faulting_replace(fresh_oracle):
    counts = {}
    om = fresh_oracle.OracleMap(HASH, 8, 8, 16, fd=A)
    pair = ut.di_count(A, counts)
    for di in (3, 0, 3):
        _run_both(pair, 7, 0, di)
    assert ut.oracle_dict(om) == counts == {3: 2, 0: 1}
    rep = ut.replace_faulting_at(3, 5)
    _run_both(rep, 7, 0, 2)
    # (the faulting path is the device's window check; the oracle interpreter
    # checks no bounds, so only the callable is asked)
    try:
        rep[1](_env(7, 0, 3))
        assert False
    except um.Failed:
        pass


def test_program_major_differs_from_serial():
    """One thread, two calls: program-major runs both entries, then both
    returns, so the second entry overwrites starts[tid] before the first
    return reads it.  The serial order files durations 4 and 64; program-major
    files 1000 - 1100 (a wrapped difference: slot 31) and 64."""
    func = [um.FUNCS[0]] * 2
    regs = np.zeros((2, 21), dtype=np.uint64)
    pid, clock = [(1 << 32) | 100] * 2, [(1000, 1004), (1100, 1164)]

    def replay(program_major):
        starts, hist = {}, [0] * ut.SLOTS
        ent, ret = ut.funclat_entry(A, starts)[1], ut.funclat_return(A, B, starts, hist)[1]
        if not program_major:
            m = um.Model()
            m.attach(func[0], um.UPROBE, ent)
            m.attach(func[0], um.URETPROBE, ret)
            assert m.dispatch(func, regs, regs, pid_tgid=pid, clock=clock) == 0
        else:
            for phase, prog in ((0, ent), (1, ret)):
                for i in range(2):
                    prog(um.Env(regs[i].copy(), func[i], 0, pid[i], clock[i][phase], None, False))
        return hist
    serial, major = replay(False), replay(True)
    assert serial[2] == 1 and serial[6] == 1 and sum(serial) == 2
    assert major[31] == 1 and major[6] == 1 and major != serial
