"""The event-list replay's test inputs and model (tests/_uprobe_events.py): the
trace generator's invariants, the call-depth pair's bytes against its callables
in the oracle interpreter, and the reason the event list exists -- on every GPU
shape with n >= 64 the nested replay and the flat replay of the same records
differ in the funclatency histogram, the call-depth histogram and the `seen`
map, so a replay that ignores the list cannot pass the GPU tests.  No GPU."""
import numpy as np
import pytest

from bpftime_amd import isa

import _uprobe as um
import _uprobe_events as ue
import _uprobe_threads as ut

HASH, ARRAY = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_ARRAY
A, B = 21, 22                                           # map fds the bytes name
F0, F1, F2 = um.FUNCS
SHAPES = [(1, 1), (64, 64), (65, 3), (65, 65), (257, 64), (257, 65), (1031, 1), (1031, 3), (1031, 65), (1031, 130)]
NESTED = [s for s in SHAPES if s[0] >= 64]


@pytest.mark.parametrize("n,threads", SHAPES)
def test_trace_invariants(n, threads):
    r = ue.traces(n, threads)
    ev = r["events"]
    assert ev.dtype == np.uint32 and (ev >> 1).max() < n
    assert len(set(int(w) for w in ev)) == len(ev)       # no event twice
    deepest = ue.depth_profile(r)                        # properly nested per thread
    assert deepest <= 5
    # the clocks increase strictly along the list
    t = [int(r["clock"][int(w) >> 1, int(w) & 1]) for w in ev]
    assert all(a < b for a, b in zip(t, t[1:]))
    # unpaired records: the caps, and both kinds from n = 64 on
    has_e = set(int(w) >> 1 for w in ev if not int(w) & 1)
    has_r = set(int(w) >> 1 for w in ev if int(w) & 1)
    assert sorted(has_r - has_e) == r["ret_only"] and sorted(has_e - has_r) == r["ent_only"]
    assert has_e | has_r == set(range(n))
    assert len(r["ret_only"]) + len(r["ent_only"]) <= n // 16
    if n >= 64:
        assert r["ret_only"] and r["ent_only"] and deepest >= 3
        own = r["owner"]
        for i in r["ret_only"]:                          # at the start of its thread
            assert i == min(np.flatnonzero(own == own[i]))
        mine = [int(w) >> 1 for w in ev if own[int(w) >> 1] == own[r["ent_only"][0]]]
        assert mine[-1] in r["ent_only"]                 # at its end
    # ut.records' skew
    per = np.bincount(r["owner"])
    t = max(1, min(threads, n // 2))
    assert len(per) == t and per.min() >= 1 and per[0] == per.max()
    if t >= 2:
        singles = per[t // 2:]
        assert (singles == 1).all() and per[0] >= (n - len(singles)) // 3


@pytest.mark.parametrize("n,threads", NESTED)
def test_trace_has_recursion_and_a_call_inside_another(n, threads):
    r = ue.traces(n, threads)
    open_, rec_depth, inner = {}, 0, False
    for w in r["events"]:
        i, phase = int(w) >> 1, int(w) & 1
        st = open_.setdefault(int(r["owner"][i]), [])
        if phase == 0:
            st.append(i)
            run = 1
            while run < len(st) and r["func"][st[-1 - run]] == r["func"][i]:
                run += 1
            rec_depth = max(rec_depth, run)
            inner |= len(st) >= 2 and r["func"][st[-2]] == F0 and r["func"][i] == F1
        elif st and st[-1] == i:
            st.pop()
    assert rec_depth >= 3 and inner


def _env(pid_tgid, ktime=0):
    return um.Env(np.arange(21, dtype=np.uint64), F0, 0, pid_tgid, ktime, None, False)


def test_depth_pair(fresh_oracle):
    depth, by = {}, [0] * ue.SLOTS
    od = fresh_oracle.OracleMap(HASH, 4, 8, 16, fd=A)
    ob = fresh_oracle.OracleMap(ARRAY, 4, 4 * ue.SLOTS, 1, fd=B)
    ent, ret = ue.depth_entry(A, B, depth, by), ue.depth_return(A, depth)

    def both(pair, pid):
        ep, eb = _env(pid), _env(pid)
        want = pair[1](ep)
        rc, r0 = um.run_bytes(pair[0], eb)
        assert rc == 0 and r0 == want and (eb.regs == ep.regs).all()
        assert ut.oracle_dict(od) == depth and ut.oracle_hist(ob) == by
    p, q = (1 << 32) | 100, (2 << 32) | 101
    both(ret, p)                                         # absent: nothing changes
    assert depth == {}
    for pair, pid in ((ent, p), (ent, p), (ent, q), (ent, p), (ret, p), (ent, p), (ret, q), (ret, q)):
        both(pair, pid)
    assert by[:4] == [2, 1, 2, 0] and depth == {100: 3, 101: um.M64}
    for _ in range(2):                                   # a wrapped depth files in the last slot
        both(ent, q)
    assert by[31] == 1 and by[0] == 3 and depth[101] == 1


def _replay(r, nested):
    """The funclatency pair on F0, the depth pair on F0 and F1, the seq pair on
    F1: (hist, bydepth, seen) of the nested or the flat replay."""
    m = ue.EventModel()
    starts, hist, depth, by, cnt, order, seen = {}, [0] * ut.SLOTS, {}, [0] * ue.SLOTS, {}, {}, {}
    m.attach(F0, um.UPROBE, ut.funclat_entry(A, starts)[1])
    m.attach(F0, um.URETPROBE, ut.funclat_return(A, B, starts, hist)[1])
    for f in (F0, F1):
        m.attach(f, um.UPROBE, ue.depth_entry(A, B, depth, by)[1])
        m.attach(f, um.URETPROBE, ue.depth_return(A, depth)[1])
    m.attach(F1, um.UPROBE, ut.seq_entry(A, B, cnt, order)[1])
    m.attach(F1, um.URETPROBE, ut.seq_return(A, B, cnt, seen)[1])
    if nested:
        assert m.dispatch_events(r["events"], r["func"], r["enter"], r["leave"], pid_tgid=r["pid"],
                                 clock=r["clock"]) == 0
    else:
        assert m.dispatch(r["func"], r["enter"], r["leave"], pid_tgid=r["pid"], clock=r["clock"]) == 0
    return hist, by, seen


@pytest.mark.parametrize("n,threads", NESTED)
def test_nesting_changes_the_expected_results(n, threads):
    r = ue.traces(n, threads)
    nested, flat = _replay(r, True), _replay(r, False)
    assert nested[0] != flat[0], "the funclatency histogram does not see the nesting"
    assert nested[1] != flat[1], "the call-depth histogram does not see the nesting"
    assert nested[2] != flat[2], "the seen map does not see the nesting"
    assert sum(nested[1][1:]) > 0 and sum(flat[1][1:]) == 0     # flat: every call begins at depth 0


@pytest.mark.parametrize("n,threads", SHAPES)
def test_flat_list_is_the_call_dispatch(n, threads):
    r = ut.records(n, threads)
    out = []
    for flat in (True, False):
        m = ue.EventModel()
        starts, hist, cnt, order, seen, c = {}, [0] * ut.SLOTS, {}, {}, {}, {}
        m.attach(F0, um.UPROBE, ut.funclat_entry(A, starts)[1])
        m.attach(F0, um.URETPROBE, ut.funclat_return(A, B, starts, hist, delete=True)[1])
        m.attach(F1, um.UPROBE, ut.seq_entry(A, B, cnt, order)[1])
        m.attach(F1, um.URETPROBE, ut.seq_return(A, B, cnt, seen)[1])
        m.attach(F2, um.UREPLACE, um.replace_with_arg0_plus(3)[1])
        st, rets = np.full(n, 6, np.uint32), np.full(n, -5, np.int64)
        kw = dict(pid_tgid=r["pid"], clock=r["clock"], out_state=st, out_rets=rets)
        if flat:
            failed = m.dispatch_events(ue.flat_events(n), r["func"], r["enter"], r["leave"], **kw)
        else:
            failed = m.dispatch(r["func"], r["enter"], r["leave"], **kw)
        out.append((failed, starts, hist, cnt, order, seen, list(st), list(rets)))
    assert out[0] == out[1]
