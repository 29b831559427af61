"""The CPU-side preconditions of the many-thread device tests, without a
device, so that they hold before any GPU time is spent:

* tests/test_gpu_syscall_many_threads.py: every parametrisation's records name
  exactly the thread count it is about and contain the ragged classes (one
  record, hundreds, exit-only, id -1 only), and after the oracle's run over
  them every hash map holds at most half its max_entries -- the condition that
  keeps the unpinned "inserts race for the last free slot" case out;
* tests/test_gpu_uprobe_asm.py's many-wave cases: the records name exactly
  the thread count, and the model's containers stay within half the maps;
* tests/test_gpu_thread_groups.py: every key set builds, has the distinct keys
  it is meant to have, and the stable-argsort reference is consistent with
  itself (the checker accepts it, and rejects an unstable order and an order
  that treats the keys as signed)."""
import numpy as np
import pytest

import _syscall_threads as st
import _thread_groups as tg
import _uprobe as um
import _uprobe_asm as ua
import _uprobe_events as ue
import _uprobe_threads as ut


@pytest.mark.parametrize("case", st.ALL, ids=st.case_id)
def test_records_and_map_sizes(fresh_oracle, case):
    name, threads, kw = case
    c = st.BUILDERS[name](fresh_oracle, None, threads, **kw)
    w = st.assert_shape(c.recs, threads)
    assert len(c.recs) == st.PER_THREAD * threads <= (1 << 17) + 8
    # monotonic clocks within a thread
    order = np.lexsort((np.arange(len(w)), w[:, 11]))
    same = w[order[1:], 11] == w[order[:-1], 11]
    assert (w[order[1:], 12][same] > w[order[:-1], 12][same]).all()
    out = c.o.dispatch(c.recs)
    assert len(out) == len(c.recs) and fresh_oracle.OracleSyscallDispatch.failed() == 0
    for m in c.hash_maps():
        assert m.max_entries >= 2 * threads
    st.half_full(*c.hash_maps())
    start = c.hash_maps()[0].items()
    if kw.get("filter_pid"):
        assert sorted(int.from_bytes(k, "little") - 2000 for k in start) == [128, 129, 130, 131]
    else:
        assert threads // 2 < len(start) <= threads


def test_the_cut_off_is_an_edge():
    assert st.EDGES[-2:] == [st.SEQ_ASM_THREADS, st.SEQ_ASM_THREADS + 1]
    assert [st.auto_tier(t) for t in st.EDGES] == [1, 1, 1, 1, 0]


@pytest.mark.parametrize("threads,calls", ua.MANY_WAVES, ids=[str(t) for t, _ in ua.MANY_WAVES])
def test_uprobe_many_wave_records(threads, calls):
    """tests/test_gpu_uprobe_asm.py's many-wave shapes: exactly `threads`
    recorded threads of calls[0] .. calls[1] - 1 calls, clocks that increase
    inside every thread, and in the model's run starts holds at most a key per
    thread and the tag map at most a key per call -- half of what the device
    maps hold (2 x threads + 8, 2 x calls + 16)."""
    r = ua.ragged(threads, calls=calls)
    n = len(r["func"])
    assert len(np.unique(r["pid"])) == threads and [ua.auto_tier(t) for t, _ in ua.MANY_WAVES] == [1, 1, 0]
    per = np.bincount(r["owner"], minlength=threads)
    assert per.min() == calls[0] and per.max() == calls[1] - 1 and n == per.sum()
    assert (np.diff(r["clock"].reshape(-1).astype(np.int64)) > 0).all()
    m = ue.EventModel()
    starts, hist, tags, ips = {}, [0] * ut.SLOTS, {}, {}
    F1, F2 = ua.FUNCS[1:3]
    m.attach(F1, um.UPROBE, ut.funclat_entry(5, starts)[1])
    m.attach(F1, um.URETPROBE, ut.funclat_return(5, 6, starts, hist)[1])
    m.attach(F2, um.UPROBE, ut.di_count(7, tags)[1])
    m.attach(F2, um.UPROBE, ut.di_count(8, ips)[1])
    m.attach(F1, um.URETPROBE, ut.di_count(7, tags)[1])
    st_, rets = np.full(n, 6, np.uint32), np.full(n, -5, np.int64)
    assert m.dispatch(r["func"], r["enter"], r["leave"], pid_tgid=r["pid"], clock=r["clock"], out_state=st_,
                      out_rets=rets) == 0
    assert 0 < len(starts) <= threads and 0 < len(tags) <= n and len(ips) <= 4
    assert sum(hist) == int((r["func"] == F1).sum())


@pytest.mark.parametrize("f,n,distinct", tg.CASES, ids=tg.IDS)
def test_grouping_reference(f, n, distinct):
    keys = tg.keys_of(f, n)
    assert (keys == tg.keys_of(f, n)).all()              # a fixed seed
    if distinct is not None:
        assert len(np.unique(keys)) == distinct(n)
    perm, seg = tg.reference(keys)
    tg.check(keys, perm, seg, len(seg) - 1)
    assert (keys[perm][1:] >= keys[perm][:-1]).all()     # (an unsigned comparison)


def test_grouping_checker_notices():
    """What the device test must catch, fed to the checker by hand: a sort that
    ignores bit 0 (unstable against the full key), reversed ties, a signed
    order, and a wrong segment list."""
    keys = tg.keys_of(tg.unsigned_mix, 1031)
    perm, seg = tg.reference(keys)
    nseg = len(seg) - 1
    top63 = np.argsort(keys >> np.uint64(1), kind="stable").astype(np.uint32)
    assert (top63 != perm).any()
    with pytest.raises(AssertionError, match="stable argsort"):
        tg.check(keys, top63, seg, nseg)
    ties = np.lexsort((-np.arange(len(keys)), keys)).astype(np.uint32)
    with pytest.raises(AssertionError, match="stable argsort"):
        tg.check(keys, ties, seg, nseg)
    signed = np.argsort(keys.view(np.int64), kind="stable").astype(np.uint32)
    with pytest.raises(AssertionError, match="stable argsort"):
        tg.check(keys, signed, seg, nseg)
    with pytest.raises(AssertionError, match="nseg"):
        tg.check(keys, perm, seg[:-1], nseg - 1)
    moved = seg.copy()
    moved[3] += 1
    with pytest.raises(AssertionError, match="run heads"):
        tg.check(keys, perm, moved, nseg)
    flat = seg.copy()
    flat[4] = flat[3]
    with pytest.raises(AssertionError, match="strictly increasing"):
        tg.check(keys, perm, flat, nseg)
