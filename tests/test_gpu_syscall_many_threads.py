"""The thread-ordered syscall dispatch (k_sys_seq, vm_seq.cpp seq_dispatch) at
many waves and on both sides of the automatic tier cut-off, bit-exact against
the oracle's record-by-record dispatch_syscall (oracle/drivers.c
orc_sys_dispatch): every element of `out`, every entry of every map and the
failed-callback count.

Thread counts are edges: 257 and 1,025 (one lane in the last 256-lane block),
4,096 (the measured shape), 16,384 (the last count the library puts in the asm
tier) and 16,385 (the first it puts in the C++ tier, a last block of one
lane).  The records average 8 per thread with an explicit ragged owner
assignment (tests/_syscall_threads.py ragged_owner): threads with one record
beside threads with 300, threads whose only records are exit / exit_group, and
threads whose only records carry id -1.

Every hash map holds at least twice the threads, so that no insert races for a
last free slot: asserted on the oracle after its run
(and, for every parametrisation, in tests/test_syscall_many_threads_model.py
without a device)."""
import numpy as np
import pytest

from bpftime_amd import gen

import _syscall_threads as st

pytestmark = pytest.mark.gpu


def run_device(dev, recs, soa=False):
    """One dispatch under the automatic plan: (failed, out)."""
    n = len(recs)
    out = dev.DeviceBuffer.from_array(np.full(n, -77, dtype=np.int64))
    if soa:
        enter, exit_, clock = gen.syscall_records_soa(recs)
        failed = dev.syscall_dispatch_soa(dev.DeviceBuffer.from_array(exit_), n, enter=dev.DeviceBuffer.from_array(enter),
                                          clock=dev.DeviceBuffer.from_array(clock), out=out)
    else:
        d = dev.DeviceBuffer.from_array(recs)
        failed = dev.syscall_dispatch(d, n, record_size=dev.SYSCALL_RECORD_TIMED, out=out)
        assert (d.download().reshape(n, 128) == recs).all()          # the records were not written
    return failed, out.download(np.int64)


def device_maps(case):
    return [dm.hash_items() if dm.type == st.HASH else dm.lookup(b"\0" * 4) for _, dm in case.pairs]


def oracle_maps(case):
    return [om.items() if om.type == st.HASH else om.lookup(b"\0" * 4) for om, _ in case.pairs]


def run_both(po, dev, case, threads, tier, soa=False):
    """The oracle's run, its preconditions, then the device's: everything
    compared; returns (out, maps) for comparisons between runs."""
    st.assert_shape(case.recs, threads)
    want = case.o.dispatch(case.recs)
    st.half_full(*case.hash_maps())
    want_maps = oracle_maps(case)
    assert dev.syscall_dispatch_plan() == 1
    failed, got = run_device(dev, case.recs, soa)
    assert dev.last_seq_tier() == tier
    assert failed == po.OracleSyscallDispatch.failed()
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), bad[:10], got[bad[:10]], want[bad[:10]])
    for i, (g, w) in enumerate(zip(device_maps(case), want_maps)):
        assert g == w, f"map {i}: {len(g)} entries, the oracle's {len(w)}"
    return want, want_maps


def fresh(po, dev):
    po.reset()
    dev.reset_runtime()
    dev.set_ncpu(64)


@pytest.mark.parametrize("threads", st.EDGES)
def test_syscount_latency_pair_at_each_edge(fresh_oracle, fresh_runtime, monkeypatch, threads):
    """syscount's enter + exit pair with measure_latency, the tier left to the library."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
    case = st.build_syscount(po, dev, threads)
    _, (start, data) = run_both(po, dev, case, threads, st.auto_tier(threads))
    assert len(start) > threads // 2 and len(data) > 50
    assert any(int.from_bytes(v[8:16], "little") for v in data.values())     # the latency path ran


@pytest.mark.parametrize("threads", st.TWO)
def test_syscount_latency_pair_three_ways(fresh_oracle, fresh_runtime, monkeypatch, threads):
    """The tier left to the library, BPFTIME_AMD_SEQ_ASM=1, =0, each on fresh
    maps and a fresh runtime.  Forcing the asm tier past its cut-off is a
    supported configuration: the contended regime, where the asm tier adds to
    memory through its ORDERED links and the C++ tier keeps private stacks."""
    po, dev = fresh_oracle, fresh_runtime
    seen = []
    for mode, tier in zip((None, "1", "0"), (st.auto_tier(threads), 1, 0)):
        fresh(po, dev)
        if mode is None:
            monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
        else:
            monkeypatch.setenv("BPFTIME_AMD_SEQ_ASM", mode)
        seen.append(run_both(po, dev, st.build_syscount(po, dev, threads), threads, tier))
    for out, maps in seen[1:]:
        assert (out == seen[0][0]).all() and maps == seen[0][1]


@pytest.mark.parametrize("threads", st.TWO)
def test_count_by_process(fresh_oracle, fresh_runtime, monkeypatch, threads):
    """data keyed by tgid: four neighbouring lanes race through lookup-or-init
    on one key while the other waves insert thousands of other keys."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
    case = st.build_syscount(po, dev, threads, count_by_process=True)
    _, (_, data) = run_both(po, dev, case, threads, st.auto_tier(threads))
    assert len(data) > threads // 8


@pytest.mark.parametrize("threads,opts", st.FILTERS, ids=["filter_pid-16385", "filter_failed-4096"])
def test_filters(fresh_oracle, fresh_runtime, monkeypatch, threads, opts):
    """filter_pid on one tgid: four live lanes in one wave, every other wave
    runs nothing.  filter_failed: most exits return before they touch a map."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
    case = st.build_syscount(po, dev, threads, **opts)
    _, (start, data) = run_both(po, dev, case, threads, st.auto_tier(threads))
    if "filter_pid" in opts:
        assert sorted(int.from_bytes(k, "little") for k in start) == [2128, 2129, 2130, 2131] and data
    else:
        assert len(start) > threads // 2 and data


@pytest.mark.parametrize("threads", st.TWO)
def test_struct_of_arrays(fresh_oracle, fresh_runtime, monkeypatch, threads):
    """syscall_dispatch_soa over the same calls (the grouping reads the caller
    at stride 32 in the exit array): the AoS run's results and the oracle's."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
    aos = run_both(po, dev, st.build_syscount(po, dev, threads), threads, st.auto_tier(threads))
    fresh(po, dev)
    soa = run_both(po, dev, st.build_syscount(po, dev, threads), threads, st.auto_tier(threads), soa=True)
    assert (aos[0] == soa[0]).all() and aos[1] == soa[1]


def test_plain_write_pair(fresh_oracle, fresh_runtime, monkeypatch):
    """start[tid] = value at enter, read at exit and summed into an ARRAY
    slot, at 16,385 threads under the automatic plan."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
    threads = st.SEQ_ASM_THREADS + 1
    _, (start, total) = run_both(po, dev, st.build_plain(po, dev, threads), threads, 0)
    assert len(start) > threads // 2 and any(total)


def test_overrides_and_per_syscall_attachments(fresh_oracle, fresh_runtime, monkeypatch):
    """bpf_override_return at sys_enter_write, bpf_set_retval at sys_exit and
    per-syscall counters at 4,096 threads."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
    out, (_, total, cnt) = run_both(po, dev, st.build_overrides(po, dev, 4096), 4096, 1)
    c = np.frombuffer(cnt, dtype=np.uint64)
    assert c[0] > 0 and c[1] > 0 and 0 < c[2] < len(out) and (out == -1).sum() > len(out) // 40 and any(total)


def test_scratch_grows_and_is_reused(fresh_oracle, fresh_runtime, monkeypatch):
    """One runtime, no reset: 257 threads, then 16,385, then 257 again; before
    each run the device maps are restored to their empty snapshots and the
    oracle's are created anew at the same fds.  The per-stream scratch behind
    the grouping grows for the second dispatch and is reused by the third."""
    po, dev = fresh_oracle, fresh_runtime
    monkeypatch.delenv("BPFTIME_AMD_SEQ_ASM", raising=False)
    _, _, dmaps = st.syscount_all(po, dev, entries=st.entries_for(st.SEQ_ASM_THREADS + 1))
    empty = [dm.snapshot() for dm in dmaps[:2]]
    for threads, seed in st.REUSE:
        po.reset()
        o, omaps, _ = st.syscount_all(po, dev, beside=dmaps)
        for dm, raw in zip(dmaps, empty):
            dm.restore(raw)
            assert dm.count() == 0
        case = st.Case(o, st.ragged_records(threads, seed), list(zip(omaps[:2], dmaps[:2])))
        _, (start, _) = run_both(po, dev, case, threads, st.auto_tier(threads))
        assert threads // 2 < len(start) <= threads
