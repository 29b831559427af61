"""bpf_perf_event_output (25) through a PERF_EVENT_ARRAY on the device against
the model (tests/_perfout.py): return values, the ring's positions and the
fetched records.  ORDERED runs are compared byte for byte (neither side
writes padding, so even the stale bytes agree); parallel runs as a multiset of
records, with the stream parsed end to end.  Every bad pointer is one the range
guard answers -EFAULT before any access; the batch lies inside a larger device
buffer whose slack holds a sentinel."""
import struct
from collections import Counter

import numpy as np
import pytest

from bpftime_amd import gen, isa

import _perfout as pm

pytestmark = pytest.mark.gpu

PEA, HASH = isa.BPF_MAP_TYPE_PERF_EVENT_ARRAY, isa.BPF_MAP_TYPE_HASH
STRIDE, SLACK, SENTINEL = pm.STRIDE, 256, 0x5A
NS = [1, 63, 64, 65, 130]
MIX = [0, 1, 5, 52, 12, 64, 4, 33]
TRACEPOINT = 5


def units_of(n, sizes, seed=3):
    u = np.random.default_rng(seed).integers(0, 256, (n, STRIDE), dtype=np.uint8)
    u[:, 0] = [sizes[i % len(sizes)] for i in range(n)]
    u[:, 4:8] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    return u


class Rig:
    """A perf array over software perf events, on the device and in the model."""

    def __init__(self, dev, max_entries=64, ring=1 << 16, events=1):
        self.dev = dev
        self.map, self.model = dev.Map(PEA, 4, 4, max_entries), pm.PerfArray(max_entries)
        self.ev, self.rings = [], {}
        for _ in range(events):
            e = dev.PerfEvent(data_bytes=ring)
            self.ev.append(e)
            self.rings[e.fd] = pm.Ring(ring)
        for k in range(max_entries):
            self.set(k, self.ev[k % events].fd)

    def set(self, k, fd):
        assert self.map.update(struct.pack("<i", k), struct.pack("<i", fd)) == 0
        assert self.model.update(struct.pack("<i", k), struct.pack("<i", fd)) == 0

    def run(self, code, units, ordered=False, first_unit=0, size=None, data_at=pm.DATA_OFF, array="model",
            range_ok=None, calls=1):
        """Runs the batch; returns the device r0s after checking them against
        the model's (array: the PerfArray r2 names, None for no perf array)."""
        dev, n = self.dev, units.shape[0]
        host = np.full(2 * SLACK + n * STRIDE, SENTINEL, dtype=np.uint8)
        host[SLACK:SLACK + n * STRIDE] = units.reshape(-1)
        d, out = dev.DeviceBuffer.from_array(host), dev.DeviceBuffer(8 * n)
        vm = dev.VM()
        vm.load(code)
        assert vm.info()["big_stack"]                      # the scratch-stack kernels carry the helper
        flags = dev.BATCH_SYNC | (dev.BATCH_ORDERED if ordered else 0)
        assert vm.exec_batch(dev.CTX_RAW, d, n, STRIDE, fixed_len=STRIDE, rets=out, flags=flags,
                             data_offset=SLACK, first_unit=first_unit) == 0
        got = out.download(np.uint64)
        assert (d.download() == host).all()                # the units and the slack stay as they were
        flat = units.reshape(-1)
        want = []
        for i in range(n):
            sz = int(units[i, 0]) if size is None else size
            at = i * STRIDE + data_at
            ok = (sz <= pm.MAX_DATA and at + sz <= n * STRIDE) if range_ok is None else range_ok
            arr = self.model if array == "model" else array
            w = pm.output(arr, ((first_unit + i) // 64) % 64, self.rings, flat[at:at + sz].tobytes() if ok else None,
                          sz, ok)
            want.append(w)
        assert got.tolist() == want, [(i, hex(int(g)), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:6]
        return got

    def check(self, exact, k=0, among=None):
        """The ring's positions and its fetched records against the model's."""
        e, ring = self.ev[k], self.rings[self.ev[k].fd]
        h, t, b = e.state()
        assert (h, t, b) == (ring.head, ring.tail, ring.data_bytes) and h - t <= max(b - 1, 0)
        n, raw = e.fetch_raw()
        wn, wraw = ring.fetch()
        recs = pm.parse(raw)                               # parses end to end
        assert n == wn == len(recs) and len(raw) == len(wraw) == h - t
        if exact:
            assert raw == wraw
        elif among is None:
            assert Counter(recs) == Counter(pm.parse(wraw))
        else:                                              # which of the callers won is the schedule's
            assert not Counter(recs) - Counter(among)
        assert e.state()[:2] == (ring.head, ring.head)
        return recs


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("src", ["unit", "stack"])
@pytest.mark.parametrize("n", NS)
def test_mixed_sizes_per_lane(fresh_runtime, n, src, ordered):
    rig = Rig(fresh_runtime)
    rig.run(pm.emit_prog(rig.map.fd, src=src), units_of(n, MIX), ordered=ordered)
    recs = rig.check(exact=ordered)
    assert sum(rs for rs, _ in recs) == sum(pm.record_size(MIX[i % len(MIX)]) for i in range(n))


@pytest.mark.parametrize("size", [0, 1, 5, 52])
def test_one_size(fresh_runtime, size):
    rig = Rig(fresh_runtime)
    rig.run(pm.emit_prog(rig.map.fd, size=size), units_of(65, [0]), size=size)
    recs = rig.check(exact=False)
    assert len(recs) == 65 and all(rs == pm.record_size(size) for rs, _ in recs)


@pytest.mark.parametrize("ordered", [False, True])
def test_wrap(fresh_runtime, ordered):
    rig = Rig(fresh_runtime, ring=64)
    code = pm.emit_prog(rig.map.fd, size=5)
    rig.run(code, units_of(2, [0], seed=1), ordered=ordered, size=5)
    assert len(rig.check(exact=ordered)) == 2
    rig.run(code, units_of(2, [0], seed=2), ordered=ordered, size=5)   # 48..72: straddles the ring's end
    assert rig.ev[0].state()[:2] == (96, 48)
    assert len(rig.check(exact=ordered)) == 2


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("before", [0, 3])
def test_full_ring(fresh_runtime, ordered, before):
    rig = Rig(fresh_runtime, ring=256)
    code = pm.emit_prog(rig.map.fd, size=5)
    if before:
        rig.run(code, units_of(before, [0], seed=9), ordered=True, size=5)
    used = 24 * before
    got = rig.run(code, units_of(130, [0]), ordered=ordered, size=5)   # every call still answers 0
    assert not got.any()
    h, t, b = rig.ev[0].state()
    assert (h - used) // 24 == (256 - 1 - used) // 24 and h <= t + b - 1
    u = units_of(130, [0])
    every = [(24, u[i, 8:13].tobytes() + bytes(7)) for i in range(130)] + \
            [(24, units_of(before, [0], seed=9)[i, 8:13].tobytes() + bytes(7)) for i in range(before)]
    assert len(rig.check(exact=ordered, among=None if ordered else every)) == before + (256 - 1 - used) // 24


def test_mixed_sizes_on_a_nearly_full_ring_ordered(fresh_runtime):
    rig = Rig(fresh_runtime, ring=128)
    sizes = [52, 28, 12, 4, 20, 4, 1, 52, 0]      # 64, 40 (fits), 24 (no), 16 (fits), then nothing but ...
    rig.run(pm.emit_prog(rig.map.fd), units_of(len(sizes), sizes), ordered=True)
    assert [rs for rs, _ in rig.check(exact=True)] == [64, 40, 16]


def test_no_ring(fresh_runtime):
    dev = fresh_runtime
    rig = Rig(dev, events=0 + 1, ring=0)
    got = rig.run(pm.emit_prog(rig.map.fd), units_of(65, MIX))
    assert not got.any() and rig.ev[0].state() == (0, 0, 0) and rig.ev[0].fetch_raw() == (0, b"")


def test_minus_one_cases(fresh_runtime):
    dev = fresh_runtime
    rig = Rig(dev)
    u = units_of(65, MIX)
    h = dev.Map(HASH, 4, 4, 8)
    rig.run(pm.emit_prog(h.fd), u, array=None)                              # r2 is a HASH map
    rig.run(pm.emit_prog(rig.map.fd, size=65517), u, size=65517)
    rig.run(pm.emit_prog(rig.map.fd, size=1 << 63), u, size=1 << 63)
    for k in range(64):
        rig.set(k, -1)
    rig.run(pm.emit_prog(rig.map.fd), u)                                    # empty slots
    tp = dev.lib().bpftime_tracepoint_create(-1, -1, 123)
    assert tp >= 0
    for k in range(64):
        rig.set(k, tp)
    rig.run(pm.emit_prog(rig.map.fd), u)                                    # a tracepoint perf event
    gone = dev.PerfEvent(data_bytes=256)
    for k in range(64):
        rig.set(k, gone.fd)
    gone.close()
    rig.run(pm.emit_prog(rig.map.fd), u)                                    # a closed fd
    for k in range(64):
        rig.set(k, 5000)
    rig.run(pm.emit_prog(rig.map.fd), u)                                    # an fd >= the table
    assert rig.ev[0].state()[:2] == (0, 0)


def test_cpu_past_the_array_in_the_same_wave(fresh_runtime):
    # units 32..63 of the numbering are CPU 0, 64..95 CPU 1: one wave, two CPUs, one slot
    rig = Rig(fresh_runtime, max_entries=1)
    got = rig.run(pm.emit_prog(rig.map.fd), units_of(64, MIX), first_unit=32)
    assert not got[:32].any() and (got[32:] == pm.FAIL).all()
    assert len(rig.check(exact=False)) == 32


def test_two_rings_in_one_wave(fresh_runtime):
    rig = Rig(fresh_runtime, max_entries=2, events=2)
    rig.run(pm.emit_prog(rig.map.fd), units_of(96, MIX), first_unit=32)
    a, b = rig.check(exact=False, k=0), rig.check(exact=False, k=1)
    assert len(a) == 32 and len(b) == 64                   # CPU 0 for units 32..63, CPU 1 for 64..127


def test_two_maps_in_one_program(fresh_runtime):
    dev = fresh_runtime
    rig = Rig(dev)
    other, e2 = dev.Map(PEA, 4, 4, 64), dev.PerfEvent(data_bytes=1 << 14)
    for k in range(64):
        assert other.set_perf(k, e2) == 0
    d = dev.DeviceBuffer.from_array(units_of(65, MIX))
    out = dev.DeviceBuffer(8 * 65)
    vm = dev.VM()
    vm.load(pm.emit_prog(rig.map.fd, second_map=other.fd))
    assert vm.exec_batch(dev.CTX_RAW, d, 65, STRIDE, fixed_len=STRIDE, rets=out) == 0
    assert not out.download(np.uint64).any()
    ra, rb = pm.parse(rig.ev[0].fetch_raw()[1]), pm.parse(e2.fetch_raw()[1])
    assert len(ra) == 65 and Counter(ra) == Counter(rb)


@pytest.mark.parametrize("ordered", [False, True])
def test_two_launches_without_a_fetch(fresh_runtime, ordered):
    rig = Rig(fresh_runtime)
    code = pm.emit_prog(rig.map.fd)
    rig.run(code, units_of(65, MIX, seed=1), ordered=ordered)
    h1 = rig.ev[0].state()[0]
    rig.run(code, units_of(63, MIX, seed=2), ordered=ordered)
    assert rig.ev[0].state()[0] > h1 > 0
    assert len(rig.check(exact=ordered)) == 128


@pytest.mark.parametrize("data,size", [(("null",), 8), (("stack", -8), 16), (("stack", -64), 65)])
def test_efault_leaves_the_ring_alone(fresh_runtime, data, size):
    rig = Rig(fresh_runtime)
    got = rig.run(pm.emit_prog(rig.map.fd, data=data, size=size), units_of(65, [0]), size=size, range_ok=False)
    assert (got == pm.EFAULT).all() and rig.ev[0].state()[:2] == (0, 0)


@pytest.mark.parametrize("n", [1, 65])
def test_efault_past_the_batch(fresh_runtime, n):
    # 16 bytes from unit + 120: inside the batch (the next unit's head) for every unit but the last
    rig = Rig(fresh_runtime)
    got = rig.run(pm.emit_prog(rig.map.fd, data=("unit", 120), size=16), units_of(n, [0]), size=16, data_at=120)
    assert got[-1] == pm.EFAULT and not got[:-1].any()
    assert len(rig.check(exact=False)) == n - 1


def test_flags_are_not_read(fresh_runtime):
    streams = []
    for flags in (0, 0xFFFFFFFF, 5):
        fresh_runtime.reset_runtime()
        rig = Rig(fresh_runtime)
        rig.run(pm.emit_prog(rig.map.fd, flags=flags), units_of(65, MIX), ordered=True)
        streams.append(rig.ev[0].fetch_raw())
    assert streams[0][0] == 65 and streams[0] == streams[1] == streams[2]


def test_a_map_handle_the_loader_cannot_place(fresh_runtime):
    rig = Rig(fresh_runtime)
    rig.run(pm.emit_prog(None, raw_r2=rig.map.fd), units_of(65, MIX))
    assert len(rig.check(exact=False)) == 65


@pytest.mark.parametrize("plan", ["ordered", "threads"])
def test_syscall_dispatch_events(fresh_runtime, plan):
    dev = fresh_runtime
    rig = Rig(dev, ring=1 << 15)
    dev.syscall_attach(dev.prog_create(pm.sys_enter_emitter(rig.map.fd), "emit", TRACEPOINT), -1, True)
    n = 512
    recs = gen.syscall_records_timed(n, threads=8)
    d = dev.DeviceBuffer.from_array(recs)
    flags = dev.BATCH_SYNC | (dev.BATCH_ORDERED if plan == "ordered" else dev.DISPATCH_THREADS)
    assert dev.syscall_dispatch(d, n, record_size=dev.SYSCALL_RECORD_TIMED, flags=flags) == 0
    w = recs.view(np.uint64).reshape(n, 16)
    # (exit and exit_group run no callback: syscall_trace_attach_impl.cpp:23-26)
    want = [struct.pack("<QQ", int(w[i, 11]), int(w[i, 1])) for i in range(n) if int(w[i, 1]) not in (60, 231)]
    got = [d for _, d in pm.parse(rig.ev[0].fetch_raw()[1])]
    assert all(len(g) == 20 for g in got)                  # 16 bytes + the padding to 8 of 12 + 16
    got = [g[:16] for g in got]
    if plan == "ordered":
        assert got == want                                 # the reference's per-call order
    else:
        assert Counter(got) == Counter(want)
        for tid in {x[:8] for x in want}:                  # each thread's calls in its own order
            assert [g for g in got if g[:8] == tid] == [x for x in want if x[:8] == tid]
