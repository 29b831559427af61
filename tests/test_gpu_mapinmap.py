"""BPF_MAP_TYPE_ARRAY_OF_MAPS on the device: programs that look an inner map up
in an outer one and then use it, bit-exact against the oracle interpreter
running the same bytecode with the outer map answered by the model
(tests/_mapinmap.py).  The inner fd differs between the lanes of a wave in
every case that draws the slot from the unit.

Where the keys come from.  DESIGN.md ("Copy and compare helpers") records an
older defect whose cause is not established: in a scratch-stack program a
lookup of an ARRAY map with its key on the stack returns the wrong element for
a non-zero key when the wave runs a single lane (an ORDERED batch, a wave's
lone last unit).  Every map-in-map program is a scratch-stack program, so the
cases that leave a lone lane -- 1 unit, 65 units, every ORDERED batch,
ebpf_exec -- and the 63-unit case take the outer index and the inner key from
the unit itself (a flat pointer into the packet); the 64- and 130-unit
parallel cases take them from the stack."""
import ctypes as C
import struct

import numpy as np
import pytest

from bpftime_amd import isa
from bpftime_amd.isa import Asm

import _mapinmap as mm

pytestmark = pytest.mark.gpu

AOM, ARRAY, HASH = isa.BPF_MAP_TYPE_ARRAY_OF_MAPS, isa.BPF_MAP_TYPE_ARRAY, isa.BPF_MAP_TYPE_HASH
PHASH, PARRAY = isa.BPF_MAP_TYPE_PERCPU_HASH, isa.BPF_MAP_TYPE_PERCPU_ARRAY
FAIL = 0xFFFFFFFFFFFFFFFF
EINVAL64, ENOTSUP64 = (-22) & FAIL, (-95) & FAIL
NO_INNER, NO_VALUE = 0xDEAD0, 0xDEAD1
u32 = lambda v: struct.pack("<I", v)  # noqa: E731

# (units, ORDERED, keys on the stack): see the module docstring
SHAPES = [(1, False, False), (63, False, False), (64, False, True), (65, False, False), (130, False, True),
          (1, True, False), (65, True, False), (130, True, False)]
SHAPE_IDS = [f"{n}{'-ordered' if o else ''}{'-stackkeys' if s else ''}" for n, o, s in SHAPES]


def prologue(kind, stack_keys):
    """r6 = the unit {u32 outer index, u32 inner key, u8 op, ..., u64 value at
    16}; with stack_keys the two keys are copied to r10 - 4 / r10 - 8."""
    a = Asm()
    if kind == "xdp":
        a.ldx(8, 6, 1, 0)
    else:
        a.mov64(6, "r1")
    if stack_keys:
        a.ldx(4, 2, 6, 0).stx(4, 10, -4, "r2").ldx(4, 2, 6, 4).stx(4, 10, -8, "r2")
    return a


def key_ptr(a, reg, which, stack_keys):
    """reg = a pointer to the outer index (which = 0) or the inner key (1)."""
    if stack_keys:
        a.mov64(reg, "r10").add64(reg, -4 - 4 * which)
    else:
        a.mov64(reg, "r6").add64(reg, 4 * which)


def lookup_inner(a, outer_fd, stack_keys):
    """r7 = the inner map's handle; leaves with NO_INNER when the slot is
    NULL."""
    a.ld_map_fd(1, outer_fd)
    key_ptr(a, 2, 0, stack_keys)
    a.call(1).mov64(7, "r0").mov64(0, NO_INNER).jmp("jeq", 7, 0, "out")


def counter_prog(kind, outer_fd, stack_keys, readback=False):
    """inner = outer[idx]; v = inner[key]; atomic v[0] += 1 (u64); v[8] = key
    (u32, a plain store: every writer of an element stores the same word).
    Returns 2 + key.  With readback: loads v[0], adds the unit's u64 at 16
    atomically, loads v[0] again and returns after - before -- its own addend
    when no other unit shares the element."""
    a = prologue(kind, stack_keys)
    lookup_inner(a, outer_fd, stack_keys)
    a.mov64(1, "r7")
    key_ptr(a, 2, 1, stack_keys)
    a.call(1).mov64(8, "r0").mov64(0, NO_VALUE).jmp("jeq", 8, 0, "out")
    if readback:
        a.ldx(8, 3, 6, 16).ldx(8, 4, 8, 0)            # r4 = before
        a.atomic(8, 0x00, 8, 0, 3)                    # v[0] += r3
        a.ldx(8, 0, 8, 0).alu64("sub", 0, "r4")       # after - before
    else:
        a.mov64(2, 1).atomic(8, 0x00, 8, 0, 2)
        a.ldx(4, 3, 6, 4).stx(4, 8, 8, "r3")
        a.mov64(0, "r3").add64(0, 2)
    a.label("out").exit()
    return a.assemble()


def run_both(dev, po, code, units, models, kind="raw", ordered=False, ncpu=64):
    """The program over `units` on the device and on the oracle (wave by wave,
    so per-CPU maps see the device's virtual CPUs); returns (got, want)."""
    n = len(units)
    ovm = po.OracleVM()
    cbs = mm.register(ovm, po, models)
    ovm.load(code)
    vm = dev.VM()
    vm.load(code)
    assert vm.info()["big_stack"]  # the scratch-stack kernels carry the helper
    ou = units.copy()
    want = np.zeros(n, dtype=np.uint64)
    for w0 in range(0, n, 64):
        po.set_cpu((w0 // 64) % ncpu)
        part = np.ascontiguousarray(ou[w0:w0 + 64])
        want[w0:w0 + 64] = ovm.run_xdp(part, fixed_len=64) if kind == "xdp" else ovm.run_raw(part, 64)
    d = dev.DeviceBuffer.from_array(units)
    flags = dev.BATCH_SYNC | (dev.BATCH_ORDERED if ordered else 0)
    if kind == "xdp":
        out = dev.DeviceBuffer(4 * n)
        assert vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=64, verdicts=out, flags=flags) == 0
        got = out.download(np.uint32).astype(np.uint64)
        want &= np.uint64(0xFFFFFFFF)
    else:
        out = dev.DeviceBuffer(8 * n)
        assert vm.exec_batch(dev.CTX_RAW, d, n, 64, fixed_len=64, rets=out, flags=flags) == 0
        got = out.download(np.uint64)
    del cbs
    return got, want


def make_units(n, seed, idx_hi, key_hi):
    rng = np.random.default_rng(seed)
    units = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    w = units.view(np.uint32).reshape(n, 16)
    w[:, 0] = rng.integers(0, idx_hi, n)
    w[:, 1] = rng.integers(0, key_hi, n)
    return units


INNER_SHAPES = [(16, 3), (24, 5), (32, 8), (48, 2)]  # (value_size, max_entries) per slot


def array_world(dev, po, slots=4):
    """An outer of `slots` slots over ARRAY maps of different shapes, on the
    device and (the inner maps) in the oracle; the outer's oracle twin only
    makes the lddw resolve."""
    outer, model = dev.Map(AOM, 4, 4, slots), mm.Outer(slots)
    po.OracleMap(ARRAY, 4, 4, 1, fd=outer.fd)
    inner = []
    for i, (vs, mx) in enumerate(INNER_SHAPES[:slots]):
        m = dev.Map(ARRAY, 4, vs, mx)
        inner.append((m, po.OracleMap(ARRAY, 4, vs, mx, fd=m.fd)))
        assert outer.set_inner(i, m) == 0 and model.update(u32(i), struct.pack("<i", m.fd)) == 0
    return outer, model, inner


def same_inner(inner):
    for m, om in inner:
        np.testing.assert_array_equal(m.snapshot(), om.raw())


# ---- (a) divergent inner ARRAY maps ------------------------------------------
@pytest.mark.parametrize("kind", ["xdp", "raw"])
@pytest.mark.parametrize("n,ordered,stack_keys", SHAPES, ids=SHAPE_IDS)
def test_inner_arrays(fresh_oracle, fresh_runtime, kind, n, ordered, stack_keys):
    po, dev = fresh_oracle, fresh_runtime
    outer, model, inner = array_world(dev, po)
    units = make_units(n, n * 3 + ordered, 6, 9)  # indexes 4, 5 and keys past each map's end: NULL
    if n == 1:
        units.view(np.uint32)[0, :2] = (2, 7)  # a non-zero key in a non-zero slot
    got, want = run_both(dev, po, counter_prog(kind, outer.fd, stack_keys), units, {outer.fd: model}, kind, ordered)
    np.testing.assert_array_equal(got, want)
    if n >= 63:
        assert {NO_INNER, NO_VALUE} <= set(int(x) for x in want) and len(set(int(x) for x in want)) >= 5
    same_inner(inner)
    assert any(om.raw().any() for _, om in inner)
    assert outer.inner_fds() == model.slots


def test_exec_one_unit(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    outer, model, inner = array_world(dev, po)
    code = counter_prog("raw", outer.fd, False)
    ovm = po.OracleVM()
    cbs = mm.register(ovm, po, {outer.fd: model})
    ovm.load(code)
    vm = dev.VM()
    vm.load(code)
    for idx, key in [(1, 4), (3, 1), (0, 3), (5, 0), (2, 0)]:
        mem = bytearray(64)
        struct.pack_into("<II", mem, 0, idx, key)
        assert vm.exec(bytearray(mem)) == ovm.exec(bytearray(mem))
    same_inner(inner)
    assert inner[1][1].raw().any()
    del cbs


# ---- (b) inner HASH / PERCPU_HASH / PERCPU_ARRAY ------------------------------
def keyed_prog(outer_fd, stack_keys):
    """op (the unit's byte 8): 0 lookup -> the value's u64 (or NO_VALUE), 1
    update(inner, key, &unit[16], BPF_ANY) -> r0, 2 delete -> r0."""
    a = prologue("raw", stack_keys)
    lookup_inner(a, outer_fd, stack_keys)
    a.ldx(1, 8, 6, 8).mov64(1, "r7")
    key_ptr(a, 2, 1, stack_keys)
    a.jmp("jeq", 8, 1, "upd").jmp("jeq", 8, 2, "del")
    a.call(1).mov64(1, "r0").mov64(0, NO_VALUE).jmp("jeq", 1, 0, "out").ldx(8, 0, 1, 0).ja("out")
    a.label("upd").mov64(3, "r6").add64(3, 16).mov64(4, 0).call(2).ja("out")
    a.label("del").call(3)
    a.label("out").exit()
    return a.assemble()


@pytest.mark.parametrize("n,ordered,stack_keys", [(65, False, False), (130, False, True), (65, True, False)],
                         ids=["65", "130-stackkeys", "65-ordered"])
def test_inner_keyed_maps(fresh_oracle, fresh_runtime, n, ordered, stack_keys):
    """Batches of one operation each (so a parallel batch's result does not
    depend on the order of its units): inserts, lookups that hit and miss,
    deletes, lookups again.  Every unit's value is a function of its key."""
    po, dev = fresh_oracle, fresh_runtime
    po.set_ncpu(64)
    outer, model = dev.Map(AOM, 4, 4, 4), mm.Outer(4)
    po.OracleMap(ARRAY, 4, 4, 1, fd=outer.fd)
    inner = []
    for i, (t, mx) in enumerate([(HASH, 64), (PHASH, 64), (PARRAY, 8)]):
        m = dev.Map(t, 4, 8, mx)
        inner.append((m, po.OracleMap(t, 4, 8, mx, fd=m.fd)))
        assert outer.set_inner(i, m) == 0 and model.update(u32(i), struct.pack("<i", m.fd)) == 0
    code = keyed_prog(outer.fd, stack_keys)

    def batch(op, key_lo, key_hi, seed):
        units = make_units(n, seed, 4, 1)  # slot 3 is empty: NO_INNER
        w = units.view(np.uint32).reshape(n, 16)
        w[:, 1] = key_lo + np.random.default_rng(seed).integers(0, key_hi - key_lo, n)
        units[:, 8] = op
        units.view(np.uint64).reshape(n, 8)[:, 2] = w[:, 1].astype(np.uint64) * np.uint64(0x100000001) + np.uint64(7)
        got, want = run_both(dev, po, code, units, {outer.fd: model}, "raw", ordered)
        np.testing.assert_array_equal(got, want)
        return set(int(x) for x in want)

    assert batch(1, 0, 12, 1) >= {0, NO_INNER}            # inserts (PERCPU_ARRAY: keys 8.. fail)
    seen = batch(0, 0, 20, 2)                             # hits and misses
    assert NO_VALUE in seen and len(seen) > 4
    batch(2, 0, 6, 3)                                     # deletes
    assert NO_VALUE in batch(0, 0, 12, 4)                 # a deleted key misses
    batch(1, 4, 16, 5)                                    # inserts after deletes
    for m, om in inner[:2]:
        assert m.hash_items() == om.items() and m.count() == om.count() > 0
        walk, k = [], m.next_key(None)  # the host's next_key walk sees the inserted keys
        while k is not None:
            walk.append(k)
            k = m.next_key(k)
        assert sorted(walk) == sorted(om.items())
    np.testing.assert_array_equal(inner[2][0].snapshot(), inner[2][1].raw())


# ---- (c) slots that name no usable map ------------------------------------------
def test_slot_edges(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    outer, model, inner = array_world(dev, po, slots=2)
    big, bmodel = dev.Map(AOM, 4, 4, 8), mm.Outer(8)
    po.OracleMap(ARRAY, 4, 4, 1, fd=big.fd)
    gone = dev.Map(ARRAY, 4, 16, 4)
    never = gone.fd + 5  # no handle was ever created there
    slots = [inner[0][0].fd, 0, mm.MAX_FDS, -1, never, gone.fd, -(2 ** 31), 2 ** 31 - 1]
    for i, v in enumerate(slots):
        assert big.set_inner(i, v) == 0 and bmodel.update(u32(i), struct.pack("<i", v)) == 0
    gone.close()  # closed after the slot was written
    before = [m.snapshot() for m, _ in inner]
    for n, ordered in [(130, False), (65, True)]:
        units = make_units(n, 11 + n, 10, 3)  # indexes 8, 9: past the end
        w = units.view(np.uint32).reshape(n, 16)
        w[0, 0], w[1, 0], w[2, 0] = 8, 0xFFFFFFFF, 0  # == max_entries, the largest index, a live slot
        got, want = run_both(dev, po, counter_prog("raw", big.fd, False), units, {big.fd: bmodel}, "raw", ordered)
        np.testing.assert_array_equal(got, want)
        assert got[0] == got[1] == NO_INNER
        idx = w[:, 0]
        assert (got[(idx == 1) | (idx >= 8)] == NO_INNER).all()   # the empty slot, past the end
        assert (got[(idx >= 2) & (idx < 8)] == NO_VALUE).all()    # a handle that names no map: NULL
        assert (got[idx == 0] >= 2).all() and (got[idx == 0] <= 4).all()
    same_inner(inner)  # slot 0's map counted; nothing else changed
    np.testing.assert_array_equal(inner[1][0].snapshot(), before[1])
    # the outer's own fd in a slot: a nested map, refused at launch
    assert big.set_inner(1, big) == 0
    vm = dev.VM()
    vm.load(counter_prog("raw", big.fd, False))
    d, out = dev.DeviceBuffer.from_array(make_units(4, 1, 1, 1)), dev.DeviceBuffer(32)
    with pytest.raises(dev.EbpfError, match=rf"ARRAY_OF_MAPS map fd {big.fd} slot 1 holds map fd {big.fd} of type 12"):
        vm.exec_batch(dev.CTX_RAW, d, 4, 64, fixed_len=64, rets=out)


# ---- (d) program-side update / delete / push / pop / peek on the outer ----------
def test_program_side_ops_on_outer(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    outer, model, inner = array_world(dev, po)
    a = prologue("raw", False)
    a.ldx(1, 8, 6, 8)
    a.ld_map_fd(1, outer.fd).mov64(2, "r6").mov64(3, "r6").add64(3, 16).mov64(4, 0)
    for op, helper in [(1, 3), (2, 87), (3, 88), (4, 89)]:
        a.jmp("jeq", 8, op, f"h{helper}")
    a.call(2).ja("out")
    a.label("h3").call(3).ja("out")
    a.label("h87").mov64(2, "r3").mov64(3, 0).call(87).ja("out")
    a.label("h88").mov64(2, "r3").call(88).ja("out")
    a.label("h89").mov64(2, "r3").call(89)
    a.label("out").exit()
    for n, ordered in [(65, False), (64, True)]:
        units = make_units(n, 5, 4, 4)
        units[:, 8] = np.arange(n) % 5
        got, want = run_both(dev, po, a.assemble(), units, {outer.fd: model}, "raw", ordered)
        np.testing.assert_array_equal(got, want)
        assert list(got[:5]) == [EINVAL64, EINVAL64, ENOTSUP64, ENOTSUP64, ENOTSUP64]
    assert outer.inner_fds() == model.slots == [m.fd for m, _ in inner]  # slots unchanged


# ---- (e) the host rewrites a slot between two batches ------------------------------
def test_host_swaps_a_slot(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    outer, model, inner = array_world(dev, po)
    code = counter_prog("raw", outer.fd, True)
    units = make_units(130, 9, 1, 2)  # slot 0, keys 0 / 1 (valid in every inner map)
    got, want = run_both(dev, po, code, units, {outer.fd: model})
    np.testing.assert_array_equal(got, want)
    first = inner[0][0].snapshot()
    assert first.any() and not inner[3][0].snapshot().any()
    new = inner[3][0]
    assert outer.set_inner(0, new) == 0 and model.update(u32(0), struct.pack("<i", new.fd)) == 0
    got, want = run_both(dev, po, code, units, {outer.fd: model})
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(inner[0][0].snapshot(), first)  # the old table: left alone
    same_inner(inner)
    assert new.snapshot().any()


# ---- (f) refused inner types ---------------------------------------------------------
REFUSED = [(isa.BPF_MAP_TYPE_LRU_HASH, 4, 8, 8), (isa.BPF_MAP_TYPE_LPM_TRIE, 8, 8, 8),
           (isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 4096), (isa.BPF_MAP_TYPE_PROG_ARRAY, 4, 4, 4),
           (isa.BPF_MAP_TYPE_QUEUE, 0, 8, 4), (isa.BPF_MAP_TYPE_STACK, 0, 8, 4),
           (isa.BPF_MAP_TYPE_BLOOM_FILTER, 0, 8, 16), (AOM, 4, 4, 2)]


@pytest.mark.parametrize("shape", REFUSED, ids=[str(s[0]) for s in REFUSED])
@pytest.mark.parametrize("ordered", [False, True])
def test_refused_inner_types(fresh_oracle, fresh_runtime, shape, ordered):
    po, dev = fresh_oracle, fresh_runtime
    outer, model, inner = array_world(dev, po, slots=3)
    flags = 1 if shape[0] == isa.BPF_MAP_TYPE_LPM_TRIE else 0  # BPF_F_NO_PREALLOC
    bad = dev.Map(shape[0], shape[1], shape[2], shape[3], flags=flags)
    assert outer.set_inner(2, bad) == 0
    vm = dev.VM()
    vm.load(counter_prog("raw", outer.fd, False))
    units = make_units(65, 2, 2, 2)  # no unit even selects the slot
    d, out = dev.DeviceBuffer.from_array(units), dev.DeviceBuffer.from_array(np.full(65, 0x5A5A, np.uint64))
    snaps = [m.snapshot() for m, _ in inner] + [bad.snapshot()]
    want = rf"ARRAY_OF_MAPS map fd {outer.fd} slot 2 holds map fd {bad.fd} of type {shape[0]}\b"
    with pytest.raises(dev.EbpfError, match=want):
        vm.exec_batch(dev.CTX_RAW, d, 65, 64, fixed_len=64, rets=out,
                      flags=dev.BATCH_SYNC | (dev.BATCH_ORDERED if ordered else 0))
    assert (out.download(np.uint64) == 0x5A5A).all()  # nothing was launched
    for m, s in zip([m for m, _ in inner] + [bad], snaps):
        np.testing.assert_array_equal(m.snapshot(), s)
    assert outer.set_inner(2, 0) == 0  # the slot emptied: the launch runs
    assert vm.exec_batch(dev.CTX_RAW, d, 65, 64, fixed_len=64, rets=out) == 0


# ---- (g) a unit sees its own add --------------------------------------------------------
@pytest.mark.parametrize("n,stack_keys", [(64, True), (65, False)], ids=["64-stackkeys", "65"])
def test_own_add_is_visible(fresh_oracle, fresh_runtime, n, stack_keys):
    """Each unit has an element to itself (slot i % 4, key i // 4 of an inner
    map of 17 entries), adds its u64 and loads the word back: after - before
    is its own addend, in a parallel batch too."""
    po, dev = fresh_oracle, fresh_runtime
    outer, model = dev.Map(AOM, 4, 4, 4), mm.Outer(4)
    po.OracleMap(ARRAY, 4, 4, 1, fd=outer.fd)
    inner = []
    for i in range(4):
        m = dev.Map(ARRAY, 4, 8, 17)
        inner.append((m, po.OracleMap(ARRAY, 4, 8, 17, fd=m.fd)))
        assert outer.set_inner(i, m) == 0 and model.update(u32(i), struct.pack("<i", m.fd)) == 0
    units = make_units(n, 21, 1, 1)
    w = units.view(np.uint32).reshape(n, 16)
    w[:, 0], w[:, 1] = np.arange(n) % 4, np.arange(n) // 4
    got, want = run_both(dev, po, counter_prog("raw", outer.fd, stack_keys, readback=True), units, {outer.fd: model})
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, units.view(np.uint64).reshape(n, 8)[:, 2])
    same_inner(inner)


# ---- (h) the syscall dispatch --------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_syscall_dispatch(fresh_oracle, fresh_runtime, n):
    """A sys_enter program: inner = outer[(u32)args[0]], v = inner[(u32)args[1]],
    v[0] += 1; the keys are read in place from the record."""
    po, dev = fresh_oracle, fresh_runtime
    outer, model, inner = array_world(dev, po)
    a = Asm().mov64(6, "r1")
    a.ld_map_fd(1, outer.fd).mov64(2, "r6").add64(2, 16).call(1).jmp("jeq", 0, 0, "out")
    a.mov64(1, "r0").mov64(2, "r6").add64(2, 24).call(1).jmp("jeq", 0, 0, "out")
    a.mov64(2, 1).atomic(8, 0x00, 0, 0, 2)
    a.label("out").mov64(0, 0).exit()
    code = a.assemble()
    rng = np.random.default_rng(n)
    recs = np.zeros((n, 8), dtype=np.uint64)
    recs[:, 1] = 1
    recs[:, 2], recs[:, 3] = rng.integers(0, 6, n), rng.integers(0, 9, n)
    if n == 1:
        recs[0, 2:4] = (1, 3)
    recs = recs.view(np.uint8).reshape(n, 64)
    dev.syscall_attach(dev.prog_create(code, "p", 5), -1, True)  # BPF_PROG_TYPE_TRACEPOINT
    ovm = po.OracleVM()
    cbs = mm.register(ovm, po, {outer.fd: model})
    ovm.load(code)
    assert po.lib().orc_sys_attach(ovm.h, -1, 1) > 0
    d, out = dev.DeviceBuffer.from_array(recs), dev.DeviceBuffer(8 * n)
    assert dev.syscall_dispatch(d, n, record_size=dev.SYSCALL_RECORD, out=out) == 0
    want = np.zeros(n, dtype=np.int64)
    assert po.lib().orc_sys_dispatch(recs.ctypes.data, n, 64, want.ctypes.data) >= 0
    np.testing.assert_array_equal(out.download(np.int64), want)
    same_inner(inner)
    assert any(om.raw().any() for _, om in inner)
    # a refused inner type refuses the dispatch too
    ring = dev.Map(isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 4096)
    assert outer.set_inner(3, ring) == 0
    snaps = [m.snapshot() for m, _ in inner]
    for plan in (dev.DISPATCH_THREADS, dev.DISPATCH_PROGRAMS):
        with pytest.raises(dev.EbpfError):
            dev.syscall_dispatch(d, n, record_size=dev.SYSCALL_RECORD, out=out, flags=dev.BATCH_SYNC | plan)
    for (m, _), s in zip(inner, snaps):
        np.testing.assert_array_equal(m.snapshot(), s)
    del cbs
