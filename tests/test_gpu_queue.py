"""BPF_MAP_TYPE_QUEUE / BPF_MAP_TYPE_STACK on the device: creation and host
KATs against the model (tests/_queue.py); ORDERED batches bit-exact against
the oracle interpreter running the same bytecode on the model; parallel
add-only, remove-only and peek-only batches; the launch-time refusals (which
return before any kernel launch) and the loader's routing."""
import ctypes as C
import errno
import importlib.util
import pathlib
import struct

import numpy as np
import pytest

from bpftime_amd import _lib, isa, programs
from bpftime_amd.isa import Asm
from bpftime_amd.object import BpfObject

import _elf

# (by path: the interpreter has a built-in module named _queue)
_spec = importlib.util.spec_from_file_location("_queue_model", pathlib.Path(__file__).with_name("_queue.py"))
_queue = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_queue)

pytestmark = pytest.mark.gpu

QUEUE, STACK, ARRAY = isa.BPF_MAP_TYPE_QUEUE, isa.BPF_MAP_TYPE_STACK, isa.BPF_MAP_TYPE_ARRAY
TYPES = [QUEUE, STACK]
FAIL = 0xFFFFFFFFFFFFFFFF
FAIL32 = 0xFFFFFFFF
ENOTSUP64 = (-95) & FAIL
PUSH, POP, PEEK = isa.BPF_FUNC_map_push_elem, isa.BPF_FUNC_map_pop_elem, isa.BPF_FUNC_map_peek_elem


def make(dev, type_, value_size, max_entries, key_size=0):
    m = dev.Map(type_, key_size, value_size, max_entries)
    return m, _queue.Ring(value_size, max_entries, lifo=type_ == STACK)


def same(m, model):
    """The device ring is the model's, byte for byte (head, tail, every slot
    with its pad bytes), and decodes to the model's elements, oldest first."""
    assert m.count() == model.count() == model.tail - model.head
    assert m.queue_items() == model.items
    np.testing.assert_array_equal(m.snapshot(), model.image())


def test_creation(fresh_runtime):
    dev = fresh_runtime
    for t in TYPES:
        for ks, vs, mx in [(0, 0, 4), (0, 4, 0), (4, 0, 0)]:
            with pytest.raises(dev.EbpfError):
                dev.Map(t, ks, vs, mx)
        for ks in (0, 4, 7):  # the key size is not looked at
            m = dev.Map(t, ks, 5, 3)
            assert m.storage_bytes() == 128 + 8 * 3 and not m.snapshot().any() and m.count() == 0
            a = _lib.BpfMapAttr()
            assert _lib.lib().bpftime_map_get_info(m.fd, C.byref(a), None, None) == 0
            assert (a.type, a.key_size, a.value_size, a.max_ents) == (t, ks, 5, 3)
            f = dev.Map.from_fd(m.fd)
            assert (f.type, f.value_size, f.max_entries) == (t, 5, 3)


@pytest.mark.parametrize("type_", TYPES)
@pytest.mark.parametrize("mx", [1, 3, 64])
def test_host_kats(fresh_runtime, type_, mx):
    """Every host entry point against the model after every step: return
    value, errno and the ring."""
    dev = fresh_runtime
    L = _lib.lib()
    for vs in (1, 4, 5, 8, 12, 40):
        m, model = make(dev, type_, vs, mx)
        rng = np.random.default_rng(vs * 100 + mx)
        nxt = lambda: rng.integers(0, 256, vs, dtype=np.uint8).tobytes()  # noqa: E731

        def push(v, flags=0):
            C.set_errno(0)
            buf = C.create_string_buffer(v, vs) if v is not None else None
            rc = L.bpftime_map_push_elem(m.fd, buf, flags)
            assert rc == model.push(v, flags)
            assert rc == 0 or C.get_errno() == model.err
            same(m, model)
            return rc

        def take(fn, mfn):
            C.set_errno(0)
            buf = C.create_string_buffer(vs)
            rc = fn(m.fd, buf)
            mrc, mv = mfn()
            assert rc == mrc
            if rc == 0:
                assert buf.raw[:vs] == mv
            else:
                assert C.get_errno() == model.err
            same(m, model)
            return rc

        pop = lambda: take(L.bpftime_map_pop_elem, model.pop)  # noqa: E731
        peek = lambda: take(L.bpftime_map_peek_elem, model.peek)  # noqa: E731

        assert pop() == -1 and peek() == -1 and C.get_errno() == errno.ENOENT
        for _ in range(mx):  # fill to capacity
            assert push(nxt()) == 0
        assert push(nxt()) == -1 and C.get_errno() == errno.E2BIG
        assert push(nxt(), 1) == -1 and C.get_errno() == errno.EINVAL  # BPF_NOEXIST
        assert push(None) == -1 and C.get_errno() == errno.EINVAL
        assert L.bpftime_map_pop_elem(m.fd, None) == -1 and C.get_errno() == errno.EINVAL
        assert L.bpftime_map_peek_elem(m.fd, None) == -1 and C.get_errno() == errno.EINVAL
        for _ in range(2 * mx + 1):  # BPF_EXIST evictions: head wraps past slot mx - 1 twice
            assert push(nxt(), isa.BPF_EXIST) == 0
        for _ in range(2 * mx + 1):  # pop / push pairs: both ends wrap
            assert peek() == 0 and pop() == 0 and push(nxt()) == 0
        # the generic operations
        key = C.create_string_buffer(8)
        C.set_errno(0)
        assert L.bpftime_map_get_next_key(m.fd, None, key) == -1 and C.get_errno() == errno.EINVAL
        assert m.lookup(b"\0" * 4) == model.lookup()[1]
        v = nxt()
        assert m.update(b"\0" * 4, v, 1) == model.update(v, 1) == -1 and C.get_errno() == errno.E2BIG  # full; flags not validated
        assert m.update(b"\0" * 4, v, isa.BPF_EXIST) == model.update(v, isa.BPF_EXIST) == 0
        same(m, model)
        assert L.bpftime_map_delete_elem(m.fd, None) == model.delete() == 0
        same(m, model)
        assert m.update(b"\0" * 4, v, 1) == model.update(v, 1) == 0  # not full: any flags
        same(m, model)
        # the bpf(2) pop path
        vp = C.create_string_buffer(vs)
        rc, _ = dev.sys_bpf(21, dev.attr_map_elem(m.fd, 0, C.addressof(vp)))  # BPF_MAP_LOOKUP_AND_DELETE_ELEM
        mrc, mv = model.pop()
        assert rc == mrc == 0 and vp.raw[:vs] == mv
        same(m, model)
        while model.count():  # drain to empty
            assert m.pop_value() == model.pop()[1]
        assert m.pop_value() is None and m.peek_value() is None and m.lookup(b"") is None
        C.set_errno(0)
        assert L.bpftime_map_delete_elem(m.fd, None) == -1 and C.get_errno() == errno.ENOENT
        assert m.count() == 0


def test_other_types_unchanged(fresh_runtime):
    dev = fresh_runtime
    L = _lib.lib()
    buf = C.create_string_buffer(8)
    for m in (dev.Map(ARRAY, 4, 8, 4), dev.Map(isa.BPF_MAP_TYPE_HASH, 4, 8, 4)):
        assert m.push(b"\0" * 8) == -95 and m.pop() == -95 and L.bpftime_map_peek_elem(m.fd, buf) == -95
    b = dev.Map(isa.BPF_MAP_TYPE_BLOOM_FILTER, 0, 8, 64)
    C.set_errno(0)
    assert b.push(b"\1" * 8, flags=2) == -1 and C.get_errno() == errno.EINVAL
    assert b.push(b"\1" * 8) == 0 and b.peek(b"\1" * 8)
    C.set_errno(0)
    assert b.pop() == -1 and C.get_errno() == errno.EOPNOTSUPP
    assert L.bpftime_map_peek_elem(b.fd, None) == -1 and C.get_errno() == errno.EINVAL
    assert dev.sys_bpf(21, dev.attr_map_elem(b.fd, 0, C.addressof(buf)))[0] == -errno.ENOTSUP


# ---- ORDERED parity ---------------------------------------------------------
def mixed_prog(kind, base, qfd, afd):
    """Per unit {u32 index at base, u8 op at base + 4, value bytes from base +
    5 (an odd offset), a u64 at base + 16}: one of eight operations on the
    map, then {the value buffer, r0} stored into arr[index]; returns r0."""
    a = Asm()
    if kind == "xdp":
        a.ldx(8, 6, 1, 0)
    else:
        a.mov64(6, "r1")
    a.ldx(4, 7, 6, base).ldx(1, 8, 6, base + 4)
    a.stx(4, 10, -4, "r7").st(8, 10, -16, 0)
    for op in range(1, 8):
        a.jmp("jeq", 8, op, f"op{op}")
    pkt = lambda r: a.mov64(r, "r6").add64(r, base + 5)  # noqa: E731
    stk = lambda r, off: a.mov64(r, "r10").add64(r, off)  # noqa: E731
    # 0: push from the packet, flags 0
    a.ld_map_fd(1, qfd)
    pkt(2)
    a.mov64(3, 0).call(PUSH).ja("store")
    a.label("op1")  # push from the stack, BPF_EXIST
    a.ldx(8, 2, 6, base + 16).stx(8, 10, -16, "r2").ld_map_fd(1, qfd)
    stk(2, -16)
    a.mov64(3, isa.BPF_EXIST).call(PUSH).ja("store")
    a.label("op2").ld_map_fd(1, qfd)  # pop
    stk(2, -16)
    a.call(POP).ja("store")
    a.label("op3").ld_map_fd(1, qfd)  # peek
    stk(2, -16)
    a.call(PEEK).ja("store")
    a.label("op4").ld_map_fd(1, qfd)  # lookup: a pointer to the head / top
    stk(2, -4)
    a.call(isa.BPF_FUNC_map_lookup_elem).jmp("jeq", 0, 0, "store")
    a.ldx(8, 2, 0, 0).stx(8, 10, -16, "r2").mov64(0, 1).ja("store")
    a.label("op5").ld_map_fd(1, qfd)  # update from the packet, flags 1 (not validated)
    stk(2, -4)
    pkt(3)
    a.mov64(4, 1).call(isa.BPF_FUNC_map_update_elem).ja("store")
    a.label("op6").ld_map_fd(1, qfd)  # delete
    stk(2, -4)
    a.call(3).ja("store")
    a.label("op7").ld_map_fd(1, qfd)  # push with invalid flags
    pkt(2)
    a.mov64(3, 5).call(PUSH)
    a.label("store").mov64(9, "r0").ld_map_fd(1, afd)
    stk(2, -4)
    a.call(isa.BPF_FUNC_map_lookup_elem).jmp("jeq", 0, 0, "out")
    a.ldx(8, 2, 10, -16).stx(8, 0, 0, "r2").stx(8, 0, 8, "r9")
    a.label("out").mov64(0, "r9").exit()
    return a.assemble()


@pytest.mark.parametrize("type_", TYPES)
@pytest.mark.parametrize("mx", [3, 64])
@pytest.mark.parametrize("kind", ["xdp", "raw", "syscall"])
def test_ordered_parity(fresh_oracle, fresh_runtime, type_, mx, kind):
    po, dev = fresh_oracle, fresh_runtime
    n, base = 130, 16 if kind == "syscall" else 0
    q, model = make(dev, type_, 8, mx)
    arr = dev.Map(ARRAY, 4, 16, n)
    oarr = po.OracleMap(ARRAY, 4, 16, n, fd=arr.fd)
    po.OracleMap(ARRAY, 4, 4, 1, fd=q.fd)  # makes the lddw resolve
    rng = np.random.default_rng(mx * 7 + type_)
    units = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    if kind == "syscall":
        units[:, :16] = 0
        units[:, 8] = 1  # the syscall id: never exit / exit_group
    units[:, base:base + 4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    # pushes dominate first, so a ring of 64 fills; then every operation
    units[:, base + 4] = np.where(np.arange(n) < 70, rng.choice([0, 0, 1, 5, 3, 4], n), rng.integers(0, 8, n))
    code = mixed_prog(kind, base, q.fd, arr.fd)
    ovm = po.OracleVM()
    cbs = _queue.register(ovm, po, {q.fd: model})
    ovm.load(code)
    vm = dev.VM()
    vm.load(code)
    assert vm.info()["big_stack"]  # the scratch-stack kernels carry the helpers
    d = dev.DeviceBuffer.from_array(units)
    flags = dev.BATCH_SYNC | dev.BATCH_ORDERED
    if kind == "xdp":
        out = dev.DeviceBuffer(4 * n)
        assert vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=64, verdicts=out, flags=flags) == 0
        got, want = out.download(np.uint32), ovm.run_xdp(units.copy(), fixed_len=64)
    else:
        out = dev.DeviceBuffer(8 * n)
        ck = dev.CTX_SYSCALL if kind == "syscall" else dev.CTX_RAW
        assert vm.exec_batch(ck, d, n, 64, fixed_len=64, rets=out, flags=flags) == 0
        got = out.download(np.uint64)
        want = ovm.run_syscall(units.copy())[0] if kind == "syscall" else ovm.run_raw(units.copy(), 64)
    np.testing.assert_array_equal(got, want)
    assert len(set(int(x) & 0xFFFFFFFF for x in want)) >= 3  # successes, failures and a found lookup
    np.testing.assert_array_equal(arr.snapshot(), oarr.raw())  # every popped / peeked value and r0
    same(q, model)
    assert model.count() > 0
    del cbs


# ---- parallel batches -------------------------------------------------------
def push_prog(fds, value_size=8):
    """XDP: push the value at packet offset 5 (odd) onto the map the packet's
    byte 4 bit 0 picks among `fds`; returns the helper's r0."""
    a = Asm().ldx(8, 6, 1, 0).ld_map_fd(1, fds[0])
    if len(fds) > 1:
        a.ldx(1, 2, 6, 4).alu64("and", 2, 1).jmp("jeq", 2, 0, "go").ld_map_fd(1, fds[1]).label("go")
    a.mov64(2, "r6").add64(2, 5).mov64(3, 0).call(PUSH).exit()
    return a.assemble()


def index_packets(n, value_size=8):
    pk = np.zeros((n, 64), dtype=np.uint8)
    pk[:, 12] = 0x08
    vals = []
    for i in range(n):
        v = struct.pack("<I", 0xA5000000 | i) + bytes([(7 * i + j) & 0xFF for j in range(value_size - 4)])
        pk[i, 5:5 + value_size] = np.frombuffer(v, dtype=np.uint8)
        vals.append(v)
    return pk, vals


def run_xdp(dev, code, pk, flags=None):
    vm = dev.VM()
    vm.load(code)
    n = pk.shape[0]
    d = dev.DeviceBuffer.from_array(pk)
    dv = dev.DeviceBuffer(4 * n)
    kw = {} if flags is None else {"flags": flags}
    assert vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=64, verdicts=dv, **kw) == 0
    np.testing.assert_array_equal(d.download().reshape(pk.shape), pk)  # the packets are unmodified
    return dv.download(np.uint32)


def drain(m):
    out = []
    while True:
        v = m.pop_value()
        if v is None:
            return out
        out.append(v)


@pytest.mark.parametrize("type_", TYPES)
@pytest.mark.parametrize("n", [64, 65, 130])
def test_parallel_add_only(fresh_runtime, type_, n):
    dev = fresh_runtime
    for cap, vs in [(200, 8), (130, 5), (37, 12)]:
        m, _ = make(dev, type_, vs, cap)
        pk, vals = index_packets(n, vs)
        got = run_xdp(dev, push_prog([m.fd], vs), pk)
        assert set(np.unique(got)) <= {0, FAIL32}
        ok = [vals[i] for i in range(n) if got[i] == 0]
        assert len(ok) == min(n, cap)
        assert m.count() == min(n, cap)
        assert sorted(m.queue_items()) == sorted(ok)  # exactly the values of the units that got 0
        assert sorted(drain(m)) == sorted(ok) and m.count() == 0


@pytest.mark.parametrize("type_", TYPES)
def test_parallel_two_maps(fresh_runtime, type_):
    """The lanes of a wave split between two maps by a packet bit."""
    dev = fresh_runtime
    n = 130
    m1, _ = make(dev, type_, 8, 37)
    m2, _ = make(dev, STACK if type_ == QUEUE else QUEUE, 8, 200)
    pk, vals = index_packets(n)
    pk[:, 4] = (np.arange(n) * 5 // 3) & 1
    got = run_xdp(dev, push_prog([m1.fd, m2.fd]), pk)
    for m, bit, cap in ((m1, 0, 37), (m2, 1, 200)):
        mine = [i for i in range(n) if pk[i, 4] == bit]
        ok = [vals[i] for i in mine if got[i] == 0]
        assert len(ok) == min(len(mine), cap) == m.count()
        assert sorted(m.queue_items()) == sorted(ok)


@pytest.mark.parametrize("type_", TYPES)
def test_parallel_add_preloaded(fresh_runtime, type_):
    """A map the host pre-loaded, its head not at slot 0: the batch's pushes
    wrap past the last slot."""
    dev = fresh_runtime
    m, model = make(dev, type_, 8, 10)
    for i in range(5):
        v = bytes([0xEE, i]) + bytes(6)
        assert m.push(v) == 0 and model.push(v) == 0
    for _ in range(3):
        assert m.pop_value() == model.pop()[1]
    if type_ == STACK:  # a stack pops at the tail: move its bottom off slot 0 too
        for i in range(9):
            v = bytes([0xDD, i]) + bytes(6)
            assert m.push(v, isa.BPF_EXIST) == 0 and model.push(v, isa.BPF_EXIST) == 0
        for _ in range(8):
            assert m.pop_value() == model.pop()[1]
    head = int(m.snapshot()[:8].view(np.uint64)[0])
    assert head % 10 != 0 and model.count() == 2
    pk, vals = index_packets(130)
    got = run_xdp(dev, push_prog([m.fd]), pk)
    ok = [vals[i] for i in range(130) if got[i] == 0]
    assert len(ok) == 8 and m.count() == 10
    items = m.queue_items()
    assert items[:2] == model.items and sorted(items[2:]) == sorted(ok)


def pop_prog(fd, helper=POP):
    """Raw: pop (or peek) a u32 into the stack; returns it, or -1 on failure."""
    a = Asm().st(8, 10, -8, 0).ld_map_fd(1, fd).mov64(2, "r10").add64(2, -8).call(helper)
    a.jmp("jne", 0, 0, "out").ldx(4, 0, 10, -8).label("out").exit()
    return a.assemble()


def run_raw(dev, code, n, flags=None):
    units = np.arange(n * 8, dtype=np.uint64).view(np.uint8).reshape(n, 64)
    vm = dev.VM()
    vm.load(code)
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * n)
    kw = {} if flags is None else {"flags": flags}
    assert vm.exec_batch(dev.CTX_RAW, d, n, 64, fixed_len=64, rets=dr, **kw) == 0
    return dr.download(np.uint64)


@pytest.mark.parametrize("type_", TYPES)
@pytest.mark.parametrize("k", [0, 37, 130, 200])
def test_parallel_remove_only(fresh_runtime, type_, k):
    dev = fresh_runtime
    m, model = make(dev, type_, 4, 256)
    for i in range(3):  # head off slot 0
        assert m.push(struct.pack("<I", i)) == 0 and model.push(struct.pack("<I", i)) == 0
    for i in range(3):
        assert m.pop_value() == model.pop()[1]
    for i in range(k):
        v = struct.pack("<I", 1000 + i)
        assert m.push(v) == 0 and model.push(v) == 0
    got = run_raw(dev, pop_prog(m.fd), 130)
    won = sorted(int(x) for x in got if x != FAIL)
    take = min(130, k)
    assert len(won) == take and len(set(won)) == take
    want = [struct.unpack("<I", model.pop()[1])[0] for _ in range(take)]  # the oldest / the newest
    assert won == sorted(want)
    same(m, model)  # what remains, in order


@pytest.mark.parametrize("type_", TYPES)
def test_parallel_remove_by_delete(fresh_runtime, type_):
    dev = fresh_runtime
    m, model = make(dev, type_, 4, 64)
    for i in range(50):
        v = struct.pack("<I", i)
        m.push(v), model.push(v)
    a = Asm().ld_map_fd(1, m.fd).mov64(2, "r10").add64(2, -8).call(3).exit()
    got = run_raw(dev, a.assemble(), 65)
    assert int((got == 0).sum()) == 50 and int((got == FAIL).sum()) == 15 and m.count() == 0


@pytest.mark.parametrize("type_", TYPES)
def test_parallel_peek_only(fresh_runtime, type_):
    dev = fresh_runtime
    m, model = make(dev, type_, 4, 8)
    assert (run_raw(dev, pop_prog(m.fd, PEEK), 130) == FAIL).all()  # empty
    for i in range(5):
        v = struct.pack("<I", 70 + i)
        m.push(v), model.push(v)
    before = m.snapshot().copy()
    top = struct.unpack("<I", model.peek()[1])[0]
    assert (run_raw(dev, pop_prog(m.fd, PEEK), 130) == top).all()
    a = Asm().ld_map_fd(1, m.fd).mov64(2, "r10").add64(2, -8).call(isa.BPF_FUNC_map_lookup_elem)
    a.jmp("jeq", 0, 0, "out").ldx(4, 0, 0, 0).label("out").exit()
    assert (run_raw(dev, a.assemble(), 130) == top).all()
    np.testing.assert_array_equal(m.snapshot(), before)


# ---- the launch rule (every refusal returns before any kernel launch) -------
def test_launch_refusals(fresh_runtime):
    dev = fresh_runtime
    q, _ = make(dev, QUEUE, 8, 16)
    s, _ = make(dev, STACK, 8, 16)
    units = np.zeros((4, 64), dtype=np.uint8)
    d = dev.DeviceBuffer.from_array(units)

    def launch(code, flags=dev.BATCH_SYNC):
        vm = dev.VM()
        vm.load(code)
        assert vm.info()["big_stack"]
        return vm.exec_batch(dev.CTX_RAW, d, 4, 64, fixed_len=64, flags=flags)

    val = lambda a: a.mov64(2, "r10").add64(2, -8)  # noqa: E731
    mixed = Asm().st(8, 10, -8, 0).ld_map_fd(1, q.fd)
    val(mixed).mov64(3, 0).call(PUSH).ld_map_fd(1, q.fd)
    val(mixed).call(POP).exit()
    with pytest.raises(dev.EbpfError, match=rf"bpf_map_pop_elem on QUEUE map fd {q.fd} beside bpf_map_push_elem.*"
                                            r"add-only.*remove-only.*peek-only.*EBPF_BATCH_ORDERED"):
        launch(mixed.assemble())
    assert launch(mixed.assemble(), dev.BATCH_SYNC | dev.BATCH_ORDERED) == 0
    assert q.count() == 0  # four pushes, four pops

    exist = Asm().st(8, 10, -8, 0).ld_map_fd(1, s.fd)
    val(exist).mov64(3, isa.BPF_EXIST).call(PUSH).exit()
    with pytest.raises(dev.EbpfError, match=rf"bpf_map_push_elem on STACK map fd {s.fd} with flags not proven 0"):
        launch(exist.assemble())
    unproven = Asm().st(8, 10, -8, 0).ldx(8, 4, 1, 0).ld_map_fd(1, s.fd)
    val(unproven).mov64(3, "r10").add64(3, -8).call(isa.BPF_FUNC_map_update_elem).exit()
    with pytest.raises(dev.EbpfError, match=rf"bpf_map_update_elem on STACK map fd {s.fd} with flags not proven 0"):
        launch(unproven.assemble())

    peek_pop = Asm().ld_map_fd(1, s.fd)  # lookup (a peek) beside delete (a pop)
    val(peek_pop).call(isa.BPF_FUNC_map_lookup_elem).ld_map_fd(1, s.fd)
    val(peek_pop).call(3).exit()
    with pytest.raises(dev.EbpfError, match=rf"bpf_map_delete_elem on STACK map fd {s.fd} beside bpf_map_lookup_elem"):
        launch(peek_pop.assemble())

    blind = Asm().st(8, 10, -8, 0).mov64(1, q.fd)  # the fd as a plain number
    val(blind).mov64(3, 0).call(PUSH).exit()
    with pytest.raises(dev.EbpfError, match=r"bpf_map_push_elem on a map fd the loader cannot resolve"):
        launch(blind.assemble())

    # two maps, one kind each: accepted
    two = Asm().st(8, 10, -8, 0).ld_map_fd(1, q.fd)
    val(two).mov64(3, 0).call(PUSH).ld_map_fd(1, s.fd)
    val(two).call(POP).mov64(0, 0).exit()
    assert launch(two.assemble()) == 0 and q.count() == 4


def test_dispatch_refusal(fresh_runtime):
    dev = fresh_runtime
    q, _ = make(dev, QUEUE, 4, 64)
    a = Asm().mov64(2, "r1").add64(2, 8).ld_map_fd(1, q.fd).mov64(3, 0).call(PUSH).mov64(0, 0).exit()
    pfd = dev.prog_create(a.assemble(), "q_ids", 5)  # BPF_PROG_TYPE_TRACEPOINT
    assert dev.syscall_attach(pfd, -1) > 0
    recs = np.zeros((8, 64), dtype=np.uint8)
    recs[:, 8] = np.arange(1, 9)
    d = dev.DeviceBuffer.from_array(recs)
    with pytest.raises(dev.EbpfError, match="QUEUE / STACK"):
        dev.syscall_dispatch(d, 8, dev.SYSCALL_RECORD)
    assert q.count() == 0
    assert dev.syscall_dispatch(d, 8, dev.SYSCALL_RECORD, flags=dev.BATCH_SYNC | dev.BATCH_ORDERED) == 0
    assert [struct.unpack("<I", v)[0] for v in q.queue_items()] == list(range(1, 9))  # record order


# ---- the demo programs, from an ELF object ----------------------------------
def demo_object(code, maps) -> bytes:
    """`code` (its map lddws at the pcs maps[name][3]) in section xdp, with
    BTF-defined maps {name: (type, value bytes, max_entries, [pcs])}."""
    b = _elf.Btf()
    u32 = b.int_("unsigned int", 4)
    i32 = b.int_("int", 4, signed=True)
    u64 = b.int_("unsigned long long", 8)
    e = _elf.Elf()
    e.section("xdp", code, flags=_elf.SHF_ALLOC | _elf.SHF_EXECINSTR)
    e.section(".maps", bytes(32 * len(maps)), flags=_elf.SHF_ALLOC | _elf.SHF_WRITE)
    secinfo = []
    for k, (name, (t, vs, mx, pcs)) in enumerate(maps.items()):
        p = {nm: b.ptr(b.array(i32, i32, v)) for nm, v in [("type", t), ("max_entries", mx)]}
        members = [("type", p["type"], 0), ("value", b.ptr(u64 if vs == 8 else u32), 64),
                   ("max_entries", p["max_entries"], 128)]
        if t == ARRAY:
            members.append(("key", b.ptr(u32), 192))
        secinfo.append((b.var(name, b.struct_("", 32, members)), 32 * k, 32))
        e.symbol(name, ".maps", 32 * k, 32)
    b.func("prog", b.func_proto(i32, [("ctx", b.ptr(u32))]))
    b.datasec(".maps", 32 * len(maps), secinfo)
    e.section("license", b"GPL\0", flags=_elf.SHF_ALLOC | _elf.SHF_WRITE, align=1)
    e.section(".BTF", b.encode(), align=4)
    e.section(".BTF.ext", _elf.btf_ext(b, []), align=4)
    e.symbol("prog", "xdp", 0, len(code), type_=_elf.STT_FUNC)
    e.symbol("_license", "license", 0, 4)
    for name, (_, _, _, pcs) in maps.items():
        for pc in pcs:
            e.reloc("xdp", pc * 8, name)
    return e.encode()


def lddw_pcs(code, fd):
    """The pcs of the lddw instructions that name map `fd`."""
    out = []
    for pc in range(len(code) // 8):
        op, regs, _, imm = struct.unpack_from("<BBhi", code, 8 * pc)
        if op == 0x18 and regs >> 4 == 1 and imm == fd:
            out.append(pc)
    return out


def test_demo_queue_sample(fresh_runtime):
    dev = fresh_runtime
    code = programs.queue_sample(900)
    o = BpfObject.from_bytes(demo_object(code, {"samples": (QUEUE, 8, 100, lddw_pcs(code, 900))}), "qs")
    o.load()
    q = dev.Map.from_fd(o.map_fd("samples"))
    assert (q.type, q.value_size, q.max_entries) == (QUEUE, 8, 100)
    vm = dev.prog_instantiate(o.program_fd("prog"))
    n = 130
    pk = np.zeros((n, 64), dtype=np.uint8)
    pk[:, 12] = 0x08
    pk[:, 26:30] = (np.arange(n, dtype=np.uint32) + 0x0A000000).view(np.uint8).reshape(n, 4)
    pk[3::7, 12] = 0x86  # not IPv4: passes, no sample
    d = dev.DeviceBuffer.from_array(pk)
    dv = dev.DeviceBuffer(4 * n)
    assert vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=64, verdicts=dv) == 0
    got = dv.download(np.uint32)
    ipv4 = pk[:, 12] == 0x08
    assert (got[~ipv4] == isa.XDP_PASS).all()
    assert int((got[ipv4] == 0).sum()) == 100 and int((got[ipv4] == FAIL32).sum()) == int(ipv4.sum()) - 100
    recs = sorted(struct.unpack("<II", v) for v in drain(q))
    assert recs == sorted((0x0A000000 + i, 64) for i in range(n) if ipv4[i] and got[i] == 0)


def test_demo_stack_take_id(fresh_runtime):
    dev = fresh_runtime
    code = programs.stack_take_id(900, 901)
    obj = demo_object(code, {"ids": (STACK, 4, 64, lddw_pcs(code, 900)),
                             "slots": (ARRAY, 4, 130, lddw_pcs(code, 901))})
    o = BpfObject.from_bytes(obj, "take")
    o.load()
    s, arr = dev.Map.from_fd(o.map_fd("ids")), dev.Map.from_fd(o.map_fd("slots"))
    for i in range(40):
        assert s.push(struct.pack("<I", 500 + i)) == 0
    vm = dev.prog_instantiate(o.program_fd("prog"))
    n = 130
    pk = np.zeros((n, 64), dtype=np.uint8)
    pk[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    d = dev.DeviceBuffer.from_array(pk)
    dv = dev.DeviceBuffer(4 * n)
    assert vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=64, verdicts=dv) == 0
    got = dv.download(np.uint32)
    assert int((got == isa.XDP_PASS).sum()) == 40 and int((got == isa.XDP_DROP).sum()) == 90
    slots = arr.snapshot().view(np.uint32)
    assert sorted(int(x) for x in slots[got == isa.XDP_PASS]) == list(range(500, 540))  # each id to one unit
    assert not slots[got == isa.XDP_DROP].any() and s.count() == 0
