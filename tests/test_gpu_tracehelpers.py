"""bpf_trace_printk (6), bpf_get_current_uid_gid / _comm (15 / 16),
bpf_probe_write_user (36) and bpf_ktime_get_boot_ns / _coarse_ns (125 / 160)
on the device against the Python model (tests/_tracehelpers.py, itself
checked against libc): shapes of 1, 63, 64, 65 and 130 units -- a lone lane,
the wave boundary, a lone last lane, three waves with a partial one.

Every batch lies inside a larger device buffer whose slack bytes hold a
sentinel, so an address just outside the batch is mapped memory: a wrong
guard shows as a wrong value, never as a fault.  Map values are reached
through map-value lddws."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from bpftime_amd import gen, isa, programs
from bpftime_amd.isa import Asm

import _tracehelpers as th

pytestmark = pytest.mark.gpu

ARRAY, HASH = isa.BPF_MAP_TYPE_ARRAY, isa.BPF_MAP_TYPE_HASH
STRIDE, SLACK, SENTINEL, CANARY = 128, 256, 0x5A, 0xAA
NS = [1, 63, 64, 65, 130]
M64 = th.M64
EFAULT, EINVAL = th.EFAULT, th.EINVAL
PRINTK, UIDGID, COMM, WRITE, BOOT, COARSE = 6, 15, 16, 36, 125, 160
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def drained(fresh_runtime):
    """bpf_trace_printk enabled (a runtime reset turns it off again) and an
    empty trace log (it outlives a reset)."""
    fresh_runtime.enable_trace_printk()
    while True:
        r = fresh_runtime.trace_read()
        if r is None or (not r[0] and not r[1]):
            break
    yield


def stack_bytes(a, off, data, tmp=9):
    """data (padded to 8s) at r10 + off."""
    data = data + bytes(-len(data) % 8)
    for i in range(0, len(data), 8):
        a.lddw(tmp, int.from_bytes(data[i:i + 8], "little")).stx(8, 10, off + i, f"r{tmp}")
    return a


def run(dev, vm, units, ordered=False, kind="raw", sync=True, **kw):
    """-> (r0 per unit, the units afterwards); the slack keeps its sentinel."""
    n = units.shape[0]
    host = np.full(2 * SLACK + n * STRIDE, SENTINEL, dtype=np.uint8)
    host[SLACK:SLACK + n * STRIDE] = units.reshape(-1)
    d = dev.DeviceBuffer.from_array(host)
    flags = (dev.BATCH_SYNC if sync else 0) | (dev.BATCH_ORDERED if ordered else 0)
    if kind == "xdp":
        out = dev.DeviceBuffer(4 * n)
        failed = vm.exec_batch(dev.CTX_XDP, d, n, STRIDE, fixed_len=STRIDE, verdicts=out, flags=flags,
                               data_offset=SLACK, **kw)
        dt = np.uint32
    else:
        out = dev.DeviceBuffer(8 * n)
        failed = vm.exec_batch(dev.CTX_RAW, d, n, STRIDE, fixed_len=STRIDE, rets=out, flags=flags,
                               data_offset=SLACK, **kw)
        dt = np.uint64
    assert failed == 0
    if not sync:
        return out, d, dt
    return finish(out, d, dt, n)


def finish(out, d, dt, n):
    got = out.download(dt).astype(np.uint64)
    after = d.download()
    assert (after[:SLACK] == SENTINEL).all() and (after[SLACK + n * STRIDE:] == SENTINEL).all()
    return got, after[SLACK:SLACK + n * STRIDE].reshape(n, STRIDE)


def load(dev, code, big=True):
    vm = dev.VM()
    rc, msg = vm.try_load(code)
    assert rc == 0, msg
    assert vm.info()["big_stack"] == big
    return vm


def lines_by_unit(dev):
    lines, lost = dev.trace_read()
    assert lost == 0
    return sorted(lines, key=lambda l: l[0]), lines


# ---- load ----------------------------------------------------------------------------
@pytest.mark.parametrize("helper", [PRINTK, UIDGID, COMM, WRITE, BOOT, COARSE])
def test_every_new_id_loads(fresh_runtime, helper):
    dev = fresh_runtime
    a = Asm().st(8, 10, -8, 0).st(8, 10, -16, 0).mov64(1, "r10").add64(1, -8)
    if helper == WRITE:
        a.mov64(2, "r10").add64(2, -16).mov64(3, 8)
    else:
        a.mov64(2, 8).mov64(3, 0).mov64(4, 0).mov64(5, 0)
    vm = dev.VM()
    rc, msg = vm.try_load(a.call(helper).mov64(0, 0).exit().assemble())
    assert rc == 0, msg
    # the clocks stay with helper 5 (no scratch-stack instance); the rest sit beside helper_mem
    assert vm.info()["big_stack"] == (helper not in (BOOT, COARSE))
    pvm = dev.prog_instantiate(dev.prog_create(a.assemble(), "p", 2))
    out = dev.DeviceBuffer(8)
    u = np.zeros((1, 64), dtype=np.uint8)
    assert pvm.exec_batch(dev.CTX_RAW, dev.DeviceBuffer.from_array(u), 1, 64, fixed_len=64, rets=out) == 0


def test_printk_is_refused_until_enabled(fresh_runtime):
    """Off (the state after a reset) the helper is no default helper and a
    program that calls it is refused, naming it; VMs made while it is on load."""
    dev = fresh_runtime
    code = Asm().st(8, 10, -8, 0).mov64(1, "r10").add64(1, -8).mov64(2, 8).call(PRINTK).exit().assemble()
    assert dev.enable_trace_printk(False) is True          # (the fixture turned it on)
    rc, msg = dev.VM().try_load(code)
    assert rc == -22 and msg == "call to nonexistent function 6 at PC 4"
    vm = dev.VM()
    vm.register(6, "bpf_trace_printk")
    rc, msg = vm.try_load(code)
    assert rc == -22 and "helper 6 (bpf_trace_printk) has no device implementation" in msg
    assert dev.enable_trace_printk(True) is False
    assert dev.VM().try_load(code)[0] == 0
    dev.reset_runtime()
    assert dev.enable_trace_printk(True) is False           # a reset turned it off


# ---- 15 / 16 --------------------------------------------------------------------------
def identity_prog():
    """unit[0:8] = uid_gid, unit[8:24] = comm (16 bytes)."""
    a = Asm().mov64(6, "r1").call(UIDGID).stx(8, 6, 0, "r0")
    return a.mov64(1, "r6").add64(1, 8).mov64(2, 16).call(COMM).exit().assemble()


@pytest.mark.parametrize("n", NS)
def test_identity_defaults_and_two_vms(fresh_runtime, n):
    dev = fresh_runtime
    code = identity_prog()
    va, vb, vc = load(dev, code), load(dev, code), load(dev, code)
    va.set_task(comm=b"alpha", uid_gid=(7 << 32) | 8)
    vb.set_task(comm=b"sixteen-bytes-xyz-and-more", uid_gid=M64)
    units = np.full((n, STRIDE), CANARY, dtype=np.uint8)
    # back to back, no wait between the launches: each sees its own identity
    pend = [run(dev, v, units, sync=False) for v in (va, vb, vc)]
    want = [(b"alpha", (7 << 32) | 8), (b"sixteen-bytes-xyz-and-more", M64), (th.default_comm(), th.default_uid_gid())]
    for (out, d, dt), (comm, ug) in zip(pend, want):
        got, after = finish(out, d, dt, n)
        assert (got == 0).all()
        for u in after:
            assert bytes(u[:8]) == struct.pack("<Q", ug)
            assert bytes(u[8:24]) == th.get_current_comm(comm, 16)
            assert (u[24:] == CANARY).all()


COMM_NAME = b"worker-7"


@pytest.mark.parametrize("dst", ["stack", "map", "packet"])
@pytest.mark.parametrize("size", [0, 1, len(COMM_NAME), len(COMM_NAME) + 1, 16, 64])
def test_comm_sizes_and_destinations(fresh_runtime, dst, size):
    """The destination byte for byte, zero fill included, canaries on both
    sides untouched: 8 canary bytes, 64 of destination, 8 more, read back
    through unit bytes 16..96."""
    dev = fresh_runtime
    m = dev.Map(ARRAY, 4, 80, 1)
    m.update(b"\0" * 4, bytes([CANARY]) * 80)
    a = Asm().mov64(6, "r1")
    if dst == "stack":
        for i in range(10):
            stack_bytes(a, -80 + 8 * i, bytes([CANARY]) * 8)
        a.mov64(7, "r10").add64(7, -80)
    elif dst == "map":
        a.ld_map_value(7, m.fd, 0)
    else:
        a.mov64(7, "r6").add64(7, 16)
    a.mov64(1, "r7").add64(1, 8).mov64(2, size).call(COMM).stx(8, 6, 0, "r0")
    if dst != "packet":
        for i in range(10):
            a.ldx(8, 2, 7, 8 * i).stx(8, 6, 16 + 8 * i, "r2")
    vm = load(dev, a.ldx(8, 0, 6, 0).exit().assemble())
    vm.set_task(comm=COMM_NAME)
    want = bytes([CANARY]) * 8 + th.get_current_comm(COMM_NAME, size) + bytes([CANARY]) * (72 - size)
    for n in NS:
        got, after = run(dev, vm, np.full((n, STRIDE), CANARY, dtype=np.uint8))
        assert (got == 0).all()
        for u in after:
            assert bytes(u[16:96]) == want
            assert (u[96:] == CANARY).all()
    if dst == "map":
        assert m.lookup(b"\0" * 4) == want


@pytest.mark.parametrize("case", ["crosses_stack_top", "null", "huge", "past_batch"])
def test_comm_efault_writes_nothing(fresh_runtime, case):
    dev = fresh_runtime
    a = Asm().mov64(6, "r1")
    stack_bytes(a, -8, bytes([CANARY]) * 8)
    if case == "crosses_stack_top":
        a.mov64(1, "r10").add64(1, -4).mov64(2, 8)
    elif case == "null":
        a.mov64(1, 0).mov64(2, 8)
    elif case == "huge":
        a.mov64(1, "r10").add64(1, -8).lddw(2, 1 << 63)
    else:  # the last 4 bytes of the unit and 4 more: inside the batch except for the last unit
        a.mov64(1, "r6").add64(1, STRIDE - 4).mov64(2, 8)
    a.call(COMM).ldx(8, 2, 10, -8).stx(8, 6, 0, "r2").exit()
    vm = load(dev, a.assemble())
    for n in (1, 65):
        units = np.full((n, STRIDE), CANARY, dtype=np.uint8)
        got, after = run(dev, vm, units)
        want_r0 = np.full(n, EFAULT, dtype=np.uint64)
        want = units.copy()
        if case == "past_batch":   # only the last unit's range leaves the window
            want_r0[:-1] = 0
            c = th.get_current_comm(th.default_comm(), 8)
            for i in range(n - 1):
                want[i, STRIDE - 4:] = np.frombuffer(c[:4], np.uint8)
                want[i + 1, :4] = np.frombuffer(c[4:], np.uint8)
        np.testing.assert_array_equal(got, want_r0)
        if case == "past_batch":
            # (unit i + 1 stores its canary word over the bytes unit i wrote into it: either order)
            assert (after[:, 8:STRIDE - 4] == CANARY).all() and (after[-1, STRIDE - 4:] == CANARY).all()
            for i in range(n - 1):
                assert bytes(after[i, STRIDE - 4:]) == bytes(want[i, STRIDE - 4:])
        else:
            np.testing.assert_array_equal(after, want)


# ---- 36 ---------------------------------------------------------------------------------
def test_probe_write_user(fresh_runtime):
    """Per unit {src offset, dst offset, len} from its header (offset 0: a
    NULL pointer): congruent and incongruent alignments x lengths 0, 1, 7, 8,
    9, 33, overlap forward and backward by 3, a negative length, a bad source
    and a bad destination -- divergent lanes of one wave."""
    dev = fresh_runtime
    a = Asm().mov64(6, "r1")
    a.ldx(8, 1, 6, 8).jmp("jeq", 1, 0, "d0").alu64("add", 1, "r6").label("d0")
    a.ldx(8, 2, 6, 0).jmp("jeq", 2, 0, "s0").alu64("add", 2, "r6").label("s0")
    vm = load(dev, a.ldx(8, 3, 6, 16).call(WRITE).exit().assemble())
    rows = [(32 + sa, 80 + da, ln) for sa, da in ((0, 0), (3, 3), (1, 2), (5, 0)) for ln in (0, 1, 7, 8, 9, 33)]
    rows += [(40, 43, 20), (43, 40, 20), (32, 80, -1), (32, 80, -(1 << 63)), (0, 80, 8), (32, 0, 8),
             (32, 80, 1 << 40)]
    for n in NS:
        units = np.zeros((n, STRIDE), dtype=np.uint8)
        units[:, 24:] = (np.arange(n * (STRIDE - 24)) * 7 + 3).reshape(n, -1) & 0xff
        want = units.copy()
        want_r0 = np.zeros(n, dtype=np.uint64)
        for i in range(n):
            s, d, ln = rows[i % len(rows)]
            units[i, :24] = np.frombuffer(struct.pack("<QQq", s, d, ln), np.uint8)
            want[i, :24] = units[i, :24]
            last = i == n - 1
            bad = s == 0 or d == 0 or ln < 0 or max(s, d) + ln > (STRIDE if last else (n - i) * STRIDE)
            if ln == 0 and not ln < 0:
                continue
            if bad:
                want_r0[i] = EFAULT
                continue
            row = bytearray(want[i].tobytes())
            for k in range(ln):            # ascending bytes: the overlap contract
                row[d + k] = row[s + k]
            want[i] = np.frombuffer(bytes(row), np.uint8)
        got, after = run(dev, vm, units)
        np.testing.assert_array_equal(got, want_r0)
        np.testing.assert_array_equal(after, want)


# ---- 125 / 160 ----------------------------------------------------------------------------
def clocks_prog():
    """r0 = the clock when helpers 5, 125 and 160 agree, else 0."""
    a = Asm().call(isa.BPF_FUNC_ktime_get_ns).mov64(6, "r0").call(BOOT).mov64(7, "r0").call(COARSE)
    a.jmp("jne", 6, "r7", "no").jmp("jne", 7, "r0", "no").exit()
    return a.label("no").mov64(0, 0).exit().assemble()


@pytest.mark.parametrize("n", NS)
def test_clocks_replay_the_recorded_clock(fresh_runtime, n):
    dev = fresh_runtime
    vm = load(dev, clocks_prog(), big=False)
    recs = gen.syscall_records_timed(n, threads=3)
    out = dev.DeviceBuffer(8 * n)
    d = dev.DeviceBuffer.from_array(recs)
    assert vm.exec_batch(dev.CTX_SYSCALL, d, n, 128, rets=out, ktime_off=96) == 0
    np.testing.assert_array_equal(out.download(np.uint64), recs.view(np.uint64).reshape(n, 16)[:, 12])


@pytest.mark.parametrize("n", NS)
def test_clocks_without_a_replay(fresh_runtime, n):
    dev = fresh_runtime
    a = Asm().call(BOOT).mov64(6, "r0").call(COARSE).mov64(7, "r0").call(isa.BPF_FUNC_ktime_get_ns)
    a.jmp("jeq", 6, 0, "no").jmp("jgt", 6, "r7", "no").jmp("jgt", 7, "r0", "no").mov64(0, 1).exit()
    vm = load(dev, a.label("no").mov64(0, 0).exit().assemble(), big=False)
    got, _ = run(dev, vm, np.zeros((n, STRIDE), dtype=np.uint8))
    assert (got == 1).all()


@pytest.mark.parametrize("plan", ["programs", "threads_asm", "threads_cpp"])
def test_clocks_in_a_dispatch_on_both_tiers(fresh_runtime, plan, monkeypatch):
    """map[low 32 bits of the clock] = the clock when 5, 125 and 160 agree."""
    dev = fresh_runtime
    if plan != "programs":
        monkeypatch.setenv("BPFTIME_AMD_SEQ_ASM", "1" if plan == "threads_asm" else "0")
    m = dev.Map(HASH, 4, 8, 256)
    a = Asm().call(isa.BPF_FUNC_ktime_get_ns).mov64(6, "r0").call(BOOT).mov64(7, "r0").call(COARSE)
    a.jmp("jne", 6, "r7", "no").jmp("jne", 7, "r0", "no").ja("ok").label("no").mov64(6, 0).label("ok")
    a.stx(4, 10, -4, "r0").stx(8, 10, -16, "r6")
    a.ld_map_fd(1, m.fd).mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16).mov64(4, 0)
    code = a.call(isa.BPF_FUNC_map_update_elem).mov64(0, 0).exit().assemble()
    assert dev.syscall_attach(dev.prog_create(code, "clk", 5), -1, True) > 0
    n = 130
    recs = gen.syscall_records_timed(n, threads=3)
    w = recs.view(np.uint64).reshape(n, 16)
    w[:, 1] = np.array([0, 1, 57, 0, 1, 60, 231, 3, 202], np.uint64)[np.arange(n) % 9]
    flags = dev.BATCH_SYNC | (dev.DISPATCH_PROGRAMS if plan == "programs" else dev.DISPATCH_THREADS)
    assert dev.syscall_dispatch(dev.DeviceBuffer.from_array(recs), n, record_size=dev.SYSCALL_RECORD_TIMED,
                                flags=flags) == 0
    want = {struct.pack("<I", int(t) & 0xffffffff): struct.pack("<Q", int(t)) for i, t in zip(w[:, 1], w[:, 12])
            if int(i) not in (60, 231)}
    assert m.hash_items() == want


# ---- 6 --------------------------------------------------------------------------------------
FMT3 = b"%d %llx %s"


def printk3_prog(fmt=FMT3, odd_only=False, twice=False):
    """printk(fmt, unit word 0, unit u64 at 8, unit + 16); the format on the stack."""
    a = Asm().mov64(6, "r1")
    if odd_only:
        a.ldx(4, 2, 6, 0).alu64("and", 2, 1).jmp("jeq", 2, 0, "skip")
    stack_bytes(a, -96, fmt + b"\0")
    reps = [b"A", b"B"] if twice else [None]
    for tag in reps:
        if tag:
            a.st(1, 10, -96, tag[0])
        a.mov64(1, "r10").add64(1, -96).mov64(2, len(fmt) + 1)
        a.ldx(4, 3, 6, 0).ldx(8, 4, 6, 8).mov64(5, "r6").add64(5, 16).call(PRINTK)
    a.exit()
    if odd_only:
        a.label("skip").mov64(0, 99).exit()
    return a.assemble()


def units3(n):
    u = np.zeros((n, STRIDE), dtype=np.uint8)
    for i in range(n):
        s = b"unit-%d" % i + b"!" * (i % 5)
        u[i, :16] = np.frombuffer(struct.pack("<iIQ", i * 37 - 1000, 0, (i * 0x9E3779B97F4A7C15) & M64), np.uint8)
        u[i, 16:16 + len(s)] = np.frombuffer(s, np.uint8)
    return u


def want3(u, fmt=FMT3):
    flat = u.reshape(-1)
    out = []
    for i in range(u.shape[0]):
        w0, w1 = struct.unpack_from("<IQ", u[i].tobytes(), 0)[0], struct.unpack_from("<Q", u[i].tobytes(), 8)[0]
        cv = th.scan(fmt)
        s = th.capture_str(flat[i * STRIDE + 16:].tobytes(), cv[2].prec)
        out.append((i, th.format_line(fmt, [w0, w1, s])))
    return out


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("n", NS)
def test_printk_every_unit(fresh_runtime, n, ordered):
    dev = fresh_runtime
    vm = load(dev, printk3_prog())
    u = units3(n)
    got, _ = run(dev, vm, u, ordered=ordered)
    assert (got == 0).all()
    by_unit, raw = lines_by_unit(dev)
    assert by_unit == want3(u)
    if ordered:
        assert [l[0] for l in raw] == list(range(n))      # the sequential order itself
    assert dev.trace_read() == ([], 0)


def test_printk_first_unit_and_exec(fresh_runtime):
    dev = fresh_runtime
    vm = load(dev, printk3_prog())
    u = units3(3)
    run(dev, vm, u[1:], first_unit=1000)                  # the global unit index
    assert [l[0] for l in lines_by_unit(dev)[0]] == [1000, 1001]
    mem = bytearray(u[2].tobytes())
    assert vm.exec(mem) == (0, 0)                         # ebpf_exec of one unit
    (unit, line), = dev.trace_read()[0]
    assert unit == 0 and line == th.format_line(FMT3, [struct.unpack_from("<I", mem, 0)[0],
                                                        struct.unpack_from("<Q", mem, 8)[0], b"unit-2!!"])


@pytest.mark.parametrize("n", NS)
def test_printk_twice_keeps_a_units_order(fresh_runtime, n):
    dev = fresh_runtime
    fmt = b"X %d %llx %s"
    vm = load(dev, printk3_prog(fmt, twice=True))
    u = units3(n)
    run(dev, vm, u)
    lines, lost = dev.trace_read()
    assert lost == 0 and len(lines) == 2 * n
    wa, wb = dict(want3(u, b"A" + fmt[1:])), dict(want3(u, b"B" + fmt[1:]))
    seen = {}
    for unit, line in lines:
        seen.setdefault(unit, []).append(line)
    assert seen == {i: [wa[i], wb[i]] for i in range(n)}


@pytest.mark.parametrize("n", NS)
def test_printk_from_odd_units_only(fresh_runtime, n):
    dev = fresh_runtime
    vm = load(dev, printk3_prog(odd_only=True))
    u = units3(n)
    u[:, 0] = np.arange(n) & 0xff                         # word 0 = the index (low byte decides)
    got, _ = run(dev, vm, u)
    np.testing.assert_array_equal(got, np.where(np.arange(n) & 1, 0, 99).astype(np.uint64))
    assert lines_by_unit(dev)[0] == [w for w in want3(u) if w[0] & 1]


def test_printk_string_sources(fresh_runtime):
    """%s from the stack, the packet and a map value; NULL and wild pointers;
    a string cut by the cap, by the precision and by the packet's end."""
    dev = fresh_runtime
    m = dev.Map(ARRAY, 4, 64, 1)
    m.update(b"\0" * 4, b"from-a-map-value".ljust(64, b"\0"))
    fmt = b"%s|%s|%s"
    a = Asm().mov64(6, "r1")
    stack_bytes(a, -32, fmt + b"\0")
    stack_bytes(a, -64, b"on-the-stack\0")
    a.mov64(1, "r10").add64(1, -32).mov64(2, len(fmt) + 1)
    a.mov64(3, "r10").add64(3, -64).mov64(4, "r6").add64(4, 16).ld_map_value(5, m.fd, 0).call(PRINTK)
    a.mov64(1, "r10").add64(1, -32).mov64(2, len(fmt) + 1)
    a.mov64(3, 0).mov64(4, 0x10).mov64(5, "r6").add64(5, STRIDE - 3).call(PRINTK)       # NULL, wild, the unit's end
    stack_bytes(a, -32, b"%.5s|%-12.3s|%s\0")
    a.mov64(1, "r10").add64(1, -32).mov64(2, 16)
    a.mov64(3, "r6").add64(3, 16).mov64(4, "r6").add64(4, 16).mov64(5, "r6").add64(5, 64).call(PRINTK)
    vm = load(dev, a.exit().assemble())
    for n in (1, 65):
        u = np.zeros((n, STRIDE), dtype=np.uint8)
        u[:, 16:28] = np.frombuffer(b"in-the-pkt-0", np.uint8)
        u[:, 64:] = ord("z")                              # 64 bytes and no NUL: cut by the cap / the batch's end
        u[:, 0] = ord("n")                                # (the next unit starts with a non-NUL byte)
        got, _ = run(dev, vm, u)
        assert (got == 0).all()
        lines, lost = dev.trace_read()
        per = {}
        for unit, line in lines:
            per.setdefault(unit, []).append(line)
        for i in range(n):
            tail = b"zzz" if i == n - 1 else b"zzz" + b"n"    # the last unit's string ends with the batch
            pkt = b"in-the-pkt-0"
            assert per[i] == [th.format_line(fmt, [b"on-the-stack", pkt, b"from-a-map-value"]),
                              th.format_line(fmt, [th.NULL, th.EFAULTSTR, tail]),
                              th.format_line(b"%.5s|%-12.3s|%s", [pkt[:5], pkt[:3], b"z" * 47])], (i, per[i])
            assert per[i][1] == b"(null)|(efault)|" + tail and per[i][2].startswith(b"in-th|in-    ")


BAD = [(b"%*d", None, EINVAL), (b"%n", None, EINVAL), (b"%f", None, EINVAL), (b"%d%d%d%d", None, EINVAL),
       (b"tail%", None, EINVAL), (b"%q", None, EINVAL), (b"%65d", None, EINVAL), (b"%.65s", None, EINVAL),
       (b"ok %d", 0, EINVAL), (b"ok %d", 5, EINVAL), (b"k" * 96, 200, EINVAL), (b"k" * 95, 200, 0),
       (b"%64d|%.64x", None, 0)]


@pytest.mark.parametrize("fmt,size,want", BAD)
def test_printk_rejections_log_nothing(fresh_runtime, fmt, size, want):
    dev = fresh_runtime
    a = Asm()
    stack_bytes(a, -128, fmt + b"\0")
    a.mov64(1, "r10").add64(1, -128).mov64(2, len(fmt) + 1 if size is None else size)
    vm = load(dev, a.mov64(3, 1).mov64(4, 2).mov64(5, 3).call(PRINTK).exit().assemble())
    got, _ = run(dev, vm, np.zeros((65, STRIDE), dtype=np.uint8))
    assert (got == np.uint64(want)).all()
    lines, lost = dev.trace_read()
    assert lost == 0 and len(lines) == (65 if want == 0 else 0)
    if want == 0:
        assert {l[1] for l in lines} == {th.format_line(fmt, [1, 2, 3])}


@pytest.mark.parametrize("case", ["null", "wild", "runs_off_the_batch", "crosses_stack_top"])
def test_printk_format_efault(fresh_runtime, case):
    dev = fresh_runtime
    a = Asm().mov64(6, "r1")
    stack_bytes(a, -8, b"abcdefgh")
    if case == "null":
        a.mov64(1, 0)
    elif case == "wild":
        a.mov64(1, 0x1000)
    elif case == "runs_off_the_batch":
        a.mov64(1, "r6").add64(1, STRIDE - 4)
    else:
        a.mov64(1, "r10").add64(1, -8)                    # 8 bytes, no NUL before the stack's top
    vm = load(dev, a.mov64(2, 64).call(PRINTK).exit().assemble())
    u = np.full((1, STRIDE), ord("f"), dtype=np.uint8)
    got, _ = run(dev, vm, u)
    assert int(got[0]) == EFAULT
    assert dev.trace_read() == ([], 0)


def test_trace_read_in_pieces(fresh_runtime):
    dev = fresh_runtime
    vm = load(dev, printk3_prog())
    u = units3(65)
    run(dev, vm, u, ordered=True)
    first, lost = dev.trace_read(max_lines=10)
    assert len(first) == 10 and lost == 0
    rest, lost = dev.trace_read()
    assert len(rest) == 55 and lost == 0
    assert first + rest == want3(u)
    # a text buffer with room for two lines and a bit
    run(dev, vm, u[:5], ordered=True)
    w = want3(u[:5])
    cap = len(w[0][1]) + 1 + len(w[1][1]) + 1 + 3
    assert dev.trace_read(text_cap=cap) == (w[:2], 0)
    assert dev.trace_read() == (w[2:], 0)
    assert dev.trace_read() == ([], 0)


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from bpftime_amd import vm as dev
import test_gpu_tracehelpers as t
dev.enable_trace_printk()
vm = t.load(dev, t.printk3_prog())
u = t.units3(130)
t.run(dev, vm, u)
lines, lost = dev.trace_read()
assert len(lines) == 100 and lost == 30, (len(lines), lost)
want = dict(t.want3(u))
assert len(set(l[0] for l in lines)) == 100 and all(want[i] == s for i, s in lines)
assert dev.trace_read() == ([], 0)
t.run(dev, vm, u[:7])                      # the tickets started over
assert sorted(dev.trace_read()[0]) == t.want3(u[:7])
print("OK")
"""


def test_a_full_log_counts_what_it_loses(gpu):
    """BPFTIME_AMD_TRACE_RECORDS is read once, so in a fresh process: 100
    records under 130 units."""
    env = dict(os.environ, BPFTIME_AMD_TRACE_RECORDS="100")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr


# ---- syscall dispatch ---------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["programs", "threads"])
def test_sys_enter_tracer(fresh_runtime, plan):
    """programs.sys_enter_tracer over 48 recorded calls from 3 threads: a line
    per record (pid from the record, comm from the VM), the per-uid count."""
    dev = fresh_runtime
    comm = th.default_comm()[:15]
    ro = dev.Map(ARRAY, 4, 16, 1)
    ro.update(b"\0" * 4, comm.ljust(16, b"\0"))
    counts = dev.Map(HASH, 4, 8, 16)
    code = programs.sys_enter_tracer(ro.fd, counts.fd)
    assert dev.syscall_attach(dev.prog_create(code, "tracer", 5), -1, True) > 0
    n = 48
    recs = gen.syscall_records_timed(n, threads=3)
    w = recs.view(np.uint64).reshape(n, 16)
    w[:, 1] = np.array([0, 1, 57, 0, 1, 60, 231, 3, 202], np.uint64)[np.arange(n) % 9]
    flags = dev.BATCH_SYNC | (dev.DISPATCH_PROGRAMS if plan == "programs" else dev.DISPATCH_THREADS)
    assert dev.syscall_dispatch(dev.DeviceBuffer.from_array(recs), n, record_size=dev.SYSCALL_RECORD_TIMED,
                                flags=flags) == 0
    live = [i for i in range(n) if int(w[i, 1]) not in (60, 231)]
    want = [(i, b"%d %s\n" % (int(w[i, 11]) >> 32, comm)) for i in live]
    assert lines_by_unit(dev)[0] == want
    uid = th.default_uid_gid() & 0xffffffff
    assert counts.hash_items() == {struct.pack("<I", uid): struct.pack("<Q", len(live))}
    # a VM whose comm differs prints and counts nothing
    ro.update(b"\0" * 4, b"someone-else".ljust(16, b"\0"))
    assert dev.syscall_dispatch(dev.DeviceBuffer.from_array(recs), n, record_size=dev.SYSCALL_RECORD_TIMED,
                                flags=flags) == 0
    assert dev.trace_read() == ([], 0)


# ---- the loader's analyses ------------------------------------------------------------------
def test_printk_sees_the_units_own_counter_add(fresh_runtime):
    """A unit adds 1 to a counter and prints it with %s through a map-value
    pointer: the add is not deferred past the call (loader.cpp accesses), so
    the line shows the value after the add."""
    dev = fresh_runtime
    m = dev.Map(ARRAY, 4, 8, 1)
    m.update(b"\0" * 4, b"@BA\0\0\0\0\0")
    a = Asm().ld_map_value(7, m.fd, 0).mov64(2, 1).atomic(8, isa.ATOMIC_ADD, 7, 0, "r2")
    stack_bytes(a, -8, b"%s\0")
    a.mov64(1, "r10").add64(1, -8).mov64(2, 3).mov64(3, "r7").call(PRINTK)
    vm = load(dev, a.exit().assemble())
    assert vm.counter_info(dev.CTX_RAW)[0] == 0            # no deferred add
    run(dev, vm, np.zeros((1, STRIDE), dtype=np.uint8))
    assert dev.trace_read() == ([(0, b"ABA")], 0)
    assert m.lookup(b"\0" * 4) == b"ABA\0\0\0\0\0"


@pytest.mark.parametrize("n", [1, 65])
def test_comm_into_the_xdp_ctx_keeps_the_packet_bounds(fresh_runtime, n):
    """bpf_get_current_comm into the ctx's data_meta .. egress_ifindex words
    (bytes 16..32): the ctx kinds are distrusted from then on, and data /
    data_end read afterwards still bound the packet."""
    dev = fresh_runtime
    a = Asm().mov64(6, "r1").mov64(1, "r6").add64(1, 16).mov64(2, 16).call(COMM)
    a.ldx(8, 2, 6, 0).ldx(8, 3, 6, 8).mov64(0, "r3").alu64("sub", 0, "r2")
    a.mov64(4, "r2").add64(4, 8).jmp("jgt", 4, "r3", "out").ldx(1, 5, 2, 7).alu64("add", 0, "r5")
    vm = load(dev, a.label("out").exit().assemble())
    vm.set_task(comm=b"xdp-comm-16bytes")
    u = np.zeros((n, STRIDE), dtype=np.uint8)
    u[:, 7] = np.arange(n) & 0x7f
    got, after = run(dev, vm, u, kind="xdp")
    np.testing.assert_array_equal(got, (STRIDE + (np.arange(n) & 0x7f)).astype(np.uint64))
    np.testing.assert_array_equal(after, u)
