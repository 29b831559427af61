"""bpftime_amd_xdp_complete on the device against the numpy model
(tests/_xdp_complete.py), bit for bit: the lists, the unit indices, the counts
and every byte of every output buffer, the sentinel-filled space behind what
should be written included."""
import ctypes as C

import numpy as np
import pytest

from bpftime_amd import _lib, isa
from bpftime_amd.isa import Asm

import _xdp_complete as X
from _xdp_complete import ABORTED, DROP, PASS, REDIRECT, TX

pytestmark = pytest.mark.gpu

CHUNK = 2048
T = _lib.lib().bpftime_amd_xdp_complete_tile()
K = _lib.lib().bpftime_amd_xdp_complete_scan_tiles()


def _ring_case(n, pat, seed, **kw):
    rng = np.random.default_rng(seed)
    ub, d = X.shuffled_ring(n, rng)
    return X.Case(X.pattern(pat, n, rng), CHUNK, ub, descs=d, **kw)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 200003])
def test_counts_around_the_wave_and_the_tile(fresh_runtime, n):
    c = _ring_case(n, "uniform7", 100 + n)
    X.check(c, X.run_device(fresh_runtime, c))


def test_more_tiles_than_one_scan_pass(fresh_runtime):
    """K * T units fill one pass of the tile-offset scan; the carry into the
    second pass is where a scan goes wrong.  Strided mode, indices only."""
    n = K * T + 2 * T + 5
    rng = np.random.default_rng(9)
    off = np.full(n, 16, np.int32)
    off[::1000] = 250                                   # 250 + 60 crosses the 256-B slot
    c = X.Case(X.pattern("uniform7", n, rng), 256, n * 256, off=off, ln=np.full(n, 60, np.uint32),
               cap=[n, 5, n, 0, 17])
    got = X.run_device(fresh_runtime, c, out_null=(ABORTED, PASS))
    r = X.check(c, got, out_null=(ABORTED, PASS))
    assert min(r.counts) > n // 8


@pytest.mark.parametrize("pat", ["all0", "all1", "all2", "all3", "all4", "alternate", "tx16", "uniform7", "no_pass"])
def test_patterns(fresh_runtime, pat):
    c = _ring_case(3 * T + 17, pat, 7)
    r = X.check(c, X.run_device(fresh_runtime, c))
    if pat == "no_pass":
        assert r.counts[PASS] == 0 and min(r.counts[k] for k in (ABORTED, DROP, TX, REDIRECT)) > 0
    if pat == "uniform7":
        assert r.counts[ABORTED] > 2 * r.counts[DROP]      # verdicts 5 and 6 fold into class 0


def test_strided_mode_with_a_head(fresh_runtime):
    n, head = 2 * T + 9, 256
    rng = np.random.default_rng(21)
    off = np.full(n, head, np.int32)
    off[::3] += 14
    c = X.Case(X.pattern("uniform7", n, rng), CHUNK, n * CHUNK, off=off, ln=rng.integers(0, 1500, n).astype(np.uint32))
    r = X.check(c, X.run_device(fresh_runtime, c))
    assert int(r.lists[TX][0]["addr"][0]) % CHUNK in (head, head + 14)
    assert (r.lists[DROP][0]["addr"] % CHUNK == 0).all()


def test_hand_made_post_program_arrays(fresh_runtime):
    """Every offset with every length, at chunk + 256 and at chunk + 2: frames
    that end exactly on the chunk end, cross it by one byte, or start before
    the chunk."""
    offs, lens = [-14, 0, 14, 2040, -2, -3, -256, -257], [0, 1, 60, 2048, 1792, 1793, 1778, 1779, 2046, 2047, 6, 7]
    grid = [(o, ln, h) for o in offs for ln in lens for h in (256, 2)]
    n = len(grid)
    addr = np.arange(n, dtype=np.uint64) * np.uint64(CHUNK) + np.array([h for _, _, h in grid], np.uint64)
    c = X.Case(np.full(n, TX, np.uint32), CHUNK, n * CHUNK, descs=X.descs_of(addr, 64, np.arange(n)),
               off=[o for o, _, _ in grid], ln=[ln for _, ln, _ in grid], frame_mask=0x1F)
    r = X.check(c, X.run_device(fresh_runtime, c))
    kept = {grid[i] for i in r.lists[TX][1]}
    assert (0, 1792, 256) in kept and (0, 1793, 256) not in kept      # ends on / one past the chunk end
    assert (14, 1778, 256) in kept and (14, 1779, 256) not in kept
    assert (-2, 2048, 2) in kept and (-3, 60, 2) not in kept           # the chunk's first byte / one before it
    assert (-256, 2048, 256) in kept and (-257, 1, 256) not in kept
    assert (2040, 6, 2) in kept and (2040, 7, 2) not in kept and (2040, 0, 256) not in kept
    assert r.counts[TX] + r.counts[ABORTED] == n and r.counts[ABORTED] > 0


def test_descriptors_outside_the_umem_and_wide_addresses(fresh_runtime):
    top = (1 << 64) - 1
    ub = 64 * CHUNK
    addr = np.array([256, ub - CHUNK + 256, ub + 256, ub - 1, top, top - CHUNK, 1 << 63, 3 * CHUNK + 2], np.uint64)
    c = X.Case(np.full(8, PASS, np.uint32), CHUNK, ub - 1, descs=X.descs_of(addr, 64, 5), off=[0, 0, 0, 0, 1, 0, -1, 0],
               ln=[64] * 8)
    r = X.check(c, X.run_device(fresh_runtime, c))
    assert list(r.lists[PASS][1]) == [0, 7]                # (the last chunk ends past umem_bytes = ub - 1)
    # a stride that is no power of two takes the division path
    c = X.Case(np.full(6, TX, np.uint32), 3000, 10 * 3000, descs=X.descs_of([0, 2999, 3000, 8999, 29999, 30000], 1, 0),
               off=[0, 0, -1, 1, 0, 0], ln=[3000, 1, 1, 1, 1, 1])
    r = X.check(c, X.run_device(fresh_runtime, c))
    assert list(r.lists[TX][1]) == [0, 1, 4]


def _adjust_head_program() -> bytes:
    """IPv4 frames: bpf_xdp_adjust_head(+14), XDP_TX; the rest XDP_DROP."""
    a = Asm().mov64(6, "r1").ldx(8, 2, 6, 0).ldx(8, 3, 6, 8).mov64(4, "r2").add64(4, 14)
    a.mov64(0, 1).jmp("jgt", 4, "r3", "out")
    a.ldx(2, 5, 2, 12).jmp("jne", 5, 0x0008, "out")
    a.mov64(1, "r6").mov64(2, 14).call(isa.BPF_FUNC_xdp_adjust_head)
    a.mov64(0, 3).label("out").exit()
    return a.assemble()


def test_end_to_end_after_exec_batch(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    n = 4096
    rng = np.random.default_rng(33)
    ub, d = X.shuffled_ring(n, rng)
    frames = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    ipv4 = rng.integers(0, 2, n).astype(bool)
    frames[:, 12], frames[:, 13] = np.where(ipv4, 0x08, 0x86), np.where(ipv4, 0x00, 0xDD)
    umem = np.zeros(ub, np.uint8)
    for i in range(n):
        a = int(d["addr"][i])
        umem[a:a + 64] = frames[i]
    code = _adjust_head_program()
    ovm = po.OracleVM()
    ovm.load(code)
    ov, ooff, olen = ovm.run_xdp(frames.copy(), fixed_len=64, want_meta=True)
    vm = dev.VM()
    vm.load(code)
    du, dd = dev.DeviceBuffer.from_array(umem), dev.DeviceBuffer.from_array(d)
    dv, doff, dln = dev.DeviceBuffer(4 * n), dev.DeviceBuffer(4 * n), dev.DeviceBuffer(4 * n)
    assert vm.exec_batch(dev.CTX_XDP, du, n, CHUNK, verdicts=dv, descs=dd, umem_bytes=ub, data_off_out=doff,
                         len_out=dln) == 0
    np.testing.assert_array_equal(dv.download(np.uint32), ov)
    np.testing.assert_array_equal(doff.download(np.int32), ooff)
    np.testing.assert_array_equal(dln.download(np.uint32), olen)
    c = X.Case(ov, CHUNK, ub, descs=d, off=ooff, ln=olen, gather_mask=1 << TX, gather_stride=64, gather_cap=n,
               umem=du.download())
    bufs = {"verdicts": dv, "descs": dd, "off": doff, "ln": dln, "umem": du}
    r = X.check(c, X.run_device(dev, c, bufs=bufs))
    tx, drop = np.flatnonzero(ipv4), np.flatnonzero(~ipv4)
    assert X.same(r.lists[TX][1], tx.astype(np.uint32)) and X.same(r.lists[DROP][1], drop.astype(np.uint32))
    assert X.same(r.lists[TX][0], X.descs_of(d["addr"][tx] + np.uint64(14), 50, d["options"][tx]))
    assert X.same(r.lists[DROP][0], X.descs_of(d["addr"][drop] // np.uint64(CHUNK) * np.uint64(CHUNK), 0, 0))
    assert r.counts == [0, len(drop), 0, len(tx), 0] and r.g_count == len(tx)


@pytest.mark.parametrize("cap", ["zero", "one", "count-1"])
def test_caps_leave_the_space_behind_them_alone(fresh_runtime, cap):
    c = _ring_case(2 * T + 100, "uniform7", 44)
    counts = X.model(c).counts
    c.cap = [{"zero": 0, "one": 1, "count-1": k - 1}[cap] for k in counts]
    X.check(c, X.run_device(fresh_runtime, c))


def test_either_list_pointer_may_be_null(fresh_runtime):
    c = _ring_case(T + 77, "uniform7", 45)
    out_null, index_null = (ABORTED, TX, REDIRECT), (DROP, TX)   # (TX: counted only)
    X.check(c, X.run_device(fresh_runtime, c, out_null=out_null, index_null=index_null), out_null=out_null,
            index_null=index_null)


def _gather_case(n, gather_stride, seed, gather_cap=None, lens=(0, 1, 15, 16, 17, 64, 1500, 2048)):
    """Frames of every length at source offsets 0, 2 and 7 modulo 16, each
    filling its chunk from its start (so a 2048-B frame sits at offset 0)."""
    rng = np.random.default_rng(seed)
    ln = np.array([lens[i % len(lens)] for i in range(n)], np.uint32)
    head = np.array([(0, 2, 7)[(i // len(lens)) % 3] for i in range(n)], np.uint64)
    head = np.where(ln + head > CHUNK, 0, head).astype(np.uint64)
    chunks = rng.permutation(n + 8)[:n].astype(np.uint64)
    ub = (n + 8) * CHUNK
    umem = rng.integers(0, 256, ub, dtype=np.uint8)
    v = rng.choice(np.array([DROP, PASS, TX, TX], np.uint32), n)
    return X.Case(v, CHUNK, ub, descs=X.descs_of(chunks * np.uint64(CHUNK) + head, ln, np.arange(n) + 1),
                  gather_mask=(1 << TX) | (1 << PASS), gather_stride=gather_stride,
                  gather_cap=n if gather_cap is None else gather_cap, umem=umem)


@pytest.mark.parametrize("gather_stride", [64, 2048, 2050])
def test_gather_lengths_alignments_and_strides(fresh_runtime, gather_stride):
    c = _gather_case(T + 200, gather_stride, 50 + gather_stride)
    r = X.check(c, X.run_device(fresh_runtime, c))
    assert r.g_count > 100
    assert (r.g_skipped > 0) == (gather_stride == 64)      # 1500- and 2048-B frames do not fit 64-B slots


def test_gather_cap_below_the_total(fresh_runtime):
    c = _gather_case(T + 200, 2048, 61, gather_cap=37)
    r = X.check(c, X.run_device(fresh_runtime, c))
    assert r.g_count > 37


def test_gather_into_pinned_host_memory(fresh_runtime):
    dev = fresh_runtime
    c = _gather_case(300, 2050, 62)
    nbytes = (c.gather_cap + X.PAD) * c.gather_stride
    host = dev.lib().bpftime_amd_host_alloc(nbytes)
    assert host
    try:
        C.memset(host, X.SENTINEL, nbytes)
        r = X.check(c, X.run_device(dev, c, gather_host=host))
        got = np.frombuffer(C.string_at(host, nbytes), np.uint8)
        assert X.same(got, X.gather_image(c, r, c.gather_cap + X.PAD))
    finally:
        dev.lib().bpftime_amd_host_free(C.c_void_p(host))


def test_on_a_stream_behind_an_async_batch_and_twice_in_a_row(fresh_oracle, fresh_runtime):
    """exec_batch without a sync, then xdp_complete twice on the same stream
    (the second reuses the first's scratch, with fewer tiles): both equal the
    synchronous result."""
    po, dev = fresh_oracle, fresh_runtime
    n = 3 * T + 5
    rng = np.random.default_rng(71)
    ub, d = X.shuffled_ring(n, rng)
    umem = rng.integers(0, 256, ub, dtype=np.uint8)
    for a in d["addr"][::2]:
        umem[int(a) + 12:int(a) + 14] = (0x08, 0x00)
    vm = dev.VM()
    vm.load(_adjust_head_program())
    du, dd = dev.DeviceBuffer.from_array(umem), dev.DeviceBuffer.from_array(d)
    dv, doff, dln = dev.DeviceBuffer(4 * n), dev.DeviceBuffer(4 * n), dev.DeviceBuffer(4 * n)
    s = dev.lib().bpftime_amd_stream_create()
    try:
        assert vm.exec_batch(dev.CTX_XDP, du, n, CHUNK, verdicts=dv, descs=dd, umem_bytes=ub, data_off_out=doff,
                             len_out=dln, flags=0, stream=s) == 0
        bufs = {"verdicts": dv, "descs": dd, "off": doff, "ln": dln, "umem": du}
        shape = X.Case(np.zeros(n, np.uint32), CHUNK, ub, descs=d, gather_mask=1 << TX, gather_stride=64, gather_cap=n)
        got_async = X.run_device(dev, shape, bufs=bufs, stream=s, sync=False)
        c = X.Case(dv.download(np.uint32), CHUNK, ub, descs=d, off=doff.download(np.int32),
                   ln=dln.download(np.uint32), gather_mask=1 << TX, gather_stride=64, gather_cap=n, umem=du.download())
        r = X.check(c, got_async)
        assert r.counts[TX] >= n // 2 and r.counts[DROP] > 0
        X.check(c, X.run_device(dev, c, bufs=bufs, stream=s), r)
        # back to back, no sync between: a smaller batch, then the full one again
        m = T + 3
        small = X.Case(c.verdicts[:m], CHUNK, ub, descs=d[:m], off=c.off[:m], ln=c.ln[:m])
        first = X.launch(dev, small, bufs=bufs, stream=s, sync=False)
        second = X.launch(dev, c, bufs=bufs, stream=s, sync=False)
        X.check(small, X.collect(first))
        X.check(c, X.collect(second), r)
    finally:
        dev.lib().bpftime_amd_stream_sync(s)
        dev.lib().bpftime_amd_stream_destroy(s)
