"""bpf_probe_read* (4 / 112 / 113), bpf_probe_read_*_str (45 / 114 / 115) and
bpf_strncmp (182) on the device, bit-exact (return values, unit bytes with
the slack around the batch, map values) against the oracle interpreter
running the same bytecode with the model (tests/_memhelpers.py) registered:
copies over every size x co-alignment class between packet, stack, map value
and ctx; divergent lanes; overlap; the string forms; -EFAULT with the
destination untouched; a deferred counter add observed by a probe read; the
syscall dispatch under both plans; routing and the programs.py example.

Every batch lies inside a larger device buffer whose slack bytes hold a
sentinel: an out-of-window address a test uses is mapped memory, so a wrong
guard shows as a wrong return value and a copied sentinel, never as a fault."""
import ctypes as C
import struct

import numpy as np
import pytest

from bpftime_amd import gen, isa, programs
from bpftime_amd.isa import Asm

import _memhelpers as mh
from _helpers import make_maps

pytestmark = pytest.mark.gpu

ARRAY, HASH = isa.BPF_MAP_TYPE_ARRAY, isa.BPF_MAP_TYPE_HASH
STRIDE, SLACK, SENTINEL, FILL = 128, 256, 0x5A, 0xAA
A_OFF, A_LEN, B_OFF, B_LEN = 8, 80, 88, 40     # unit: 8-byte header, areas A and B
NS = [1, 63, 64, 65, 130]                      # a lane, a partial wave, a wave, a wave + 1, two waves and a bit
SIZES = [0, 1, 3, 4, 5, 7, 8, 9, 16, 31, 48, 64]
MODES = {"default": None, "cpp_lane_groups": "BPFTIME_AMD_NO_ASM_DIVERGENCE"}   # (test_gpu_atomics.MODES)
EFAULT = mh.EFAULT
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little")


@pytest.fixture(params=list(MODES))
def mode(request, monkeypatch):
    if MODES[request.param]:
        monkeypatch.setenv(MODES[request.param], "1")
    return request.param


def _map_window(po, fd):
    n = C.c_size_t(0)
    p = po.lib().orc_map_raw(fd, C.byref(n))
    return (p, p + n.value)


class Pair:
    """One program loaded on the oracle (with the model) and on the device."""

    def __init__(self, po, dev, code, kind="raw", map_fds=()):
        self.po, self.dev, self.kind, self.map_fds = po, dev, kind, map_fds
        self.win = mh.Windows()
        self.ovm = po.OracleVM()
        self.cbs = mh.register(self.ovm, po, self.win)
        self.ovm.load(code)
        self.vm = dev.VM()
        self.vm.load(code)
        assert self.vm.info()["big_stack"]     # the scratch-stack kernels carry the helpers

    def run(self, units, ordered=False, check=True):
        """-> (device r0s, device units, oracle r0s, oracle units); the slack
        on both sides keeps its sentinel."""
        po, dev = self.po, self.dev
        n = units.shape[0]
        host = np.full(2 * SLACK + n * STRIDE, SENTINEL, dtype=np.uint8)
        host[SLACK:SLACK + n * STRIDE] = units.reshape(-1)
        d = dev.DeviceBuffer.from_array(host)
        ou = host[SLACK:SLACK + n * STRIDE].reshape(n, STRIDE)
        base = ou.ctypes.data
        self.win.windows = [(base, base + n * STRIDE)] + [_map_window(po, fd) for fd in self.map_fds]
        self.win.fences = [(base - SLACK, base), (base + n * STRIDE, base + n * STRIDE + SLACK)]
        flags = dev.BATCH_SYNC | (dev.BATCH_ORDERED if ordered else 0)
        if self.kind == "xdp":
            out = dev.DeviceBuffer(4 * n)
            failed = self.vm.exec_batch(dev.CTX_XDP, d, n, STRIDE, fixed_len=STRIDE, verdicts=out, flags=flags,
                                        data_offset=SLACK, ifindex=0x11223344, rxq=0x55667788)
            got = out.download(np.uint32).astype(np.uint64)
            want = self.ovm.run_xdp(ou, fixed_len=STRIDE, ifindex=0x11223344, rxq=0x55667788).astype(np.uint64)
        else:
            out = dev.DeviceBuffer(8 * n)
            failed = self.vm.exec_batch(dev.CTX_RAW, d, n, STRIDE, fixed_len=STRIDE, rets=out, flags=flags,
                                        data_offset=SLACK)
            got = out.download(np.uint64)
            want = self.ovm.run_raw(ou, STRIDE)
        assert failed == 0
        dhost = d.download()
        if check:
            np.testing.assert_array_equal(got, want)
            off = np.flatnonzero(dhost != host)
            where = [(int(o - SLACK) // STRIDE, int(o - SLACK) % STRIDE, int(dhost[o]), int(host[o])) for o in off[:8]]
            assert not len(off), f"{len(off)} bytes differ; (unit, offset, device, oracle): {where}; " \
                                 f"unit header {units[where[0][0] % n, :8].tolist()}"
        assert (dhost[:SLACK] == SENTINEL).all() and (dhost[-SLACK:] == SENTINEL).all()
        return got, dhost[SLACK:-SLACK].reshape(n, STRIDE), want, ou


def _same_maps(om, dm, n):
    for k in range(n):
        key = struct.pack("<I", k)
        assert dm.lookup(key) == om.lookup(key), k


def _fill_maps(om, dm, n, value):
    for k in range(n):
        v = value(k)
        assert om.update(struct.pack("<I", k), v) == 0 and dm.update(struct.pack("<I", k), v) == 0


# ---- copies --------------------------------------------------------------------
def copy_prog(helper, srck, dstk, kind="raw", mfd=-1):
    """Unit: u8 size @0, u8 source offset @1, u8 destination offset @2, u32
    unit index @4, area A @8 (80 bytes), area B @88 (40 bytes).
    r0 = helper(dst + doff, size, src + soff) with
      src: "pkt" A; "stack" fp-80.. (a copy of A); "map" value[index]; "ctx" ctx + 16
      dst: "pkt" A (B when the source is A); "stack" fp-80.. (pre-filled, then
           stored over A so it shows); "map" value[index]."""
    a = Asm()
    if kind == "xdp":
        a.mov64(8, "r1").add64(8, 16).ldx(8, 6, 1, 0)       # r8 = ctx + 16, r6 = data
    else:
        a.mov64(6, "r1")
    if srck == "stack":
        for i in range(A_LEN // 8):
            a.ldx(8, 2, 6, A_OFF + 8 * i).stx(8, 10, -A_LEN + 8 * i, "r2")
    if dstk == "stack" or (srck == "stack" and dstk == "pkt"):
        a.lddw(2, FILL64)
        for i in range(A_LEN // 8):
            if dstk == "stack":
                a.stx(8, 10, -A_LEN + 8 * i, "r2")
            else:
                a.stx(8, 6, A_OFF + 8 * i, "r2")
    if "map" in (srck, dstk):
        # value[index] through a map-value lddw (libbpf's .rodata / .bss form)
        a.ldx(4, 2, 6, 4).alu64("mul", 2, A_LEN).ld_map_value(7, mfd, 0).add64(7, "r2")

    def base(r, k, other):
        if k == "stack":
            a.mov64(r, "r10").add64(r, -A_LEN)
        elif k == "map":
            a.mov64(r, "r7")
        elif k == "ctx":
            a.mov64(r, "r8")
        else:
            a.mov64(r, "r6").add64(r, B_OFF if (r == 1 and other == "pkt") else A_OFF)
    base(3, srck, dstk)
    a.ldx(1, 2, 6, 1).add64(3, "r2")
    base(1, dstk, srck)
    a.ldx(1, 2, 6, 2).add64(1, "r2")
    a.ldx(1, 2, 6, 0)
    a.call(helper)
    if dstk == "stack":
        for i in range(A_LEN // 8):
            a.ldx(8, 2, 10, -A_LEN + 8 * i).stx(8, 6, A_OFF + 8 * i, "r2")
    return a.exit().assemble()


def copy_units(n, params, seed=1):
    """params[i % len]: (size, soff, doff) of unit i; A random, B pre-filled."""
    u = np.random.default_rng(seed).integers(0, 256, (n, STRIDE), dtype=np.uint8)
    p = np.array([params[i % len(params)] for i in range(n)], dtype=np.uint8)
    u[:, 0:3] = p
    u[:, 3] = 0
    u[:, 4:8] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    u[:, B_OFF:] = FILL
    return u


# every size meets every co-alignment class: equal modulo 8, modulo 4 only, unequal
CLASSES = {"mod8": (1, 1), "mod4": (3, 7), "unequal": (2, 1)}
ALL = [(s, so, do) for s in SIZES for so in range(8) for do in (0, 1, 4, 7)]


def _limit(params, srck, dstk):
    """The sizes the areas of this pair hold (B: 40 bytes; the ctx: 16)."""
    cap = 9 if srck == "ctx" else 31 if (srck, dstk) == ("pkt", "pkt") else 64
    return [p for p in params if p[0] <= cap]


PAIRS = [("pkt", "stack"), ("stack", "pkt"), ("map", "pkt"), ("pkt", "map"), ("pkt", "pkt"), ("map", "stack"),
         ("stack", "map"), ("ctx", "pkt"), ("ctx", "stack")]


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
@pytest.mark.parametrize("srck,dstk", PAIRS, ids=[f"{s}_to_{d}" for s, d in PAIRS])
def test_copy_matrix(fresh_oracle, fresh_runtime, mode, srck, dstk, ordered):
    """Uniform waves (every lane one size and alignment: each size in each
    co-alignment class) and divergent ones (130 units cycling through every
    size x source offset 0..7 x destination offset 0, 1, 4, 7), at every batch
    size, through the three ids in turn."""
    po, dev = fresh_oracle, fresh_runtime
    kind = "xdp" if srck == "ctx" else "raw"
    om = dm = None
    if "map" in (srck, dstk):
        (om,), (dm,) = make_maps([(ARRAY, 4, A_LEN, 130)], po, dev)
    rng = np.random.default_rng(5)
    pairs = [Pair(po, dev, copy_prog(h, srck, dstk, kind, dm.fd if dm else -1), kind, (dm.fd,) if dm else ())
             for h in mh.COPY_IDS]

    def go(n, params, seed):
        if dm:
            _fill_maps(om, dm, n, lambda k: bytes([FILL]) * A_LEN if dstk == "map" else rng.bytes(A_LEN))
        pairs[seed % 3].run(copy_units(n, params, seed), ordered)
        if dm:
            _same_maps(om, dm, n)
    uniform = _limit([(s,) + CLASSES[c] for s in SIZES for c in CLASSES], srck, dstk)
    for i, p in enumerate(uniform):
        go(NS[i % len(NS)], [p], i)
    every = _limit(ALL, srck, dstk)
    for n in NS:
        for at in range(0, len(every), 130) if n == 130 else [7 * n % len(every)]:
            go(n, every[at:at + 130], n + at)


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
def test_divergent_sizes_in_one_wave(fresh_oracle, fresh_runtime, mode, ordered):
    """Size (0..48) and source offset come from unit bytes: a wave's lanes
    leave the copy's loops at different trips, and no lane waits."""
    po, dev = fresh_oracle, fresh_runtime
    p = Pair(po, dev, copy_prog(113, "pkt", "stack"))
    rng = np.random.default_rng(9)
    for n in NS:
        params = [(int(rng.integers(0, 49)), int(rng.integers(0, 8)), int(rng.integers(0, 8))) for _ in range(n)]
        assert len({q[0] for q in params[:64]}) > min(n, 20) // 2
        p.run(copy_units(n, params, n), ordered)


# ---- addresses by delta: overlap, -EFAULT, strings at the window's end ---------
def delta_prog(helper):
    """Unit: i64 source delta @8, u64 size @16, i64 destination delta @24;
    r0 = helper(unit + ddelta, size, unit + sdelta)."""
    a = Asm().mov64(6, "r1")
    a.ldx(8, 3, 6, 8).add64(3, "r6").ldx(8, 2, 6, 16).ldx(8, 1, 6, 24).add64(1, "r6")
    return a.call(helper).exit().assemble()


def delta_units(n, rows, seed=3, data=None):
    """rows[i % len]: (sdelta, size, ddelta), each an int or a function of
    (unit index, n); bytes 32.. random (or data(i))."""
    u = np.random.default_rng(seed).integers(1, 256, (n, STRIDE), dtype=np.uint8)
    w = u.view(np.uint64).reshape(n, STRIDE // 8)
    for i in range(n):
        r = [f(i, n) if callable(f) else f for f in rows[i % len(rows)]]
        w[i, 0], w[i, 1:4] = i, [x & mh.M64 for x in r]
        if data:
            u[i, 32:] = np.frombuffer(data(i), dtype=np.uint8)
    return u


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
def test_overlap_is_ascending_bytes(fresh_oracle, fresh_runtime, mode, ordered):
    """dst = src + 3 (the three bytes in front of dst repeat) and dst = src - 3
    (a memmove), n = 16, inside the unit; beside disjoint rows."""
    po, dev = fresh_oracle, fresh_runtime
    rows = [(40, 16, 43), (43, 16, 40), (40, 16, 80), (41, 5, 42), (48, 16, 48)]
    for h in mh.COPY_IDS:
        p = Pair(po, dev, delta_prog(h))
        for n in NS:
            got, du, _, _ = p.run(delta_units(n, rows, n), ordered)
            assert (got == 0).all()
            src = delta_units(n, rows, n)
            np.testing.assert_array_equal(du[0, 43:59], np.tile(src[0, 40:43], 6)[:16])
            if n > 1:
                np.testing.assert_array_equal(du[1, 40:56], src[1, 43:59])


def _before(i, n):
    return -i * STRIDE - 16                     # 16 bytes of slack in front of the batch


def _after(i, n):
    return (n - i) * STRIDE                     # the first byte behind the batch


FAULTS = [  # (sdelta, size, ddelta): every one answers -EFAULT
    (_before, 16, 32), (_after, 16, 32), (32, 16, _before), (32, 16, _after),
    (lambda i, n: _after(i, n) - 8, 16, 32),    # straddles the window's end
    (lambda i, n: _before(i, n) + 8, 16, 32),   # starts in the slack, runs into the window
    (32, 16, lambda i, n: _after(i, n) - 1),    # destination: last byte inside, the rest outside
    (32, -1, 64), (32, -(1 << 63), 64), (32, 1 << 62, 64),
    (lambda i, n: _after(i, n) - 1, 2, 32),
]
FINE = [(32, 16, 64), (lambda i, n: _after(i, n) - 16, 16, 32), (lambda i, n: -i * STRIDE, 8, 64), (32, 0, _before),
        (_before, 0, 32)]


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
def test_efault_leaves_the_destination(fresh_oracle, fresh_runtime, mode, ordered):
    """Ranges outside the batch window (in the sentinel slack before and
    behind it), straddling its ends, size -1: r0 = -14, nothing written --
    the unit bytes are the oracle's (untouched), the slack keeps its sentinel."""
    po, dev = fresh_oracle, fresh_runtime
    rows = FAULTS + FINE
    bad = np.array([True] * len(FAULTS) + [False] * len(FINE))
    for h in mh.COPY_IDS:
        p = Pair(po, dev, delta_prog(h))
        for n in NS:
            u = delta_units(n, rows, n)
            got, du, _, _ = p.run(u, ordered)
            want_bad = bad[np.arange(n) % len(rows)]
            assert (got[want_bad] == EFAULT).all() and (got[~want_bad] == 0).all()
            np.testing.assert_array_equal(du[want_bad], u[want_bad])   # pre-fill intact
    # the string forms and strncmp over the same addresses (sizes as unsigned)
    srows = [(_before, 16, 32), (_after, 16, 32), (32, 16, _before), (32, 16, _after),
             (32, 16, lambda i, n: _after(i, n) - 8), (32, 16, 64), (32, 0, _after)]
    for h in mh.STR_IDS + (mh.STRNCMP_ID,):
        p = Pair(po, dev, delta_prog(h))
        for n in (1, 65, 130):
            got, _, _, _ = p.run(delta_units(n, srows, n), ordered)
            k = np.arange(n) % len(srows)
            # (strncmp over a range that straddles the window's end answers
            # the byte difference it meets before the end: row 4 is the oracle's)
            assert (got[k < (4 if h == mh.STRNCMP_ID else 5)] == EFAULT).all() and (got[k == 6] == 0).all()


def test_efault_on_the_stack(fresh_runtime, mode):
    """fp - 8 for 16 bytes crosses the stack's top, as a source (into the
    unit) and as a destination: -14 and the unit untouched.  (Stated
    directly: on the oracle the same read would leave the interpreter's own
    stack array.)  fp - 16 for 16 bytes is inside: 0."""
    dev = fresh_runtime
    for n in NS:
        for src_off, dst_off, size, want in [(-8, None, 16, EFAULT), (None, -8, 16, EFAULT), (-16, None, 16, 0),
                                             (-512, None, 8, 0), (-520, None, 16, EFAULT), (-8, None, 9, EFAULT)]:
            a = Asm().mov64(6, "r1").lddw(2, 0x0123456789ABCDEF).stx(8, 10, -8, "r2").stx(8, 10, -16, "r2")
            a.stx(8, 10, -512, "r2")
            if src_off is not None:
                a.mov64(1, "r6").add64(1, 32).mov64(3, "r10").add64(3, src_off)
            else:
                a.mov64(3, "r6").add64(3, 32).mov64(1, "r10").add64(1, dst_off)
            code = a.mov64(2, size).call(113).exit().assemble()
            vm = dev.VM()
            vm.load(code)
            u = np.full((n, STRIDE), FILL, dtype=np.uint8)
            d = dev.DeviceBuffer.from_array(u)
            out = dev.DeviceBuffer(8 * n)
            assert vm.exec_batch(dev.CTX_RAW, d, n, STRIDE, fixed_len=STRIDE, rets=out) == 0
            assert (out.download(np.uint64) == want).all(), (src_off, dst_off, size)
            du = d.download().reshape(n, STRIDE)
            if want:
                assert (du == FILL).all()
            else:
                assert (du[:, 32:32 + size].view(np.uint64) == 0x0123456789ABCDEF).all()


# ---- the string forms -------------------------------------------------------------
def _str_data(nul):
    """A source without a zero byte but at `nul` (None: nowhere), random bytes
    and a second NUL behind it."""
    def f(i):
        b = bytearray(np.random.default_rng(100 + i).integers(1, 256, STRIDE - 32, dtype=np.uint8).tobytes())
        k = nul(i) if callable(nul) else nul
        if k is not None:
            b[k] = 0
            b[k + 2] = 0
        return bytes(b)
    return f


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
def test_probe_read_str(fresh_oracle, fresh_runtime, mode, ordered):
    """strncpy into a 0xAA pre-fill: the NUL at index 0, in the middle, at
    bufsz - 1 and nowhere (then no NUL is added); bufsz 0, 1, 16; sources at
    offsets 0..7 from unit + 32, destinations at unit + 96 + (0, 1, 4, 7)."""
    po, dev = fresh_oracle, fresh_runtime
    for h in mh.STR_IDS:
        p = Pair(po, dev, delta_prog(h))
        for bufsz in (0, 1, 16):
            rows = [(32 + so, bufsz, 96 + do) for so in range(8) for do in (0, 1, 4, 7)]
            for nul in (0, 5, max(bufsz - 1, 0), None):
                so_of = lambda i: i % len(rows) // 4                    # noqa: E731
                data = _str_data(None if nul is None else (lambda i, nul=nul: so_of(i) + nul))
                n = NS[(bufsz + (nul or 0)) % len(NS)]

                def units():
                    u = delta_units(n, rows, n, data)
                    u[:, 96:] = FILL
                    return u
                got, du, _, _ = p.run(units(), ordered)
                assert (got == 0).all()
                if bufsz == 16 and nul == 5:    # spot check beside the oracle: bytes, NUL, zero padding, pre-fill
                    src = units()
                    assert bytes(du[0, 96:112]) == bytes(src[0, 32:37]) + bytes(11) and du[0, 112] == FILL


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
def test_str_nul_is_the_windows_last_byte(fresh_oracle, fresh_runtime, mode, ordered):
    """The source string ends with the unit: for the batch's last unit its NUL
    is the window's last byte, and the copy succeeds without a read behind
    it; without that NUL the same call runs off the window: -EFAULT."""
    po, dev = fresh_oracle, fresh_runtime
    p = Pair(po, dev, delta_prog(115))
    for n in NS:
        for nul in (True, False):
            u = delta_units(n, [(STRIDE - 8, 16, 32)], n)
            u[:, STRIDE - 1] = 0 if nul else 7
            u[:, 32:48] = FILL
            got, du, _, _ = p.run(u, ordered)
            assert got[-1] == (0 if nul else EFAULT)
            want = bytes(u[-1, STRIDE - 8:STRIDE - 1]) + bytes(9) if nul else bytes([FILL]) * 16
            assert bytes(du[-1, 32:48]) == want


# ---- strncmp -------------------------------------------------------------------------
CMP = [  # (s1, s2, n, r0 as a signed number)
    (b"GET /index", b"GET /index", 10, 0), (b"abc\0", b"abc\0", 16, 0),
    (b"b", b"a", 1, 1), (b"a", b"c", 1, -2), (b"\x80", b"\x7f", 1, 1), (b"\x7f", b"\xff", 1, -128),
    (b"\xff", b"\0", 1, 255), (b"\0", b"\xff", 4, -255),
    (b"abcX", b"abcY", 3, 0),           # a difference at index n
    (b"ab\0X", b"ab\0Y", 8, 0),         # a difference behind a common NUL
    (b"X", b"Y", 0, 0), (b"abcdefgh1", b"abcdefgh2", 9, -1), (b"ab\0", b"ab\0Z", 3, 0), (b"abc", b"ab\0", 3, ord("c")),
]


def _cmp_units(n):
    u = np.random.default_rng(4).integers(1, 256, (n, STRIDE), dtype=np.uint8)
    u[:, 4:8] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    for i in range(n):
        s1, s2, k, _ = CMP[i % len(CMP)]
        u[i, 0] = k
        u[i, 32:32 + len(s1)] = np.frombuffer(s1, dtype=np.uint8)
        u[i, 65:65 + len(s2)] = np.frombuffer(s2, dtype=np.uint8)     # (an odd offset)
    return u


def _cmp_want(n):
    return np.array([CMP[i % len(CMP)][3] & mh.M64 for i in range(n)], dtype=np.uint64)


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
@pytest.mark.parametrize("s2_in_map", [False, True], ids=["packet", "map_value"])
def test_strncmp(fresh_oracle, fresh_runtime, mode, s2_in_map, ordered):
    """Equal strings, a differing first byte of either sign (bytes >= 0x80
    compare as unsigned), a difference at index s1_sz or behind a common NUL
    (ignored), s1_sz 0; s2 in the unit or in an ARRAY map value.  r0 is the
    byte difference sign-extended to 64 bits."""
    po, dev = fresh_oracle, fresh_runtime
    a = Asm().mov64(6, "r1")
    fds = ()
    if s2_in_map:
        (om,), (dm,) = make_maps([(ARRAY, 4, 32, 130)], po, dev)
        fds = (dm.fd,)
        a.ldx(4, 2, 6, 4).alu64("mul", 2, 32).ld_map_value(3, dm.fd, 1).add64(3, "r2")   # value[index] + 1
    else:
        a.mov64(3, "r6").add64(3, 65)
    code = a.mov64(1, "r6").add64(1, 32).ldx(1, 2, 6, 0).call(mh.STRNCMP_ID).exit().assemble()
    p = Pair(po, dev, code, map_fds=fds)
    for n in NS:
        u = _cmp_units(n)
        if s2_in_map:
            _fill_maps(om, dm, n, lambda k: bytes(u[k, 64:96]))
        got, _, _, _ = p.run(u, ordered)
        np.testing.assert_array_equal(got, _cmp_want(n))


# ---- the loader's analyses ----------------------------------------------------------
def test_probe_read_sees_the_units_own_counter_add(fresh_oracle, fresh_runtime, mode):
    """One unit adds 1 to an ARRAY counter and probe-reads it: the add is not
    deferred past the read (loader.cpp accesses), so r0 = the value before
    the batch + 1."""
    po, dev = fresh_oracle, fresh_runtime
    for via_lookup in (False, True):
        (om,), (dm,) = make_maps([(ARRAY, 4, 8, 1)], po, dev)
        _fill_maps(om, dm, 1, lambda k: struct.pack("<Q", 41))
        a = Asm().mov64(6, "r1")
        if via_lookup:
            a.st(4, 10, -12, 0).ld_map_fd(1, dm.fd).mov64(2, "r10").add64(2, -12).call(isa.BPF_FUNC_map_lookup_elem)
            a.jmp("jne", 0, 0, "found").mov64(0, 77).exit().label("found").mov64(7, "r0")
        else:
            a.ld_map_value(7, dm.fd, 0)
        a.mov64(2, 1).atomic(8, isa.ATOMIC_ADD, 7, 0, "r2")
        a.mov64(1, "r10").add64(1, -8).mov64(2, 8).mov64(3, "r7").call(113)
        code = a.ldx(8, 0, 10, -8).exit().assemble()
        p = Pair(po, dev, code, map_fds=(dm.fd,))
        got, _, _, _ = p.run(delta_units(1, [(0, 0, 0)]))
        assert got[0] == 42
        _same_maps(om, dm, 1)
        assert dm.lookup(b"\0" * 4) == struct.pack("<Q", 42)


@pytest.mark.parametrize("plan", ["programs", "threads"])
def test_syscall_dispatch_copies_an_argument(fresh_runtime, plan):
    """A sys_enter program copies args[1] out of its ctx with
    bpf_probe_read_kernel and stores it in a HASH map keyed by syscall id: 130
    records of 3 recorded threads under both plans (the thread-ordered one runs
    it in k_sys_seq, whose ctx is an LDS copy)."""
    dev = fresh_runtime
    m = dev.Map(HASH, 4, 8, 64)
    a = Asm().mov64(6, "r1").ldx(4, 2, 6, 8).stx(4, 10, -4, "r2")
    a.mov64(1, "r10").add64(1, -16).mov64(2, 8).mov64(3, "r6").add64(3, 24).call(113)
    a.ld_map_fd(1, m.fd).mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16).mov64(4, 0)
    code = a.call(isa.BPF_FUNC_map_update_elem).mov64(0, 0).exit().assemble()
    vm = dev.VM()
    vm.load(code)
    assert vm.info()["big_stack"]
    assert dev.syscall_attach(dev.prog_create(code, "copy_arg", 5), -1, True) > 0
    n = 130
    recs = gen.syscall_records_timed(n, threads=3)
    w = recs.view(np.uint64).reshape(n, 16)
    assert len(np.unique(w[:, 11])) == 3
    w[:, 1] = np.array([0, 1, 57, 0, 1, 60, 231, 3, 202], np.uint64)[np.arange(n) % 9]
    w[:, 3] = w[:, 1] * np.uint64(0x0101010101010101) + np.uint64(0x8000000000000007)   # args[1]: a function of the id
    d = dev.DeviceBuffer.from_array(recs)
    flags = dev.BATCH_SYNC | (dev.DISPATCH_PROGRAMS if plan == "programs" else dev.DISPATCH_THREADS)
    assert dev.syscall_dispatch(d, n, record_size=dev.SYSCALL_RECORD_TIMED, flags=flags) == 0
    want = {struct.pack("<I", int(i)): struct.pack("<Q", int(v)) for i, v in zip(w[:, 1], w[:, 3])
            if int(i) not in (60, 231)}
    assert m.hash_items() == want


# ---- routing and surface ---------------------------------------------------------------
@pytest.mark.parametrize("helper", sorted(mh.NAMES))
def test_routing(fresh_runtime, helper):
    """A program calling any of the seven ids loads, runs in the scratch-stack
    kernels, and instantiates from a prog record."""
    dev = fresh_runtime
    code = (Asm().st(8, 10, -8, 0).st(8, 10, -16, 0).mov64(1, "r10").add64(1, -8).mov64(2, 8).mov64(3, "r10")
            .add64(3, -16).call(helper).exit().assemble())
    vm = dev.VM()
    rc, msg = vm.try_load(code)
    assert rc == 0, msg
    assert vm.info()["big_stack"] and vm.info()["stack_size"] == 512
    assert getattr(isa, "BPF_FUNC_" + mh.NAMES[helper].decode()[4:]) == helper
    pvm = dev.prog_instantiate(dev.prog_create(code, "p", 2))   # (a kprobe record: r1 = the unit)
    u = np.zeros((1, 64), dtype=np.uint8)
    out = dev.DeviceBuffer(8)
    assert pvm.exec_batch(dev.CTX_RAW, dev.DeviceBuffer.from_array(u), 1, 64, fixed_len=64, rets=out) == 0
    assert out.download(np.uint64)[0] == 0


def test_payload_prefix_drop(fresh_runtime):
    """programs.payload_prefix_drop over 130 packets: the model's verdicts."""
    dev = fresh_runtime
    sig = b"ATTACK/1\0"
    m = dev.Map(ARRAY, 4, 16, 1)
    assert m.update(b"\0" * 4, sig.ljust(16, b"\0")) == 0
    vm = dev.VM()
    vm.load(programs.payload_prefix_drop(m.fd, 12))
    n = 130
    pk = np.random.default_rng(6).integers(1, 256, (n, 64), dtype=np.uint8)
    payloads = [sig + b"xyz", sig[:5] + b"Q" + sig[6:] + b"xyz", b"ATTACK/1\0\0\0\0", b"ATTACK/2\0abc", b"\0" * 12,
                b"ATTACK/1" + b"\x01abc"]
    for i in range(n):
        if i % 7:
            pk[i, 42:54] = np.frombuffer(payloads[i % len(payloads)][:12].ljust(12, b"z"), dtype=np.uint8)
    lens = np.where(np.arange(n) % 11 == 3, 50, 64).astype(np.uint32)      # too short for the prefix: passes
    d, dl, dv = dev.DeviceBuffer.from_array(pk), dev.DeviceBuffer.from_array(lens), dev.DeviceBuffer(4 * n)
    assert vm.exec_batch(dev.CTX_XDP, d, n, 64, lens=dl, verdicts=dv) == 0
    want = [isa.XDP_DROP if lens[i] == 64 and mh.strncmp(bytes(pk[i, 42:54]), 12, sig.ljust(16, b"\0")) == 0
            else isa.XDP_PASS for i in range(n)]
    assert dv.download(np.uint32).tolist() == want
    assert want.count(isa.XDP_DROP) > 20 and want.count(isa.XDP_PASS) > 20
