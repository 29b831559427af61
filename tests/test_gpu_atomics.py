"""Device parity of every BPF_ATOMIC form: {4, 8 bytes} x {ADD, OR, AND, XOR}
x {plain, FETCH}, XCHG and CMPXCHG, on every kind of target (the unit's own
bytes inside and past the staged window, the LDS stack, the scratch stack, a
map value through map_lookup_elem and through a map-value lddw), in the asm
tier and the C++ tier, bit-exact against the oracle; and, on addresses
shared by all lanes, the invariants atomicity implies whatever the order."""
import functools
import struct

import numpy as np
import pytest

from bpftime_amd import gen, isa
from bpftime_amd.isa import Asm

from _helpers import make_maps

pytestmark = pytest.mark.gpu

M32 = np.uint64(0xFFFFFFFF)
HI32 = np.uint64(0xFFFFFFFF00000000)
OPS = {"add": isa.ATOMIC_ADD, "or": isa.ATOMIC_OR, "and": isa.ATOMIC_AND, "xor": isa.ATOMIC_XOR}

# (id, bytes, imm, source register): the 20 forms, and CMPXCHG whose new
# value is r0 itself (the oracle defines it: memory keeps its value)
FORMS = []
for _sz in (8, 4):
    for _op, _imm in OPS.items():
        FORMS.append((f"{_op}{_sz * 8}", _sz, _imm, "r3"))
        FORMS.append((f"{_op}_fetch{_sz * 8}", _sz, _imm | isa.ATOMIC_FETCH, "r3"))
    FORMS.append((f"xchg{_sz * 8}", _sz, isa.ATOMIC_XCHG, "r3"))
    FORMS.append((f"cmpxchg{_sz * 8}", _sz, isa.ATOMIC_CMPXCHG, "r3"))
    FORMS.append((f"cmpxchg{_sz * 8}_src_r0", _sz, isa.ATOMIC_CMPXCHG, "r0"))
FORM_IDS = [f[0] for f in FORMS]

# unit layout: u64 A @0, u64 B @8, u64 operand @16, u64 r0 for CMPXCHG @24,
# u32 unit index @32, u8 lane group @36; the 16-byte cell of the own-bytes
# targets @40 (staged) or @72 (past the 64 staged bytes, stride 128)
TARGETS = ["own_staged", "own_past_window", "lds_stack", "scratch_stack", "map_lookup", "map_value_lddw"]
MODES = {"default": None, "cpp_lane_groups": "BPFTIME_AMD_NO_ASM_DIVERGENCE", "unfused": "BPFTIME_AMD_NO_FUSE"}
N = 1000  # four blocks, the last wave partly filled


def _operands(n, seed):
    """Random, small and high-word-set values (test_gpu_parity._operands)."""
    r = gen.sm64(seed, np.arange(2 * n, dtype=np.uint64)).reshape(n, 2)
    small = (r % np.uint64(70)).astype(np.uint64)
    pick = (gen.sm64(seed + 1, np.arange(2 * n, dtype=np.uint64)) % np.uint64(3)).reshape(n, 2)
    r = np.where(pick == 0, small, r)
    r[pick == 1] = r[pick == 1] | HI32
    return r


def _expected_r0(old, x, pick, sz):
    """r0 for CMPXCHG: half of the lanes match `old`; a 4-byte match carries
    garbage in the high word, an 8-byte miss may differ in the high word only."""
    if sz == 8:
        return np.where(pick < 2, old, np.where(pick == 2, old ^ np.uint64(1 << 40), x))
    hi = (x & HI32) | np.uint64(1 << 32)
    return np.where(pick < 2, old | hi, np.where(pick == 2, (old ^ np.uint64(0x80000000)) | hi, x))


@functools.lru_cache(maxsize=None)
def _units(n, sz, stride, groups=None):
    """groups: per lane group the size of its form (the divergence test);
    else every lane runs a form of `sz` bytes."""
    a, b, v, x = _operands(2 * n, 90 + sz).reshape(n, 4).T
    pick = gen.sm64(7, np.arange(n, dtype=np.uint64)) % np.uint64(4)
    group = gen.sm64(8, np.arange(n, dtype=np.uint64)) % np.uint64(4)
    e8, e4 = _expected_r0(b, x, pick, 8), _expected_r0(a >> np.uint64(32), x, pick, 4)
    if groups is None:
        e = e8 if sz == 8 else e4
    else:
        e = np.where(np.array(groups, dtype=np.uint64)[group.astype(np.int64)] == 8, e8, e4)
    u = gen.sm64(9, np.arange(n * (stride // 8), dtype=np.uint64)).reshape(n, stride // 8)
    u[:, 0], u[:, 1], u[:, 2], u[:, 3] = a, b, v, e
    u[:, 4] = np.arange(n, dtype=np.uint64) | (group << np.uint64(32))
    u = u.view(np.uint8).reshape(n, stride)
    u.setflags(write=False)
    return u


def _prologue(a, target, fd):
    """r6 = the unit, r7 = the 16-byte cell seeded {A, B}; r3 = operand,
    r0 = the unit's r0 for CMPXCHG."""
    a.mov64(6, "r1")
    if target == "own_staged":
        a.mov64(7, "r6").add64(7, 40)
    elif target == "own_past_window":
        a.mov64(7, "r6").add64(7, 72)
    elif target in ("lds_stack", "scratch_stack", "stack"):
        a.mov64(7, "r10").add64(7, -16)
    elif target == "map_lookup":
        a.ldx(4, 1, 6, 32).stx(4, 10, -4, "r1").ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).call(1)
        a.jmp("jeq", 0, 0, "null").mov64(7, "r0")
    else:
        a.ldx(4, 1, 6, 32).alu64("lsh", 1, 4).ld_map_value(7, fd, 0).add64(7, "r1")
    a.ldx(8, 2, 6, 0).ldx(8, 4, 6, 8).ldx(8, 3, 6, 16).ldx(8, 0, 6, 24)
    a.stx(8, 7, 0, "r2").stx(8, 7, 8, "r4")
    if target == "scratch_stack":
        a.stx(8, 10, -256, "r2")   # deeper than the LDS stack: the program runs on scratch
    # a 64-bit register move of the operand last: whatever temporaries the
    # atomic's handler inherits hold its high word, not zeros
    return a.mov64(5, "r3")


def _fold(a, target, regs):
    """r0 = 3 * cell[0:8] + 5 * cell[8:16] + 7 * each of regs + 11 * r0 (odd
    multipliers: any one wrong term changes the result).  The 8-byte reads
    cover the 4-byte target at +4 and both of its neighbours."""
    a.ldx(8, 8, 7, 0).ldx(8, 9, 7, 8)
    a.mov64(1, "r8").alu64("mul", 1, 3).mov64(2, "r9").alu64("mul", 2, 5).add64(1, "r2")
    for r in regs:
        a.mov64(2, r).alu64("mul", 2, 7).add64(1, "r2")
    a.alu64("mul", 0, 11).add64(0, "r1").exit()
    if target == "map_lookup":
        a.label("null").mov64(0, 0).exit()
    return a.assemble()


def _cell_off(sz):
    return 8 if sz == 8 else 4


def _handlers(sz, imm):
    """Handlers the loader may give the form (None: it has none, C++ runs it)."""
    if imm in (isa.ATOMIC_XCHG, isa.ATOMIC_CMPXCHG):
        return None
    op = {v: k for k, v in OPS.items()}[imm & ~isa.ATOMIC_FETCH].upper()
    if imm & isa.ATOMIC_FETCH:
        return {f"ATOM{sz}_{op}_F"}
    if op == "ADD":  # (a counter add: deferred, direct or map-value handler)
        return {f"ATOM{sz}_ADD", f"ATOMMV{sz}_ADD", f"ATOMD{sz}"}
    return {f"ATOM{sz}_{op}"}


def _map_bytes(om, dm, n):
    o = b"".join(om.lookup(struct.pack("<I", k)) for k in range(n))
    return np.frombuffer(o, dtype=np.uint8), dm.snapshot()[:len(o)]


def _both(po, dev, code, units, stride):
    n = units.shape[0]
    ovm = po.OracleVM()
    ovm.load(code)
    ou = units.copy()
    orets = ovm.run_raw(ou, stride)
    vm = dev.VM()
    vm.load(code)
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * n)
    failed = vm.exec_batch(dev.CTX_RAW, d, n, stride, fixed_len=stride, rets=dr)
    return orets, ou, dr.download(np.uint64), d.download().reshape(n, stride), failed, vm


def _check(po, dev, code, units, stride, om=None, dm=None):
    orets, ou, drets, du, failed, vm = _both(po, dev, code, units, stride)
    assert failed == 0
    np.testing.assert_array_equal(drets, orets)
    np.testing.assert_array_equal(du, ou)
    if om is not None:
        o, d = _map_bytes(om, dm, units.shape[0])
        np.testing.assert_array_equal(d, o)
    return vm


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("mode", list(MODES))
def test_atomic_matrix(fresh_oracle, fresh_runtime, monkeypatch, mode, target, form):
    """One unit, one private target: seed, atomic, read back, fold."""
    if MODES[mode]:
        monkeypatch.setenv(MODES[mode], "1")
    po, dev = fresh_oracle, fresh_runtime
    _, sz, imm, src = form
    stride = 128 if target == "own_past_window" else 64
    om = dm = None
    if target.startswith("map"):
        (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 16, N)], po, dev)
    a = _prologue(Asm(), target, dm.fd if dm else -1)
    at = a.pc
    a.atomic(sz, imm, 7, _cell_off(sz), src)
    code = _fold(a, target, [] if src == "r0" else [src])
    vm = _check(po, dev, code, _units(N, sz, stride), stride, om, dm)
    assert vm.info()["big_stack"] == (target == "scratch_stack")
    want = _handlers(sz, imm)
    if mode == "default" and want and target in ("own_past_window", "map_lookup", "map_value_lddw"):
        assert vm.fast_handler(dev.CTX_RAW, at) in want   # the asm tier ran it, not C++


ALIAS_FORMS = [(f"{name}{sz * 8}", sz, imm, name) for sz in (8, 4) for name, imm in
               [("add_fetch", isa.ATOMIC_ADD | isa.ATOMIC_FETCH), ("xor_fetch", isa.ATOMIC_XOR | isa.ATOMIC_FETCH),
                ("xchg", isa.ATOMIC_XCHG), ("cmpxchg", isa.ATOMIC_CMPXCHG)]]


@pytest.mark.parametrize("form", ALIAS_FORMS, ids=[f[0] for f in ALIAS_FORMS])
@pytest.mark.parametrize("target", ["own_past_window", "stack", "map_lookup"])
def test_atomic_src_is_dst(fresh_oracle, fresh_runtime, target, form):
    """The operand register is the address register: the operand is the
    pointer, the address is taken before the fetched value lands in it.
    Pointers differ between oracle and device, so the program takes the
    pointer back out of what it read (old + p - p, old ^ p ^ p, p ^ p) and
    puts the cell's bytes back before it exits.  (A stack pointer used as an
    operand escapes the loader's depth analysis: that program runs on the
    scratch stack.)"""
    po, dev = fresh_oracle, fresh_runtime
    _, sz, imm, name = form
    stride = 128 if target == "own_past_window" else 64
    om = dm = None
    if target == "map_lookup":
        (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 16, N)], po, dev)
    a = _prologue(Asm(), target, dm.fd if dm else -1)
    a.mov64(5, "r7").add64(5, _cell_off(sz)).mov64(9, "r5")
    a.atomic(sz, imm, 5, 0, "r5")
    a.ldx(sz, 8, 9, 0)
    alu = a.alu64 if sz == 8 else a.alu32
    if name == "add_fetch":
        alu("sub", 8, "r9")
    elif name != "cmpxchg":
        alu("xor", 8, "r9")
    else:
        a.mov64(8, 0).mov64(5, 0)    # (memory holds p where r0 matched; r5 is still p)
    a.stx(sz, 9, 0, "r2").mov64(3, "r8")
    code = _fold(a, target, ["r3", "r5"])
    vm = _check(po, dev, code, _units(N, sz, stride), stride, om, dm)
    assert vm.info()["big_stack"] == (target == "stack")


FAMILIES = {
    op: [(8, imm), (8, imm | isa.ATOMIC_FETCH), (4, imm), (4, imm | isa.ATOMIC_FETCH)] for op, imm in OPS.items()
}
FAMILIES["swap"] = [(8, isa.ATOMIC_XCHG), (4, isa.ATOMIC_CMPXCHG), (8, isa.ATOMIC_CMPXCHG), (4, isa.ATOMIC_XCHG)]


@pytest.mark.parametrize("asm_groups", [True, False], ids=["asm_lane_groups", "cpp_lane_groups"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_atomics_in_lane_groups(fresh_oracle, fresh_runtime, monkeypatch, family, asm_groups):
    """Four lane groups (a unit byte) run four forms of one family on the
    unit's map value, reconverge, and run one more fetch form."""
    if not asm_groups:
        monkeypatch.setenv("BPFTIME_AMD_NO_ASM_DIVERGENCE", "1")
    po, dev = fresh_oracle, fresh_runtime
    n = 4096
    (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 16, n)], po, dev)
    forms = FAMILIES[family]
    a = _prologue(Asm(), "map_lookup", dm.fd)
    a.ldx(1, 5, 6, 36)
    for g in range(3):
        a.jmp("jeq", 5, g, f"g{g}")
    for g in (3, 0, 1, 2):
        if g != 3:
            a.label(f"g{g}")
        a.atomic(forms[g][0], forms[g][1], 7, _cell_off(forms[g][0]), "r3").ja("join")
    a.label("join")
    last = isa.ATOMIC_XCHG if family == "swap" else OPS[family] | isa.ATOMIC_FETCH
    a.atomic(8, last, 7, 8, "r4")
    code = _fold(a, "map_lookup", ["r3", "r4"])
    units = _units(n, 8, 64, tuple(f[0] for f in forms))
    assert len(np.unique(units[:64, 36])) >= 3           # the first wave splits
    _check(po, dev, code, units, 64, om, dm)


# ---- shared addresses: every lane hits value[unit & 3] of a 4-entry map ----
# value: the 8-byte target @0, the 4-byte target @8, its neighbour @12
NS = 4096


def _shared(po, dev, sz, imm, operand, r0=None, seed=0):
    """Runs `atomic [value + (0 | 8)], r3` from NS units (r3 = operand[unit],
    r0 = r0[unit]) and returns (oracle, device) x (rets, the 4 values)."""
    (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 16, 4)], po, dev)
    for k in range(4):
        v = struct.pack("<QII", seed if sz == 8 else 0x1111111111111111, seed if sz == 4 else 0x22222222, 0x33333333)
        om.update(struct.pack("<I", k), v)
        dm.update(struct.pack("<I", k), v)
    units = np.zeros((NS, 8), dtype=np.uint64)
    units[:, 0] = operand
    units[:, 1] = r0 if r0 is not None else 0
    units[:, 2] = np.arange(NS, dtype=np.uint64) & np.uint64(3)
    units = units.view(np.uint8).reshape(NS, 64)
    a = Asm().mov64(6, "r1").ldx(4, 1, 6, 16).stx(4, 10, -4, "r1").ld_map_fd(1, dm.fd).mov64(2, "r10").add64(2, -4)
    a.call(1).jmp("jeq", 0, 0, "null").mov64(7, "r0").ldx(8, 3, 6, 0).ldx(8, 0, 6, 8)
    a.mov64(5, "r3")               # (the handler's temporaries now hold the operand's high word)
    at = a.pc
    a.atomic(sz, imm, 7, 0 if sz == 8 else 8, "r3")
    if imm != isa.ATOMIC_CMPXCHG:
        a.mov64(0, "r3")
    a.exit().label("null").mov64(0, -1).exit()
    orets, ou, drets, du, failed, vm = _both(po, dev, a.assemble(), units, 64)
    assert failed == 0
    np.testing.assert_array_equal(du, ou)
    want = _handlers(sz, imm)
    if want:
        assert vm.fast_handler(dev.CTX_RAW, at) in want
    vals = [[m.lookup(struct.pack("<I", k)) for k in range(4)] for m in (om, dm)]
    # whatever the order: nothing but the target changed
    for k in range(4):
        keep = slice(8, 16) if sz == 8 else slice(0, 8)
        assert vals[1][k][keep] == vals[0][k][keep] and vals[1][k][12:] == vals[0][k][12:]
    tgt = [[int.from_bytes(v[0:8] if sz == 8 else v[8:12], "little") for v in side] for side in vals]
    return orets, drets, tgt[0], tgt[1]


def _garbage_high(v, sz):
    """A 4-byte form must ignore the operand's high word."""
    return v if sz == 8 else (v & M32) | HI32


@pytest.mark.parametrize("sz", [8, 4])
@pytest.mark.parametrize("op", list(OPS))
def test_shared_commutative(fresh_oracle, fresh_runtime, op, sz):
    """Plain ADD / OR / AND / XOR commute: the final values are the oracle's."""
    v = _operands(NS, 40 + sz)[:, 0]
    seed = ((1 << (8 * sz)) - 1) if op == "and" else 0x0123456789ABCDEF & ((1 << (8 * sz)) - 1)
    orets, drets, ofin, dfin = _shared(fresh_oracle, fresh_runtime, sz, OPS[op], v, seed=seed)
    assert dfin == ofin
    np.testing.assert_array_equal(drets, orets)          # (the operand comes back untouched)


@pytest.mark.parametrize("sz", [8, 4])
def test_shared_fetch_add_hands_out_every_value_once(fresh_oracle, fresh_runtime, sz):
    seed = 0 if sz == 8 else 0xFFFFFFF0                   # the 4-byte counter wraps
    one = _garbage_high(np.full(NS, 1, dtype=np.uint64), sz)
    _, drets, ofin, dfin = _shared(fresh_oracle, fresh_runtime, sz, isa.ATOMIC_ADD | isa.ATOMIC_FETCH, one, seed=seed)
    assert dfin == ofin
    mask = (1 << (8 * sz)) - 1
    for k in range(4):
        got = np.sort(drets[k::4])
        want = np.sort(np.array([(seed + i) & mask for i in range(NS // 4)], dtype=np.uint64))
        np.testing.assert_array_equal(got, want)         # (4-byte: zero-extended, or it is not in `want`)
        assert dfin[k] == (seed + NS // 4) & mask


@pytest.mark.parametrize("sz", [8, 4])
def test_shared_xchg_is_a_permutation(fresh_oracle, fresh_runtime, sz):
    seed = 0xDEAD000000000000 if sz == 8 else 0x80000000
    ids = np.arange(1, NS + 1, dtype=np.uint64)
    _, drets, _, dfin = _shared(fresh_oracle, fresh_runtime, sz, isa.ATOMIC_XCHG, _garbage_high(ids, sz), seed=seed)
    for k in range(4):
        got = np.sort(np.append(drets[k::4], np.uint64(dfin[k])))
        want = np.sort(np.append(ids[k::4], np.uint64(seed)))
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("sz", [8, 4])
def test_shared_cmpxchg_one_claim_wins(fresh_oracle, fresh_runtime, sz):
    ids = np.arange(1, NS + 1, dtype=np.uint64)
    r0 = np.zeros(NS, dtype=np.uint64) if sz == 8 else np.full(NS, HI32, dtype=np.uint64)  # low word 0
    _, drets, _, dfin = _shared(fresh_oracle, fresh_runtime, sz, isa.ATOMIC_CMPXCHG, _garbage_high(ids, sz), r0=r0)
    for k in range(4):
        r, mine = drets[k::4], ids[k::4]
        won = np.flatnonzero(r == 0)
        assert len(won) == 1
        assert dfin[k] == mine[won[0]]
        assert (np.delete(r, won[0]) == np.uint64(dfin[k])).all()


@pytest.mark.parametrize("sz", [8, 4])
@pytest.mark.parametrize("op", ["or", "and", "xor"])
def test_shared_fetch_bit_ops(fresh_oracle, fresh_runtime, op, sz):
    """Single-bit operands.  OR / AND: a fetched value differs from the final
    one only in bits some unit of the key set / cleared.  XOR: the units
    toggling one bit see it alternate from the seed's, so exactly
    (count + seed bit) // 2 of them fetch it set."""
    bits = [0, 5, 31, 32, 47, 63] if sz == 8 else [0, 5, 16, 31]
    mask = (1 << (8 * sz)) - 1
    bit = np.array(bits, dtype=np.uint64)[(np.arange(NS) // 4) % len(bits)]
    one = np.uint64(1) << bit
    seed = mask if op == "and" else 0 if op == "or" else 0x8000000080000021 & mask
    v = one ^ np.uint64(mask) if op == "and" else one
    _, drets, ofin, dfin = _shared(fresh_oracle, fresh_runtime, sz, OPS[op] | isa.ATOMIC_FETCH,
                                   _garbage_high(v, sz), seed=seed)
    assert dfin == ofin
    assert (drets >> np.uint64(8 * sz - 1) >> np.uint64(1) == 0).all()       # zero-extended
    for k in range(4):
        r, b = drets[k::4], bit[k::4]
        touched = np.bitwise_or.reduce(one[k::4])
        if op != "xor":
            assert ((r ^ np.uint64(dfin[k])) & ~touched == 0).all()
            fin = np.uint64(dfin[k])
            assert ((r & ~fin if op == "or" else ~r & fin) == 0).all()       # bits only get set / cleared
            continue
        for x in bits:
            mine = r[b == x]
            assert int(((mine >> np.uint64(x)) & np.uint64(1)).sum()) == (len(mine) + ((seed >> x) & 1)) // 2, (k, x)


@pytest.mark.parametrize("sz", [8, 4])
@pytest.mark.parametrize("name,imm", [("add_fetch", isa.ATOMIC_ADD | isa.ATOMIC_FETCH), ("xchg", isa.ATOMIC_XCHG),
                                      ("cmpxchg", isa.ATOMIC_CMPXCHG)], ids=["add_fetch", "xchg", "cmpxchg"])
def test_oob_atomic_fails_lane_not_gpu(fresh_runtime, name, imm, sz):
    """An atomic through a wild pointer fails its lane like any other
    access outside the window (test_oob_access_fails_lane_not_gpu)."""
    dev = fresh_runtime
    a = Asm().ldx(8, 2, 1, 0).jmp("jeq", 2, 0, "ok").lddw(3, 0x1000).mov64(4, 7).mov64(0, 0)
    a.atomic(sz, imm, 3, 0, "r4").mov64(0, "r4").exit()
    a.label("ok").mov64(0, 5).exit()
    vm = dev.VM()
    vm.load(a.assemble())
    n = 256
    units = np.zeros((n, 8), dtype=np.uint8)
    units[::2, 0] = 1
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * n)
    failed = vm.exec_batch(dev.CTX_RAW, d, n, 8, fixed_len=8, rets=dr)
    r = dr.download(np.uint64)
    assert failed == n // 2
    assert (r[1::2] == 5).all() and (r[::2] == 0).all()
