"""Deferred counter adds at small shapes: counter shapes x address patterns x
launch plans, bit-exact against the oracle and against an independent numpy
total (np.add.at in wrapping arithmetic on the initial bytes).

What is under test: the two-entry per-wave delta cache (gen_fast.py
counter_cache), the per-block LDS combining table (comb_add, comb_peel, the
fused atomic pair), the three block-end flush paths (interp.hip: no log when
grid <= kMergeGroup; the flush log and k_comb_merge; a block that holds more
than kMergeEntries / 8 nonzero deltas adds them itself), the miss log and
k_miss_merge, and the launch plan exec_batch builds around them.  Every case
asserts the plan it ran on through VM.last_launch() and its sites' handlers
through VM.fast_handler / VM.counter_info.

Every program ends without reading a counter, so the loader defers each add.
Every 4-byte counter starts in [0xFFFFFFF0, 0xFFFFFFFF], every 8-byte counter
within 16 of 2^64, the bytes between them hold a random pattern: every
counter wraps, a carry or a stray write into a neighbour shows.

Unit (64 bytes): u32 key @0, u8 branch byte @4, u64 value @8, random rest."""
import functools
import struct

import numpy as np
import pytest

from bpftime_amd import gen, isa
from bpftime_amd.isa import Asm

from _helpers import make_maps

pytestmark = pytest.mark.gpu

STRIDE = 64
VSIZE = 64            # four 16-byte granules per value
NCPU = 8              # (PERCPU_ARRAY cases)
K_MERGE_GROUP = 16    # common.hpp kMergeGroup
K_SELF_FLUSH = 512    # kMergeEntries / 8

# ---- programs: (kind, bytes, value offset) sites, run in this order -------
# kind "rmw": ldx/add/stx (the loader fuses it); "atomic": BPF_ATOMIC add
# without fetch.  Adjacent 8-byte atomics at off, off + 8 become a fused pair
# (loader.cpp), so the single atomics are listed in an order that never pairs.
PROGRAMS = {
    "rmw8": [("rmw", 8, 0), ("rmw", 8, 8), ("rmw", 8, 24)],
    "rmw4": [("rmw", 4, 0), ("rmw", 4, 4), ("rmw", 4, 8), ("rmw", 4, 12), ("rmw", 4, 20)],
    "atom8": [("atomic", 8, 0), ("atomic", 8, 24), ("atomic", 8, 8)],
    "atom4": [("atomic", 4, 0), ("atomic", 4, 4), ("atomic", 4, 8), ("atomic", 4, 12), ("atomic", 4, 20)],
    "pair0": [("atomic", 8, 0), ("atomic", 8, 8)],
    # the pair at (8, 16) straddles a granule; then single counters at 16 and 24
    "pair8": [("atomic", 8, 8), ("atomic", 8, 16), ("rmw", 8, 16), ("rmw", 8, 24)],
    # 4-byte and 8-byte sites on one granule (separate table entries: tag bit 0)
    "mix48": [("rmw", 4, 0), ("atomic", 4, 4), ("atomic", 8, 8), ("rmw", 8, 0 + 16), ("atomic", 4, 24)],
    # wave-uniform constant addresses (lddw of the map value + offset): the
    # third distinct one finds both wave-cache entries taken
    "const3": [("rmw", 8, 0), ("rmw", 4, 20), ("rmw", 8, 24)],
    "const4": [("rmw", 8, 0), ("rmw", 4, 20), ("rmw", 8, 24), ("rmw", 4, 8)],
}
# branch programs: lanes with an odd branch byte run the first list, the others
# the second, all of them the third after the join
BRANCHED = {
    "br_rmw": ([("rmw", 8, 0), ("rmw", 4, 20)], [("rmw", 4, 8), ("rmw", 8, 24)], [("rmw", 4, 12)]),
    "br_atom": ([("atomic", 8, 0), ("atomic", 8, 8)], [("atomic", 4, 20), ("atomic", 8, 24)], [("atomic", 4, 4)]),
}
# values: "imm1" / "immneg1" immediates, "lane" per-lane with random high words,
# "wave" equal within a wave and different between waves
# per-wave address patterns: (name, number of elements)
ADDRS = {"one": 1, "d2": 5, "d4": 5, "d5": 5, "d64": 64, "k1": 1, "k5": 5, "k300": 300, "k5000": 5000}


def _sites_of(prog):
    """[(kind, sz, off, group)]: group 0 / 1 = the branch arm, 2 = every lane."""
    if prog in PROGRAMS:
        return [(k, s, o, 2) for k, s, o in PROGRAMS[prog]]
    a, b, c = BRANCHED[prog]
    return [(k, s, o, 0) for k, s, o in a] + [(k, s, o, 1) for k, s, o in b] + [(k, s, o, 2) for k, s, o in c]


def _emit_site(a, site, value):
    kind, sz, off, _ = site
    if kind == "rmw":
        at = a.pc
        a.ldx(sz, 2, 7, off)
        a.add64(2, {"imm1": 1, "immneg1": -1}.get(value, "r3"))
        a.stx(sz, 7, off, "r2")
    else:
        at = a.pc
        a.atomic(sz, isa.ATOMIC_ADD, 7, off, "r3")
    return at


def build_program(prog, fd, target, value, xdp):
    """-> (code, [pc of each site]).  r6 = the unit, r7 = the value the sites
    add to (a map_lookup_elem of the unit's key, or the constant address of
    element 0), r3 = the unit's u64 value or the immediate; r0 = key + 3 * branch byte."""
    a = Asm()
    if xdp:
        a.ldx(8, 6, 1, 0).ldx(8, 3, 1, 8).mov64(4, "r6").add64(4, 16).mov64(0, 0).jmp("jgt", 4, "r3", "out")
    else:
        a.mov64(6, "r1")
    if target == "const":
        a.ld_map_value(7, fd, 0)
    else:
        a.ldx(4, 1, 6, 0).stx(4, 10, -4, "r1").ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4)
        a.call(isa.BPF_FUNC_map_lookup_elem).mov64(7, "r0").mov64(0, 0).jmp("jeq", 7, 0, "out")
    if value in ("imm1", "immneg1"):
        a.mov64(3, 1 if value == "imm1" else -1)   # (an atomic's operand is a register)
    else:
        a.ldx(8, 3, 6, 8)
    sites = _sites_of(prog)
    pcs = []
    if prog in BRANCHED:
        a.ldx(1, 5, 6, 4).alu64("and", 5, 1).jmp("jeq", 5, 0, "even")
        pcs += [_emit_site(a, s, value) for s in sites if s[3] == 0]
        a.ja("join").label("even")
        pcs += [_emit_site(a, s, value) for s in sites if s[3] == 1]
        a.label("join")
        pcs += [_emit_site(a, s, value) for s in sites if s[3] == 2]
    else:
        pcs = [_emit_site(a, s, value) for s in sites]
    a.ldx(4, 0, 6, 0).ldx(1, 5, 6, 4).alu64("mul", 5, 3).add64(0, "r5").alu64("and", 0, 0xFFFF)
    a.label("out").exit()
    return a.assemble(), pcs


def want_handler(site, target, value, paired):
    kind, sz, _, _ = site
    k = "I" if value in ("imm1", "immneg1") else "R"
    if kind == "rmw":
        return {f"RMWK{sz}_{k}"} if target == "const" else {f"RMWMV{sz}_{k}"}
    if paired:
        return {"ATOMMV8_ADD2"}
    return {f"ATOMMV{sz}_ADD"}


def paired_sites(sites, no_pair=False):
    """Indices of the first halves of the loader's fused atomic pairs."""
    out, i = set(), 0
    while i + 1 < len(sites) and not no_pair:
        s, t = sites[i], sites[i + 1]
        if s[0] == t[0] == "atomic" and s[1] == t[1] == 8 and t[2] == s[2] + 8 and s[3] == t[3]:
            out.add(i)
            i += 2
        else:
            i += 1
    return out


# ---- inputs -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_units(n, addr, value):
    """(units, element index per unit, added value per unit, branch arm)."""
    idx = np.arange(n, dtype=np.uint64)
    lane, wave = idx % np.uint64(64), idx // np.uint64(64)
    nelem = ADDRS[addr]
    if addr.startswith("k"):
        e = gen.sm64(21, idx) % np.uint64(nelem)
    elif addr == "one":
        e = np.zeros(n, dtype=np.uint64)
    elif addr == "d64":
        e = lane.copy()
    else:
        d = np.uint64(int(addr[1:]))
        e = (lane % d + wave) % np.uint64(nelem)      # d distinct counters per wave, rotated per wave
    if value == "lane":
        v = gen.sm64(22, idx)                          # random high words
        v[::7] = np.uint64(0xFFFFFFFF00000000) | (v[::7] & np.uint64(0xFF))
        v[3::11] = np.uint64(2 ** 64 - 1) - (v[3::11] & np.uint64(0xFF))   # small negatives
    elif value == "wave":
        v = gen.sm64(23, wave) | np.uint64(1 << 63)    # equal within a wave, differs between waves
    else:
        v = np.full(n, 1 if value == "imm1" else 2 ** 64 - 1, dtype=np.uint64)
    u = gen.sm64(24, np.arange(n * 8, dtype=np.uint64)).reshape(n, 8)
    u[:, 0] = e | ((u[:, 0] >> np.uint64(32)) << np.uint64(32))
    u[:, 1] = v
    u = u.view(np.uint8).reshape(n, STRIDE)
    arm = 1 - (u[:, 4] & 1).astype(np.int64)           # odd byte: arm 0
    for x in (u, e, v, arm):
        x.setflags(write=False)
    return u, e.astype(np.int64), v, arm


def key_of(mtype, e):
    """The map key of element e: the index, or a scattered u32 on HASH."""
    return int(e) if mtype != isa.BPF_MAP_TYPE_HASH else (int(e) * 2654435761 + 12345) & 0xFFFFFFFF


def initial_values(nelem, sites, ncopies, seed=31):
    """[nelem, ncopies, VSIZE] bytes: random, counters about to wrap."""
    raw = gen.sm64(seed, np.arange(nelem * ncopies * VSIZE // 8, dtype=np.uint64)).view(np.uint8)
    raw = raw.reshape(nelem, ncopies, VSIZE).copy()
    r = gen.sm64(seed + 1, np.arange(nelem * ncopies * 16, dtype=np.uint64)).reshape(nelem, ncopies, 16) % np.uint64(16)
    for _, sz, off, _ in sites:
        if sz == 4:
            raw.view(np.uint32)[:, :, off // 4] = (np.uint64(0xFFFFFFF0) + r[:, :, off // 4]).astype(np.uint32)
        else:
            raw.view(np.uint64)[:, :, off // 8] = np.uint64(2 ** 64 - 1) - r[:, :, off // 8]
    return raw


def numpy_total(init, sites, e, v, arm, cpu):
    """The final bytes from the inputs alone: every add wraps in its width."""
    out = init.copy()
    for _, sz, off, grp in sites:
        m = np.ones(len(e), dtype=bool) if grp == 2 else arm == grp
        if sz == 4:
            np.add.at(out.view(np.uint32)[:, :, off // 4], (e[m], cpu[m]), v[m].astype(np.uint32))
        else:
            np.add.at(out.view(np.uint64)[:, :, off // 8], (e[m], cpu[m]), v[m])
    return out


def touched_mask(sites):
    m = np.zeros(VSIZE, dtype=bool)
    for _, sz, off, _ in sites:
        m[off:off + sz] = True
    return m


# ---- one run ----------------------------------------------------------------
MAP_TYPES = {"array": isa.BPF_MAP_TYPE_ARRAY, "hash": isa.BPF_MAP_TYPE_HASH, "percpu": isa.BPF_MAP_TYPE_PERCPU_ARRAY}


def run_case(po, dev, prog, mtype, target, value, addr, n, xdp=False, ordered=False, no_pair=False):
    """Builds the maps, runs oracle and device, compares rets, units and every
    value byte with the oracle and the numpy total; -> (vm, launch info, e)."""
    mt = MAP_TYPES[mtype]
    percpu = mtype == "percpu"
    ncopies = NCPU if percpu else 1
    if percpu:
        po.set_ncpu(NCPU)
        dev.set_ncpu(NCPU)
    nelem = 1 if target == "const" else ADDRS[addr]
    (om,), (dm,) = make_maps([(mt, 4, VSIZE, nelem if mt != isa.BPF_MAP_TYPE_HASH else 2 * nelem)], po, dev)
    sites = _sites_of(prog)
    init = initial_values(nelem, sites, ncopies)
    keys = [struct.pack("<I", key_of(mt, k)) for k in range(nelem)]
    for k in range(nelem):
        for m in (om, dm):
            assert m.update(keys[k], init[k].tobytes()) == 0
    units, e, v, arm = make_units(n, addr, value)
    if target == "const":
        e = np.zeros(n, dtype=np.int64)
    elif mt == isa.BPF_MAP_TYPE_HASH:
        units = units.copy()
        units.view(np.uint32)[:, 0] = np.array([key_of(mt, x) for x in range(nelem)], dtype=np.uint32)[e]
    code, pcs = build_program(prog, dm.fd, target, value, xdp)
    if prog not in BRANCHED:
        arm = np.full(n, 2, dtype=np.int64)
    cpu = (np.arange(n) // 64) % NCPU if percpu else np.zeros(n, dtype=np.int64)

    ovm = po.OracleVM()
    ovm.load(code)
    ou = units.copy()
    if percpu:   # the unit's virtual CPU is (unit // 64) % ncpu on both sides
        orets = np.zeros(n, dtype=np.uint32 if xdp else np.uint64)
        for w0 in range(0, n, 64):
            po.set_cpu((w0 // 64) % NCPU)
            s = ou[w0:w0 + 64]
            orets[w0:w0 + 64] = ovm.run_xdp(s, fixed_len=STRIDE) if xdp else ovm.run_raw(s, STRIDE)
    else:
        orets = ovm.run_xdp(ou, fixed_len=STRIDE) if xdp else ovm.run_raw(ou, STRIDE)

    vm = dev.VM()
    vm.load(code)
    kind = dev.CTX_XDP if xdp else dev.CTX_RAW
    # every site is a counter add the loader defers, on the handler it claims
    assert vm.counter_info(kind) == (len(sites), 0)
    pairs = paired_sites(sites, no_pair)
    for i, (s, pc) in enumerate(zip(sites, pcs)):
        if i - 1 in pairs:
            continue                    # (the pair's second half: run by the first's dispatch)
        assert vm.fast_handler(kind, pc) in want_handler(s, target, value, i in pairs), (i, s)
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer((4 if xdp else 8) * n)
    flags = dev.BATCH_SYNC | (dev.BATCH_ORDERED if ordered else 0)
    if xdp:
        failed = vm.exec_batch(kind, d, n, STRIDE, fixed_len=STRIDE, verdicts=dr, flags=flags)
    else:
        failed = vm.exec_batch(kind, d, n, STRIDE, fixed_len=STRIDE, rets=dr, flags=flags)
    assert failed == 0
    np.testing.assert_array_equal(dr.download(np.uint32 if xdp else np.uint64), orets)
    np.testing.assert_array_equal(d.download().reshape(n, STRIDE), ou)

    want = numpy_total(init, sites, e, v, arm, cpu)
    got_o = np.stack([np.frombuffer(om.lookup(k), dtype=np.uint8).reshape(ncopies, VSIZE) for k in keys])
    got_d = np.stack([np.frombuffer(dm.lookup(k), dtype=np.uint8).reshape(ncopies, VSIZE) for k in keys])
    np.testing.assert_array_equal(got_o, want)            # the two references agree
    np.testing.assert_array_equal(got_d, got_o)           # the device is bit-exact
    keep = ~touched_mask(sites)
    np.testing.assert_array_equal(got_d[:, :, keep], init[:, :, keep])
    li = vm.last_launch()
    assert li["units"] == n and li["ordered"] == ordered
    return vm, li, e


def default_plan(li, n, comb=True, xdp=False):
    """The plan a parallel launch of these programs gets with no switch set:
    1024-lane blocks and the register copy (an XDP ctx too) in global memory
    when the launch holds a combining table, else 256-lane blocks."""
    block = 1024 if comb else 256
    assert not li["ordered"] and li["block"] == block and li["grid"] == -(-n // block)
    assert li["gregs"] == comb and li["gctx"] == (xdp and comb)
    assert (li["comb_entries"] >= 512) if comb else (li["comb_entries"] == 0)
    assert li["flush_log"] == (comb and li["grid"] > K_MERGE_GROUP)
    assert not li["miss_log"] and li["miss_cap"] == 0 and li["occupancy"] >= 1


def ordered_plan(li):
    assert li["ordered"] and li["grid"] == 1 and li["comb_entries"] == 0
    assert not li["flush_log"] and not li["miss_log"] and not li["gregs"] and not li["gctx"]


# ---- the shapes: every one runs on the default plan and ORDERED -------------
# (program, map, target, value, address pattern, n, xdp)
SHAPES = []
for _p, _v, _a, _n in [("rmw8", "imm1", "one", 64), ("rmw8", "immneg1", "d2", 65), ("rmw8", "lane", "d5", 1025),
                       ("rmw8", "wave", "d64", 1025), ("rmw8", "lane", "k300", 1025),
                       ("rmw8", "lane", "k5000", 20000),
                       ("rmw4", "imm1", "d4", 63), ("rmw4", "immneg1", "one", 1025), ("rmw4", "lane", "d5", 65),
                       ("rmw4", "wave", "k5", 1025), ("rmw4", "lane", "d64", 1025),
                       ("atom8", "imm1", "d5", 1025), ("atom8", "immneg1", "d64", 64), ("atom8", "lane", "one", 65),
                       ("atom8", "wave", "d2", 1025), ("atom8", "lane", "k1", 1),
                       ("atom4", "imm1", "one", 1025), ("atom4", "immneg1", "d5", 1025), ("atom4", "lane", "d4", 63),
                       ("atom4", "wave", "d64", 65), ("atom4", "lane", "k300", 1025),
                       ("pair0", "imm1", "d2", 1025), ("pair0", "lane", "d5", 1025), ("pair0", "wave", "one", 65),
                       ("pair8", "imm1", "one", 64), ("pair8", "immneg1", "d4", 1025), ("pair8", "lane", "d5", 1025),
                       ("pair8", "wave", "d64", 1025), ("pair8", "lane", "k5", 1),
                       ("mix48", "imm1", "d5", 1025), ("mix48", "immneg1", "one", 65), ("mix48", "lane", "d2", 1025),
                       ("mix48", "wave", "k300", 1025)]:
    SHAPES.append((_p, "array", "lookup", _v, _a, _n, False))
for _p in ("const3", "const4"):
    for _v, _n in [("imm1", 1025), ("immneg1", 65), ("lane", 1025), ("wave", 1025)]:
        SHAPES.append((_p, "array", "const", _v, "one", _n, False))
# a subset again on HASH (key from the unit), PERCPU_ARRAY and as an XDP program
SHAPES += [("rmw4", "hash", "lookup", "lane", "d5", 1025, False), ("pair8", "hash", "lookup", "wave", "k300", 1025, False),
           ("mix48", "hash", "lookup", "immneg1", "d64", 65, False),
           ("rmw8", "percpu", "lookup", "lane", "d5", 1025, False), ("atom4", "percpu", "lookup", "imm1", "one", 1025, False),
           ("pair8", "percpu", "lookup", "wave", "k5", 65, False),
           ("rmw8", "array", "lookup", "lane", "d4", 1025, True), ("pair0", "array", "lookup", "immneg1", "k5", 65, True)]
SHAPE_IDS = ["-".join(str(x) for x in s[:6]) + ("-xdp" if s[6] else "") for s in SHAPES]


@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_counter_shape(fresh_oracle, fresh_runtime, shape, ordered):
    prog, mtype, target, value, addr, n, xdp = shape
    _, li, _ = run_case(fresh_oracle, fresh_runtime, prog, mtype, target, value, addr, n, xdp=xdp, ordered=ordered)
    if ordered:
        ordered_plan(li)
    else:
        # per-lane values on a constant address still go through the table
        # code, with no table: the launch holds none when no site needs one
        default_plan(li, n, comb=target != "const", xdp=xdp)


@pytest.mark.parametrize("asm_groups", [True, False], ids=["asm_lane_groups", "cpp_lane_groups"])
@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered"])
@pytest.mark.parametrize("value", ["imm1", "lane"])
@pytest.mark.parametrize("prog", list(BRANCHED))
def test_counters_behind_a_branch(fresh_oracle, fresh_runtime, monkeypatch, prog, value, ordered, asm_groups):
    """The adds behind a branch on a unit byte: exec is partial and lane
    groups are pending, in the asm tier's divergence handling and in the
    C++ tier's (BPFTIME_AMD_NO_ASM_DIVERGENCE).  That switch is a kernel
    parameter (fast_div) neither the launch info nor the handlers show: the
    cpp_lane_groups cases are parity-only for it."""
    if not asm_groups:
        monkeypatch.setenv("BPFTIME_AMD_NO_ASM_DIVERGENCE", "1")
    n = 1025
    units, _, _, arm = make_units(n, "d5", value)
    assert 8 < int(arm[:64].sum()) < 56                 # the first wave splits
    _, li, _ = run_case(fresh_oracle, fresh_runtime, prog, "array", "lookup", value, "d5", n, ordered=ordered)
    ordered_plan(li) if ordered else default_plan(li, n)


# ---- sizes: the three block-end flush paths, many units per lane -------------
def block_slices(li, n):
    """Unit ranges per block of a launch whose grid covers the batch once."""
    assert li["grid"] == -(-n // li["block"])
    return [(b * li["block"], min(n, (b + 1) * li["block"])) for b in range(li["grid"])]


def distinct_counters(sites, e, v, arm, lo, hi):
    """Counters a block's units leave a nonzero delta on, and the granules
    (16 bytes; a pair site its own 8-byte-aligned 16) they touch."""
    counters, granules = set(), set()
    for _, sz, off, grp in sites:
        m = np.ones(hi - lo, dtype=bool) if grp == 2 else arm[lo:hi] == grp
        mask = np.uint64(2 ** (8 * sz) - 1)
        tot = {}
        for el, val in zip(e[lo:hi][m], v[lo:hi][m]):
            tot[el] = (tot.get(el, 0) + int(val)) & int(mask)
        counters |= {(el, off) for el, t in tot.items() if t}
        granules |= {(el, off // 16, sz) for el in tot}
    return len(counters), len(granules)


FLUSH = [  # (id, program, address pattern, n, env, the path)
    ("no_log", "rmw8", "k300", 1025, {}, "direct"),
    ("logged", "pair0", "k5", 20000, {}, "logged"),
    ("logged_4byte", "atom4", "k5", 20000, {}, "logged"),
    ("self_flush", "rmw8", "k5000", 20000, {}, "self"),
    ("logged_block256", "pair0", "k5", 5000, {"BPFTIME_AMD_BLOCK": "256"}, "logged"),
    ("no_merge", "pair0", "k5", 20000, {"BPFTIME_AMD_NO_MERGE": "1"}, "direct"),
]


@pytest.mark.parametrize("case", FLUSH, ids=[c[0] for c in FLUSH])
def test_block_end_flush_paths(fresh_oracle, fresh_runtime, monkeypatch, case):
    """interp.hip's block-end flush: straight to memory (grid <= kMergeGroup,
    or BPFTIME_AMD_NO_MERGE), through the flush log and k_comb_merge (a grid
    just above kMergeGroup blocks: a merge that covered only its first block
    would lose the other blocks' adds), or added by the block itself (more
    than 512 nonzero deltas).  The host checks on the input which it is: a
    block's distinct nonzero counters bound what its table and wave caches
    can hold from above; for the self-flush case the block's input has more
    than 512 of them on at least twice as many granules as the table has
    entries.  (The kernel's condition is on what the table and wave caches
    hold at the end.  A resident granule holds one nonzero 8-byte delta, the
    value's first granule two (offsets 0 and 8), so a table of 512 entries
    that filled up holds more than 512 deltas as soon as one entry is a
    first granule; that it fills up follows from the sets' occupancy -- over
    1024 granules on 64 sets of 8 ways -- not from the inequality alone.)"""
    _, prog, addr, n, env, path = case
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    _, li, e = run_case(fresh_oracle, fresh_runtime, prog, "array", "lookup", "lane", addr, n)
    assert li["block"] == (256 if "BPFTIME_AMD_BLOCK" in env else 1024)
    _, _, v, _ = make_units(n, addr, "lane")
    arm = np.full(n, 2)
    sites = _sites_of(prog)
    if path == "direct":
        assert not li["flush_log"]
        assert li["grid"] <= K_MERGE_GROUP or "BPFTIME_AMD_NO_MERGE" in env
        assert "BPFTIME_AMD_NO_MERGE" not in env or li["grid"] > K_MERGE_GROUP
        return
    assert li["flush_log"] and li["grid"] > K_MERGE_GROUP
    counts = [distinct_counters(sites, e, v, arm, lo, hi) for lo, hi in block_slices(li, n)]
    if path == "logged":
        assert all(c + 2 * li["block"] // 64 <= K_SELF_FLUSH for c, _ in counts)   # (+ the wave caches' entries)
    else:
        assert all(c > K_SELF_FLUSH and g >= 2 * li["comb_entries"] for c, g in counts[:-1])


@pytest.mark.parametrize("prog,value,addr", [("mix48", "lane", "k300"), ("const4", "imm1", "one"),
                                             ("pair8", "wave", "d5")])
def test_many_units_per_lane(fresh_oracle, fresh_runtime, monkeypatch, prog, value, addr):
    """BPFTIME_AMD_MAX_GRID=2: each lane takes ten units or more, its wave
    cache and the block's table live across them."""
    monkeypatch.setenv("BPFTIME_AMD_MAX_GRID", "2")
    const = prog.startswith("const")
    _, li, _ = run_case(fresh_oracle, fresh_runtime, prog, "array", "const" if const else "lookup", value, addr, 20000)
    assert li["grid"] == 2 and li["block"] == (256 if const else 1024) and not li["flush_log"]


# ---- plans x six shapes that hold every site kind ------------------------------
PLAN_SHAPES = [("rmw8", "array", "lookup", "lane", "k5000", 20000, False),
               ("atom4", "array", "lookup", "lane", "k300", 20000, False),
               ("pair8", "array", "lookup", "wave", "d5", 1025, False),
               ("mix48", "hash", "lookup", "immneg1", "k5", 20000, False),
               ("const4", "array", "const", "imm1", "one", 1025, False),
               ("br_atom", "array", "lookup", "lane", "k300", 5000, True)]
PLAN_SHAPE_IDS = ["-".join(str(x) for x in s[:6]) + ("-xdp" if s[6] else "") for s in PLAN_SHAPES]
PLANS = {
    "block256": {"BPFTIME_AMD_BLOCK": "256"},
    "no_merge": {"BPFTIME_AMD_NO_MERGE": "1"},
    "comb256": {"BPFTIME_AMD_COMB_ENTRIES": "256"},
    "miss_log": {"BPFTIME_AMD_MISS_LOG": "1", "BPFTIME_AMD_COMB_ENTRIES": "256"},
    "miss_log_cap2": {"BPFTIME_AMD_MISS_LOG": "1", "BPFTIME_AMD_COMB_ENTRIES": "256", "BPFTIME_AMD_MISS_CAP": "2"},
    "lds_regs": {"BPFTIME_AMD_LDS_REGS": "1"},
    "lds_ctx": {"BPFTIME_AMD_LDS_CTX": "1"},
    "no_pair": {"BPFTIME_AMD_NO_PAIR": "1"},
    "no_fuse": {"BPFTIME_AMD_NO_FUSE": "1"},
}


PLAN_CASES = [pytest.param(p, s, id=f"{p}-{i}") for p in PLANS for s, i in zip(PLAN_SHAPES, PLAN_SHAPE_IDS)
              if s[2] != "const" or p in ("lds_ctx", "no_fuse")]


@pytest.mark.parametrize("plan,shape", PLAN_CASES)
def test_counter_plan(fresh_oracle, fresh_runtime, monkeypatch, plan, shape):
    """Every plan switch on six shapes (the default plan and ORDERED run every
    shape above); each asserts through last_launch() and the handlers that
    the switch took -- but for no_fuse: superinstruction fusion happens at
    link time, after what fast_handler reports, so its cases are parity-only.
    The table-less const4 shape runs only the plans that change its launch."""
    prog, mtype, target, value, addr, n, xdp = shape
    if plan == "lds_ctx":
        xdp = True                                     # the ctx is an XDP launch's
    for k, val in PLANS[plan].items():
        monkeypatch.setenv(k, val)
    comb = target != "const"
    _, li, e = run_case(fresh_oracle, fresh_runtime, prog, mtype, target, value, addr, n, xdp=xdp,
                        no_pair=plan == "no_pair")
    # the register copy stays in global memory while a table is there, and
    # only such launches run 1024-lane blocks
    gregs = comb and plan != "lds_regs"
    block = 1024 if gregs and plan != "block256" else 256
    assert li["block"] == block and li["grid"] == -(-n // block) and not li["ordered"]
    assert li["gregs"] == gregs
    assert li["gctx"] == (xdp and gregs and plan != "lds_ctx")
    if not comb:
        assert li["comb_entries"] == 0 and not li["flush_log"] and not li["miss_log"]
        return
    if "BPFTIME_AMD_COMB_ENTRIES" in PLANS[plan]:
        assert li["comb_entries"] == 256
    else:
        assert li["comb_entries"] >= 512 and li["comb_entries"] % 8 == 0
    assert li["flush_log"] == (li["grid"] > K_MERGE_GROUP and plan != "no_merge")
    if plan.startswith("miss_log"):
        assert li["miss_log"] == (li["grid"] > 1)
        if plan == "miss_log_cap2" and li["miss_log"]:
            assert li["miss_cap"] == 2
    else:
        assert not li["miss_log"] and li["miss_cap"] == 0
    if "BPFTIME_AMD_COMB_ENTRIES" in PLANS[plan] and addr == "k5000":
        # set-full / direct path of comb_add: every block's slice touches at
        # least twice as many granules as its table has entries, so by
        # pigeonhole some adds find no way
        _, _, v, _ = make_units(n, addr, value)
        sites = _sites_of(prog)
        for lo, hi in block_slices(li, n)[:-1]:
            assert distinct_counters(sites, e, v, np.full(n, 2), lo, hi)[1] >= 2 * li["comb_entries"]
