"""Every A/B switch of the launch plan against the oracle: each names a
second implementation of the same semantics (several are what a launch falls
back to on its own), so each runs the smallest program that reaches the
mechanism, at a few thousand units, with the switch off and on, bit-exact
against the oracle both times, and asserts through VM.last_launch() /
VM.fast_handler that the switch changed what it claims to.

BPFTIME_AMD_LANE_PAD is read once per process (a static in vm_plan.cpp) and
cannot be switched inside a test run: it is left out.  BPFTIME_AMD_NO_LPM_FLAT
chooses how the host builds an LPM trie's device replica, which neither the
launch info nor a handler shows: its case is parity-only.  The lookup cache's
set count (loader.cpp lcache_sets) is latched the same way and accepts only
powers of two from 256: BPFTIME_AMD_LCACHE_SETS=8 therefore cannot shrink
the cache here; what the variable does change per launch is that a
1024-lane block keeps the plain 1024 sets instead of the doubled 2048, and
the case below makes the keys collide in the 2-way sets by their number
(4000 flows on 2048 slots)."""
import struct

import numpy as np
import pytest

from bpftime_amd import gen, isa, programs
from bpftime_amd.isa import Asm

from _helpers import make_maps, update_existing_prog, update_existing_units

pytestmark = pytest.mark.gpu


# ---- workloads: each checks itself against the oracle and returns its VM ------
def _xdp(po, dev, code, slots, stride, lens=None, fixed_len=0, data_offset=0, flat=None):
    """Runs an XDP program on oracle and device; -> (vm, verdicts equal and
    packet bytes equal asserted)."""
    n = slots.shape[0]
    ovm = po.OracleVM()
    ovm.load(code)
    opk = slots.copy()
    want = ovm.run_xdp(opk, lens=lens, fixed_len=fixed_len)
    vm = dev.VM()
    vm.load(code)
    d = dev.DeviceBuffer.from_array(slots if flat is None else flat)
    dl = dev.DeviceBuffer.from_array(lens) if lens is not None else None
    dv = dev.DeviceBuffer(4 * n)
    assert vm.exec_batch(dev.CTX_XDP, d, n, stride, lens=dl, fixed_len=fixed_len, verdicts=dv,
                         data_offset=data_offset) == 0
    np.testing.assert_array_equal(dv.download(np.uint32), want)
    got = d.download()
    if flat is not None:
        got = got[data_offset:data_offset + n * stride]
    np.testing.assert_array_equal(got.reshape(n, stride), opk)
    return vm


def flow(po, dev, n=20000, nflows=4000):
    """flow-hash: hash lookups through the lookup cache, inserts, and the
    fused {packets, bytes} atomic pair through the combining table."""
    (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_HASH, 16, 16, 8192)], po, dev)
    code = programs.flow_hash(dm.fd)
    slots, lens = gen.flow_packets(n, nflows=nflows, stride=2048)
    vm = _xdp(po, dev, code, slots, 2048, lens=lens)
    assert dm.hash_items() == om.items() and len(om.items()) > nflows // 2
    return vm


def staged_slots(po, dev, n=3000, stride=64, data_offset=0):
    """Static loads and stores inside the unit (the staged window): every
    unit rewrites its bytes 16..31 from bytes 0..15 and returns a fold."""
    a = Asm()
    a.ldx(8, 6, 1, 0).ldx(8, 3, 1, 8).mov64(4, "r6").add64(4, 40).mov64(0, 1).jmp("jgt", 4, "r3", "out")
    a.ldx(8, 2, 6, 0).ldx(4, 4, 6, 8).ldx(2, 5, 6, 12).ldx(1, 7, 6, 14)
    a.mov64(0, "r2").alu64("xor", 0, "r4").add64(0, "r5").add64(0, "r7")
    a.stx(8, 6, 16, "r0").stx(4, 6, 24, "r2").stx(2, 6, 28, "r4").stx(1, 6, 30, "r7").st(1, 6, 31, 0x5A)
    a.alu64("and", 0, 3).label("out").exit()
    slots = gen.xdp_packets(n, stride=stride, seed=5)
    flat = None
    if data_offset:
        flat = np.zeros(n * stride + 16, dtype=np.uint8)
        flat[data_offset:data_offset + n * stride] = slots.reshape(-1)
    return _xdp(po, dev, a.assemble(), slots, stride, fixed_len=64, data_offset=data_offset, flat=flat)


def const_load(po, dev, n=3000):
    """A load from a constant map-value address (F_KLDX)."""
    (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 16, 1)], po, dev)
    for m in (om, dm):
        m.update(b"\0\0\0\0", struct.pack("<QQ", 0x1122334455667788, 0xFFFFFFFF00000007))
    a = Asm().ldx(8, 5, 1, 0).ld_map_value(1, dm.fd, 8)
    at = a.pc
    a.ldx(8, 0, 1, 0).alu64("xor", 0, "r5").exit()
    units = gen.sm64(3, np.arange(n, dtype=np.uint64)).view(np.uint8).reshape(n, 8)
    ovm = po.OracleVM()
    ovm.load(a.assemble())
    want = ovm.run_raw(units.copy(), 8)
    vm = dev.VM()
    vm.load(a.assemble())
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * n)
    assert vm.exec_batch(dev.CTX_RAW, d, n, 8, fixed_len=8, rets=dr) == 0
    np.testing.assert_array_equal(dr.download(np.uint64), want)
    vm.site = vm.fast_handler(dev.CTX_RAW, at)
    return vm


def update_existing(po, dev, n=4096):
    """bpf_map_update_elem of a HASH map, key and value on the stack, half of
    the keys present: the asm update and the C++ helper."""
    (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_HASH, 4, 16, 2 * n)], po, dev)
    for k in range(n // 2):
        key, val = struct.pack("<I", k), struct.pack("<QQ", 7 * k, k)
        assert om.update(key, val) == 0 and dm.update(key, val) == 0
    code, at = update_existing_prog(dm.fd)
    units = update_existing_units(n)
    ovm = po.OracleVM()
    ovm.load(code)
    want = ovm.run_raw(units.copy(), 32)
    vm = dev.VM()
    vm.load(code)
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * n)
    assert vm.exec_batch(dev.CTX_RAW, d, n, 32, fixed_len=32, rets=dr) == 0
    np.testing.assert_array_equal(dr.download(np.uint64), want)
    assert dm.hash_items() == om.items()
    vm.site = vm.fast_handler(dev.CTX_RAW, at)
    return vm


def ring(po, dev, n=4096):
    """A sampler that also counts: every frame adds 1 to the counter its
    first byte names (a deferred add: the launch holds a combining table),
    every fourth sends its bytes 16..31 to a ring large enough for block
    staging.  The record source at packet offset 16 is the only static access
    past byte 0, so the staged window is 32 bytes while the asm tier writes
    the record and 16 when the C++ helper does; and the table makes the
    launch a 1024-lane one unless ring staging keeps 256-lane blocks."""
    (oc,), (dc,) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 8, 4)], po, dev)
    dm = dev.Map(isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 1 << 26)
    om = po.OracleMap(isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 1 << 26, fd=dm.fd)
    a = Asm().ldx(8, 6, 1, 0).ldx(8, 3, 1, 8).mov64(0, isa.XDP_PASS)
    a.mov64(4, "r6").add64(4, 48).jmp("jgt", 4, "r3", "out")
    a.ldx(1, 8, 6, 0).alu64("and", 8, 3).stx(4, 10, -4, "r8")
    a.ld_map_fd(1, dc.fd).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_lookup_elem)
    a.mov64(1, "r0").mov64(0, isa.XDP_ABORTED).jmp("jeq", 1, 0, "out")
    a.mov64(2, 1).atomic(8, isa.ATOMIC_ADD, 1, 0, "r2")
    a.mov64(0, isa.XDP_PASS).jmp("jne", 8, 0, "out")
    a.ld_map_fd(1, dm.fd).mov64(2, "r6").add64(2, 16).mov64(3, 16).mov64(4, 0).call(isa.BPF_FUNC_ringbuf_output)
    a.mov64(1, "r0").mov64(0, isa.XDP_PASS).jmp("jeq", 1, 0, "out").mov64(0, isa.XDP_DROP)
    a.label("out").exit()
    vm = _xdp(po, dev, a.assemble(), gen.xdp_packets(n, seed=8), 64, fixed_len=64)
    drecs, orecs = dm.ringbuf_fetch(), om.ringbuf_fetch()
    assert sorted(drecs) == sorted(orecs) and len(drecs) > n // 8
    for k in range(4):
        assert dc.lookup(struct.pack("<I", k)) == oc.lookup(struct.pack("<I", k))
    assert vm.counter_info(dev.CTX_XDP) == (1, 0) and vm.last_launch()["comb_entries"] > 0
    return vm


def lpm(po, dev, n=4096):
    """LPM_TRIE routing: one lookup per frame (4-byte data: the flat table)."""
    rng = np.random.default_rng(6)
    routes = [(8, i << 24, 1 + (i % 3)) for i in range(256)]
    for _ in range(300):
        plen = int(rng.integers(12, 29))
        routes.append((plen, int(rng.integers(0, 1 << 32)) & ((0xFFFFFFFF << (32 - plen)) & 0xFFFFFFFF),
                       int(rng.integers(1, 4))))
    (om,), (dm,) = make_maps([(isa.BPF_MAP_TYPE_LPM_TRIE, 8, 4, len(routes))], po, dev)
    for plen, net, v in routes:
        for m in (om, dm):
            m.update(struct.pack("<I", plen) + struct.pack(">I", net), struct.pack("<I", v))
    return _xdp(po, dev, programs.lpm_route(dm.fd), gen.xdp_packets(n, seed=9), 64, fixed_len=64)


# switch -> (workload, what last_launch / the handler shows without it, with it)
def _li(**kw):
    return lambda vm: all(vm.last_launch()[k] == v for k, v in kw.items())


SWITCHES = {
    "BPFTIME_AMD_NO_STAGING": (staged_slots, "1", lambda vm: vm.last_launch()["stage"] >= 32, _li(stage=0)),
    "BPFTIME_AMD_LDS_REGS": (flow, "1", _li(gregs=True, block=1024), _li(gregs=False, gctx=False, block=256)),
    "BPFTIME_AMD_LDS_CTX": (flow, "1", _li(gctx=True), _li(gctx=False, gregs=True)),
    "BPFTIME_AMD_BLOCK": (flow, "256", _li(block=1024, grid=20), _li(block=256, grid=79)),
    "BPFTIME_AMD_NO_MERGE": (flow, "1", _li(flush_log=True, grid=20), _li(flush_log=False, grid=20)),
    "BPFTIME_AMD_NO_PAIR": (flow, "1", lambda vm: _handlers(vm, 1).count("ATOMMV8_ADD2") == 1,
                            lambda vm: "ATOMMV8_ADD2" not in _handlers(vm, 1) and
                            _handlers(vm, 1).count("ATOMMV8_ADD") == 2),
    "BPFTIME_AMD_NO_LCACHE": (flow, "1", lambda vm: vm.last_launch()["lcache_sets"] >= 1024, _li(lcache_sets=0)),
    "BPFTIME_AMD_LCACHE_SETS": (flow, "8", _li(lcache_sets=2048, block=1024), _li(lcache_sets=1024, block=1024)),
    "BPFTIME_AMD_NO_KLDX": (const_load, "1", lambda vm: vm.site == "KLDX", lambda vm: vm.site != "KLDX"),
    "BPFTIME_AMD_NO_ASM_UPDATE": (update_existing, "1", lambda vm: vm.site == "CALL_UPDATE_STK",
                                  lambda vm: vm.site != "CALL_UPDATE_STK"),
    # ring staging keeps 256-lane blocks; without it the table's launch runs 1024-lane ones
    "BPFTIME_AMD_NO_RB_STAGE": (ring, "1", _li(block=256, gregs=True), _li(block=1024, gregs=True)),
    # the asm ring-buffer site widens the staged window to its record source
    "BPFTIME_AMD_NO_ASM_RINGBUF": (ring, "1", _li(stage=32, block=256), _li(stage=16, block=256)),
    # parity only: the flat table is the map's host-side replica, no launch plan shows it
    "BPFTIME_AMD_NO_LPM_FLAT": (lpm, "1", lambda vm: True, lambda vm: True),
}


def _handlers(vm, kind):
    return [vm.fast_handler(kind, pc) for pc in range(vm.info()["n_insns"])]


@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_plan_switch(fresh_oracle, fresh_runtime, monkeypatch, switch, on):
    """(BPFTIME_AMD_NO_LPM_FLAT leaves no trace in the launch info or the
    handlers: its two cases are parity-only, they check the results against
    the oracle and nothing else.  BPFTIME_AMD_GRID_MULT has a test of its
    own below.)"""
    work, value, without, with_ = SWITCHES[switch]
    monkeypatch.delenv(switch, raising=False)
    if on:
        monkeypatch.setenv(switch, value)
    vm = work(fresh_oracle, fresh_runtime)
    assert (with_ if on else without)(vm), (vm.last_launch(), getattr(vm, "site", None))


@pytest.mark.parametrize("route", ["stride72", "data_offset8"])
def test_staging_falls_back_on_unaligned_units(fresh_oracle, fresh_runtime, route):
    """What a launch falls back to on its own: a stride that is no multiple
    of 16, or a 16-aligned buffer entered at data_offset 8, runs unstaged
    (stage == 0) and matches the oracle, packet bytes included."""
    if route == "stride72":
        vm = staged_slots(fresh_oracle, fresh_runtime, stride=72)
    else:
        vm = staged_slots(fresh_oracle, fresh_runtime, data_offset=8)
    assert vm.last_launch()["stage"] == 0
    vm2 = staged_slots(fresh_oracle, fresh_runtime)       # aligned again: staged
    assert vm2.last_launch()["stage"] >= 32


def test_grid_mult_raises_the_grid_cap(fresh_oracle, fresh_runtime, monkeypatch):
    """BPFTIME_AMD_GRID_MULT multiplies the cap cus * occupancy on the grid
    (grid = min(blocks wanted, cap)), so it shows only where the cap binds:
    2^20 + 4096 units in 256-lane blocks want 4112 blocks, more than twice
    the 256-lane blocks a device holds (at most 8 per CU).  Without it the
    grid is a whole number of blocks per CU below the wanted count; with 2
    it is min(wanted, twice that); bit-exact against the oracle both times."""
    monkeypatch.delenv("BPFTIME_AMD_GRID_MULT", raising=False)
    n = (1 << 20) + 4096
    li = staged_slots(fresh_oracle, fresh_runtime, n=n).last_launch()
    want = -(-n // 256)
    assert li["block"] == 256 and li["occupancy"] >= 1
    assert li["grid"] < want and li["grid"] % li["occupancy"] == 0    # the cap binds: grid = cus * occupancy
    monkeypatch.setenv("BPFTIME_AMD_GRID_MULT", "2")
    li2 = staged_slots(fresh_oracle, fresh_runtime, n=n).last_launch()
    assert li2["block"] == 256 and li2["occupancy"] == li["occupancy"]
    assert li2["grid"] == min(want, 2 * li["grid"]) > li["grid"]
