"""bpf_get_stackid (27) / bpf_get_stack (67) over a batch's recorded call stacks
and a STACK_TRACE map on the device, against the model (tests/_stacktrace.py),
bit-exact: return values, every slot's frames, and stack_count's counts map.
A parallel batch must leave the map as the model's serial run leaves it
(helper claims + k_stack_commit).  Every bad input here is a refusal at launch
or an error return; nothing provokes a fault."""
import numpy as np
import pytest

from bpftime_amd import isa, programs, shard

import _stacktrace as sm

pytestmark = pytest.mark.gpu

ST, ARRAY = isa.BPF_MAP_TYPE_STACK_TRACE, isa.BPF_MAP_TYPE_ARRAY
U, FAST, REUSE = sm.USER_STACK, sm.FAST_CMP, sm.REUSE
ENTRIES, VALUE, DEPTH, STRIDE = 16, 64, 8, 192
NS = [1, 63, 64, 65, 130]


def stacks_of(n, seed=11):
    """Depth 0..8 per unit; at most 8 distinct stacks per length, so equal
    stacks recur and distinct ones collide in 16 slots."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d, v = int(rng.integers(0, DEPTH + 1)), int(rng.integers(0, 8))
        out.append([0x7f0000001000 + 0x100000 * v + 16 * k + d for k in range(d)])
    return out


class Rig:
    def __init__(self, dev, entries=ENTRIES, value=VALUE):
        self.dev = dev
        self.map, self.model = dev.Map(ST, 4, value, entries), sm.StackMap(4, value, entries)
        self.entries = entries

    def arrays(self, stacks, layout, depth=DEPTH):
        n = len(stacks)
        arr = np.zeros((n, depth), dtype=np.uint64)
        dep = np.zeros(n, dtype=np.uint32)
        for i, s in enumerate(stacks):
            arr[i, :len(s)], dep[i] = s, len(s)
        if layout == "frame_major":
            arr, us, fs = np.ascontiguousarray(arr.T), 8, 8 * n
        else:
            us, fs = 8 * depth, 8
        dev = self.dev
        return dict(stacks=dev.DeviceBuffer.from_array(arr.view(np.uint8).reshape(-1)), stack_unit_stride=us,
                    stack_frame_stride=fs, stack_depths=dev.DeviceBuffer.from_array(dep.view(np.uint8)),
                    stack_max_depth=depth)

    def run(self, code, stacks, layout="rows", ordered=False, first_unit=0, units=None, with_stacks=True,
            expect_error=None, **over):
        dev, n = self.dev, len(stacks)
        host = np.zeros((n, STRIDE), dtype=np.uint8) if units is None else units
        d, out = dev.DeviceBuffer.from_array(host.reshape(-1)), dev.DeviceBuffer(8 * n)
        vm = dev.VM()
        vm.load(code)
        assert vm.info()["big_stack"]                   # the scratch-stack kernels carry the helpers
        kw = self.arrays(stacks, layout) if with_stacks else {}
        kw.update(over)
        flags = dev.BATCH_SYNC | (dev.BATCH_ORDERED if ordered else 0)
        if expect_error is not None:
            before = bytes(self.map.snapshot())
            with pytest.raises(dev.EbpfError, match=expect_error):
                vm.exec_batch(dev.CTX_RAW, d, n, STRIDE, fixed_len=STRIDE, rets=out, flags=flags,
                              first_unit=first_unit, **kw)
            assert bytes(self.map.snapshot()) == before and (d.download() == host.reshape(-1)).all()
            return None
        assert vm.exec_batch(dev.CTX_RAW, d, n, STRIDE, fixed_len=STRIDE, rets=out, flags=flags,
                             first_unit=first_unit, **kw) == 0
        self.units = d.download().reshape(n, STRIDE)
        return [int(x) for x in out.download(np.uint64)]

    def slots(self, m=None):
        m = m or self.map
        got = {i: m.stack_frames(i) for i in range(m.max_entries)}
        return {i: f for i, f in got.items() if f is not None}

    def check_map(self):
        assert self.slots() == self.model.data
        raw = self.map.snapshot().reshape(self.entries, -1)
        assert (raw[:, :8] == 0xFF).all()               # no claim outlives its batch
        for i in range(self.entries):                   # frames, then zeros, to value_size
            want = self.model.lookup(i.to_bytes(4, "little"))
            assert bytes(raw[i, 16:]) == (want if want is not None else bytes(raw[i, 16:]))


def want_ids(model, stacks, flags):
    return [sm.get_stackid(model, s, flags) for s in stacks]


def test_the_model_shows_collisions():
    # with 130 units and at most 8 stacks per length, slots must collide
    m, firsts = sm.StackMap(4, VALUE, ENTRIES), {}
    for s in stacks_of(130):
        if s:
            firsts.setdefault(sm.get_stackid(m, s, U), set()).add(tuple(s))
    assert any(len(v) > 1 for v in firsts.values())


@pytest.mark.parametrize("layout", ["rows", "frame_major"])
@pytest.mark.parametrize("flags", [U, U | FAST, U | 1, U | 8], ids=["user", "fast_cmp", "skip1", "skip8"])
@pytest.mark.parametrize("n", NS)
def test_parallel_matches_the_serial_model(fresh_runtime, n, flags, layout):
    rig, stacks = Rig(fresh_runtime), stacks_of(n)
    got = rig.run(sm.stackid_prog(rig.map.fd, flags), stacks, layout)
    assert got == want_ids(rig.model, stacks, flags)
    rig.check_map()


@pytest.mark.parametrize("layout", ["rows", "frame_major"])
@pytest.mark.parametrize("flags", [U, U | FAST, U | 1, U | 8, U | REUSE, U | REUSE | FAST, U | REUSE | 2],
                         ids=["user", "fast_cmp", "skip1", "skip8", "reuse", "reuse_fast", "reuse_skip2"])
def test_ordered_65(fresh_runtime, flags, layout):
    rig, stacks = Rig(fresh_runtime), stacks_of(65)
    got = rig.run(sm.stackid_prog(rig.map.fd, flags), stacks, layout, ordered=True)
    assert got == want_ids(rig.model, stacks, flags)
    rig.check_map()


@pytest.mark.parametrize("n", NS)
def test_stack_count(fresh_runtime, n):
    dev = fresh_runtime
    rig, stacks = Rig(dev), stacks_of(n, seed=5)
    counts = dev.Map(ARRAY, 4, 8, ENTRIES)
    got = rig.run(programs.stack_count(rig.map.fd, counts.fd, U), stacks)
    want = want_ids(rig.model, stacks, U)
    assert got == want
    rig.check_map()
    tally = [0] * ENTRIES
    for w in want:
        if w < ENTRIES:
            tally[w] += 1
    assert [int(x) for x in counts.snapshot().view(np.uint64)] == tally


def test_error_returns(fresh_runtime):
    rig, stacks = Rig(fresh_runtime), stacks_of(65)
    assert rig.run(sm.stackid_prog(rig.map.fd, 0), stacks) == [sm.ENOTSUP] * 65                  # no USER_STACK
    assert rig.run(sm.stackid_prog(rig.map.fd, U), stacks, with_stacks=False) == [sm.ENOTSUP] * 65  # no stack source
    got = rig.run(sm.stackid_prog(rig.map.fd, U), [[]] * 65)                                     # depth-0 units
    assert got == [sm.ENOENT] * 65
    other = fresh_runtime.Map(ARRAY, 4, 8, 4)
    for code in (sm.stackid_prog(other.fd, U), sm.stackid_prog(0, U, raw_r2=999), sm.stackid_prog(0, U, raw_r2=1 << 40)):
        got = rig.run(code, stacks)
        assert got == [sm.get_stackid(None, s, U) for s in stacks] and sm.EINVAL in got          # not a STACK_TRACE
    assert rig.slots() == {}
    rig.check_map()


def test_depths_are_clamped_to_max_depth(fresh_runtime):
    rig = Rig(fresh_runtime)
    stacks = [[0x1000 + k for k in range(8)]] * 3
    got = rig.run(sm.stackid_prog(rig.map.fd, U), stacks, stack_max_depth=5)
    assert got == want_ids(rig.model, [s[:5] for s in stacks], U)
    rig.check_map()
    got = rig.run(sm.stackid_prog(rig.map.fd, U), stacks, stack_depths=None, stack_fixed_depth=3)
    assert got == want_ids(rig.model, [s[:3] for s in stacks], U)
    rig.check_map()


def test_prefilled_slots_stay(fresh_runtime):
    rig = Rig(fresh_runtime)
    first, second = stacks_of(65, seed=1), stacks_of(130, seed=2)
    assert rig.run(sm.stackid_prog(rig.map.fd, U), first, ordered=True) == want_ids(rig.model, first, U)
    before = dict(rig.model.data)
    assert rig.run(sm.stackid_prog(rig.map.fd, U), second) == want_ids(rig.model, second, U)
    rig.check_map()
    assert all(rig.model.data[i] == f for i, f in before.items())


def test_launch_refusals(fresh_runtime):
    rig, stacks = Rig(fresh_runtime), stacks_of(65)
    fd = rig.map.fd
    rule = "runs only in EBPF_BATCH_ORDERED batches"
    rig.run(sm.stackid_prog(fd, U | REUSE), stacks,
            expect_error=f"bpf_get_stackid on STACK_TRACE map fd {fd} with flags not proven free of BPF_F_REUSE_STACKID.*{rule}")
    units = np.zeros((65, STRIDE), dtype=np.uint8)
    units[:, :8] = np.frombuffer(int(U).to_bytes(8, "little"), dtype=np.uint8)
    rig.run(sm.stackid_prog(fd, 0, flags_from_unit=True), stacks, units=units,
            expect_error=f"with flags not proven free of BPF_F_REUSE_STACKID.*{rule}")
    rig.run(sm.lookup_prog(fd), stacks, expect_error=f"bpf_map_lookup_elem on STACK_TRACE map fd {fd}.*{rule}")
    small = Rig(fresh_runtime, value=32)
    small.run(sm.stackid_prog(small.map.fd, U), stacks, ordered=True,
              expect_error=f"STACK_TRACE map fd {small.map.fd} holds 4 frames per stack .value_size / 8. < stack_max_depth 8")
    for bad, msg in ((dict(stack_max_depth=0), "stack_max_depth 0: 1..127"), (dict(stack_max_depth=128), "stack_max_depth 128"),
                     (dict(stack_unit_stride=12), "stack_unit_stride 12"), (dict(stack_frame_stride=0), "stack_frame_stride 0")):
        rig.run(sm.stackid_prog(fd, U), stacks, expect_error=msg, **bad)
    # ... and the same programs run ORDERED (unit flags: USER_STACK, no constant needed)
    got = rig.run(sm.stackid_prog(fd, 0, flags_from_unit=True), stacks, units=units, ordered=True)
    assert got == want_ids(rig.model, stacks, U)
    rig.check_map()


def test_program_side_map_helpers_ordered(fresh_runtime):
    rig = Rig(fresh_runtime, entries=1)
    assert rig.run(sm.lookup_prog(rig.map.fd), [[5]], ordered=True) == [0]                        # empty: NULL
    assert rig.run(sm.stackid_prog(rig.map.fd, U), [[0x1234, 7]], ordered=True) == [0]
    assert rig.run(sm.lookup_prog(rig.map.fd), [[5]], ordered=True) == [0x1234]
    assert rig.run(sm.lookup_prog(rig.map.fd, key=1), [[5]], ordered=True) == [0]                 # past the end


@pytest.mark.parametrize("size", [0, 5, 8, 64])
@pytest.mark.parametrize("n", [1, 65])
def test_get_stack(fresh_runtime, n, size):
    rig = Rig(fresh_runtime)
    stacks = stacks_of(n, seed=9)
    for flags in (U, U | 2):
        got = rig.run(sm.getstack_prog(size, flags), stacks)
        for i, s in enumerate(stacks):
            r, data = sm.get_stack(s, size, flags)
            assert got[i] == r, (i, hex(got[i]), hex(r))
            buf = bytes(rig.units[i, 8:8 + sm.BUF])
            assert buf == data + b"\xa5" * (sm.BUF - len(data)), (i, size, flags)


def test_get_stack_errors(fresh_runtime):
    rig = Rig(fresh_runtime)
    stacks = [[0x1111111111111111 * (k + 1) for k in range(8)]] * 65
    assert rig.run(sm.getstack_prog(64, 0), stacks) == [sm.ENOTSUP] * 65
    assert rig.run(sm.getstack_prog(64, U | sm.BUILD_ID), stacks) == [sm.ENOTSUP] * 65
    assert rig.run(sm.getstack_prog(64, U), stacks, with_stacks=False) == [sm.ENOTSUP] * 65
    assert rig.run(sm.getstack_prog(64, U), [[]] * 65) == [sm.ENOENT] * 65
    # a destination the range guard refuses: -EFAULT, nothing written
    for dst in ("null", "past"):
        assert rig.run(sm.getstack_prog(64, U, dst=dst), stacks) == [sm.EFAULT] * 65
        assert (rig.units[:, 8:8 + sm.BUF] == 0xA5).all()
    assert rig.run(sm.getstack_prog(4, U, dst="past"), stacks) == [0] * 65                       # 4 bytes fit
    assert bytes(rig.units[0, 8:8 + sm.BUF]) == b"\xa5" * (sm.BUF - 4) + b"\x11" * 4
    got = rig.run(sm.getstack_prog(64, U, dst="unit"), stacks)                                   # into the unit
    assert got == [0] * 65 and bytes(rig.units[64, 8:16]) == b"\x11" * 8 and not rig.units[64, 16:].any()


def test_call_seq_orders_a_units_calls(fresh_runtime):
    # one unit, two calls that land in the one slot: skips 2 then 0.  The key
    # of the second call is the smaller number but for the call number
    rig = Rig(fresh_runtime, entries=1)
    stack = [0xA0, 0xA1, 0xA2, 0xA3]
    for ordered in (False, True):
        got = rig.run(sm.stackid_twice_prog(rig.map.fd, U | 2, U), [stack], ordered=ordered)
        assert got == [0] and rig.map.stack_frames(0) == stack[2:]
        assert rig.map.delete(bytes(4)) == 0


def test_two_shards_equal_one_batch(fresh_runtime):
    dev = fresh_runtime
    stacks = stacks_of(130, seed=21)
    whole, a, b = Rig(dev), Rig(dev), Rig(dev)
    ids = whole.run(sm.stackid_prog(whole.map.fd, U), stacks)
    lo, cnt = shard.shard_range(130, 2, 0)
    assert (lo, cnt) == (0, 65)
    ids_a = a.run(sm.stackid_prog(a.map.fd, U), stacks[:65], first_unit=0)
    ids_b = b.run(sm.stackid_prog(b.map.fd, U), stacks[65:], first_unit=65)
    assert ids_a + ids_b == ids == want_ids(whole.model, stacks, U)
    assert shard.merge_stack_traces({}, [a.slots(), b.slots()]) == whole.slots() == whole.model.data
