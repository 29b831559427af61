"""The launch plan of exec_batch, pinned field by field: for a matrix of small
batches (4096 units at most, so the grid is the blocks the units want and
never how many fit the chip) VM.last_launch() must equal what
tests/golden/launch_plans.json records, every field, and every launch-time
refusal must carry the recorded text, byte for byte.  The file was recorded
from this module (python tests/test_gpu_launch_plans.py) before exec_batch was
split into stages (csrc/vm_exec.cpp, vm_plan.cpp, vm_upkeep.cpp); the refusals
launch no kernel.

The lookup cache's set count is latched once per process (loader.cpp
lcache_sets), so the one case that needs another count -- the LDS-fit refusal
of flow-hash with BPFTIME_AMD_COMB_ENTRIES=2000 BPFTIME_AMD_LCACHE_SETS=2048 --
runs in a process of its own."""
import contextlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GOLDEN = os.path.join(TESTS, "golden", "launch_plans.json")

pytestmark = pytest.mark.gpu

# every variable the planner reads per launch: a case runs with exactly its own
PLAN_ENV = ["BPFTIME_AMD_" + v for v in (
    "BLOCK", "LCACHE_SETS", "COMB_ENTRIES", "TAIL_LDS", "GRID_MULT", "MAX_GRID", "LDS_REGS", "LDS_CTX", "NO_STAGING",
    "NO_RB_STAGE", "NO_MERGE", "MISS_LOG", "MISS_CAP", "DBG")]


@contextlib.contextmanager
def plan_env(env):
    old = {k: os.environ.get(k) for k in PLAN_ENV}
    for k in PLAN_ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _mods():
    from bpftime_amd import gen, isa, programs
    from bpftime_amd import vm as dev
    return dev, gen, isa, programs


# ---- the workloads: each launches one batch and returns its VM ----------------
def xdp_counter(n, flags, stride=64):
    dev, gen, isa, programs = _mods()
    ctl = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 4, 2)
    bss = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 4096, 1)
    vm = dev.VM()
    vm.load(programs.xdp_counter(ctl.fd, bss.fd))
    d = dev.DeviceBuffer.from_array(gen.xdp_packets(n, stride=stride))
    vm.exec_batch(dev.CTX_XDP, d, n, stride, fixed_len=64, verdicts=dev.DeviceBuffer(4 * n), flags=flags)
    return vm


def xdp_counter72(n, flags):
    return xdp_counter(n, flags, stride=72)


def flow_hash(n, flags):
    dev, gen, isa, programs = _mods()
    flows = dev.Map(isa.BPF_MAP_TYPE_HASH, 16, 16, 8192)
    vm = dev.VM()
    vm.load(programs.flow_hash(flows.fd))
    slots, lens = gen.flow_packets(n, nflows=1000, stride=2048)
    d, dl = dev.DeviceBuffer.from_array(slots), dev.DeviceBuffer.from_array(lens)
    vm.exec_batch(dev.CTX_XDP, d, n, 2048, lens=dl, verdicts=dev.DeviceBuffer(4 * n), flags=flags)
    return vm


def syscall_agg(n, flags):
    dev, gen, isa, programs = _mods()
    counts = dev.Map(isa.BPF_MAP_TYPE_HASH, 4, 32, 8192)
    vm = dev.VM()
    vm.load(programs.syscall_agg(counts.fd))
    d = dev.DeviceBuffer.from_array(gen.syscall_records(n))
    vm.exec_batch(dev.CTX_SYSCALL, d, n, 64, rets=dev.DeviceBuffer(8 * n), flags=flags)
    return vm


def tail_call(n, flags):
    """The caller tail-calls slot data[0] & 3 of {0: a packet writer, 1: a
    counter, 2: empty, 3: a counter that tail-calls slot 0}."""
    dev, gen, isa, programs = _mods()
    pa = dev.Map(isa.BPF_MAP_TYPE_PROG_ARRAY, 4, 4, 4)
    cnt = dev.Map(isa.BPF_MAP_TYPE_PERCPU_ARRAY, 4, 8, 4)
    targets = {0: programs.tail_target_write(0xA1), 1: programs.tail_target_count(cnt.fd),
               3: programs.tail_target_recurse(pa.fd, cnt.fd, 0)}
    for k, code in targets.items():
        pa.update(struct.pack("<i", k), struct.pack("<i", dev.prog_create(code, "t%d" % k, 6)))
    vm = dev.VM()
    vm.load(programs.tail_xdp_caller(pa.fd, cnt.fd))
    d = dev.DeviceBuffer.from_array(gen.xdp_packets(n, seed=7))
    vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=64, verdicts=dev.DeviceBuffer(4 * n), flags=flags, ifindex=5)
    return vm


def ringbuf(n, flags):
    dev, gen, isa, programs = _mods()
    rb = dev.Map(isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 1 << 22)
    vm = dev.VM()
    vm.load(programs.ringbuf_sampler(rb.fd))
    d = dev.DeviceBuffer.from_array(gen.xdp_packets(n, seed=8))
    vm.exec_batch(dev.CTX_XDP, d, n, 64, fixed_len=64, verdicts=dev.DeviceBuffer(4 * n), flags=flags)
    return vm


def big_stack(n, flags):
    """A stack of 128 bytes, above the 64 a lane keeps in LDS (kLdsStackMax)."""
    dev, gen, isa, _ = _mods()
    a = isa.Asm().ldx(8, 2, 1, 0).stx(8, 10, -128, "r2").stx(8, 10, -8, "r2").ldx(8, 0, 10, -128).exit()
    vm = dev.VM()
    vm.load(a.assemble())
    d = dev.DeviceBuffer.from_array(gen.sm64(3, np.arange(n, dtype=np.uint64)).view(np.uint8).reshape(n, 8))
    vm.exec_batch(dev.CTX_RAW, d, n, 8, fixed_len=8, rets=dev.DeviceBuffer(8 * n), flags=flags)
    return vm


WORKLOADS = {"xdp_counter": xdp_counter, "xdp_counter72": xdp_counter72, "flow_hash": flow_hash,
             "syscall_agg": syscall_agg, "tail_call": tail_call, "ringbuf": ringbuf, "big_stack": big_stack}

SYNC, ORDERED = 0x1, 0x2
# case -> (workload, units, flags, environment).  ORDERED batches run on one
# lane: 256 units keep them quick.
CASES = {w: (w, 4096, SYNC, {}) for w in WORKLOADS}
CASES.update({w + "-ordered": (w, 256, SYNC | ORDERED, {}) for w in WORKLOADS})
CASES.update({
    "xdp_counter-odd": ("xdp_counter", 4001, SYNC, {}),
    "xdp_counter-max_grid3": ("xdp_counter", 4096, SYNC, {"BPFTIME_AMD_MAX_GRID": "3"}),
    "flow_hash-block256": ("flow_hash", 4096, SYNC, {"BPFTIME_AMD_BLOCK": "256"}),
    "flow_hash-lcache_sets": ("flow_hash", 4096, SYNC, {"BPFTIME_AMD_LCACHE_SETS": "8"}),
    "flow_hash-max_grid2": ("flow_hash", 4096, SYNC, {"BPFTIME_AMD_MAX_GRID": "2"}),
    "tail_call-tail_lds1": ("tail_call", 4096, SYNC, {"BPFTIME_AMD_TAIL_LDS": "1"}),
    "syscall_agg-lds_regs": ("syscall_agg", 4096, SYNC, {"BPFTIME_AMD_LDS_REGS": "1"}),
})


def run_case(name):
    dev = _mods()[0]
    work, n, flags, env = CASES[name]
    dev.reset_runtime()
    dev.set_ncpu(64)
    with plan_env(env):
        vm = WORKLOADS[work](n, flags)
    li = vm.last_launch()
    dev.reset_runtime()
    return li


# ---- refusals: one batch per branch, none launches a kernel -------------------
def _refused(dev, vm, **fields):
    """The VM's error text for the raw ebpf_batch `fields`."""
    import ctypes as C
    from bpftime_amd._lib import EbpfBatch, lib
    b = EbpfBatch(**fields)
    assert lib().ebpf_exec_batch(C.c_void_p(vm.h), C.byref(b)) == -1, fields
    return lib().bpftime_amd_vm_error(C.c_void_p(vm.h)).decode()


def _loaded(dev, isa):
    vm = dev.VM()
    vm.load(isa.Asm().mov64(0, 0).exit().assemble())
    return vm


def batch_refusals():
    """name -> text, for every refusal that depends on the ebpf_batch alone."""
    dev, gen, isa, _ = _mods()
    out = {}
    out["not_loaded"] = _refused(dev, dev.VM(), ctx_kind=dev.CTX_RAW, count=1)
    vm = _loaded(dev, isa)
    buf = dev.DeviceBuffer(4096)
    p = buf.ptr
    assert p % 16 == 0
    ok = dict(count=4, data=p, stride=256)
    r = lambda **kw: _refused(dev, vm, **{**ok, **kw})  # noqa: E731
    out["ctx_kind"] = r(ctx_kind=5)
    out["no_data"] = r(ctx_kind=dev.CTX_RAW, data=None)
    out["no_stride"] = r(ctx_kind=dev.CTX_RAW, stride=0)
    out["uprobe_stride"] = r(ctx_kind=dev.CTX_UPROBE, stride=160)
    out["uprobe_unaligned"] = r(ctx_kind=dev.CTX_UPROBE, data=p + 4)
    out["uprobe_descs"] = r(ctx_kind=dev.CTX_UPROBE, descs=p, umem_bytes=4096)
    out["sys_state_xdp"] = r(ctx_kind=dev.CTX_XDP, sys_state=p, sys_phase=1)
    out["sys_state_phase"] = r(ctx_kind=dev.CTX_SYSCALL, sys_state=p, sys_phase=3)
    out["sys_state_uprobe_phase"] = r(ctx_kind=dev.CTX_UPROBE, sys_state=p, sys_phase=0)
    out["descs_syscall"] = r(ctx_kind=dev.CTX_SYSCALL, descs=p, umem_bytes=4096)
    out["descs_no_umem"] = r(ctx_kind=dev.CTX_XDP, descs=p)
    out["pid_off_xdp"] = r(ctx_kind=dev.CTX_XDP, pid_tgid_off=8)
    out["ktime_off_raw_descs"] = r(ctx_kind=dev.CTX_RAW, descs=p, umem_bytes=4096, ktime_off=8)
    out["pid_both"] = r(ctx_kind=dev.CTX_SYSCALL, pid_tgid_off=8, pid_tgid_arr=p, pid_tgid_stride=8)
    out["pid_off_unaligned"] = r(ctx_kind=dev.CTX_SYSCALL, stride=64, pid_tgid_off=4)
    out["pid_off_past_unit"] = r(ctx_kind=dev.CTX_SYSCALL, stride=64, pid_tgid_off=64)
    out["pid_off_exit_extent"] = r(ctx_kind=dev.CTX_SYSCALL_EXIT, stride=96, pid_tgid_off=32)
    out["pid_arr_stride"] = r(ctx_kind=dev.CTX_SYSCALL, pid_tgid_arr=p, pid_tgid_stride=0)
    out["ktime_off_negative"] = r(ctx_kind=dev.CTX_SYSCALL, ktime_off=-8)
    out["ktime_arr_unaligned"] = r(ctx_kind=dev.CTX_UPROBE, ktime_arr=p + 4, ktime_stride=8)
    st = dict(ctx_kind=dev.CTX_RAW, stack_arr=p, stack_unit_stride=64, stack_frame_stride=8, stack_max_depth=8)
    out["stack_arr_unaligned"] = r(**{**st, "stack_arr": p + 4})
    out["stack_unit_stride"] = r(**{**st, "stack_unit_stride": 12})
    out["stack_frame_stride"] = r(**{**st, "stack_frame_stride": 0})
    out["stack_depths_unaligned"] = r(**{**st, "stack_depths": p + 2})
    out["stack_max_depth_0"] = r(**{**st, "stack_max_depth": 0})
    out["stack_max_depth_128"] = r(**{**st, "stack_max_depth": 128})
    return out


def map_refusals():
    """The unordered-LPM-write and the QUEUE / STACK refusals (parallel batches)."""
    dev, gen, isa, _ = _mods()
    Asm = isa.Asm
    out = {}
    units = dev.DeviceBuffer.from_array(np.zeros((4, 64), dtype=np.uint8))

    def refused(code):
        vm = dev.VM()
        vm.load(code)
        with pytest.raises(dev.EbpfError) as e:
            vm.exec_batch(dev.CTX_RAW, units, 4, 64, fixed_len=64)
        return str(e.value)

    trie = dev.Map(isa.BPF_MAP_TYPE_LPM_TRIE, 8, 4, 16)
    key = lambda a: a.st(4, 10, -16, 32).st(4, 10, -12, 0).st(4, 10, -8, 1).ld_map_fd(1, trie.fd) \
        .mov64(2, "r10").add64(2, -16)  # noqa: E731
    out["lpm_update"] = refused(key(Asm()).mov64(3, "r10").add64(3, -8).mov64(4, 0)
                                .call(isa.BPF_FUNC_map_update_elem).exit().assemble())
    out["lpm_delete"] = refused(key(Asm()).call(isa.BPF_FUNC_map_delete_elem).exit().assemble())
    q = dev.Map(isa.BPF_MAP_TYPE_QUEUE, 0, 8, 16)
    val = lambda a: a.mov64(2, "r10").add64(2, -8)  # noqa: E731
    mixed = Asm().st(8, 10, -8, 0).ld_map_fd(1, q.fd)
    val(mixed).mov64(3, 0).call(87).ld_map_fd(1, q.fd)
    val(mixed).call(88).exit()
    out["queue_mixed"] = refused(mixed.assemble())
    exist = Asm().st(8, 10, -8, 0).ld_map_fd(1, q.fd)
    val(exist).mov64(3, isa.BPF_EXIST).call(87).exit()
    out["queue_flags"] = refused(exist.assemble())
    return out


def lds_fit_refusal():
    """flow-hash with BPFTIME_AMD_COMB_ENTRIES=2000 BPFTIME_AMD_LCACHE_SETS=2048,
    in a process that latches 2048 sets."""
    env = dict(os.environ, BPFTIME_AMD_COMB_ENTRIES="2000", BPFTIME_AMD_LCACHE_SETS="2048")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_launch_plans as t\n"
            "from bpftime_amd import vm as dev\n"
            "dev.reset_runtime(); dev.set_ncpu(64)\n"
            "try:\n    t.flow_hash(4096, 1)\n    print('launched')\n"
            "except dev.EbpfError as e:\n    print(e)\n" % (ROOT, TESTS))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip()


def all_refusals():
    dev = _mods()[0]
    dev.reset_runtime()
    dev.set_ncpu(64)
    with plan_env({}):
        out = batch_refusals()
        dev.reset_runtime()
        out.update(map_refusals())
        dev.reset_runtime()
        out["lds_fit"] = lds_fit_refusal()
    return out


# ---- the tests ------------------------------------------------------------------
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_plan(gpu, name):
    want = _golden()["plans"][name]
    got = run_case(name)
    print(name, got)
    assert set(got) == set(want)
    for field in want:
        assert got[field] == want[field], (name, field, got, want)


def test_refusal_texts(gpu):
    want = _golden()["refusals"]
    got = all_refusals()
    for name, text in got.items():
        print(name, "->", text)
    assert set(got) == set(want)
    for name in want:
        assert got[name] == want[name], name


if __name__ == "__main__":  # record the fixture
    sys.path.insert(0, ROOT)
    doc = {"plans": {name: run_case(name) for name in CASES}, "refusals": all_refusals()}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
