"""Uprobe replay surface: helper ids 173 / 174, the new entry points, cookies on
links and the dispatch's named refusals.  Attaching instantiates the program on
the device, so every test that attaches is marked `gpu`; the rest need none."""
import ctypes as C
import errno

import numpy as np
import pytest

from bpftime_amd import _lib, isa, programs
from bpftime_amd import vm as dev
from bpftime_amd.vm import VM

import _uprobe as um

KPROBE = 2          # the program type of a uprobe program (bpftime_shm.hpp:144-151); only XDP / TRACEPOINT are special here
F = um.FUNCS[0]


def test_ids():
    assert (isa.BPF_FUNC_get_func_ip, isa.BPF_FUNC_get_attach_cookie) == (173, 174)
    assert (dev.CTX_UPROBE, dev.PT_REGS_BYTES) == (4, 168)
    assert (dev.UPROBE, dev.URETPROBE, dev.UPROBE_OVERRIDE, dev.UREPLACE) == (6, 7, 1008, 1009)
    assert (programs.PT_REGS_PARM1_OFF, programs.PT_REGS_RC_OFF, programs.PT_REGS_IP_OFF) == (112, 80, 128)


@pytest.mark.parametrize("code,hid", [(programs.func_ip_count(5), 173), (programs.cookie_tag(5), 174)],
                         ids=["func_ip_count", "cookie_tag"])
def test_programs_pass_the_loader(code, hid):
    rc, msg = VM().try_load(code)
    assert rc == 0 or "no HIP device" in msg, (rc, msg)
    assert "no device implementation" not in msg
    rc, msg = VM(default_helpers=False).try_load(code)
    assert rc == -22 and (msg.startswith(f"call to nonexistent function {hid} at PC ") or
                          msg.startswith("invalid call immediate at PC ")), (rc, msg)


def test_batch_struct_unchanged_and_symbols():
    fields = [f for f, _ in _lib.EbpfBatch._fields_]
    assert fields[-6:] == ["stack_arr", "stack_unit_stride", "stack_frame_stride", "stack_depths",
                           "stack_fixed_depth", "stack_max_depth"] and fields[-7] == "ktime_stride"
    assert C.sizeof(_lib.EbpfBatch) == 232 and C.sizeof(_lib.CallRecords) == 88
    L = _lib.lib()
    for s in ("bpftime_amd_vm_set_attach", "bpftime_attach_perf_to_bpf_with_cookie", "bpftime_amd_uprobe_attach",
              "bpftime_amd_uprobe_attach_link", "bpftime_amd_uprobe_link_bound", "bpftime_amd_uprobe_detach",
              "bpftime_amd_uprobe_dispatch", "bpftime_amd_uprobe_last_ms"):
        assert hasattr(L, s), s
    assert callable(dev.uprobe_dispatch) and callable(VM.set_attach) and callable(programs.override_if_arg0)


def test_cookie_link_on_bad_fds():
    L = _lib.lib()
    dev.reset_runtime()
    try:
        prog = dev.prog_create(programs.cookie_tag(5), "tag", KPROBE)
        perf = L.bpftime_uprobe_create(-1, -1, b"/bin/true", 0x10, False, 0)
        assert perf >= 0
        for pf, bf in ((prog, prog), (perf, perf), (999, prog), (perf, 999)):
            C.set_errno(0)
            assert L.bpftime_attach_perf_to_bpf_with_cookie(pf, bf, 7) == -1 and C.get_errno() == errno.ENOENT
        # a uprobe link is a record: it drives no syscall attachment and is not bound
        lfd = L.bpftime_attach_perf_to_bpf_with_cookie(perf, prog, 7)
        assert lfd >= 0 and L.bpftime_amd_link_attached(lfd) == 0 and L.bpftime_amd_uprobe_link_bound(lfd) == 0
        assert L.bpftime_amd_uprobe_link_bound(prog) == -1
        C.set_errno(0)
        assert L.bpftime_amd_uprobe_attach_link(prog, F) == -1 and C.get_errno() == errno.EINVAL
        C.set_errno(0)
        assert L.bpftime_amd_uprobe_detach(12345) == -1 and C.get_errno() == errno.ENOENT
        C.set_errno(0)
        assert L.bpftime_amd_uprobe_attach(perf, F, dev.UPROBE, None) == -1 and C.get_errno() == errno.EINVAL
        assert L.bpftime_amd_uprobe_attach(prog, F, 5, None) == -1 and C.get_errno() == errno.EINVAL
    finally:
        dev.reset_runtime()


def _refused(match, **kw):
    with pytest.raises(dev.EbpfError, match=match):
        dev.uprobe_dispatch(**kw)


def test_dispatch_refusals_without_attachments():
    L = _lib.lib()
    assert L.bpftime_amd_uprobe_dispatch(None, None, None, 0, None) == -1
    assert b"no records" in L.bpftime_amd_last_error()
    _refused("no func array", func=None, n=4)
    assert dev.uprobe_dispatch(func=None, n=0) == 0


def _raw_refused(match, **fields):
    """The dispatch through the C ABI with made-up device addresses: every one
    of these is refused before anything reads them."""
    L = _lib.lib()
    base = dict(func=0x10000, enter=0x20000, leave=0x30000, count=4)
    base.update(fields)
    r = _lib.CallRecords(**base)
    assert L.bpftime_amd_uprobe_dispatch(C.byref(r), None, None, 0, None) == -1
    assert match in L.bpftime_amd_last_error(), L.bpftime_amd_last_error()


def test_dispatch_refuses_misaligned_and_oversized_records():
    dev.reset_runtime()
    for name in ("func", "enter", "leave", "pid_tgid", "clock"):
        _raw_refused(b"the record arrays must be 8-aligned", **{name: 0x40004})
    _raw_refused(b"more than 2^32 records", count=(1 << 32) + 1)
    _raw_refused(b"more than 2^32 records", count=1 << 32)
    ok = dict(stack_arr=0x50000, stack_unit_stride=32, stack_frame_stride=8, stack_max_depth=4)
    _raw_refused(b"stack_arr: an 8-aligned array", **dict(ok, stack_arr=0x50004))
    _raw_refused(b"stack_depths: a 4-aligned array", **dict(ok, stack_depths=0x60002))
    _raw_refused(b"stack_unit_stride 12", **dict(ok, stack_unit_stride=12))
    _raw_refused(b"stack_frame_stride 4", **dict(ok, stack_frame_stride=4))
    _raw_refused(b"stack_max_depth 128", **dict(ok, stack_max_depth=128))


@pytest.mark.gpu
def test_link_binding_and_eexist(fresh_runtime):
    L = _lib.lib()
    m = dev.Map(isa.BPF_MAP_TYPE_HASH, 8, 8, 16)
    prog = dev.prog_create(programs.cookie_tag(m.fd), "tag", KPROBE)
    perf = L.bpftime_uprobe_create(-1, -1, b"/bin/true", 0x10, False, 0)
    lfd = dev.link_create(prog, perf, 41, cookie=0xC00C1E)
    assert lfd >= 0 and L.bpftime_amd_link_attached(lfd) == 0 and L.bpftime_amd_uprobe_link_bound(lfd) == 0
    i = dev.uprobe_attach_link(lfd, F)
    assert i > 0 and L.bpftime_amd_link_attached(lfd) == 0 and L.bpftime_amd_uprobe_link_bound(lfd) == 1
    with pytest.raises(dev.EbpfError, match="already bound"):
        dev.uprobe_attach_link(lfd, F)
    # the cookie travels from the link record
    func = dev.DeviceBuffer.from_array(np.array([F, F, um.NOBODY], dtype=np.uint64).view(np.uint8))
    enter = dev.DeviceBuffer.from_array(np.zeros(3 * 168, dtype=np.uint8))
    assert dev.uprobe_dispatch(func, 3, enter=enter) == 0
    assert um.hash_counts(m, [0xC00C1E, 0]) == {0xC00C1E: 2}
    # closing the link detaches
    dev.close_fd(lfd)
    assert dev.uprobe_detach(i) == -1
    # override first: exclusive
    G = um.FUNCS[1]
    o = dev.uprobe_attach(prog, G, dev.UPROBE_OVERRIDE)
    for kind in (dev.UPROBE, dev.URETPROBE, dev.UPROBE_OVERRIDE, dev.UREPLACE):
        C.set_errno(0)
        assert L.bpftime_amd_uprobe_attach(prog, G, kind, None) == -1 and C.get_errno() == errno.EEXIST
    assert dev.uprobe_detach(o) == 0 and dev.uprobe_attach(prog, G, dev.UPROBE) > 0
    # a late override is accepted (and never runs: test_gpu_uprobe.py)
    assert dev.uprobe_attach(prog, G, dev.UPROBE_OVERRIDE) > 0


@pytest.mark.gpu
def test_dispatch_refusals(fresh_runtime):
    m = dev.Map(isa.BPF_MAP_TYPE_HASH, 8, 8, 16)
    prog = dev.prog_create(programs.cookie_tag(m.fd), "tag", KPROBE)
    func = dev.DeviceBuffer.from_array(np.full(4, F, dtype=np.uint64).view(np.uint8))
    regs = dev.DeviceBuffer.from_array(np.zeros(4 * 168, dtype=np.uint8))
    u = dev.uprobe_attach(prog, F, dev.UPROBE)
    _refused("need the enter registers", func=func, n=4, leave=regs)
    for kw, msg in ((dict(stack_unit_stride=4, stack_frame_stride=8, stack_max_depth=4), "stack_unit_stride 4"),
                    (dict(stack_unit_stride=8, stack_frame_stride=0, stack_max_depth=4), "stack_frame_stride 0"),
                    (dict(stack_unit_stride=8, stack_frame_stride=8, stack_max_depth=0), "stack_max_depth 0"),
                    (dict(stack_unit_stride=8, stack_frame_stride=8, stack_max_depth=128), "stack_max_depth 128")):
        _refused(msg, func=func, n=4, enter=regs, stacks=regs, **kw)
    dev.uprobe_detach(u)
    dev.uprobe_attach(prog, F, dev.URETPROBE)
    _refused("need the leave registers", func=func, n=4, enter=regs)
    ovr = dev.prog_create(programs.override_if_arg0(1, 0), "ovr", KPROBE)
    dev.uprobe_attach(ovr, um.FUNCS[1], dev.UPROBE_OVERRIDE)
    st = dev.DeviceBuffer(16)
    _refused("out_state and out_rets", func=func, n=4, enter=regs, leave=regs)
    _refused("out_state and out_rets", func=func, n=4, enter=regs, leave=regs, out_state=st)
    assert m.count() == 0                              # nothing ran
