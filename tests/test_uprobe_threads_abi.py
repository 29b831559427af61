"""bpftime_amd_uprobe_dispatch_plan and the plan flags of
bpftime_amd_uprobe_dispatch (include/bpftime_amd.h): the symbol, the plan per
flag combination, and every refusal of the thread-ordered plan that the public
interface can reach -- each before any launch.  (More than 16 task identities
cannot be reached: every attachment's VM carries the process's identity.)"""
import os
import re

import numpy as np
import pytest

from bpftime_amd import _lib, isa
from bpftime_amd import vm as dev
from bpftime_amd.isa import Asm

import _stacktrace as sm
import _uprobe as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0, F1, F2 = um.FUNCS
HASH, KPROBE = isa.BPF_MAP_TYPE_HASH, 2
P, T, O = dev.DISPATCH_PROGRAMS, dev.DISPATCH_THREADS, dev.BATCH_ORDERED
MAP_PUSH = 87


def test_header_library_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "bpftime_amd.h")).read()
    assert re.search(r"\bint\s+bpftime_amd_uprobe_dispatch_plan\s*\(\s*uint32_t\s+flags\s*\)\s*;", hdr)
    fn = _lib.lib().bpftime_amd_uprobe_dispatch_plan
    assert fn.argtypes is not None and len(fn.argtypes) == 1
    assert callable(dev.uprobe_dispatch_plan)


def buf(a):
    return dev.DeviceBuffer.from_array(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def attach(code, func, kind=dev.UPROBE, name="p"):
    return dev.uprobe_attach(dev.prog_create(code, name, KPROBE), func, kind)


def dispatch(r, n, flags):
    return dev.uprobe_dispatch(buf(r["func"]), n, enter=buf(r["enter"]), leave=buf(r["leave"]),
                               flags=dev.BATCH_SYNC | flags)


def both_refuse(r, n, flags, match):
    """The plan query and a dispatch with the same flags give the same named error."""
    with pytest.raises(dev.EbpfError, match=match):
        dev.uprobe_dispatch_plan(flags)
    with pytest.raises(dev.EbpfError, match=match):
        dispatch(r, n, flags)


@pytest.mark.gpu
def test_plan_per_flag_combination(fresh_runtime):
    from bpftime_amd import programs
    n = 65
    r = um.records(n)

    def accepted():
        assert dev.uprobe_dispatch_plan(0) == 0 and dev.uprobe_dispatch_plan(P) == 0
        assert dev.uprobe_dispatch_plan(O) == 0 and dev.uprobe_dispatch_plan(P | O) == 0
        assert dev.uprobe_dispatch_plan(T) == 1 and dev.uprobe_dispatch_plan(T | O) == 1
        both_refuse(r, n, P | T, "name different plans")
        both_refuse(r, n, P | T | O, "name different plans")
    accepted()                                           # nothing attached
    ma, mb = dev.Map(HASH, 8, 8, 64), dev.Map(HASH, 8, 8, 64)
    attach(programs.func_ip_count(ma.fd), F0, name="one")
    second = attach(programs.func_ip_count(mb.fd), F1, dev.URETPROBE, name="two")
    accepted()                                           # a commuting pair
    assert ma.count() == 0 and mb.count() == 0           # (the refused dispatches ran nothing)
    dev.uprobe_detach(second)
    attach(programs.cookie_tag(ma.fd), F1, dev.URETPROBE, name="two")
    for flags in (0, P, O, P | O):                       # a pair that may not commute
        both_refuse(r, n, flags, "'one' .* and 'two' .* may not commute on map fd %d.*DISPATCH_THREADS" % ma.fd)
    both_refuse(r, n, P | T, "name different plans")
    assert ma.count() == 0
    assert dev.uprobe_dispatch_plan(T) == 1 and dev.uprobe_dispatch_plan(T | O) == 1
    hits = int((r["func"] == F0).sum()), int((r["func"] == F1).sum())
    assert dispatch(r, n, T) == 0
    assert um.hash_counts(ma, [F0, 0]) == {k: v for k, v in ((F0, hits[0]), (0, hits[1])) if v}


@pytest.mark.gpu
def test_thread_ordered_refusals(fresh_runtime):
    from bpftime_amd import programs
    n = 65
    r = um.records(n)
    m = dev.Map(HASH, 8, 8, 64)
    attach(programs.func_ip_count(m.fd), F0, name="counter")
    # a program that reads the recorded stacks: the commit order is the batch path's
    stm = dev.Map(isa.BPF_MAP_TYPE_STACK_TRACE, 4, 8 * 6, 64)
    stk = attach(sm.stackid_prog(stm.fd, sm.USER_STACK), F1, name="stk")
    for flags in (T, T | O):
        both_refuse(r, n, flags, "'stk' calls bpf_get_stackid / bpf_get_stack")
    assert dev.uprobe_dispatch_plan(0) == 0              # program-major still takes it
    dev.uprobe_detach(stk)
    # a QUEUE: only with EBPF_BATCH_ORDERED
    q = dev.Map(isa.BPF_MAP_TYPE_QUEUE, 0, 8, 128)
    push = Asm().st(8, 10, -8, 7).mov64(2, "r10").add64(2, -8).mov64(3, 0).ld_map_fd(1, q.fd).call(MAP_PUSH)
    qa = attach(push.mov64(0, 0).exit().assemble(), F1, name="pusher")
    both_refuse(r, n, T, "'pusher' touches a QUEUE / STACK map.*EBPF_BATCH_ORDERED")
    assert m.count() == 0 and len(q.queue_items()) == 0
    assert dev.uprobe_dispatch_plan(T | O) == 1 and dispatch(r, n, T | O) == 0
    assert len(q.queue_items()) == int((r["func"] == F1).sum()) and m.count() == 1
    dev.uprobe_detach(qa)
    # more running attachments than the kernel-argument table holds (64)
    m2 = dev.Map(HASH, 8, 8, 64)
    attach(programs.func_ip_count(m2.fd), F2, name="counter2")
    nop = Asm().mov64(0, 0).exit().assemble()
    for i in range(63):
        attach(nop, 0x900000 + 16 * i, name="nop%d" % i)
    both_refuse(r, n, T, "65 running attachments.*at most 64")
    both_refuse(r, n, T | O, "65 running attachments.*at most 64")
    assert m2.count() == 0
    assert dev.uprobe_dispatch_plan(0) == 0
