"""The host surface of the task and trace helpers, without a device: the new
symbols, bpftime_amd_vm_set_task's argument checks, the reference's defaults
(the basename of /proc/self/exe, the gid in both halves) and
bpftime_amd_trace_read before any log exists."""
import ctypes as C
import os
import subprocess
import sys

import _tracehelpers as th
from bpftime_amd import isa
from bpftime_amd.isa import Asm
from bpftime_amd import vm as dev


def test_symbols_and_ids():
    for name in ("bpftime_amd_vm_set_task", "bpftime_amd_vm_get_task", "bpftime_amd_trace_read",
                 "bpftime_amd_enable_trace_printk"):
        assert hasattr(dev.lib(), name)
    assert (isa.BPF_FUNC_trace_printk, isa.BPF_FUNC_get_current_uid_gid, isa.BPF_FUNC_get_current_comm,
            isa.BPF_FUNC_probe_write_user, isa.BPF_FUNC_ktime_get_boot_ns,
            isa.BPF_FUNC_ktime_get_coarse_ns) == (6, 15, 16, 36, 125, 160)


def test_trace_printk_switch_reports_the_previous_setting():
    was = dev.enable_trace_printk(True)
    assert dev.enable_trace_printk(False) is True
    assert dev.enable_trace_printk(False) is False
    # off: registered by hand it is still refused at load, naming the helper (no device needed)
    vm = dev.VM()
    vm.register(6, "bpf_trace_printk")
    rc, msg = vm.try_load(Asm().call(6).exit().assemble())
    assert rc == -22 and "has no device implementation" in msg
    dev.enable_trace_printk(was)


def test_defaults_are_the_reference_answers():
    vm = dev.VM()
    comm, uid_gid = vm.get_task()
    assert comm == os.path.basename(os.readlink("/proc/self/exe")).encode()[:63] == th.default_comm()
    assert uid_gid == (os.getgid() << 32) | os.getgid() == th.default_uid_gid()


def test_set_task_checks_its_arguments():
    vm = dev.VM()
    vm.set_task(comm=b"worker", uid_gid=(1000 << 32) | 1001)
    assert vm.get_task() == (b"worker", (1000 << 32) | 1001)
    vm.set_task(comm=b"other")                      # NULL uid_gid: left alone
    assert vm.get_task() == (b"other", (1000 << 32) | 1001)
    vm.set_task(uid_gid=5)                          # NULL comm: left alone
    assert vm.get_task() == (b"other", 5)
    vm.set_task(comm=b"c" * 63)                     # 63 bytes and the NUL fit
    assert vm.get_task() == (b"c" * 63, 5)
    u = C.c_uint64(9)                               # 64 bytes: refused, the VM unchanged
    assert dev.lib().bpftime_amd_vm_set_task(C.c_void_p(vm.h), b"d" * 64, C.byref(u)) == -1
    assert vm.get_task() == (b"c" * 63, 5)
    vm.set_task(comm=b"")
    assert vm.get_task() == (b"", 5)
    # the 64 bytes the kernels read are zero from the NUL on
    vm.set_task(comm=b"long-name-first")
    vm.set_task(comm=b"ab")
    raw = C.create_string_buffer(b"\xff" * 64, 64)
    assert dev.lib().bpftime_amd_vm_get_task(C.c_void_p(vm.h), raw, None) == 0
    assert raw.raw == b"ab" + bytes(62)
    other = dev.VM()                                # identity is per VM
    assert other.get_task() == (th.default_comm(), th.default_uid_gid())


def test_trace_read_without_a_log():
    # in a fresh process: no program that calls bpf_trace_printk was loaded
    # there, so no log exists (and no device is touched)
    code = ("import ctypes as C\n"
            "from bpftime_amd import vm as dev\n"
            "lost = C.c_uint64(3)\n"
            "assert dev.lib().bpftime_amd_trace_read(None, 0, None, 0, C.byref(lost)) == -1\n"
            "assert lost.value == 3\n"
            "assert dev.trace_read() is None\n"
            "print('OK')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr
