"""bpftime_amd: MI355X-native per-packet eBPF execution path.

A drop-in for bpftime's VM C ABI (vm/vm-core/include/ebpf-vm.h) backed by a
gfx950 HIP interpreter kernel, plus device-resident maps behind the
bpftime_shm-style map / prog / link API.  See DESIGN.md.
"""
__all__ = ["isa", "programs", "gen", "trace_read"]


def trace_read(*args, **kwargs):
    """bpf_trace_printk's lines since the last read: vm.trace_read (loads the
    native library on first use)."""
    from .vm import trace_read as read
    return read(*args, **kwargs)
