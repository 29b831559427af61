"""The range guard of the copy / compare helpers (bpftime_amd/csrc/
mem_guard.hpp: what bpf_probe_read*, bpf_probe_read_*_str and bpf_strncmp may
touch) on the host: NULL, one byte before and after each window, ranges
straddling a window's end or spanning two adjacent windows, wrap-around at
2^64, n = 0 and n = 2^63, stack ranges crossing the stack's top and bottom,
the ctx copy, and bounds checking turned off (tests/cpp/mem_guard_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bpftime_amd", "lib", "mem_guard_test")


def test_guard_accepts_only_ranges_inside_one_region():
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
