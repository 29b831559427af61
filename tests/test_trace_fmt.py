"""bpf_trace_printk's format scanner and host line formatter (bpftime_amd/
csrc/trace_fmt.hpp) on the host: every accepted conversion with every length
modifier, each rejection, the caps at, below and above, a '%' as the last
byte, fmt_size ending before the NUL, the formatter's lines against snprintf
for edge values, flags, widths and precisions, and (null) / (efault) / cut
strings (tests/cpp/trace_fmt_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bpftime_amd", "lib", "trace_fmt_test")


def test_scanner_and_formatter():
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
