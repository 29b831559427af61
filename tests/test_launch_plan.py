"""The launch plan's rules (csrc/vm_plan.cpp plan_launch) against an occupancy
model that depends only on LDS, host-only (tests/cpp/launch_plan_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bpftime_amd", "lib", "launch_plan_test")


def test_launch_plan_rules():
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
