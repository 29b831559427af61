"""bpftime_amd_last_seq_tier (include/bpftime_amd.h): the symbol, its Python
binding, and its answer before any thread-ordered dispatch.  The answer is
thread-local state of the library, so "before any" is asked in a process of
its own."""
import os
import re
import subprocess
import sys

from bpftime_amd import _lib
from bpftime_amd import vm as dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "bpftime_amd.h")).read()
    assert re.search(r"\bint\s+bpftime_amd_last_seq_tier\s*\(\s*void\s*\)\s*;", hdr)
    fn = _lib.lib().bpftime_amd_last_seq_tier
    assert fn.argtypes is not None and len(fn.argtypes) == 0
    assert callable(dev.last_seq_tier)


def test_minus_one_before_any_dispatch():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import threading\n"
            "from bpftime_amd import vm as dev\n"
            "got = [dev.last_seq_tier()]\n"
            "t = threading.Thread(target=lambda: got.append(dev.last_seq_tier()))\n"
            "t.start(); t.join()\n"
            "print(got)\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "[-1, -1]"
