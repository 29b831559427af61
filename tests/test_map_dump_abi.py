"""bpftime_amd_map_dump without a device: the three symbols are exported and
declared, the argument struct has the header's layout, and the checks that
run before any device work (NULL args, unknown flag bits, an fd that is no
map) refuse by errno."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

from bpftime_amd import _lib, vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bpftime_amd.h")
SYMBOLS = ("bpftime_amd_map_dump", "bpftime_amd_map_dump_tile", "bpftime_amd_map_dump_scan_tiles")


def test_symbols_exported_and_declared():
    l = _lib.lib()
    txt = open(HEADER).read()
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in SYMBOLS:
        assert hasattr(l, name), name
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in bound
    assert re.search(r"#define\s+BPFTIME_AMD_DUMP_DELETE\s+1u", txt)
    assert vm.DUMP_DELETE == 1
    assert "LRU_HASH it is ENOTSUP" in txt  # the header says what the PR leaves out


def test_tile_and_scan_tiles():
    l = _lib.lib()
    tile, scan = l.bpftime_amd_map_dump_tile(), l.bpftime_amd_map_dump_scan_tiles()
    assert tile >= 64 and tile % 64 == 0  # whole waves
    assert scan == 0 or scan % 64 == 0


def test_struct_matches_header(tmp_path):
    """sizeof and every field offset, from the C compiler."""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    fields = [f[0] for f in _lib.MapDumpArgs._fields_]
    src = tmp_path / "sz.c"
    prints = "".join('printf("%%zu\\n", offsetof(struct bpftime_amd_map_dump_args, %s));' % f for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpftime_amd.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(struct bpftime_amd_map_dump_args));%s return 0;}\n' % prints)
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(_lib.MapDumpArgs) == 64
    assert out[1:] == [getattr(_lib.MapDumpArgs, f).offset for f in fields]


def _call(a):
    C.set_errno(0)
    r = _lib.lib().bpftime_amd_map_dump(a)
    return r, C.get_errno()


def test_refusals_before_device_work():
    l = _lib.lib()
    assert _call(None) == (-1, errno.EINVAL)
    assert b"NULL" in l.bpftime_amd_last_error()
    a = _lib.MapDumpArgs(fd=777, cap=4)
    assert _call(C.byref(a)) == (-1, errno.ENOENT)
    assert b"777" in l.bpftime_amd_last_error()
    assert _call(C.byref(_lib.MapDumpArgs(fd=-1, cap=4))) == (-1, errno.ENOENT)
    for flags in (2, 3, 0x80000000):
        a = _lib.MapDumpArgs(fd=777, flags=flags, cap=4)
        assert _call(C.byref(a)) == (-1, errno.EINVAL), flags
        assert b"flags" in l.bpftime_amd_last_error()
    # the delete bit alone is a known flag: the fd is what is wrong
    a = _lib.MapDumpArgs(fd=777, flags=vm.DUMP_DELETE, cap=4)
    assert _call(C.byref(a)) == (-1, errno.ENOENT)


def test_batch_commands_refuse_before_device_work():
    """BPF_MAP_LOOKUP_BATCH / _AND_DELETE_BATCH are served: an fd that is no
    map is ENOENT (not the ENOTSUP of an unserved command), nonzero elem_flags
    or flags EINVAL."""
    for cmd in (vm.BPF_MAP_LOOKUP_BATCH, vm.BPF_MAP_LOOKUP_AND_DELETE_BATCH):
        assert vm.sys_bpf(cmd, vm.attr_map_batch(777, 0, 0, 0, 0, 4)) == (-1, errno.ENOENT)
        assert vm.sys_bpf(cmd, vm.attr_map_batch(777, 0, 0, 0, 0, 4, elem_flags=4)) == (-1, errno.EINVAL)
        assert vm.sys_bpf(cmd, vm.attr_map_batch(777, 0, 0, 0, 0, 4, flags=1)) == (-1, errno.EINVAL)
    a = vm.attr_map_batch(5, 1, 2, 3, 4, 6, elem_flags=7, flags=8)
    assert vm.batch_count(a) == 6 and len(a) == 128
