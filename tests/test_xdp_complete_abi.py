"""bpftime_amd_xdp_complete (include/bpftime_amd.h): the prototypes in the
header, the symbols, the ctypes structure's size, and every refusal -- each -1
with a named error before anything is launched, so none needs a device."""
import ctypes as C
import os
import re

import pytest

from bpftime_amd import _lib
from bpftime_amd import vm as dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "bpftime_amd.h")).read()
    assert re.search(r"\bint\s+bpftime_amd_xdp_complete\s*\(\s*const\s+struct\s+bpftime_amd_xdp_complete_args\s*\*\s*"
                     r"args\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+bpftime_amd_xdp_complete_from_batch\s*\(\s*const\s+struct\s+ebpf_batch\s*\*\s*batch\s*,"
                     r"\s*struct\s+bpftime_amd_xdp_complete_args\s*\*\s*args\s*\)\s*;", hdr)
    assert re.search(r"struct\s+bpftime_amd_xdp_complete_args\s*\{\s*uint32_t\s+struct_size\s*;", hdr)
    assert re.search(r"#define\s+BPFTIME_AMD_XDP_COMPLETE_SYNC\s+0x1\b", hdr)
    lib = _lib.lib()
    assert lib.bpftime_amd_xdp_complete.restype is C.c_int and len(lib.bpftime_amd_xdp_complete.argtypes) == 1
    assert lib.bpftime_amd_xdp_complete_tile() > 0 and lib.bpftime_amd_xdp_complete_tile() % 64 == 0
    assert lib.bpftime_amd_xdp_complete_scan_tiles() > 0
    assert callable(dev.xdp_complete)
    assert dev.XDP_FRAME_MASK_DEFAULT == 0x1C and dev.XDP_COMPLETE_SYNC == 1


def _host(n, ctype=C.c_uint32):
    """Host memory standing in for a device array: a refused call reads none of it."""
    keep = (ctype * n)()
    return keep, C.cast(keep, C.c_void_p).value


_KEEP = []


def _good(**over):
    """Arguments that pass every check (descriptor mode, count 4)."""
    k, v = _host(8)
    k2, d = _host(16, C.c_uint64)
    hc = (C.c_uint32 * 5)()
    _KEEP.extend([k, k2, hc])
    a = _lib.XdpCompleteArgs(struct_size=C.sizeof(_lib.XdpCompleteArgs), flags=0, count=4, verdicts=v, descs=d,
                             stride=2048, umem_bytes=1 << 20, frame_mask=0x1C)
    for name, val in over.items():
        setattr(a, name, val)
    return a


def _call(a):
    rc = _lib.lib().bpftime_amd_xdp_complete(C.byref(a) if a is not None else None)
    return rc, (_lib.lib().bpftime_amd_last_error() or b"").decode()


def test_struct_size_the_library_does_not_know_is_refused():
    size = C.sizeof(_lib.XdpCompleteArgs)
    for bad in (0, 4, size - 8, size + 8):
        rc, text = _call(_good(struct_size=bad))
        assert rc == -1 and re.search(rf"struct_size {bad}\b.*{size}", text), text
    rc, text = _call(None)
    assert rc == -1 and "args is NULL" in text


def test_each_validation_failure_is_named():
    _, v = _host(8)
    _, d = _host(16, C.c_uint64)
    _, w = _host(8)
    five = C.c_void_p * 5
    for over, what in (
            (dict(verdicts=None), "verdicts is NULL"),
            (dict(stride=0), "stride is 0"),
            (dict(count=1 << 32), r"count 4294967296.*2\^32"),
            (dict(count=(1 << 40) + 3), r"2\^32"),
            (dict(verdicts=v + 2), "verdicts: misaligned"),
            (dict(descs=d + 4), "descs: misaligned"),
            (dict(data_off_out=w + 1), "data_off_out: misaligned"),
            (dict(len_out=w + 2), "len_out: misaligned"),
            (dict(counts=w + 3), "counts: misaligned"),
            (dict(out=five(None, None, d + 4, None, None)), r"out\[2\]: misaligned"),
            (dict(index_out=five(None, None, None, w + 2, None)), r"index_out\[3\]: misaligned"),
            (dict(gather_descs=d + 4), "gather_descs: misaligned"),
            (dict(gather_index=w + 2), "gather_index: misaligned"),
            (dict(gather_count=w + 2), "gather_count: misaligned"),
            (dict(gather_skipped=w + 2), "gather_skipped: misaligned"),
            (dict(descs=None), "strided mode.*data_off_out and len_out"),
            (dict(descs=None, data_off_out=w), "strided mode.*data_off_out and len_out"),
            (dict(descs=None, data_off_out=w, len_out=w, stride=1 << 62), r"count \* stride.*2\^63"),
            (dict(frame_mask=0x20), "frame_mask 32"),
            (dict(gather=w, umem=w, gather_cap=4), "gather without gather_stride"),
            (dict(gather=w, gather_stride=64, gather_cap=4), "gather without umem"),
            (dict(gather=w, umem=w, gather_stride=1 << 62, gather_cap=4), r"gather_cap \* gather_stride.*2\^63"),
            (dict(gather_mask=0x2), "gather_mask 2 is outside frame_mask 28"),
            (dict(gather=w, umem=w, gather_stride=64, gather_mask=0x1D), "gather_mask 29 is outside frame_mask 28"),
            (dict(flags=dev.XDP_COMPLETE_SYNC), "SYNC without host_counts"),
            (dict(flags=0x8), "unknown flags"),
    ):
        rc, text = _call(_good(**over))
        assert rc == -1, (over, rc)
        assert text.startswith("xdp complete: ") and re.search(what, text), (over, text)


def test_count_zero_succeeds_with_zero_counts():
    hc = (C.c_uint32 * 5)(9, 9, 9, 9, 9)
    hg = (C.c_uint32 * 2)(9, 9)
    a = _good(count=0, flags=dev.XDP_COMPLETE_SYNC)
    a.host_counts = C.cast(hc, C.POINTER(C.c_uint32))
    a.host_gather = C.cast(hg, C.POINTER(C.c_uint32))
    rc, text = _call(a)
    assert rc == 0, text
    assert list(hc) == [0] * 5 and list(hg) == [0, 0]
    assert dev.xdp_complete(0, _Host(1), 2048, 1 << 20, descs=_Host(2, C.c_uint64)) == [0] * 5


def test_from_batch_fills_the_input_half():
    _, v = _host(8)
    _, d = _host(16, C.c_uint64)
    _, o = _host(8)
    b = _lib.EbpfBatch(ctx_kind=dev.CTX_XDP, count=4, data=0x1000, stride=2048, verdicts=v, descs=d,
                       umem_bytes=1 << 20, data_off_out=o, len_out=o + 16, stream=0x55)
    a = _lib.XdpCompleteArgs(struct_size=1, gather_mask=7, count=99)
    assert _lib.lib().bpftime_amd_xdp_complete_from_batch(C.byref(b), C.byref(a)) == 0
    assert a.struct_size == C.sizeof(_lib.XdpCompleteArgs) and a.flags == 0 and a.gather_mask == 0
    assert (a.count, a.verdicts, a.descs, a.data_off_out, a.len_out) == (4, v, d, o, o + 16)
    assert (a.umem, a.stride, a.umem_bytes, a.stream, a.frame_mask) == (0x1000, 2048, 1 << 20, 0x55, 0x1C)
    # strided mode: the slots are the umem
    b.descs, b.count, b.stride = None, 10, 256
    assert _lib.lib().bpftime_amd_xdp_complete_from_batch(C.byref(b), C.byref(a)) == 0
    assert a.descs is None and a.umem_bytes == 2560
    b.ctx_kind = dev.CTX_RAW
    assert _lib.lib().bpftime_amd_xdp_complete_from_batch(C.byref(b), C.byref(a)) == -1
    assert "not EBPF_CTX_XDP" in _lib.lib().bpftime_amd_last_error().decode()
    assert _lib.lib().bpftime_amd_xdp_complete_from_batch(None, C.byref(a)) == -1


class _Host:
    """Stands in for a DeviceBuffer in calls that are refused before anything is read."""

    def __init__(self, n, ctype=C.c_uint32):
        self.keep, self.ptr = _host(n, ctype)


def test_python_raises_with_the_library_text():
    v, d = _Host(8), _Host(16, C.c_uint64)
    with pytest.raises(dev.EbpfError, match="xdp complete: verdicts is NULL"):
        dev.xdp_complete(4, None, 2048, 1 << 20, descs=d)
    with pytest.raises(dev.EbpfError, match="xdp complete: stride is 0"):
        dev.xdp_complete(4, v, 0, 1 << 20, descs=d)
    with pytest.raises(dev.EbpfError, match="strided mode .* needs data_off_out and len_out"):
        dev.xdp_complete(4, v, 2048, 1 << 20)
    with pytest.raises(dev.EbpfError, match="gather without gather_stride"):
        dev.xdp_complete(4, v, 2048, 1 << 20, descs=d, gather=v, umem=v)
    with pytest.raises(dev.EbpfError, match="gather_mask 2 is outside frame_mask 28"):
        dev.xdp_complete(4, v, 2048, 1 << 20, descs=d, gather_mask=2)
    with pytest.raises(dev.EbpfError, match=r"count 4294967296: must be below 2\^32"):
        dev.xdp_complete(1 << 32, v, 2048, 1 << 20, descs=d)
