"""bpftime_amd_uprobe_dispatch_events (include/bpftime_amd.h): the prototype and
the event macro in the header, the symbol, the Python binding, and the refusals
that need no device -- each -1 with EINVAL and a named error."""
import ctypes as C
import errno
import os
import re

import pytest

from bpftime_amd import _lib
from bpftime_amd import vm as dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, P, O = dev.DISPATCH_THREADS, dev.DISPATCH_PROGRAMS, dev.BATCH_ORDERED


def test_header_library_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "bpftime_amd.h")).read()
    assert re.search(r"\bint64_t\s+bpftime_amd_uprobe_dispatch_events\s*\(\s*const\s+struct\s+bpftime_amd_call_records"
                     r"\s*\*\s*r\s*,\s*const\s+uint32_t\s*\*\s*events\s*,\s*uint64_t\s+n_events\s*,\s*uint32_t\s*\*\s*"
                     r"out_state\s*,\s*int64_t\s*\*\s*out_rets\s*,\s*uint32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;",
                     hdr)
    assert re.search(r"#define\s+BPFTIME_AMD_CALL_EVENT\(record,\s*phase\)\s+\(\(\(uint32_t\)\(record\)\s*<<\s*1\)\s*\|"
                     r"\s*\(\(uint32_t\)\(phase\)\s*&\s*1u\)\)", hdr)
    fn = _lib.lib().bpftime_amd_uprobe_dispatch_events
    assert fn.argtypes is not None and len(fn.argtypes) == 7 and fn.restype is C.c_int64
    assert callable(dev.uprobe_dispatch_events) and callable(dev.call_event)


def test_call_event_round_trips():
    for record in (0, 1, 64, 1030, (1 << 31) - 1):
        for phase in (0, 1):
            w = dev.call_event(record, phase)
            assert 0 <= w < 1 << 32 and w >> 1 == record and w & 1 == phase
    assert [dev.call_event(i // 2, i % 2) for i in range(6)] == list(range(6))


def _call(r, events, n_events, flags):
    C.set_errno(0)
    rc = _lib.lib().bpftime_amd_uprobe_dispatch_events(C.byref(r) if r is not None else None, events, n_events, None,
                                                       None, flags, None)
    return rc, C.get_errno(), (_lib.lib().bpftime_amd_last_error() or b"").decode()


def test_refusals_that_need_no_device():
    r = _lib.CallRecords(count=4)
    words = (C.c_uint32 * 4)(0, 1, 2, 3)                 # (host memory: a refused call reads none of it)
    ev = C.cast(words, C.c_void_p)
    for args, what in (((None, ev, 4, T), "no records"),
                       ((r, None, 4, T), "no events"),
                       ((r, ev, 0, T), "no events"),
                       ((r, ev, 4, 0), "BPFTIME_AMD_DISPATCH_THREADS"),
                       ((r, ev, 4, O), "BPFTIME_AMD_DISPATCH_THREADS"),
                       ((r, ev, 4, P), "BPFTIME_AMD_DISPATCH_THREADS"),
                       ((r, ev, 4, T | P), "BPFTIME_AMD_DISPATCH_PROGRAMS"),
                       ((r, ev, 4, T | P | O), "BPFTIME_AMD_DISPATCH_PROGRAMS"),
                       ((_lib.CallRecords(count=1 << 31), ev, 4, T), "2\\^31")):
        rc, err, text = _call(*args)
        assert rc == -1 and err == errno.EINVAL, (args, rc, err)
        assert re.search(what, text), text


class _HostWords:
    """Stands in for a DeviceBuffer in calls that are refused before anything is read."""

    def __init__(self, n):
        self.keep = (C.c_uint32 * n)(*range(n))
        self.ptr = C.cast(self.keep, C.c_void_p).value


def test_python_raises_with_the_library_text():
    with pytest.raises(dev.EbpfError, match="no events"):
        dev.uprobe_dispatch_events(None, 4, None, 0)
    with pytest.raises(dev.EbpfError, match="BPFTIME_AMD_DISPATCH_THREADS is required"):
        dev.uprobe_dispatch_events(None, 4, _HostWords(4), 4, flags=dev.BATCH_SYNC)
    with pytest.raises(dev.EbpfError, match="BPFTIME_AMD_DISPATCH_PROGRAMS"):
        dev.uprobe_dispatch_events(None, 4, _HostWords(4), 4, flags=dev.BATCH_SYNC | T | P)
