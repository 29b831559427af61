"""The thread grouping on its own (csrc/group.hip bpftime_amd_group_threads,
vm.group_threads): the stable radix sort of (pid_tgid, record index) pairs and
the select of run heads that both thread-ordered dispatches stand on, against
np.argsort(keys, kind="stable") over the uint64 keys (tests/_thread_groups.py).

perm must be the stable argsort exactly -- a thread's records in record order
is what makes the replay thread-ordered --, nseg the number of distinct keys,
seg the strictly increasing run heads with seg[0] = 0 and seg[nseg] = n.

n crosses the helper kernels' 256-lane blocks and rocprim's single-block,
merge and multi-pass sorts (1 .. 2^20 + 1).  The key sets: one thread, all
distinct, 4,096 / 16,385 / 65,537 ragged threads, keys that differ only in bit
63, only in bit 0, only in the tgid word, only in the tid word, keys at or
above 2^63 among small ones (the order is unsigned), and sorted, reverse-sorted
and thread-contiguous input.  Also the strides the dispatches use: 128 with
the key at +88 (the AoS timed record), 32 with the key at +24 (the SoA exit
array)."""
import ctypes as C

import numpy as np
import pytest

from bpftime_amd import _lib

import _thread_groups as tg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f,n,distinct", tg.CASES, ids=tg.IDS)
def test_grouping_is_the_stable_argsort(fresh_runtime, f, n, distinct):
    dev = fresh_runtime
    keys = tg.keys_of(f, n)
    if distinct is not None:
        assert len(np.unique(keys)) == distinct(n)
    perm, seg, nseg = dev.group_threads(dev.DeviceBuffer.from_array(keys), n)
    tg.check(keys, perm, seg, nseg)


@pytest.mark.parametrize("n", [257, (1 << 16) + 3])
@pytest.mark.parametrize("stride,offset", [tg.AOS_TIMED, tg.SOA_EXIT], ids=["aos128+88", "soa32+24"])
@pytest.mark.parametrize("f", [tg.unsigned_mix, tg.contiguous, tg.distinct], ids=lambda f: f.__name__)
def test_keys_inside_records(fresh_runtime, f, stride, offset, n):
    """The key read at its offset of a wider record: every other byte is noise."""
    dev = fresh_runtime
    keys = tg.keys_of(f, n)
    raw = tg.strided(keys, stride, offset, np.random.default_rng(n + stride))
    perm, seg, nseg = dev.group_threads(dev.DeviceBuffer.from_array(raw), n, stride=stride, offset=offset)
    tg.check(keys, perm, seg, nseg)


def test_invalid_input_is_refused_before_any_launch(fresh_runtime):
    """n == 0, no keys, a stride that is no multiple of 8: an error, and the
    scratch -- where every launch of the grouping writes -- is left as it was."""
    dev = fresh_runtime
    l = _lib.lib()
    assert l.bpftime_amd_group_scratch_bytes(0) == 0
    nbytes = l.bpftime_amd_group_scratch_bytes(64)
    assert nbytes > 0
    keys = dev.DeviceBuffer.from_array(tg.keys_of(tg.distinct, 64))
    scratch = dev.DeviceBuffer.from_array(np.full(nbytes, 0xA5, dtype=np.uint8))
    for ptr, stride, n in [(keys.ptr, 8, 0), (None, 8, 64), (keys.ptr, 12, 64), (keys.ptr, 4, 64)]:
        perm, seg, nseg = C.c_void_p(), C.c_void_p(), C.c_uint64(77)
        e = l.bpftime_amd_group_threads(ptr, stride, n, scratch.ptr, C.byref(perm), C.byref(seg), C.byref(nseg), None)
        assert e != 0, (ptr, stride, n)
        assert perm.value is None and seg.value is None and nseg.value == 77
    assert l.bpftime_amd_sync() == 0
    assert (scratch.download() == 0xA5).all()
    for kw in [dict(n=0), dict(n=8, stride=12)]:
        with pytest.raises(dev.EbpfError, match="hipError_t"):
            dev.group_threads(keys, **kw)
    with pytest.raises(dev.EbpfError, match="hipError_t"):
        dev.group_threads(None, 8)
    # and a valid call after the refused ones
    perm, seg, nseg = dev.group_threads(keys, 64)
    tg.check(tg.keys_of(tg.distinct, 64), perm, seg, nseg)
