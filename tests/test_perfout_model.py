"""The perf-event model (tests/_perfout.py) against cases worked out by hand
from the reference lines it cites."""
import errno
import struct

import _perfout as pm

i32 = lambda v: struct.pack("<i", v)  # noqa: E731


def test_record_sizes():
    # (12 + size + 7) & ~7
    assert [pm.record_size(s) for s in (0, 1, 4, 5, 12, 52)] == [16, 16, 16, 24, 24, 64]


def test_a_ring_of_64_holds_two_records_of_24():
    r = pm.Ring(64)
    for _ in range(5):
        assert r.output(b"\x11" * 5) == 0          # a drop answers 0 too
    assert r.head == 2 * 24 == ((64 - 1) // 24) * 24 and r.tail == 0
    n, raw = r.fetch()
    assert n == 2 and len(raw) == 48 and r.tail == r.head == 48
    assert raw[:12] == struct.pack("<IHHI", 9, 0, 24, 12) and raw[12:17] == b"\x11" * 5


def test_the_size_bound():
    r = pm.Ring(1 << 17)
    assert pm.MAX_DATA == 65516
    assert r.output(bytes(65516)) == 0 and r.head == 65528 == pm.record_size(65516)
    assert r.output(bytes(65517)) == -1 and r.head == 65528
    arr = pm.PerfArray(1)
    arr.slots[0] = 7
    assert pm.output(arr, 0, {7: r}, None, 65517) == pm.FAIL
    assert pm.output(arr, 0, {7: r}, None, 1 << 63) == pm.FAIL
    assert pm.output(arr, 0, {7: r}, None, 8) == pm.EFAULT and r.head == 65528
    assert pm.output(arr, 1, {7: r}, b"x", 1) == pm.FAIL          # cpu >= max_entries
    assert pm.output(None, 0, {7: r}, b"x", 1) == pm.FAIL         # no perf array
    assert pm.output(arr, 0, {}, b"x", 1) == pm.FAIL              # the slot names no software perf event
    assert pm.output(arr, 0, {7: pm.Ring(0)}, b"x", 1) == 0       # no ring: dropped, 0


def test_a_record_that_wraps():
    r = pm.Ring(64)
    assert r.output(b"a" * 5) == 0 and r.output(b"b" * 5) == 0
    assert r.fetch()[0] == 2 and r.tail == 48
    data = bytes(range(1, 13))
    assert r.output(data) == 0 and r.head == 72                   # 48..72 wraps at 64
    assert bytes(r.data[48:60]) == struct.pack("<IHHI", 9, 0, 24, 12)
    assert bytes(r.data[60:64]) == data[:4] and bytes(r.data[0:8]) == data[4:]
    n, raw = r.fetch()
    assert n == 1 and raw == struct.pack("<IHHI", 9, 0, 24, 12) + data and pm.parse(raw) == [(24, data)]


def test_a_small_record_fits_after_a_big_one_was_dropped():
    r = pm.Ring(64)
    assert r.output(b"x" * 28) == 0 and r.head == 40              # 24 free, one byte kept
    assert r.output(b"y" * 12) == 0 and r.head == 40              # 24 needs > 24
    assert r.output(b"z" * 4) == 0 and r.head == 56               # 16 fits
    assert [rs for rs, _ in pm.parse(r.fetch()[1])] == [40, 16]


def test_fetch_stops_at_cap_and_drops_bad_headers():
    r = pm.Ring(128)
    for k in range(3):
        r.output(bytes([k]) * 4)
    n, raw = r.fetch(cap=40)
    assert n == 2 and len(raw) == 32 and r.tail == 32
    r.data[32 + 6:32 + 8] = struct.pack("<H", 4)                  # header size < 8: the rest is dropped
    assert r.fetch() == (0, b"") and r.tail == r.head
    r.head, r.tail = 8, 16                                        # head < tail: reset
    assert r.fetch() == (0, b"") and r.tail == 8


def test_next_key_four_cases():
    a = pm.PerfArray(3)
    assert a.next_key(None) == i32(0)
    assert a.next_key(i32(2)) is None and a.err == errno.ENOENT
    for k in (3, -1, 7):
        a.err = 0
        assert a.next_key(i32(k)) is None and a.err == errno.EINVAL
    assert a.next_key(i32(0)) == i32(1) and a.next_key(i32(1)) == i32(2)


def test_array_ops():
    a = pm.PerfArray(2)
    assert a.slots == [-1, -1] and a.lookup(i32(1)) == i32(-1)
    assert a.update(i32(1), i32(9), flags=1) == 0 and a.update(i32(1), i32(5), flags=77) == 0 and a.slots == [-1, 5]
    for k in (-1, 2):
        a.err = 0
        assert a.lookup(i32(k)) is None and a.update(i32(k), i32(1)) == -1 and a.delete(i32(k)) == -1
        assert a.err == errno.EINVAL
    assert a.delete(i32(1)) == 0 and a.slots == [-1, -1]
