"""The ARRAY_OF_MAPS model (tests/_mapinmap.py) against the facts of the
reference's map_in_maps.hpp / array_map.cpp: an array of sizeof(int) slots
whose program-side lookup returns (void *)((u_int64_t)map_id), the array
map's host update / delete / next key.  No GPU."""
import errno
import struct

import _mapinmap as mm

u32 = lambda v: struct.pack("<I", v)  # noqa: E731
i32 = lambda v: struct.pack("<i", v)  # noqa: E731


def test_zero_slot_is_null_and_sign_extension():
    o = mm.Outer(4)
    assert [o.prog_lookup(k) for k in range(4)] == [0, 0, 0, 0]  # zero-filled: every slot NULL
    assert o.update(u32(1), i32(7)) == 0 and o.prog_lookup(1) == 7
    # (u_int64_t)(int)-1: all ones; INT_MIN: the top 33 bits set
    assert o.update(u32(2), i32(-1)) == 0 and o.prog_lookup(2) == 0xFFFFFFFFFFFFFFFF
    assert o.update(u32(3), i32(-2 ** 31)) == 0 and o.prog_lookup(3) == 0xFFFFFFFF80000000
    assert o.update(u32(0), i32(2 ** 31 - 1)) == 0 and o.prog_lookup(0) == 0x7FFFFFFF
    # a key out of range: NULL (the device never faults; the reference would)
    assert o.prog_lookup(4) == 0 and o.prog_lookup(0xFFFFFFFF) == 0
    assert o.update(u32(1), i32(0)) == 0 and o.prog_lookup(1) == 0  # emptied from the host


def test_host_update_errnos_and_flags():
    o = mm.Outer(3)
    assert o.update(u32(0), i32(5), 1) == -1 and o.err == errno.EEXIST  # BPF_NOEXIST on a valid index
    assert o.update(u32(3), i32(5)) == -1 and o.err == errno.E2BIG
    assert o.update(u32(3), i32(5), 1) == -1 and o.err == errno.E2BIG  # NOEXIST out of range: E2BIG
    assert o.update(u32(0xFFFFFFFF), i32(5), 2) == -1 and o.err == errno.E2BIG
    for bad in (3, 4, 8, 0xFFFFFFFF):
        assert o.update(u32(0), i32(5), bad) == -1 and o.err == errno.EINVAL
    assert o.slots == [0, 0, 0]
    assert o.update(u32(0), i32(5), 0) == 0 and o.update(u32(1), i32(6), 2) == 0
    # the high half of the flags passes the check; NOEXIST is compared whole
    assert o.update(u32(2), i32(9), (1 << 32) | 1) == 0
    assert o.slots == [5, 6, 9]
    assert o.update(u32(2), i32(123456), 0) == 0 and o.slots[2] == 123456  # any int: not an fd check


def test_host_lookup_delete_next_key():
    o = mm.Outer(3)
    o.update(u32(1), i32(-7))
    assert o.lookup(u32(1)) == i32(-7) and o.lookup(u32(0)) == i32(0)
    assert o.lookup(u32(3)) is None and o.err == errno.ENOENT
    assert o.delete(u32(1)) == -1 and o.err == errno.EINVAL and o.slots[1] == -7
    assert o.next_key(None) == u32(0) and o.next_key(u32(0)) == u32(1) and o.next_key(u32(1)) == u32(2)
    assert o.next_key(u32(2)) is None and o.err == errno.ENOENT
    assert o.next_key(u32(3)) == u32(0) and o.next_key(u32(0xFFFFFFFF)) == u32(0)
    assert o.push(b"") == o.pop() == o.peek() == -95
    assert bytes(o.image()) == i32(0) + i32(-7) + i32(0)


def test_program_side_update_delete():
    o = mm.Outer(2)
    o.update(u32(0), i32(4))
    assert o.prog_update() == o.prog_delete() == (-22) & 0xFFFFFFFFFFFFFFFF
    assert o.slots == [4, 0]
