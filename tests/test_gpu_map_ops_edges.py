"""The generic host-side map operations (bpftime_map_lookup_elem, _update_elem,
_delete_elem, _get_next_key) at their edges, for every map type: one short
fixed script replayed on the device map and on the oracle map (syscall side),
compared step by step -- return value, errno, and the bytes of the value or
next key that comes back.

Shapes: max_entries 4, key 4 bytes (LPM: u32 prefix length + 4 data bytes),
value 8 bytes (PROG_ARRAY: 4, its only legal size; BLOOM_FILTER: no key), two
CPUs for the per-CPU types.  The keys are chosen so that the device's bucket
order is the oracle's element order wherever the script asks for a next key
(the order is not part of the reference's contract for PERCPU_HASH and
LRU_HASH, oracle/maps.c): with 4-byte keys below 256 the reference hash is
29791 * k, i.e. k mod 5 for the 5 buckets of a 4-entry HASH / PERCPU_HASH and
3 k mod 11 for the 11 buckets of a 4-entry LRU_HASH.

BLOOM_FILTER, which the oracle cannot create, is checked against the literal
(return, errno) pairs of the same script."""
import ctypes as C
import errno
import struct

import pytest

from bpftime_amd import isa
from bpftime_amd._lib import lib as dlib

pytestmark = pytest.mark.gpu

HASH, ARRAY, PROG_ARRAY = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_ARRAY, isa.BPF_MAP_TYPE_PROG_ARRAY
PERCPU_HASH, PERCPU_ARRAY = isa.BPF_MAP_TYPE_PERCPU_HASH, isa.BPF_MAP_TYPE_PERCPU_ARRAY
LRU_HASH, LPM_TRIE = isa.BPF_MAP_TYPE_LRU_HASH, isa.BPF_MAP_TYPE_LPM_TRIE
RINGBUF, BLOOM_FILTER = isa.BPF_MAP_TYPE_RINGBUF, isa.BPF_MAP_TYPE_BLOOM_FILTER

MAX_ENTRIES, NCPU = 4, 2
PROG_FD0 = 100            # PROG_ARRAY values: prog records at fds 100..104 on both sides
EXIT = bytes([0xb7, 0, 0, 0, 0, 0, 0, 0, 0x95, 0, 0, 0, 0, 0, 0, 0])  # mov r0, 0; exit


def _u32(k):
    return struct.pack("<I", k)


def _lpm(k):
    return struct.pack("<I4B", 32, 10, 0, 0, k)


# keys A, B, C, D (inserted in this order), E (the fifth insert; for the array
# types the index max_entries) and M (never present / out of range)
_IDX = dict(zip("ABCDEM", (0, 1, 2, 3, 4, 7)))
KEYS = {
    HASH: dict(zip("ABCDEM", map(_u32, (1, 2, 3, 4, 6, 9)))),          # buckets 1 2 3 4
    PERCPU_HASH: dict(zip("ABCDEM", map(_u32, (1, 2, 3, 4, 6, 9)))),
    LRU_HASH: dict(zip("ABCDEM", map(_u32, (4, 1, 5, 2, 6, 9)))),      # buckets 1 3 4 6, E 7
    LPM_TRIE: dict(zip("ABCDEM", map(_lpm, (1, 2, 3, 4, 5, 9)))),
}
for _t in (ARRAY, PERCPU_ARRAY, PROG_ARRAY, RINGBUF, BLOOM_FILTER):
    KEYS[_t] = {n: _u32(i) for n, i in _IDX.items()}


def _value(mtype, i):
    if mtype == PROG_ARRAY:
        return struct.pack("<i", PROG_FD0 + i)
    if mtype in (PERCPU_HASH, PERCPU_ARRAY):       # the syscall side moves every CPU's value
        return b"".join(struct.pack("<Q", 0x1000 * (c + 1) + i) for c in range(NCPU))
    return struct.pack("<Q", 0xA0 + i)


# (op, key name[, value index, flags])
SCRIPT = [
    # an empty map: lookup, delete and next key of a missing key; the first key
    ("lookup", "A"), ("delete", "A"), ("next", "A"), ("next", None),
    # update flags: 0; 1 on a present key; 2 on a missing key; 3; 2 on a present key
    ("update", "A", 0, 0), ("update", "A", 1, 1), ("lookup", "A"),
    ("update", "B", 1, 2), ("update", "B", 1, 3), ("update", "A", 2, 2),
    # fill the map (D becomes the least recently used element)
    ("update", "B", 1, 0), ("update", "C", 2, 1), ("update", "D", 3, 0),
    ("lookup", "D"), ("lookup", "A"), ("lookup", "B"), ("lookup", "C"),
    # next key: null key, every key, from the last key, a key that is not present
    ("next", None), ("next", "A"), ("next", "B"), ("next", "C"), ("next", "D"), ("next", "M"),
    # a fifth insert into the full map / an array index >= max_entries
    ("update", "E", 4, 0), ("lookup", "E"), ("lookup", "D"), ("next", None), ("next", "E"),
    # delete of a present key, then a lookup of it, then the delete again
    ("delete", "C"), ("lookup", "C"), ("delete", "C"), ("next", None), ("next", "B"),
    ("lookup", "M"), ("delete", "M"), ("update", "M", 0, 2),
]

ENOTSUP, EOPNOTSUPP = errno.ENOTSUP, errno.EOPNOTSUPP


class _Device:
    """The C ABI, called directly: (rc, errno when it failed, bytes)."""

    def __init__(self, dev, mtype, ks, vs):
        self.l = dlib()
        self.fd = dev.Map(mtype, ks, vs, MAX_ENTRIES).fd
        self.ks = ks

    def _call(self, f, *a):
        C.set_errno(0)
        r = f(self.fd, *a)
        return r, C.get_errno()

    def lookup(self, key):
        p, e = self._call(self.l.bpftime_map_lookup_elem, key)
        if not p:
            return (-1, e, b"")
        return (0, 0, C.string_at(p, self.l.bpftime_map_value_size_from_syscall(self.fd)))

    def update(self, key, value, flags):
        r, e = self._call(self.l.bpftime_map_update_elem, key, value, flags)
        return (r, e if r else 0, b"")

    def delete(self, key):
        r, e = self._call(self.l.bpftime_map_delete_elem, key)
        return (r, e if r else 0, b"")

    def next(self, key, out=True):
        o = C.create_string_buffer(max(self.ks, 1)) if out else None
        r, e = self._call(self.l.bpftime_map_get_next_key, key, o)
        return (r, e if r else 0, o.raw[:self.ks] if r == 0 else b"")


class _Oracle:
    def __init__(self, po, mtype, ks, vs):
        self.l = po.lib()
        self.fd = po.OracleMap(mtype, ks, vs, MAX_ENTRIES).fd
        self.ks = ks

    def lookup(self, key):
        p = self.l.orc_map_lookup_user(self.fd, key)
        if not p:
            return (-1, self.l.orc_last_errno(), b"")
        return (0, 0, C.string_at(p, self.l.orc_map_value_size_user(self.fd)))

    def update(self, key, value, flags):
        r = self.l.orc_map_update_user(self.fd, key, value, flags)
        return (r, self.l.orc_last_errno() if r else 0, b"")

    def delete(self, key):
        r = self.l.orc_map_delete_user(self.fd, key)
        return (r, self.l.orc_last_errno() if r else 0, b"")

    def next(self, key):
        o = C.create_string_buffer(max(self.ks, 1))
        r = self.l.orc_map_get_next_key(self.fd, key, o)
        return (r, self.l.orc_last_errno() if r else 0, o.raw[:self.ks] if r == 0 else b"")


def _replay(m, mtype):
    tr = []
    for step in SCRIPT:
        op, kn = step[0], step[1]
        key = None if kn is None else C.create_string_buffer(KEYS[mtype][kn], len(KEYS[mtype][kn]))
        if op == "update":
            v = _value(mtype, step[2])
            tr.append(m.update(key, C.create_string_buffer(v, len(v)), step[3]))
        else:
            tr.append(getattr(m, op)(key))
    return tr


def _sizes(mtype):
    if mtype == PROG_ARRAY:
        return 4, 4
    if mtype == LPM_TRIE:
        return 8, 8
    if mtype == BLOOM_FILTER:
        return 0, 8
    return 4, 8


@pytest.fixture()
def two_cpus(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    was = dlib().bpftime_amd_get_ncpu()
    dev.set_ncpu(NCPU)
    po.set_ncpu(NCPU)
    for i in range(5):
        assert dev.prog_create(EXIT, f"p{i}", 0, fd=PROG_FD0 + i) == PROG_FD0 + i
        assert po.prog_create(PROG_FD0 + i, EXIT) == PROG_FD0 + i
    try:
        yield po, dev
    finally:
        dev.set_ncpu(was)
        po.set_ncpu(1)


# Failures the oracle answers without setting an errno (orc_last_errno then
# returns whatever an earlier call left): a ring buffer's update / delete /
# next key (only its lookup sets ENOTSUP, ringbuf_map.cpp) and a HASH lookup
# of a missing key (hash_lookup).  Pinned to the errno the host side sets.
ORACLE_SETS_NO_ERRNO = {
    RINGBUF: {"update": ENOTSUP, "delete": ENOTSUP, "next": ENOTSUP},
    HASH: {"lookup": errno.ENOENT},
}

ORACLE_TYPES = [HASH, ARRAY, PROG_ARRAY, PERCPU_HASH, PERCPU_ARRAY, LRU_HASH, LPM_TRIE, RINGBUF]
_NAMES = {HASH: "hash", ARRAY: "array", PROG_ARRAY: "prog_array", PERCPU_HASH: "percpu_hash",
          PERCPU_ARRAY: "percpu_array", LRU_HASH: "lru_hash", LPM_TRIE: "lpm_trie", RINGBUF: "ringbuf",
          BLOOM_FILTER: "bloom_filter"}


@pytest.mark.parametrize("mtype", ORACLE_TYPES, ids=lambda t: _NAMES[t])
def test_edge_script_matches_oracle(two_cpus, mtype):
    po, dev = two_cpus
    ks, vs = _sizes(mtype)
    want = _replay(_Oracle(po, mtype, ks, vs), mtype)
    got = _replay(_Device(dev, mtype, ks, vs), mtype)
    pinned = ORACLE_SETS_NO_ERRNO.get(mtype, {})
    want = [(r, pinned[s[0]] if r and s[0] in pinned else e, b) for s, (r, e, b) in zip(SCRIPT, want)]
    for i, (step, w, g) in enumerate(zip(SCRIPT, want, got)):
        print(_NAMES[mtype], i, step, "oracle", w, "device", g)
    for i, (step, w, g) in enumerate(zip(SCRIPT, want, got)):
        assert g == w, (i, step)


# bloom_filter.cpp:283-289 (lookup: peek is the lookup), :291-322 (update is a
# push, BPF_ANY only, the key ignored), :324-335 (delete and next key)
_B_LOOKUP, _B_DELETE, _B_NEXT = (-1, EOPNOTSUPP, b""), (-1, EOPNOTSUPP, b""), (-1, ENOTSUP, b"")
_B_PUSH, _B_FLAGS = (0, 0, b""), (-1, errno.EINVAL, b"")
BLOOM_EXPECT = [
    _B_LOOKUP, _B_DELETE, _B_NEXT, _B_NEXT,
    _B_PUSH, _B_FLAGS, _B_LOOKUP,
    _B_FLAGS, _B_FLAGS, _B_FLAGS,
    _B_PUSH, _B_FLAGS, _B_PUSH,
    _B_LOOKUP, _B_LOOKUP, _B_LOOKUP, _B_LOOKUP,
    _B_NEXT, _B_NEXT, _B_NEXT, _B_NEXT, _B_NEXT, _B_NEXT,
    _B_PUSH, _B_LOOKUP, _B_LOOKUP, _B_NEXT, _B_NEXT,
    _B_DELETE, _B_LOOKUP, _B_DELETE, _B_NEXT, _B_NEXT,
    _B_LOOKUP, _B_DELETE, _B_FLAGS,
]


def test_edge_script_bloom_filter_literals(two_cpus):
    _, dev = two_cpus
    assert len(BLOOM_EXPECT) == len(SCRIPT)
    got = _replay(_Device(dev, BLOOM_FILTER, 0, 8), BLOOM_FILTER)
    for i, (step, w, g) in enumerate(zip(SCRIPT, BLOOM_EXPECT, got)):
        print("bloom_filter", i, step, "expect", w, "device", g)
    for i, (step, w, g) in enumerate(zip(SCRIPT, BLOOM_EXPECT, got)):
        assert g == w, (i, step)


def test_null_key_or_value_where_the_host_side_tests_for_one(two_cpus):
    """Every NULL test of the generic operations.  The oracle dereferences
    these arguments (it restates the map classes, which the reference's
    handler calls with checked pointers), so the expected pairs are literals,
    except the LRU lookup, which both answer (lru_var_hash_map.cpp:27-41)."""
    po, dev = two_cpus
    EINVAL, ENOENT = errno.EINVAL, errno.ENOENT
    v8 = C.create_string_buffer(_value(HASH, 0), 8)

    lru = _Device(dev, LRU_HASH, 4, 8)
    assert lru.lookup(None) == (-1, ENOENT, b"") == _Oracle(po, LRU_HASH, 4, 8).lookup(None)
    assert lru.next(None, out=False) == (-1, EINVAL, b"")

    lpm = _Device(dev, LPM_TRIE, 8, 8)
    k = C.create_string_buffer(_lpm(1), 8)
    assert lpm.lookup(None) == (-1, EINVAL, b"")
    assert lpm.update(None, v8, 0) == (-1, EINVAL, b"")
    assert lpm.update(k, None, 0) == (-1, EINVAL, b"")
    assert lpm.delete(None) == (-1, EINVAL, b"")
    assert lpm.next(None, out=False) == (-1, EINVAL, b"")
    assert lpm.next(k, out=False) == (-1, EINVAL, b"")

    for t in (HASH, PERCPU_HASH):
        assert _Device(dev, t, 4, 8).next(None, out=False) == (-1, EINVAL, b"")

    bloom = _Device(dev, BLOOM_FILTER, 0, 8)
    assert bloom.update(None, None, 0) == (-1, EINVAL, b"")
    assert bloom.update(None, v8, 0) == (0, 0, b"")
