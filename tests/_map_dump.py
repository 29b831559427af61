"""Helpers of the map dump tests: the expected results, none of which comes
from the dump itself -- the next_key / lookup walk of an oracle or device map,
the live rows of a table image decoded in numpy, and the (count, next) chain a
cursor walk must produce."""
import ctypes as C

import numpy as np

from bpftime_amd import _lib

GUARD = 0xA5


def walk(m):
    """The get_next_key + lookup walk of an oracle map or a device map: a list
    of (key, value).  (On an LRU map each lookup is a use.)"""
    out, seen, k = [], set(), m.next_key(None)
    while k is not None:
        k = bytes(k)
        # (a key that deletions orphaned is not found again and restarts the walk)
        assert k not in seen, "the next_key walk revisits a key"
        seen.add(k)
        out.append((k, m.lookup(k)))
        k = m.next_key(k)
    return out


def image_entries(raw, geometry, key_size, user_value_size):
    """The live rows (state word 1) of a snapshot / restore image in bucket
    order: (bucket indices, keys[n, key_size], values[n, user_value_size])."""
    nb, ss, ko, vo = geometry[:4]
    rows = np.asarray(raw, dtype=np.uint8)[:nb * ss].reshape(nb, ss)
    state = np.ascontiguousarray(rows[:, :4]).view(np.uint32)[:, 0]
    idx = np.flatnonzero(state == 1)
    return idx, rows[idx, ko:ko + key_size].copy(), rows[idx, vo:vo + user_value_size].copy()


def chunks(idx, cap, end, start=0):
    """The chain of (count, next) a dump with `cap` yields when chained through
    next from `start` until next == end; idx: the live bucket indices."""
    live = [int(i) for i in idx if i >= start]
    out, at = [], 0
    while True:
        n = min(cap, len(live) - at)
        at += n
        nxt = live[at] if at < len(live) else end
        out.append((n, nxt))
        if nxt == end:
            return out


def make_image(geometry, live, seed):
    """A table image for Map.restore: every byte seeded-random (so each
    bucket's key and value bytes are its own and a shifted or overlapping copy
    shows, and the dead buckets hold junk that must not come out), then the
    state words: 1 for the buckets in `live`, else 0."""
    nb, ss = geometry[:2]
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (nb, ss), dtype=np.uint8)
    st = np.zeros(nb, dtype=np.uint32)
    st[np.asarray(live, dtype=np.int64)] = 1
    raw[:, :4] = st.view(np.uint8).reshape(nb, 4)
    return raw.reshape(-1)


def dump_raw(m, cap, start=0, flags=0, keys=True, values=True, room=None):
    """bpftime_amd_map_dump into guard-filled buffers of `room` (default cap)
    entries: (rc, errno, count, next, end, keys buffer, values buffer), the
    buffers whole so the bytes past count entries can be checked."""
    room = cap if room is None else room
    kb = np.full(room * m.key_size, GUARD, dtype=np.uint8)
    vb = np.full(room * m.user_value_size, GUARD, dtype=np.uint8)
    a = _lib.MapDumpArgs(fd=m.fd, flags=flags, start=start, cap=cap,
                         keys=kb.ctypes.data if keys else None, values=vb.ctypes.data if values else None)
    C.set_errno(0)
    rc = _lib.lib().bpftime_amd_map_dump(C.byref(a))
    return rc, C.get_errno(), a.count, a.next, a.end, kb, vb


def as_pairs(keys, values):
    return [(bytes(k), bytes(v)) for k, v in zip(keys, values)]


def dump_all(m, cap, start=0, delete=False):
    """Chained dumps through next until end: (pairs, [(count, next), ...])."""
    pairs, chain = [], []
    while True:
        k, v, nxt, end = m.dump(cap=cap, start=start, delete=delete)
        pairs += as_pairs(k, v)
        chain.append((len(k), nxt))
        assert len(chain) < 1 << 16
        if nxt == end:
            return pairs, chain
        assert nxt > start or len(k) == 0
        start = nxt
