#!/usr/bin/env python3
"""The numbers of DESIGN.md §6 "Map dump and drain": what reading a hash map
out costs by (A) the get_next_key + lookup_elem walk a libbpf tool does, (B)
Map.snapshot() + Map.hash_items() (the raw table to the host, decoded there),
(C) Map.dump (compacted on the device).  A and B are the yardsticks, as they
stand without the dump.

Maps: flow-hash's (HASH 16/16, 65536 entries; full and 10 % full) and a
syscount-sized one (HASH 4/8, 1024 entries, 512 live).  Every key sits in its
home bucket (the tables are written as images), so the walk's probes are the
shortest they can be.  B and C: 2 warm-ups, then 10 timed runs; A: 1 warm-up
and 3 timed runs -- over the first WALK_KEYS keys only where the map holds
more, reported per key and scaled to the whole map (marked "scaled": the cost
per key does not depend on how far the walk has come, each step copies the
whole table).  Wall-clock times of the whole call, host side included: that is
what the caller waits for.  Prints one JSON line per (map, method)."""
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from bpftime_amd import isa, vm as dev  # noqa: E402

WALK_KEYS = 2048


def key_for_bucket(t, nb, ks):
    """A key of ks bytes whose hash (h = h * 31 + byte) is t modulo nb: the
    last four bytes are h's digits in base 31 (the first may reach 255)."""
    h = t + nb  # (> 0: no all-zero key)
    d3, r = divmod(h, 31 ** 3)
    d2, r = divmod(r, 31 ** 2)
    d1, d0 = divmod(r, 31)
    assert d3 < 256
    k = np.zeros(ks, dtype=np.uint8)
    k[ks - 4:] = (d3, d2, d1, d0)
    return k


def fill(m, live):
    nb, ss, ko, vo, _ = m.geometry()
    raw = np.zeros((nb, ss), dtype=np.uint8)
    rng = np.random.default_rng(nb)
    for t in live:
        raw[t, 0] = 1
        raw[t, ko:ko + m.key_size] = key_for_bucket(int(t), nb, m.key_size)
    raw[live, vo:vo + m.value_size] = rng.integers(0, 256, (len(live), m.value_size), dtype=np.uint8)
    m.restore(raw.reshape(-1))
    assert m.count() == len(live)


def walk(m, limit):
    out, k = {}, m.next_key(None)
    while k is not None and len(out) < limit:
        out[bytes(k)] = m.lookup(k)
        k = m.next_key(k)
    return out


def timed(f, warm, runs):
    for _ in range(warm):
        f()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return r, ms


def report(case, method, entries, ms, **extra):
    print(json.dumps({"map": case, "method": method, "entries": entries, "ms_median": round(statistics.median(ms), 4),
                      "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "runs": len(ms), **extra}), flush=True)


def main():
    cases = [("flow-hash 16/16 x65536 full", 16, 16, 65536, 1), ("flow-hash 16/16 x65536 10% full", 16, 16, 65536, 10),
             ("syscount 4/8 x1024, 512 live", 4, 8, 1024, 2)]
    for case, ks, vs, mx, every in cases:
        dev.reset_runtime()
        m = dev.Map(isa.BPF_MAP_TYPE_HASH, ks, vs, mx)
        live = np.arange(0, mx, every)
        fill(m, live)
        n = len(live)
        items, ms = timed(m.hash_items, 2, 10)
        assert len(items) == n
        report(case, "snapshot+hash_items", n, ms, table_bytes=m.storage_bytes())

        def dump():
            k, v, nxt, end = m.dump()
            assert nxt == end
            return k, v
        (k, v), ms = timed(dump, 2, 10)
        assert {bytes(a): bytes(b) for a, b in zip(k, v)} == items
        report(case, "dump", n, ms, bytes_out=int(k.nbytes + v.nbytes))
        lim = min(n, WALK_KEYS)
        w, ms = timed(lambda: walk(m, lim), 1, 3)
        assert len(w) == lim and all(items[a] == b for a, b in w.items())
        if lim < n:
            report(case, "next_key+lookup walk", lim, ms, ms_per_key=round(statistics.median(ms) / lim, 4),
                   scaled_to_entries=n, ms_scaled=round(statistics.median(ms) / lim * n, 1), scaled=True)
        else:
            report(case, "next_key+lookup walk", lim, ms, ms_per_key=round(statistics.median(ms) / lim, 4))
    dev.reset_runtime()


if __name__ == "__main__":
    main()
