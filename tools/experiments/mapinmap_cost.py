#!/usr/bin/env python3
"""One number for DESIGN.md §6 (map-in-map): what reaching a counter table
through an ARRAY_OF_MAPS costs against naming it in an lddw.  A parallel batch
of 2^22 64-byte packets, (A) programs.tenant_counter: a 4-slot outer over
ARRAY maps of u64 counters, the slot picked by a packet byte, (B)
programs.tenant_counter_bound: the same program with one table bound by an
lddw.  Median kernel time of 10 EBPF_BATCH_TIMED batches after 3 warm-ups.
Prints one JSON line per case."""
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from bpftime_amd import isa, programs, vm as dev  # noqa: E402

N = 1 << 22
COUNTERS = 256


def main():
    pk = np.random.default_rng(5).integers(0, 256, (N, 64), dtype=np.uint8)
    w = pk.view(np.uint32).reshape(N, 16)
    w[:, 1] %= COUNTERS + 8  # a few keys past the table's end: XDP_DROP
    tables = [dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 8, COUNTERS) for _ in range(4)]
    outer = dev.Map(isa.BPF_MAP_TYPE_ARRAY_OF_MAPS, 4, 4, 4)
    for i, t in enumerate(tables):
        assert outer.set_inner(i, t) == 0
    want = np.where(w[:, 1] < COUNTERS, isa.XDP_PASS, isa.XDP_DROP)
    dv = dev.DeviceBuffer(4 * N)
    for name, code in (("array_of_maps_4_slots", programs.tenant_counter(outer.fd)),
                       ("inner_map_bound_by_lddw", programs.tenant_counter_bound(tables[0].fd))):
        v = dev.VM()
        v.load(code)
        d = dev.DeviceBuffer.from_array(pk)
        ms = []
        for it in range(13):
            rc = v.exec_batch(dev.CTX_XDP, d, N, 64, fixed_len=64, verdicts=dv, flags=dev.BATCH_SYNC | dev.BATCH_TIMED)
            assert rc == 0
            if it >= 3:
                ms.append(v.last_batch_ms())
        assert (dv.download(np.uint32) == want).all()
        print(json.dumps({"case": name, "packets": N, "big_stack": v.info()["big_stack"],
                          "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                          "ms_max": round(max(ms), 4)}), flush=True)
    total = sum(int(t.snapshot().view(np.uint64).sum()) for t in tables)
    assert total == 26 * int((want == isa.XDP_PASS).sum()), total


if __name__ == "__main__":
    main()
