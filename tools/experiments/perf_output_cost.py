#!/usr/bin/env python3
"""Two numbers for DESIGN.md §6 (perf event output): 2^22 units each emitting
one 32-byte event, (A) programs.perf_event_emitter through bpf_perf_event_output
into one software perf event's ring, (B) programs.ringbuf_emitter through
bpf_ringbuf_output into a RINGBUF map, both rings large enough for every
event (256 MiB).  Median kernel time of 10 EBPF_BATCH_TIMED batches after 3
warm-ups, the ring drained before each.  Prints one JSON line per case."""
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from bpftime_amd import isa, programs, vm as dev  # noqa: E402

N = 1 << 22
RING = 1 << 28


def main():
    units = np.random.default_rng(5).integers(0, 256, (N, 64), dtype=np.uint8)
    d = dev.DeviceBuffer.from_array(units)
    rets = dev.DeviceBuffer(8 * N)
    ev = dev.PerfEvent(data_bytes=RING)
    arr = dev.Map(isa.BPF_MAP_TYPE_PERF_EVENT_ARRAY, 4, 4, 64)
    for k in range(64):
        assert arr.set_perf(k, ev) == 0
    rb = dev.Map(isa.BPF_MAP_TYPE_RINGBUF, 0, 0, RING)
    L = dev.lib()

    def drain_perf():
        h, t, _ = ev.state()
        return (h - t) // 48

    def reset_perf():  # (the consumer: tail := head, without copying 192 MiB out)
        buf = np.empty(1 << 26, dtype=np.uint8)
        used = dev.C.c_uint64(0)
        while L.bpftime_amd_perf_event_fetch(ev.fd, buf.ctypes.data, buf.nbytes, dev.C.byref(used)) > 0:
            pass

    def reset_rb():
        buf = np.empty(1 << 26, dtype=np.uint8)
        used = dev.C.c_uint64(0)
        while L.bpftime_amd_ringbuf_fetch(rb.fd, buf.ctypes.data, buf.nbytes, dev.C.byref(used)) > 0:
            pass

    for name, code, reset in (("perf_event_output_32B", programs.perf_event_emitter(arr.fd), reset_perf),
                              ("ringbuf_output_32B", programs.ringbuf_emitter(rb.fd), reset_rb)):
        v = dev.VM()
        v.load(code)
        ms = []
        for it in range(13):
            rc = v.exec_batch(dev.CTX_RAW, d, N, 64, fixed_len=64, rets=rets, flags=dev.BATCH_SYNC | dev.BATCH_TIMED)
            assert rc == 0
            if it >= 3:
                ms.append(v.last_batch_ms())
            if name.startswith("perf"):
                assert drain_perf() == N
            reset()
        assert not rets.download(np.uint64).any()
        print(json.dumps({"case": name, "units": N, "event_bytes": 32, "ms_median": round(statistics.median(ms), 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}), flush=True)


if __name__ == "__main__":
    main()
