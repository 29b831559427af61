#!/usr/bin/env python3
"""Numbers for DESIGN.md §6 (XDP completion): bpftime_amd_xdp_complete over
2^24 units in descriptor mode, 64-B frames at chunk + 256 of 2048-B chunks, for
the verdicts xdp-counter leaves (all XDP_TX) and for a seeded mix with one TX
in 16 (the rest DROP), each with and without the gather of the TX frames into
64-B slots.  Device time by stream events around the call, the median of 7
after 3 warm-ups, the cases taken alternately in one process.

Beside it the host path a runner has without the call: the verdicts copied to
pinned host memory, numpy.flatnonzero per class, and one device-to-host copy
per TX frame into a pinned buffer.  The per-frame copies are timed over the
first 20000 TX frames and scaled to the TX count (16 M copies from Python
would take minutes); the line says so.
Prints one JSON line per case; with a path argument also writes the file."""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from bpftime_amd import vm as dev  # noqa: E402
import _xdp_complete as X  # noqa: E402

N, CHUNK, FRAME, REPS, WARM, SAMPLE = 1 << 24, 2048, 64, 7, 3, 20000


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else None
    L = dev.lib()
    assert L.bpftime_amd_device_count() > 0, "no GPU visible"
    rng = np.random.default_rng(16)
    descs = X.descs_of(np.arange(N, dtype=np.uint64) * np.uint64(CHUNK) + np.uint64(256), FRAME, 0)
    umem_bytes = N * CHUNK
    umem = dev.DeviceBuffer(umem_bytes)      # (its bytes are never looked at: only moved)
    dd = dev.DeviceBuffer.from_array(descs)
    verdicts = {"all_tx": np.full(N, X.TX, np.uint32),
                "tx_1_in_16": np.where(rng.integers(0, 16, N) == 0, X.TX, X.DROP).astype(np.uint32)}
    dv = {k: dev.DeviceBuffer.from_array(v) for k, v in verdicts.items()}
    out = [dev.DeviceBuffer(16 * N) if k in (X.DROP, X.TX) else None for k in range(5)]
    idx = [dev.DeviceBuffer(4 * N) if k in (X.DROP, X.TX) else None for k in range(5)]
    cap = [N if k in (X.DROP, X.TX) else 0 for k in range(5)]
    counts = dev.DeviceBuffer(32)
    gather, g_descs, g_index = dev.DeviceBuffer(N * FRAME), dev.DeviceBuffer(16 * N), dev.DeviceBuffer(4 * N)
    g_count, g_skipped = dev.DeviceBuffer(4), dev.DeviceBuffer(4)
    s = L.bpftime_amd_stream_create()
    e0, e1 = dev.Event(), dev.Event()

    def device(mix, with_gather):
        g = dict(gather=gather, gather_stride=FRAME, gather_cap=N, gather_mask=1 << X.TX, gather_descs=g_descs,
                 gather_index=g_index, gather_count=g_count, gather_skipped=g_skipped) if with_gather else {}
        e0.record(s)
        dev.xdp_complete(N, dv[mix], CHUNK, umem_bytes, descs=dd, umem=umem, out=out, index_out=idx, cap=cap,
                         counts=counts, stream=s, sync=False, **g)
        e1.record(s)
        assert L.bpftime_amd_stream_sync(s) == 0
        return e0.elapsed_ms(e1)

    pinned_v = L.bpftime_amd_host_alloc(4 * N)
    pinned_f = L.bpftime_amd_host_alloc(SAMPLE * FRAME)
    assert pinned_v and pinned_f
    host_v = np.frombuffer((C.c_uint8 * (4 * N)).from_address(pinned_v), np.uint32)

    def host(mix):
        t0 = time.perf_counter()
        assert L.bpftime_amd_memcpy_dtoh(pinned_v, C.c_void_p(dv[mix].ptr), 4 * N) == 0
        t1 = time.perf_counter()
        lists = [np.flatnonzero(host_v == k) for k in range(5)]
        t2 = time.perf_counter()
        tx = lists[X.TX]
        m = min(SAMPLE, len(tx))
        addrs = descs["addr"][tx[:m]]
        for j in range(m):
            L.bpftime_amd_memcpy_dtoh(pinned_f + j * FRAME, C.c_void_p(umem.ptr + int(addrs[j])), FRAME)
        t3 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3 / m * len(tx), len(tx)

    cases = [(mix, g) for mix in verdicts for g in (False, True)]
    dev_ms = {c: [] for c in cases}
    host_ms = {mix: [] for mix in verdicts}
    for it in range(WARM + REPS):
        for c in cases:                                   # alternately: a drift hits them all alike
            ms = device(*c)
            if it >= WARM:
                dev_ms[c].append(ms)
        if it >= WARM and it < WARM + 3:
            for mix in verdicts:
                host_ms[mix].append(host(mix))
    for mix, v in verdicts.items():                       # what was timed is also right
        got = counts_of(dev, N, dv[mix], dd, umem_bytes)
        assert got == [int((v == k).sum()) for k in range(5)], got
    lines = []
    for (mix, g), ms in dev_ms.items():
        med = statistics.median(ms)
        lines.append(json.dumps({"case": "device", "verdicts": mix, "gather": g, "units": N,
                                 "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                 "Munits_per_s": round(N / med / 1e3, 1)}))
    for mix, rows in host_ms.items():
        d2h, scan, copies = (statistics.median(r[k] for r in rows) for k in range(3))
        lines.append(json.dumps({"case": "host_path", "verdicts": mix, "units": N, "tx_frames": rows[0][3],
                                 "d2h_verdicts_ms": round(d2h, 3), "flatnonzero_x5_ms": round(scan, 3),
                                 "per_frame_copies_ms_scaled": round(copies, 1),
                                 "copies_timed": min(SAMPLE, rows[0][3]),
                                 "total_ms": round(d2h + scan + copies, 1)}))
    for line in lines:
        print(line, flush=True)
    if path:
        with open(path, "w") as f:
            f.write("# tools/xdp_complete_measure.py on one MI355X: 2^24 units, descriptor mode, 64-B frames at chunk + "
                    "256 of 2048-B chunks; DROP and TX lists with entries and indices, with and without the gather of "
                    "the TX frames into 64-B slots.\n"
                    "# device: stream events around bpftime_amd_xdp_complete (three launches), median of 7 after 3 "
                    "warm-ups, the four cases taken alternately in one process.\n"
                    "# host_path: what a runner does without the call, median of 3: verdicts to pinned host memory, "
                    "numpy.flatnonzero per class, one device-to-host copy per TX frame -- the copies timed over the "
                    "first copies_timed TX frames and scaled to tx_frames.\n")
            f.write("\n".join(lines) + "\n")
    L.bpftime_amd_host_free(C.c_void_p(pinned_v))
    L.bpftime_amd_host_free(C.c_void_p(pinned_f))
    L.bpftime_amd_stream_destroy(s)


def counts_of(dev_, n, verdicts, descs, umem_bytes):
    return dev_.xdp_complete(n, verdicts, CHUNK, umem_bytes, descs=descs)


if __name__ == "__main__":
    main()
