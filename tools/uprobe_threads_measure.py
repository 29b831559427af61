#!/usr/bin/env python3
"""Numbers for DESIGN.md §6 (uprobe replay, thread-ordered plan): the
funclatency pair (tests/_uprobe_threads.py: starts[tid] at entry, a log2
histogram at return) on one function, 2^20 recorded calls spread evenly
(seeded) over 4096 recorded threads, with recorded callers and clocks.  Per
BPFTIME_AMD_DISPATCH_THREADS dispatch, by stream events (EBPF_BATCH_TIMED): the
thread grouping (its launches and its one host wait) and the replay launch
k_up_seq; the median of 7 dispatches after 3 warm-ups.  For scale, the same
dispatch with EBPF_BATCH_ORDERED (one lane, the serial run) over the first
2^14 calls.  Prints one JSON line; with a path argument also writes the
measurement file."""
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from bpftime_amd import isa, vm as dev  # noqa: E402
import _uprobe_threads as ut  # noqa: E402

N, THREADS, N_ORDERED = 1 << 20, 4096, 1 << 14
FUNC = 0x401000


def timed(d, n, flags, reps, warm):
    L = dev.lib()
    gm, km, rows = C.c_float(), C.c_float(), C.c_uint64()
    group, kern = [], []
    for it in range(warm + reps):
        rc = dev.uprobe_dispatch(d["func"], n, enter=d["enter"], leave=d["leave"], pid_tgid=d["pid"],
                                 clock=d["clock"], flags=flags | dev.BATCH_TIMED)
        assert rc == 0
        L.bpftime_amd_uprobe_last_ms(C.byref(gm), C.byref(km), C.byref(rows))
        assert rows.value == n
        if it >= warm:
            group.append(gm.value)
            kern.append(km.value)
    return group, kern


def main():
    rng = np.random.default_rng(11)
    owner = rng.integers(0, THREADS, N)
    host = {"func": np.full(N, FUNC, dtype=np.uint64),
            "enter": rng.integers(0, 1 << 62, (N, 21), dtype=np.uint64),
            "leave": rng.integers(0, 1 << 62, (N, 21), dtype=np.uint64),
            "pid": ((np.uint64(1) << np.uint64(32)) | (owner + 100).astype(np.uint64)),
            "clock": np.cumsum(rng.integers(1, 1 << 12, 2 * N).astype(np.uint64)).reshape(N, 2)}
    d = {k: dev.DeviceBuffer.from_array(np.ascontiguousarray(v).view(np.uint8).reshape(-1)) for k, v in host.items()}
    ms = dev.Map(isa.BPF_MAP_TYPE_HASH, 4, 8, 2 * THREADS)
    mh = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 4 * ut.SLOTS, 1)
    starts, hist = {}, [0] * ut.SLOTS
    dev.uprobe_attach(dev.prog_create(ut.funclat_entry(ms.fd, starts)[0], "entry", 2), FUNC, dev.UPROBE)
    dev.uprobe_attach(dev.prog_create(ut.funclat_return(ms.fd, mh.fd, starts, hist)[0], "return", 2), FUNC,
                      dev.URETPROBE)
    group, kern = timed(d, N, dev.DISPATCH_THREADS, 7, 3)
    total = int(np.frombuffer(mh.lookup(b"\0\0\0\0"), dtype=np.uint32).sum())
    assert total == 10 * N, total                       # every call of every dispatch was filed
    og, ok = timed(d, N_ORDERED, dev.DISPATCH_THREADS | dev.BATCH_ORDERED, 5, 1)
    g, k = statistics.median(group), statistics.median(kern)
    o = statistics.median(ok)
    out = {"case": "uprobe_threads", "records": N, "threads": THREADS, "attachments": 2, "callbacks": 2 * N,
           "kernel_ms_median": round(k, 4), "kernel_ms_min": round(min(kern), 4), "kernel_ms_max": round(max(kern), 4),
           "kernel_Mrec_per_s": round(N / k / 1e3, 1),
           "grouping_ms_median": round(g, 4), "grouping_share": round(g / (g + k), 3),
           "dispatch_Mrec_per_s": round(N / (g + k) / 1e3, 1),
           "ordered_records": N_ORDERED, "ordered_kernel_ms_median": round(o, 4),
           "ordered_Mrec_per_s": round(N_ORDERED / o / 1e3, 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("# tools/uprobe_threads_measure.py on one MI355X: the funclatency pair on one function, 2^20 "
                    "recorded calls evenly over 4096 recorded threads, BPFTIME_AMD_DISPATCH_THREADS; stream events, "
                    "median of 7 dispatches after 3 warm-ups.\n"
                    "# kernel_*: the k_up_seq launch (with its 4-byte counter memset); grouping_*: "
                    "bpftime_amd_group_threads (its launches and one host wait); dispatch_Mrec_per_s: records over "
                    "both; ordered_*: the same dispatch | EBPF_BATCH_ORDERED (one lane) over the first 2^14 calls.\n"
                    "# Yardstick: the syscall thread-ordered dispatch at 4096 threads, README: about 185 Mrec/s.  "
                    "No target is set.\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
