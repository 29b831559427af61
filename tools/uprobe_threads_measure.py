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
measurement file.

--tiers asm,cpp takes the dispatches of the two execution tiers alternately in
the one process (BPFTIME_AMD_SEQ_ASM is read per dispatch) and prints a line
per tier; --threads 64,1024,... repeats the measurement per thread count (the
same 2^20 calls, spread over that many threads).  The default is one line at
4096 threads in the tier the library chooses."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from bpftime_amd import isa, vm as dev  # noqa: E402
import _uprobe_threads as ut  # noqa: E402

N, THREADS, N_ORDERED = 1 << 20, 4096, 1 << 14
FUNC = 0x401000


TIER_ENV = {"auto": None, "asm": "1", "cpp": "0"}


def set_tier(tier):
    if TIER_ENV[tier] is None:
        os.environ.pop("BPFTIME_AMD_SEQ_ASM", None)
    else:
        os.environ["BPFTIME_AMD_SEQ_ASM"] = TIER_ENV[tier]


def timed(d, n, flags, reps, warm, tiers=("auto",)):
    """{tier: (grouping ms, kernel ms, the tier that ran)}, the tiers' dispatches taken alternately."""
    L = dev.lib()
    gm, km, rows = C.c_float(), C.c_float(), C.c_uint64()
    out = {t: ([], [], set()) for t in tiers}
    for it in range(warm + reps):
        for t in tiers:
            set_tier(t)
            rc = dev.uprobe_dispatch(d["func"], n, enter=d["enter"], leave=d["leave"], pid_tgid=d["pid"],
                                     clock=d["clock"], flags=flags | dev.BATCH_TIMED)
            assert rc == 0
            out[t][2].add(dev.last_seq_tier())
            L.bpftime_amd_uprobe_last_ms(C.byref(gm), C.byref(km), C.byref(rows))
            assert rows.value == n
            if it >= warm:
                out[t][0].append(gm.value)
                out[t][1].append(km.value)
    set_tier("auto")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?")
    ap.add_argument("--tiers", default="auto")
    ap.add_argument("--threads", default=str(THREADS))
    args = ap.parse_args()
    tiers = args.tiers.split(",")
    counts = [int(x) for x in args.threads.split(",")]
    rng = np.random.default_rng(11)
    host = {"func": np.full(N, FUNC, dtype=np.uint64),
            "enter": rng.integers(0, 1 << 62, (N, 21), dtype=np.uint64),
            "leave": rng.integers(0, 1 << 62, (N, 21), dtype=np.uint64),
            "clock": np.cumsum(rng.integers(1, 1 << 12, 2 * N).astype(np.uint64)).reshape(N, 2)}
    up = lambda v: dev.DeviceBuffer.from_array(np.ascontiguousarray(v).view(np.uint8).reshape(-1))  # noqa: E731
    d = {k: up(v) for k, v in host.items()}
    ms = dev.Map(isa.BPF_MAP_TYPE_HASH, 4, 8, 2 * max(counts))
    mh = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 4 * ut.SLOTS, 1)
    starts, hist = {}, [0] * ut.SLOTS
    dev.uprobe_attach(dev.prog_create(ut.funclat_entry(ms.fd, starts)[0], "entry", 2), FUNC, dev.UPROBE)
    dev.uprobe_attach(dev.prog_create(ut.funclat_return(ms.fd, mh.fd, starts, hist)[0], "return", 2), FUNC,
                      dev.URETPROBE)
    lines = []
    for threads in counts:
        owner = np.random.default_rng(11 + threads).integers(0, threads, N)
        d["pid"] = up((np.uint64(1) << np.uint64(32)) | (owner + 100).astype(np.uint64))
        res = timed(d, N, dev.DISPATCH_THREADS, 7, 3, tiers)
        # (the one-lane run does not depend on the thread count: once)
        first = threads == counts[0]
        ores = timed(d, N_ORDERED, dev.DISPATCH_THREADS | dev.BATCH_ORDERED, 5, 1, tiers) if first else None
        for t in tiers:
            group, kern, ran = res[t]
            g, k = statistics.median(group), statistics.median(kern)
            row = {}
            if first:
                o = statistics.median(ores[t][1])
                row = {"ordered_records": N_ORDERED, "ordered_tier_ran": sorted(ores[t][2]),
                       "ordered_kernel_ms_median": round(o, 4), "ordered_Mrec_per_s": round(N_ORDERED / o / 1e3, 3)}
            lines.append(json.dumps({
                "case": "uprobe_threads", "tier": t, "tier_ran": sorted(ran), "records": N, "threads": threads,
                "attachments": 2, "callbacks": 2 * N,
                "kernel_ms_median": round(k, 4), "kernel_ms_min": round(min(kern), 4),
                "kernel_ms_max": round(max(kern), 4), "kernel_Mrec_per_s": round(N / k / 1e3, 1),
                "grouping_ms_median": round(g, 4), "grouping_share": round(g / (g + k), 3),
                "dispatch_Mrec_per_s": round(N / (g + k) / 1e3, 1), **row}))
            print(lines[-1], flush=True)
    total = int(np.frombuffer(mh.lookup(b"\0\0\0\0"), dtype=np.uint32).sum())
    assert total == len(tiers) * (len(counts) * 10 * N + 6 * N_ORDERED), total   # every call of every dispatch was filed
    if args.path:
        with open(args.path, "w") as f:
            f.write("# tools/uprobe_threads_measure.py on one MI355X: the funclatency pair on one function, 2^20 "
                    "recorded calls evenly over the recorded threads, BPFTIME_AMD_DISPATCH_THREADS; stream events, "
                    "median of 7 dispatches after 3 warm-ups; the tiers' dispatches alternate in one process "
                    "(tier: asked; tier_ran: bpftime_amd_last_seq_tier).\n"
                    "# kernel_*: the k_up_seq launch (with its 4-byte counter memset); grouping_*: "
                    "bpftime_amd_group_threads (its launches and one host wait); dispatch_Mrec_per_s: records over "
                    "both; ordered_*: the same dispatch | EBPF_BATCH_ORDERED (one lane) over the first 2^14 calls.\n"
                    "# Yardstick: the syscall thread-ordered dispatch at 4096 threads, README: about 185 Mrec/s.  "
                    "No target is set.\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
