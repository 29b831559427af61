#!/usr/bin/env python3
"""Numbers for DESIGN.md §6 (uprobe replay): 2^22 recorded calls spread evenly
(seeded) over 4 functions, a trivial uprobe (r0 = PT_REGS_PARM1) at each, with
recorded callers and clocks.  Per dispatch: the count + scan launches and the
gather launches (stream events, EBPF_BATCH_TIMED, summed over the 4
attachments), the gather's achieved GB/s against the bytes it must move, and
the dispatch's host time from call to return with EBPF_BATCH_SYNC (4 host
waits for the match counts and the interpreter batches included).  Median of
10 dispatches after 3 warm-ups.  Prints one JSON line; with a path argument
also writes the measurement file."""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from bpftime_amd import programs, vm as dev  # noqa: E402
from bpftime_amd.isa import Asm  # noqa: E402

N = 1 << 22
FUNCS = (0x401000, 0x402200, 0x403300, 0x7F0000004400)
# What the memory system can do on a streaming copy: the project's own
# calibration kernel reading 64 B of every 64-B unit (profiles/r03_calib.json,
# c_rd64of64: 6191 GB/s); the HBM3E data sheet says 8000 GB/s
CEILING_GBPS, SPEC_GBPS = 6191.1, 8000.0


def gather_bytes(n, rows):
    """Bytes the gather launches must move for `rows` matches in all, over 4
    attachments: each reads the n function addresses (8 B) and its chunk
    offsets (4 B per 64 records); per row it reads 168 B of registers, the
    8-B caller and an 8-B clock, and writes 192 B."""
    return 4 * (8 * n + 4 * ((n + 63) // 64)) + rows * (168 + 8 + 8 + 192)


def count_bytes(n):
    """... and the count + scan launches: the function addresses again, the
    chunk counts written, read and written once more by the scan."""
    return 4 * (8 * n + 3 * 4 * ((n + 63) // 64))


def main():
    rng = np.random.default_rng(7)
    func = np.array(FUNCS, dtype=np.uint64)[rng.integers(0, 4, N)]
    enter = rng.integers(0, 1 << 62, (N, 21), dtype=np.uint64)
    pid = rng.integers(1, 1 << 40, N, dtype=np.uint64)
    clock = np.arange(2 * N, dtype=np.uint64)
    up = lambda a: dev.DeviceBuffer.from_array(a.view(np.uint8).reshape(-1))  # noqa: E731
    d_func, d_enter, d_pid, d_clock = up(func), up(enter), up(pid), up(clock)
    code = Asm().ldx(8, 0, 1, programs.PT_REGS_PARM1_OFF).exit().assemble()
    for k, f in enumerate(FUNCS):
        dev.uprobe_attach(dev.prog_create(code, f"probe{k}", 2), f, dev.UPROBE)
    L = dev.lib()
    cm, gm, rows = C.c_float(), C.c_float(), C.c_uint64()
    count_ms, gather_ms, total_ms = [], [], []
    for it in range(13):
        t0 = time.perf_counter()
        rc = dev.uprobe_dispatch(d_func, N, enter=d_enter, pid_tgid=d_pid, clock=d_clock,
                                 flags=dev.BATCH_SYNC | dev.BATCH_TIMED)
        t1 = time.perf_counter()
        assert rc == 0
        L.bpftime_amd_uprobe_last_ms(C.byref(cm), C.byref(gm), C.byref(rows))
        assert rows.value == N
        if it >= 3:
            count_ms.append(cm.value)
            gather_ms.append(gm.value)
            total_ms.append(1e3 * (t1 - t0))
    g, c = statistics.median(gather_ms), statistics.median(count_ms)
    gb, cb = gather_bytes(N, N), count_bytes(N)
    out = {"case": "uprobe_dispatch", "records": N, "functions": 4, "attachments": 4,
           "gather_ms_median": round(g, 4), "gather_ms_min": round(min(gather_ms), 4),
           "gather_ms_max": round(max(gather_ms), 4), "gather_bytes": gb,
           "gather_GBps": round(gb / g / 1e6, 1), "gather_share_of_ceiling": round(gb / g / 1e6 / CEILING_GBPS, 3),
           "count_scan_ms_median": round(c, 4), "count_scan_bytes": cb, "count_scan_GBps": round(cb / c / 1e6, 1),
           "dispatch_total_ms_median": round(statistics.median(total_ms), 4),
           "dispatch_total_ms_min": round(min(total_ms), 4), "dispatch_total_ms_max": round(max(total_ms), 4),
           "ceiling_GBps": CEILING_GBPS, "spec_GBps": SPEC_GBPS}
    line = json.dumps(out)
    print(line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("# tools/experiments/uprobe_dispatch_cost.py on one MI355X: 2^22 recorded calls over 4 functions, a "
                    "trivial uprobe at each, recorded callers and clocks; median of 10 dispatches after 3 warm-ups.\n"
                    "# gather_*: the 4 k_ug_gather launches (stream events), bytes = what they must move "
                    "(gather_bytes in the script); count_scan_*: the 4 k_ug_count + k_ug_scan pairs; "
                    "dispatch_total_*: host time of the EBPF_BATCH_SYNC call.\n"
                    "# ceiling_GBps: the project's streaming-read calibration, profiles/r03_calib.json c_rd64of64 "
                    "(6191 GB/s); spec_GBps: the HBM3E data sheet.  No target is set.\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
