#!/usr/bin/env python3
"""Numbers for DESIGN.md §6 (uprobe replay, nested calls): the funclatency pair
(tests/_uprobe_threads.py) on one function, 2^20 recorded calls spread evenly
(seeded) over 4096 recorded threads, with recorded callers and clocks -- the
shape of tools/uprobe_threads_measure.py.  Three dispatches, taken alternately
in one process, by stream events (EBPF_BATCH_TIMED), the median of 7 after 3
warm-ups each:
  1. bpftime_amd_uprobe_dispatch with BPFTIME_AMD_DISPATCH_THREADS (the baseline);
  2. bpftime_amd_uprobe_dispatch_events on the flat list over the same records;
  3. the same on a nested trace of the same event count: per thread the calls
     form chains one to four deep (E E E R R R), so the function recurses.
Prints one JSON line per dispatch; with a path argument also writes the
measurement file.  --tiers asm,cpp takes every dispatch once per execution tier
(BPFTIME_AMD_SEQ_ASM, read per dispatch), all of them alternately, and prints a
line per dispatch and tier; the default is the tier the library chooses."""
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

N, THREADS, REPS, WARM = 1 << 20, 4096, 7, 3
FUNC = 0x401000


def nested_events(owner, rng):
    """Per thread, its records in chains of 1..4 nested calls; the chains of all
    threads in random order."""
    order = np.argsort(owner, kind="stable")
    sizes = rng.integers(1, 5, len(order))
    ends = np.cumsum(sizes)
    ends = ends[ends < len(order)]
    # a chain never crosses from one thread's records into the next one's
    cuts = np.union1d(ends, np.flatnonzero(np.diff(owner[order])) + 1)
    chains = np.split(order, cuts)
    out = []
    for k in rng.permutation(len(chains)):
        c = chains[k]
        out.extend(int(i) << 1 for i in c)
        out.extend((int(i) << 1) | 1 for i in c[::-1])
    depth = max(len(c) for c in chains)
    return np.array(out, dtype=np.uint32), depth


def clocks_along(events, n, rng):
    clock = np.zeros((n, 2), dtype=np.uint64)
    t = np.cumsum(rng.integers(1, 1 << 12, len(events)).astype(np.uint64))
    clock[events >> 1, events & 1] = t
    return clock


def up(a):
    return dev.DeviceBuffer.from_array(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


TIER_ENV = {"auto": None, "asm": "1", "cpp": "0"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?")
    ap.add_argument("--tiers", default="auto")
    args = ap.parse_args()
    tiers = args.tiers.split(",")
    rng = np.random.default_rng(11)
    owner = rng.integers(0, THREADS, N)
    host = {"func": np.full(N, FUNC, dtype=np.uint64),
            "enter": rng.integers(0, 1 << 62, (N, 21), dtype=np.uint64),
            "leave": rng.integers(0, 1 << 62, (N, 21), dtype=np.uint64),
            "pid": ((np.uint64(1) << np.uint64(32)) | (owner + 100).astype(np.uint64)),
            "clock": np.cumsum(rng.integers(1, 1 << 12, 2 * N).astype(np.uint64)).reshape(N, 2)}
    d = {k: up(v) for k, v in host.items()}
    flat = np.arange(2 * N, dtype=np.uint32)
    nested, depth = nested_events(owner, rng)
    assert len(nested) == len(flat) and depth <= 4
    d_flat, d_nested, d_nclock = up(flat), up(nested), up(clocks_along(nested, N, rng))
    ms = dev.Map(isa.BPF_MAP_TYPE_HASH, 4, 8, 2 * THREADS)
    mh = dev.Map(isa.BPF_MAP_TYPE_ARRAY, 4, 4 * ut.SLOTS, 1)
    starts, hist = {}, [0] * ut.SLOTS
    dev.uprobe_attach(dev.prog_create(ut.funclat_entry(ms.fd, starts)[0], "entry", 2), FUNC, dev.UPROBE)
    dev.uprobe_attach(dev.prog_create(ut.funclat_return(ms.fd, mh.fd, starts, hist)[0], "return", 2), FUNC,
                      dev.URETPROBE)
    flags = dev.BATCH_SYNC | dev.DISPATCH_THREADS | dev.BATCH_TIMED
    kw = dict(enter=d["enter"], leave=d["leave"], pid_tgid=d["pid"], flags=flags)
    cases = [("calls", lambda: dev.uprobe_dispatch(d["func"], N, clock=d["clock"], **kw), N),
             ("events_flat", lambda: dev.uprobe_dispatch_events(d["func"], N, d_flat, 2 * N, clock=d["clock"], **kw),
              2 * N),
             ("events_nested", lambda: dev.uprobe_dispatch_events(d["func"], N, d_nested, 2 * N, clock=d_nclock, **kw),
              2 * N)]
    L = dev.lib()
    gm, km, rows = C.c_float(), C.c_float(), C.c_uint64()
    keys = [(c[0], t) for c in cases for t in tiers]
    group, kern, ran = {k: [] for k in keys}, {k: [] for k in keys}, {k: set() for k in keys}
    for it in range(WARM + REPS):
        for name, run, want_rows in cases:               # alternately: a drift hits them all alike
            for t in tiers:
                if TIER_ENV[t] is None:
                    os.environ.pop("BPFTIME_AMD_SEQ_ASM", None)
                else:
                    os.environ["BPFTIME_AMD_SEQ_ASM"] = TIER_ENV[t]
                assert run() == 0
                ran[name, t].add(dev.last_seq_tier())
                L.bpftime_amd_uprobe_last_ms(C.byref(gm), C.byref(km), C.byref(rows))
                assert rows.value == want_rows
                if it >= WARM:
                    group[name, t].append(gm.value)
                    kern[name, t].append(km.value)
    total = int(np.frombuffer(mh.lookup(b"\0\0\0\0"), dtype=np.uint32).sum())
    assert total == 3 * len(tiers) * (WARM + REPS) * N, total   # every call of every dispatch was filed
    lines = []
    for name, t in keys:
        g, k = statistics.median(group[name, t]), statistics.median(kern[name, t])
        lines.append(json.dumps({
            "case": name, "tier": t, "tier_ran": sorted(ran[name, t]), "records": N, "events": 2 * N,
            "threads": THREADS, "callbacks": 2 * N,
            "nesting_depth": depth if name == "events_nested" else 1,
            "kernel_ms_median": round(k, 4), "kernel_ms_min": round(min(kern[name, t]), 4),
            "kernel_ms_max": round(max(kern[name, t]), 4), "grouping_ms_median": round(g, 4),
            "grouping_ms_min": round(min(group[name, t]), 4), "grouping_ms_max": round(max(group[name, t]), 4),
            "dispatch_Mcallbacks_per_s": round(2 * N / (g + k) / 1e3, 1)}))
    for line in lines:
        print(line, flush=True)
    if args.path:
        with open(args.path, "w") as f:
            f.write("# tools/uprobe_events_measure.py on one MI355X: the funclatency pair on one function, 2^20 "
                    "recorded calls evenly over 4096 recorded threads; stream events, median of 7 dispatches after 3 "
                    "warm-ups, the three dispatches (per asked tier; tier_ran: bpftime_amd_last_seq_tier) taken alternately "
                    "in one process.\n"
                    "# calls: bpftime_amd_uprobe_dispatch | BPFTIME_AMD_DISPATCH_THREADS (the baseline); events_flat: "
                    "bpftime_amd_uprobe_dispatch_events on E(0,0), E(0,1), E(1,0), ... over the same records; "
                    "events_nested: the same event count, per thread chains of 1..4 nested calls of the function.\n"
                    "# kernel_*: the k_up_seq launch (with its 4-byte counter memset); grouping_*: the thread grouping "
                    "with its one host wait -- for the event dispatches the key pass before it and the event-word "
                    "pass after it included, over 2^21 events instead of 2^20 records.\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
