#!/usr/bin/env python3
"""One number for DESIGN.md §6 (queues and stacks): a parallel batch of 2^22
64-byte packets in which every packet hands an 8-byte record to the host,
(A) with bpf_map_push_elem onto a QUEUE of 2^22 entries, (B) with
bpf_ringbuf_output into a ring that holds them all.  Median kernel time of 10
EBPF_BATCH_TIMED batches after 3 warm-ups; the map is emptied between
batches.  Prints one JSON line per case."""
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from bpftime_amd import isa, vm as dev  # noqa: E402
from bpftime_amd.isa import Asm  # noqa: E402

N = 1 << 22


def record_prog(fd, ring):
    """The record {u32 saddr, u32 packet length} built on the stack."""
    a = Asm().ldx(8, 6, 1, 0).ldx(8, 3, 1, 8).alu64("sub", 3, "r6")
    a.ldx(4, 4, 6, 26).stx(4, 10, -8, "r4").stx(4, 10, -4, "r3")
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -8)
    if ring:
        a.mov64(3, 8).mov64(4, 0).call(isa.BPF_FUNC_ringbuf_output)
    else:
        a.mov64(3, 0).call(isa.BPF_FUNC_map_push_elem)
    return a.exit().assemble()


def main():
    rng = np.random.default_rng(3)
    pk = rng.integers(0, 256, (N, 64), dtype=np.uint8)
    d = dev.DeviceBuffer.from_array(pk)
    dv = dev.DeviceBuffer(4 * N)
    for name, ring in (("queue_push", False), ("ringbuf_output", True)):
        if ring:
            m = dev.Map(isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 1 << 27)
        else:
            m = dev.Map(isa.BPF_MAP_TYPE_QUEUE, 0, 8, N)
        empty = m.snapshot()[:256].copy()
        v = dev.VM()
        v.load(record_prog(m.fd, ring))
        ms = []
        for it in range(13):
            m.restore(empty)  # both positions back to 0
            rc = v.exec_batch(dev.CTX_XDP, d, N, 64, fixed_len=64, verdicts=dv,
                              flags=dev.BATCH_SYNC | dev.BATCH_TIMED)
            assert rc == 0
            if it >= 3:
                ms.append(v.last_batch_ms())
        ok = int((dv.download(np.uint32) == 0).sum())
        print(json.dumps({"case": name, "packets": N, "ok": ok, "ms_median": round(statistics.median(ms), 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}), flush=True)


if __name__ == "__main__":
    main()
