#!/usr/bin/env python3
"""One number for DESIGN.md §6 (trace and task helpers): what a
bpf_trace_printk record costs against the same 4 bytes through the ring
buffer.  A parallel batch of 2^22 64-byte packets, (A) one
bpf_trace_printk("%d\\n", word) per packet into a log large enough to hold
them all (BPFTIME_AMD_TRACE_RECORDS, set here before the library loads), (B)
bpf_ringbuf_output of the same word.  Median kernel time of 10
EBPF_BATCH_TIMED batches after 3 warm-ups, the log / ring drained between
batches.  Prints one JSON line per case."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

N = 1 << 22
os.environ["BPFTIME_AMD_TRACE_RECORDS"] = str(N)
sys.path.insert(0, ".")
from bpftime_amd import isa, vm as dev  # noqa: E402
from bpftime_amd._lib import TraceLine  # noqa: E402
from bpftime_amd.isa import Asm  # noqa: E402


def prog(ring_fd):
    a = Asm().ldx(8, 6, 1, 0).ldx(4, 7, 6, 20)            # r6 = data, r7 = a packet word
    if ring_fd is None:
        a.lddw(2, int.from_bytes(b"%d\n\0\0\0\0\0", "little")).stx(8, 10, -8, "r2")
        a.mov64(1, "r10").add64(1, -8).mov64(2, 4).mov64(3, "r7").call(isa.BPF_FUNC_trace_printk)
    else:
        a.stx(4, 10, -8, "r7")
        a.ld_map_fd(1, ring_fd).mov64(2, "r10").add64(2, -8).mov64(3, 4).mov64(4, 0)
        a.call(isa.BPF_FUNC_ringbuf_output)
    return a.mov64(0, isa.XDP_PASS).exit().assemble()


def main():
    dev.enable_trace_printk()
    pk = np.random.default_rng(3).integers(0, 256, (N, 64), dtype=np.uint8)
    d = dev.DeviceBuffer.from_array(pk)
    dv = dev.DeviceBuffer(4 * N)
    lines = (TraceLine * N)()
    text = C.create_string_buffer(16 * N)
    ring = dev.Map(isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 1 << 27)   # 16 B a record: 2^26 B for them all
    for name, fd in (("trace_printk_%d", None), ("ringbuf_output_4B", ring.fd)):
        v = dev.VM()
        v.load(prog(fd))
        ms = []
        for it in range(13):
            rc = v.exec_batch(dev.CTX_XDP, d, N, 64, fixed_len=64, verdicts=dv, flags=dev.BATCH_SYNC | dev.BATCH_TIMED)
            assert rc == 0
            if it >= 3:
                ms.append(v.last_batch_ms())
            if fd is None:
                # drain the log (formatted by the host, outside the timed kernel)
                lost = C.c_uint64(0)
                got = dev.lib().bpftime_amd_trace_read(lines, N, text, len(text), C.byref(lost))
                assert got == N and lost.value == 0, (got, lost.value)
                if it == 12:
                    first = {lines[k].unit: text.raw[lines[k].text_off:lines[k].text_off + lines[k].text_len]
                             for k in range(N) if lines[k].unit < 64}
                    words = pk[:64, 20:24].copy().view(np.int32).reshape(-1)
                    assert first == {u: b"%d\n" % int(words[u]) for u in range(64)}
            else:
                assert len(ring.ringbuf_fetch(cap=1 << 27)) == N
        print(json.dumps({"case": name, "packets": N, "big_stack": v.info()["big_stack"],
                          "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                          "ms_max": round(max(ms), 4)}), flush=True)


if __name__ == "__main__":
    main()
