#!/usr/bin/env python3
"""One number for DESIGN.md §6 (copy and compare helpers): what a helper
call costs against inline loads.  A parallel batch of 2^22 64-byte packets,
(A) bpf_probe_read_kernel of 32 packet bytes (offset 8) to the stack, then a
4-byte compare of the copy, (B) four 8-byte loads of the same 32 bytes stored
to the stack, then the same compare.  Median kernel time of 10
EBPF_BATCH_TIMED batches after 3 warm-ups.  Prints one JSON line per case."""
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, ".")
from bpftime_amd import isa, vm as dev  # noqa: E402
from bpftime_amd.isa import Asm  # noqa: E402

N = 1 << 22


def prog(helper):
    a = Asm().ldx(8, 6, 1, 0)                           # r6 = data
    if helper:
        a.mov64(1, "r10").add64(1, -32).mov64(2, 32).mov64(3, "r6").add64(3, 8)
        a.call(isa.BPF_FUNC_probe_read_kernel)
    else:
        for i in range(4):
            a.ldx(8, 2, 6, 8 + 8 * i).stx(8, 10, -32 + 8 * i, "r2")
    a.ldx(4, 2, 10, -20).mov64(0, isa.XDP_PASS).jmp("jne", 2, 0x01020304, "out").mov64(0, isa.XDP_DROP)
    return a.label("out").exit().assemble()


def main():
    pk = np.random.default_rng(3).integers(0, 256, (N, 64), dtype=np.uint8)
    pk[::3, 20:24] = [4, 3, 2, 1]
    d = dev.DeviceBuffer.from_array(pk)
    dv = dev.DeviceBuffer(4 * N)
    want = np.where((pk[:, 20:24] == [4, 3, 2, 1]).all(axis=1), isa.XDP_DROP, isa.XDP_PASS)
    for name, helper in (("probe_read_kernel_32B", True), ("inline_8B_loads", False)):
        v = dev.VM()
        v.load(prog(helper))
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


if __name__ == "__main__":
    main()
