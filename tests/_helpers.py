"""Shared helpers for the parity tests: build the same maps on the oracle
(CPU checker) and on the device, run a program on both, compare."""
import struct

import numpy as np

from bpftime_amd import gen, isa
from bpftime_amd.isa import Asm


def make_maps(specs, po=None, dev=None):
    """specs: list of (type, ksize, vsize, max). Creates them at identical fds
    on the oracle and the device registry so the same bytecode loads on both."""
    om, dm = [], []
    for t, k, v, mx in specs:
        d = dev.Map(t, k, v, mx) if dev is not None else None
        fd = d.fd if d is not None else -1
        o = po.OracleMap(t, k, v, mx, fd=fd) if po is not None else None
        om.append(o)
        dm.append(d)
    return om, dm


def xdp_counter_maps(po, dev, ctl_flag=0):
    (octl, obss), (dctl, dbss) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 4, 2),
                                            (isa.BPF_MAP_TYPE_ARRAY, 4, 4096, 1)], po, dev)
    if ctl_flag:
        for m in (octl, dctl):
            if m is not None:
                m.update(struct.pack("<I", 0), struct.pack("<I", ctl_flag))
    return (octl, obss), (dctl, dbss)


def u64s(b):
    return np.frombuffer(b, dtype=np.uint64)


def update_existing_prog(fd):
    """-> (code, pc of the update call).  bpf_map_update_elem of a HASH map
    (u32 key, 16-byte value) with key and value on the stack: the unit's word
    0 is the key, its bytes 8..23 the value; then a lookup of the key; r0 =
    the value's second word + the update's return, 99 on a miss."""
    a = Asm()
    a.ldx(4, 2, 1, 0).stx(4, 10, -4, "r2")                 # key = unit word 0
    a.ldx(8, 3, 1, 8).stx(8, 10, -24, "r3")                # value = unit bytes 8..23
    a.ldx(8, 3, 1, 16).stx(8, 10, -16, "r3")
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -24).mov64(4, 0)
    at = a.pc
    a.call(isa.BPF_FUNC_map_update_elem)
    a.mov64(6, "r0")
    a.ld_map_fd(1, fd).mov64(2, "r10").add64(2, -4).call(isa.BPF_FUNC_map_lookup_elem)
    a.jmp("jeq", 0, 0, "miss")
    a.ldx(8, 0, 0, 8).alu64("add", 0, "r6").exit()
    a.label("miss").mov64(0, 99).exit()
    return a.assemble(), at


def update_existing_units(n):
    """32-byte units for update_existing_prog: key = the unit's index."""
    units = np.zeros((n, 32), dtype=np.uint8)
    units.view(np.uint32)[:, 0] = np.arange(n, dtype=np.uint32)
    units.view(np.uint64)[:, 1] = gen.sm64(11, np.arange(n, dtype=np.uint64))
    units.view(np.uint64)[:, 2] = gen.sm64(12, np.arange(n, dtype=np.uint64))
    return units
