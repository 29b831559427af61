"""AF_XDP descriptor batches (ebpf_batch::descs) at small edge shapes: the
case table, the umem builder, the oracle reference and the per-wave staging
model shared by test_umem_model.py (no GPU) and test_gpu_umem_matrix.py.

A case places n frames in a umem of (n + 5) chunks.  Chunk 0 always holds a
frame (a failed descriptor runs as addr = len = 0, so a kernel that let such a
lane write would hit it); the top chunk holds no frame unless the case's edge
puts one there.  The device buffer is the umem followed by a guard of
GUARD_BYTES the batch is not told about: every address a case names that a
kernel could dereference lies inside umem + guard, and descriptors "outside"
are outside by their addr / len fields only, which the kernel compares and
never dereferences.

In contract: frames do not overlap, no descriptor appears twice,
addr % chunk + len <= chunk, aligned-chunk addresses.
"""
import struct
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

from bpftime_amd import gen, isa, programs
from bpftime_amd.isa import Asm

from _helpers import make_maps, xdp_counter_maps

CHUNK = 2048
GUARD_BYTES = 4096
SIZES = (1, 63, 64, 65, 130, 257)
IFINDEX, RXQ = 3, 5
PAD0 = 16            # stride == 0: bytes behind the frame the reference carries along (adjust_head(-1))
RAW, XDP = 0, 1      # EBPF_CTX_RAW / EBPF_CTX_XDP
M64 = (1 << 64) - 1

# the staged window (bytes) of the programs whose launches the model follows:
# their static packet accesses end at 12, 38 and 64 B, rounded up to 16
STAGE = {"xdp_counter": 16, "flow_hash": 48, "staged_mix": 64}

LENGTH_MIX = (14, 34, 42, 60, 63, 64, 65, 1500, "rest")
FAILING_EDGES = ("top_plus1", "end_len0", "wrap")
LEGAL_EDGES = ("top", "top6", "last_byte", "len0", "top32")


@dataclass(frozen=True)
class Case:
    name: str
    prog: str
    n: int
    chunk: int = CHUNK          # the batch's stride; 0: buffer_end = frame end
    head: object = 256          # head room in the chunk, or "tail": chunk - len
    lens: object = 64           # int, a tuple cycled over the units ("rest": chunk - head), or "flow"
    odd: tuple = ()             # units moved off 16-B alignment
    all_odd: bool = False
    options: int = 0
    edge: str = ""              # descriptor edge (FAILING_EDGES / LEGAL_EDGES) ...
    edge_units: tuple = ()      # ... at these units
    nfail: int = 0              # descriptors that fail their unit
    unstaged: object = None     # waves that must fall back from staging: tuple, "all", or None (derived only)
    seed: int = 1
    first_unit: int = 0
    ncpu: int = 0
    ordered: bool = False
    meta: bool = False          # data_off_out / len_out


def _lens(case, place):
    n = case.n
    if case.lens == "flow":
        return gen.flow_packets(n, nflows=97, stride=place)[1].astype(np.int64)
    pat = case.lens if isinstance(case.lens, tuple) else (case.lens,)
    head = 0 if case.head == "tail" else int(case.head)
    return np.array([place - head if pat[i % len(pat)] == "rest" else pat[i % len(pat)] for i in range(n)], np.int64)


def _payload(case, place, lens):
    if case.prog == "flow_hash":
        return gen.flow_packets(case.n, nflows=97, stride=place)[0]
    return gen.xdp_packets(case.n, stride=(max(int(lens.max()), 64) + 7) & ~7, seed=0x5EED + case.seed)


def build(case):
    """-> (umem, descs, guard): the umem bytes, (n, 2) u64 descriptor words
    {addr, len | options << 32} in ring order, and the guard pattern that
    follows the umem in the device buffer."""
    n, place = case.n, case.chunk or CHUNK
    rng = np.random.default_rng(case.seed)
    nchunks = n + 5
    ub = nchunks * place
    umem = gen.sm64(0xBACC + case.seed, np.arange(ub // 8, dtype=np.uint64)).view(np.uint8).copy()
    chunks = 1 + rng.permutation(nchunks - 2)[:n].astype(np.int64)   # ring order is no address order
    chunks[n // 2] = 0
    assert n // 2 not in case.edge_units or n == 1, case.name
    lens = _lens(case, place)
    payload = _payload(case, place, lens)
    heads = place - lens if case.head == "tail" else np.full(n, int(case.head), np.int64)
    odd = np.zeros(n, bool)
    odd[list(case.odd)] = True
    if case.all_odd:
        odd[:] = True
    heads = np.where(odd, np.where(heads + 6 + lens > place, heads - 10, heads + 6), heads)
    assert (heads >= 0).all() and (heads + lens <= place).all(), case.name
    addrs = (chunks * place + heads).astype(np.uint64)
    lens = lens.astype(np.uint64)
    for u in case.edge_units:
        a, ln = {"top": (ub - 64, 64), "top6": (ub - 58, 58), "top32": (ub - 32, 32), "last_byte": (ub - 1, 1),
                 "len0": (int(addrs[u]), 0), "top_plus1": (ub - 63, 64), "end_len0": (ub, 0),
                 "wrap": (M64 - 7, 16)}[case.edge]
        addrs[u], lens[u] = a, ln
    for i in range(n):
        a, ln = int(addrs[i]), int(lens[i])
        if a < ub and ln <= ub - a:
            umem[a:a + ln] = payload[i, :ln]
    descs = np.zeros((n, 2), np.uint64)
    descs[:, 0] = addrs
    descs[:, 1] = lens | (np.uint64(case.options) << np.uint64(32))
    guard = (np.arange(GUARD_BYTES) * 37 % 251 + 1).astype(np.uint8)
    return umem, descs, guard


def frames(descs, ub):
    """Per descriptor (addr, len, ok): ok is begin()'s test, the 32-bit len."""
    out = []
    for a, w in descs.tolist():
        ln = w & 0xFFFFFFFF
        out.append((a, ln, a < ub and ln <= ub - a))
    return out


def owned(descs, ub, chunk, kind):
    """Mask of the umem bytes a legal unit may write: its chunk (XDP), its
    frame (RAW), its frame and PAD0 bytes behind it (stride == 0)."""
    m = np.zeros(ub, bool)
    for a, ln, ok in frames(descs, ub):
        if not ok:
            continue
        if kind == XDP and chunk:
            m[a - a % chunk:a - a % chunk + chunk] = True
        elif kind == XDP:
            m[a:min(a + ln + PAD0, ub)] = True
        else:
            m[a:a + ln] = True
    return m


def unstaged_waves(descs, ub, stage):
    """The waves of 64 units that fall back from a `stage`-byte staged window:
    one lane off 16-B alignment, or with a window that crosses the umem end
    (a failed descriptor runs at address 0: aligned, inside)."""
    fr = frames(descs, ub)
    out = []
    for w in range((len(fr) + 63) // 64):
        bad = False
        for a, _, ok in fr[64 * w:64 * w + 64]:
            a = a if ok else 0
            bad |= a % 16 != 0 or a + stage > ub
        if bad:
            out.append(w)
    return tuple(out)


# ---- programs ---------------------------------------------------------------
def ctx_reader_prog():
    """r0 = ((((data - buffer_start) * 2053 + (buffer_end - buffer_start)) * 2053
    + (data_end - data)) * 7 + ingress_ifindex) * 11 + rx_queue_index: every
    generic ctx field of xdp_md_userspace."""
    a = Asm().mov64(6, "r1")
    a.ldx(8, 1, 6, 0).ldx(8, 2, 6, 8).ldx(8, 3, 6, 32).ldx(8, 4, 6, 40)
    a.mov64(0, "r1").alu64("sub", 0, "r3").alu64("mul", 0, 2053)
    a.alu64("sub", 4, "r3").alu64("add", 0, "r4").alu64("mul", 0, 2053)
    a.alu64("sub", 2, "r1").alu64("add", 0, "r2").alu64("mul", 0, 7)
    a.ldx(4, 5, 6, 20).alu64("add", 0, "r5").alu64("mul", 0, 11)
    a.ldx(4, 5, 6, 24).alu64("add", 0, "r5").exit()
    return a.assemble()


def ctx_fold(data_off, buf_len, length, ifindex=IFINDEX, rxq=RXQ):
    return (((((data_off * 2053 + buf_len) * 2053 + length) * 7 + ifindex) * 11) + rxq) & 0xFFFFFFFF


def raw_sum_prog():
    """r0 = r2 + the frame's first 8 bytes (r1 = frame, r2 = len)."""
    return Asm().ldx(8, 0, 1, 0).alu64("add", 0, "r2").exit().assemble()


def _adjust_prog(helper, arg):
    return Asm().mov64(2, arg).call(helper).exit().assemble()


I32 = lambda v: struct.pack("<i", v)  # noqa: E731
PA_FD = 1001


def _tail_image(po, dev):
    """The prog array, targets and counters of test_gpu_tailcall._xdp_pair
    (there: device and oracle; here the device is optional)."""
    import _tailcall as tc
    pa_o = po.OracleMap(isa.BPF_MAP_TYPE_PROG_ARRAY, 4, 4, 4, fd=PA_FD)
    pa_d = dev.Map(isa.BPF_MAP_TYPE_PROG_ARRAY, 4, 4, 4, fd=PA_FD) if dev else None
    (cnt_o,), (cnt_d,) = make_maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 8, 4)], po, dev)
    cfd = (cnt_d or cnt_o).fd
    for fd, code in {900: tc.target_write(0xA1), 901: tc.target_count(cfd),
                     903: tc.target_recurse(PA_FD, cfd, 3), 904: tc.target_write(0xB2)}.items():
        po.prog_create(fd, code)
        if dev:
            assert dev.prog_create(code, f"t{fd}", 6, fd=fd) == fd
    for k, fd in ((0, 900), (1, 901), (3, 903)):
        assert pa_o.update(I32(k), I32(fd)) == 0 and (not dev or pa_d.update(I32(k), I32(fd)) == 0)
    return tc.xdp_caller(PA_FD, cfd), [(cnt_o, cnt_d)]


def setup(prog, po, dev=None):
    """The maps `prog` names, at the same fds on the oracle and (when given)
    the device, and its bytecode -> code, kind, maps [(oracle, device)],
    load_bytes (the program calls bpf_xdp_load_bytes)."""
    s = SimpleNamespace(kind=XDP, maps=[], load_bytes=False)

    def maps(specs):
        om, dm = make_maps(specs, po, dev)
        s.maps = list(zip(om, dm))
        return [(d or o).fd for o, d in s.maps]

    name, _, arg = prog.partition(":")
    if name == "xdp_counter":
        (octl, obss), (dctl, dbss) = xdp_counter_maps(po, dev)
        s.maps = [(octl, dctl), (obss, dbss)]
        s.code = programs.xdp_counter((dctl or octl).fd, (dbss or obss).fd)
    elif name == "flow_hash":
        s.code = programs.flow_hash(*maps([(isa.BPF_MAP_TYPE_HASH, 16, 16, 4096)]))
    elif name == "staged_mix":
        import test_gpu_parity as tgp
        s.code = tgp._staged_mix()
    elif name == "helper_mix":
        import test_gpu_xdp_helpers as tgh
        s.code, s.load_bytes = tgh.helper_mix_program(), True
    elif name == "ctx_reader":
        s.code = ctx_reader_prog()
    elif name == "tailcall":
        s.code, s.maps = _tail_image(po, dev)
    elif name == "percpu":
        import test_gpu_maps as tgm
        s.code, s.kind = tgm.percpu_counter_prog(*maps([(isa.BPF_MAP_TYPE_PERCPU_ARRAY, 4, 8, 4)])), RAW
    elif name == "sampler":
        import test_gpu_counters as tgc
        s.code = tgc.prog_sampler(*maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 8, 1), (isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 1 << 16)]))
    elif name == "random":
        import test_gpu_parity as tgp
        s.code = tgp._random_xdp_program(np.random.default_rng(int(arg)), *maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 8, 4)]))
    elif name == "raw_sum":
        s.code, s.kind = raw_sum_prog(), RAW
    elif name == "raw_staged":
        import test_gpu_parity as tgp
        s.code, s.kind = tgp.staged_raw_prog(), RAW
    elif name == "last_writer":
        import test_gpu_parity as tgp
        s.code, s.kind = tgp.last_writer_prog(*maps([(isa.BPF_MAP_TYPE_ARRAY, 4, 8, 1)])), RAW
    elif name == "adjust_head":
        s.code = _adjust_prog(isa.BPF_FUNC_xdp_adjust_head, int(arg))
    elif name == "adjust_tail":
        s.code = _adjust_prog(isa.BPF_FUNC_xdp_adjust_tail, int(arg))
    else:
        raise KeyError(prog)
    return s


def map_state(m, device):
    """A map's contents in a form equal on both sides: ring records sorted
    (a parallel batch commits them in any order), hash items as a dict."""
    if m.type == isa.BPF_MAP_TYPE_RINGBUF:
        return sorted(m.ringbuf_fetch())
    if m.type == isa.BPF_MAP_TYPE_HASH:
        return m.hash_items() if device else m.items()
    return [m.lookup(I32(k)) for k in range(m.max_entries)]


# ---- the reference ----------------------------------------------------------
def reference(po, code, umem, descs, chunk, *, kind=XDP, ncpu=0, first_unit=0, ordered=False, load_bytes=False,
              ifindex=IFINDEX, rxq=RXQ):
    """The oracle, one unit at a time in ring order (so `ordered` changes
    nothing here: it is what an ORDERED batch must reproduce, and what a
    parallel batch of a program whose map updates commute must reproduce) ->
    (umem_after, verdicts (XDP, u32) or rets (RAW, u64), off, ln, failed).

    XDP: unit i's whole chunk is the slot, head = addr % chunk; off is data -
    the frame's address, as the device reports it.  chunk == 0: the slot is
    exactly the frame (buffer_end = data_end), with the PAD0 bytes behind it
    carried along, because the reference's adjust_head below buffer_start
    moves the packet up instead of failing (bpf_helper.cpp:755-759).  RAW: the
    unit is the frame, r2 = len.  A descriptor outside the umem is not run:
    failed, verdict / ret 0, off 0, ln 0."""
    del ordered
    ub, n = umem.size, descs.shape[0]
    ovm = po.OracleVM()
    if load_bytes:
        ovm.register_xdp_load_bytes()
    ovm.load(code)
    after = umem.copy()
    out = np.zeros(n, np.uint32 if kind == XDP else np.uint64)
    off, ln, failed = np.zeros(n, np.int32), np.zeros(n, np.uint32), 0
    for i, (a, length, ok) in enumerate(frames(descs, ub)):
        if not ok:
            failed += 1
            continue
        if ncpu:
            po.set_cpu(((first_unit + i) // 64) % ncpu)
        if kind == RAW:
            unit = np.zeros((1, max(length, 8)), np.uint8)
            unit[0, :length] = after[a:a + length]
            out[i] = ovm.run_raw(unit, length)[0]
            after[a:a + length] = unit[0, :length]
        elif chunk:
            c0 = a - a % chunk
            slot = after[c0:c0 + chunk].reshape(1, chunk).copy()
            v, o, m = ovm.run_xdp(slot, lens=np.array([length], np.uint32), want_meta=True, ifindex=ifindex, rxq=rxq,
                                  head=a - c0)
            after[c0:c0 + chunk] = slot[0]
            out[i], off[i], ln[i] = v[0], o[0] - (a - c0), m[0]
        else:
            end = min(a + length + PAD0, ub)
            back = np.zeros((1, length + PAD0), np.uint8)
            back[0, :end - a] = after[a:end]
            v, o, m = ovm.run_xdp(back[:, :length], lens=np.array([length], np.uint32), want_meta=True, ifindex=ifindex,
                                  rxq=rxq)
            after[a:end] = back[0, :end - a]
            out[i], off[i], ln[i] = v[0], o[0], m[0]
    return after, out, off, ln, failed


# ---- the cases --------------------------------------------------------------
def _cases():
    c = []
    # 1. placement x size
    for prog in ("xdp_counter", "flow_hash"):
        for head in (0, 16, 256, 262, "tail"):
            for n in SIZES:
                flow = prog == "flow_hash"
                lens = "flow" if flow else 64
                # flow frames are 64 / 570 / 1500 B: under chunk - len the 570-B ones sit at 1478 = 6 mod 16
                un = "all" if head == 262 else None if (flow and head == "tail") else ()
                c.append(Case(f"place-{prog}-h{head}-n{n}", prog, n, head=head, lens=lens, unstaged=un, seed=n))
    # 2. one odd lane
    for prog in ("xdp_counter", "flow_hash"):
        for tag, n, odd, un in (("lane0", 130, (0,), (0,)), ("lane63", 130, (63,), (0,)), ("lane64", 130, (64,), (1,)),
                                ("last", 130, (129,), (2,)), ("last257", 257, (256,), (4,))):
            c.append(Case(f"odd-{prog}-{tag}", prog, n, lens="flow" if prog == "flow_hash" else 64, odd=odd,
                          unstaged=un, seed=7))
        c.append(Case(f"odd-{prog}-all", prog, 130, lens="flow" if prog == "flow_hash" else 64, all_odd=True,
                      unstaged="all", seed=7))
    # 3. lengths, mixed in one batch (head 256: "rest" = 1792 B, the frame that ends with its chunk)
    for prog in ("xdp_counter", "staged_mix", "flow_hash"):
        for n in (65, 257):
            c.append(Case(f"lens-{prog}-n{n}", prog, n, lens=LENGTH_MIX, unstaged=(), seed=3))
    c.append(Case("lens-xdp_counter-h0", "xdp_counter", 65, head=0, lens=LENGTH_MIX, unstaged=(), seed=4))
    # 4. descriptor edges in the middle of good waves (head 0: chunk 0's frame starts at umem + 0)
    for e in FAILING_EDGES:
        c.append(Case(f"edge-{e}", "xdp_counter", 130, head=0, edge=e, edge_units=(3, 70, 129), nfail=3, unstaged=(),
                      seed=5, meta=True))
        # (a program that reads the ctx generically: off / ln come from the ctx)
        c.append(Case(f"edge-{e}-ctx", "ctx_reader", 130, head=0, edge=e, edge_units=(3, 70, 129), nfail=3, seed=5,
                      meta=True))
    for e, un in (("top", ()), ("top6", (1,)), ("last_byte", (1,)), ("len0", ())):
        c.append(Case(f"edge-{e}", "xdp_counter", 130, head=0, edge=e, edge_units=(70,), unstaged=un, seed=5, meta=True))
    c.append(Case("edge-top32-stage64", "staged_mix", 130, head=0, edge="top32", edge_units=(70,), unstaged=(1,), seed=5))
    c.append(Case("edge-top-stage64", "staged_mix", 130, head=0, edge="top", edge_units=(70,), unstaged=(), seed=5))
    for opt in (0xFFFFFFFF, 0x80000000):
        c.append(Case(f"edge-options-{opt:x}", "xdp_counter", 130, options=opt, unstaged=(), seed=5))
        c.append(Case(f"edge-options-{opt:x}-fail", "xdp_counter", 130, head=0, options=opt, edge="top_plus1",
                      edge_units=(70,), nfail=1, unstaged=(), seed=5))
    # 5. program families
    for n in (65, 257):
        c.append(Case(f"fam-helper_mix-n{n}", "helper_mix", n, head=32, lens=tuple(range(32, 121, 7)), meta=True, seed=9))
        c.append(Case(f"fam-ctx_reader-n{n}", "ctx_reader", n, head=262, lens=LENGTH_MIX, meta=True, seed=9))
        c.append(Case(f"fam-tailcall-n{n}", "tailcall", n, seed=9))
        for fu in (0, 12345):
            c.append(Case(f"fam-percpu-n{n}-first{fu}", "percpu", n, first_unit=fu, ncpu=8, seed=9))
        c.append(Case(f"fam-sampler-n{n}", "sampler", n, seed=9))
        for k in (2024, 2025, 2026):
            c.append(Case(f"fam-random{k}-n{n}", f"random:{k}", n, lens=(64,) * 12 + (40,), seed=k))
    # 6. CTX_RAW over descriptors
    for prog in ("raw_sum", "raw_staged"):
        for n in (1, 65, 257):
            c.append(Case(f"raw-{prog}-n{n}", prog, n, lens=(64, 65, 1500, 100), seed=11))
            c.append(Case(f"raw-{prog}-n{n}-odd", prog, n, lens=(64, 65, 1500, 100), odd=(n - 1,), seed=11))
    # 7. EBPF_BATCH_ORDERED
    for n in (1, 65, 257):
        c.append(Case(f"ordered-n{n}", "last_writer", n, ordered=True, seed=13))
    # 8. stride == 0
    for n in (65,):
        c.append(Case(f"stride0-ctx_reader-n{n}", "ctx_reader", n, chunk=0, lens=(14, 60, 64, 65, 1500), meta=True, seed=15))
        for prog in ("adjust_head:-1", "adjust_tail:1", "adjust_tail:200", "adjust_head:14", "adjust_tail:-4"):
            c.append(Case(f"stride0-{prog}-n{n}", prog, n, chunk=0, lens=(60, 64, 65, 1500), meta=True, seed=15))
    return {x.name: x for x in c}


CASES = _cases()


def named(prefix):
    return [k for k in CASES if k.startswith(prefix)]


def with_options(case, options):
    return replace(case, options=options)
