"""AF_XDP descriptor batches (ebpf_batch::descs) against the oracle at small
edge shapes: 1..257 units, every head room, one misaligned lane per wave,
frames shorter than the staged window, the first and last legal descriptor,
RAW and ORDERED batches, stride 0, and every program family over frames in a
umem.  Each run compares, bit for bit: verdicts or rets, the whole umem (bytes
outside the legal units' chunks unchanged, bytes inside as the oracle left
them), the guard behind the umem, the failed count, the maps, and
data_off_out / len_out where the case asks for them.  The cases and the
reference: tests/_umem.py (checked on their own by test_umem_model.py)."""
import numpy as np
import pytest

from bpftime_amd import isa

import _umem as U

pytestmark = pytest.mark.gpu

UNUSED = dict(head=32, fixed_len=7)     # ebpf_batch fields descriptor mode does not use (include/ebpf-vm.h)


def _device(dev, case, s, umem, descs, guard, unused=False):
    """One descriptor batch of `case` on the device -> the VM and
    (umem, guard, out, off, ln, failed, maps) as it left them."""
    n = case.n
    vm = dev.VM()
    if s.load_bytes:
        assert vm.register(isa.BPF_FUNC_xdp_load_bytes, "bpf_xdp_load_bytes") == 0
    vm.load(s.code)
    du = dev.DeviceBuffer.from_array(np.concatenate([umem, guard]))
    dd = dev.DeviceBuffer.from_array(descs)
    xdp = s.kind == U.XDP
    dout = dev.DeviceBuffer.from_array(np.full(n, 0xEE, np.uint32 if xdp else np.uint64))
    doff = dev.DeviceBuffer.from_array(np.full(n, 0x77, np.int32)) if case.meta else None
    dln = dev.DeviceBuffer.from_array(np.full(n, 0x77, np.uint32)) if case.meta else None
    kw = dict(UNUSED) if unused else {}
    dlens = None
    if unused:
        dlens = kw["lens"] = dev.DeviceBuffer.from_array(np.full(n, 0xFFFFFFFF, np.uint32))
    failed = vm.exec_batch(s.kind, du, n, case.chunk, descs=dd, umem_bytes=umem.size, ifindex=U.IFINDEX, rxq=U.RXQ,
                           first_unit=case.first_unit, data_off_out=doff, len_out=dln,
                           flags=dev.BATCH_SYNC | (dev.BATCH_ORDERED if case.ordered else 0),
                           **{"verdicts" if xdp else "rets": dout}, **kw)
    if dlens is not None:
        assert (dlens.download(np.uint32) == 0xFFFFFFFF).all()
    got = du.download()
    out = dout.download(np.uint32 if xdp else np.uint64)
    # (the output arrays start as 0xEE / 0x77 patterns: a failed unit's zeros
    # are zeros the batch wrote)
    return vm, SimpleResult(got[:umem.size], got[umem.size:], out,
                            doff.download(np.int32) if case.meta else None,
                            dln.download(np.uint32) if case.meta else None, failed,
                            [U.map_state(d, True) for _, d in s.maps])


class SimpleResult:
    def __init__(self, umem, guard, out, off, ln, failed, maps):
        self.umem, self.guard, self.out, self.off, self.ln, self.failed, self.maps = umem, guard, out, off, ln, failed, maps


def run(po, dev, name, unused=False):
    """The case on the oracle and the device, everything compared."""
    case = U.CASES[name]
    if case.ncpu:
        po.set_ncpu(case.ncpu)
        dev.set_ncpu(case.ncpu)
    umem, descs, guard = U.build(case)
    s = U.setup(case.prog, po, dev)
    w_umem, w_out, w_off, w_ln, w_failed = U.reference(
        po, s.code, umem, descs, case.chunk, kind=s.kind, ncpu=case.ncpu, first_unit=case.first_unit,
        ordered=case.ordered, load_bytes=s.load_bytes)
    w_maps = [U.map_state(o, False) for o, _ in s.maps]
    vm, g = _device(dev, case, s, umem, descs, guard, unused)
    assert g.failed == w_failed == case.nfail
    np.testing.assert_array_equal(g.guard, guard)
    own = U.owned(descs, umem.size, case.chunk, s.kind)
    np.testing.assert_array_equal(g.umem[~own], umem[~own])
    np.testing.assert_array_equal(g.umem[own], w_umem[own])
    ok = np.array([f[2] for f in U.frames(descs, umem.size)])
    np.testing.assert_array_equal(g.out[ok], w_out[ok])
    assert (g.out[~ok] == 0).all()
    if case.meta:
        np.testing.assert_array_equal(g.off[ok], w_off[ok])
        np.testing.assert_array_equal(g.ln[ok], w_ln[ok])
        assert (g.off[~ok] == 0).all() and (g.ln[~ok] == 0).all()
    assert g.maps == w_maps
    return vm, g, (umem, descs)


def _staged(vm, case, want=True):
    if case.prog in U.STAGE:
        assert vm.last_launch()["stage"] == (U.STAGE[case.prog] if want else 0)


@pytest.mark.parametrize("name", U.named("place-"))
def test_placement_and_size(fresh_oracle, fresh_runtime, name):
    """Head room 0 / 16 / 256 / 262 / chunk - len at 1..257 units: staged
    loads and stores (xdp_counter's MAC swap) and flow_hash's inserts."""
    vm, _, _ = run(fresh_oracle, fresh_runtime, name)
    _staged(vm, U.CASES[name])           # the launch stages; each wave decides for its own frames


@pytest.mark.parametrize("staging", [True, False])
@pytest.mark.parametrize("name", U.named("odd-"))
def test_one_odd_lane(fresh_oracle, fresh_runtime, monkeypatch, name, staging):
    """One frame off 16-B alignment at lane 0, 63, 64 and the last lane of a
    partial wave (and all of them): that wave falls back, the others stage,
    all are exact; the same without staging at all."""
    if not staging:
        monkeypatch.setenv("BPFTIME_AMD_NO_STAGING", "1")
    vm, _, _ = run(fresh_oracle, fresh_runtime, name)
    _staged(vm, U.CASES[name], staging)


@pytest.mark.parametrize("name", U.named("lens-"))
def test_lengths(fresh_oracle, fresh_runtime, name):
    """14 .. chunk - head bytes mixed in one batch: frames shorter than the
    staged window; the bytes behind a short frame belong to its chunk and
    come back as the oracle left them."""
    vm, _, _ = run(fresh_oracle, fresh_runtime, name)
    _staged(vm, U.CASES[name])


@pytest.mark.parametrize("name", U.named("edge-"))
def test_descriptor_edges(fresh_oracle, fresh_runtime, name):
    """The last legal and first illegal addr / len in the middle of good
    waves, a nonzero options word, and a staged window across the umem end.
    Each failed unit counts once (verdict 0, off 0, ln 0: run() checks) and
    its neighbours are exact."""
    case = U.CASES[name]
    vm, g, (umem, descs) = run(fresh_oracle, fresh_runtime, name)
    _staged(vm, case)
    if case.edge in U.LEGAL_EDGES and case.prog == "xdp_counter":
        # the legal edge ran: TX for a whole Ethernet header, DROP below 14 B
        u = case.edge_units[0]
        assert g.out[u] == (isa.XDP_TX if case.edge in ("top", "top6") else isa.XDP_DROP)
    if case.prog == "xdp_counter":
        bss = g.maps[1][0]
        assert int(np.frombuffer(bss[:8], np.uint64)[0]) == case.n - case.nfail


@pytest.mark.parametrize("name", [k for k in U.named("fam-") if "random" not in k])
def test_program_families(fresh_oracle, fresh_runtime, name):
    """The helper mix with data_off_out / len_out, a reader of every generic
    ctx field (buffer_start / buffer_end = the frame's chunk), a tail-call
    image, a per-CPU counter under first_unit, and the ring-buffer sampler."""
    case = U.CASES[name]
    _, g, (_, descs) = run(fresh_oracle, fresh_runtime, name)
    if case.prog == "ctx_reader":
        lens = (descs[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert [int(v) for v in g.out] == [U.ctx_fold(int(a) % U.CHUNK, U.CHUNK, int(n)) for a, n in zip(descs[:, 0], lens)]
    if case.prog == "sampler":
        assert len(g.maps[1]) == case.n // 64


@pytest.mark.parametrize("asm_groups", [True, False])
@pytest.mark.parametrize("name", U.named("fam-random"))
def test_random_xdp_programs_over_descriptors(fresh_oracle, fresh_runtime, monkeypatch, name, asm_groups):
    if not asm_groups:
        monkeypatch.setenv("BPFTIME_AMD_NO_ASM_DIVERGENCE", "1")
    run(fresh_oracle, fresh_runtime, name)


@pytest.mark.parametrize("name", U.named("raw-"))
def test_ctx_raw_over_descriptors(fresh_oracle, fresh_runtime, name):
    """EBPF_CTX_RAW with descriptors: r1 = the frame, r2 = its len, u64 rets."""
    run(fresh_oracle, fresh_runtime, name)


@pytest.mark.parametrize("name", U.named("ordered-"))
def test_ordered_over_descriptors(fresh_oracle, fresh_runtime, name):
    """A last-writer-wins program over a ring whose order is a permutation of
    address order: the map value and every ret are the ring-order result."""
    _, g, (_, descs) = run(fresh_oracle, fresh_runtime, name)
    if U.CASES[name].n > 1:
        assert (np.diff(descs[:, 0].astype(np.int64)) < 0).any()


@pytest.mark.parametrize("name", U.named("stride0-"))
def test_stride_zero(fresh_oracle, fresh_runtime, name):
    """stride == 0: the ctx buffer is the frame.  The reader reports
    buffer_start == data and buffer_end == data_end; a growing adjust_tail
    fails; adjust_head(+14) / adjust_tail(-4) succeed; adjust_head(-1) does
    not fail in the reference (bpf_helper.cpp:755-759: data below buffer_start
    moves the packet up), so it is pinned to the oracle's byte behind the
    frame, which lies inside the frame's own chunk here."""
    case = U.CASES[name]
    _, g, (_, descs) = run(fresh_oracle, fresh_runtime, name)
    lens = (descs[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    einval = 2 ** 32 - 22
    if case.prog == "ctx_reader":
        assert [int(v) for v in g.out] == [U.ctx_fold(0, int(n), int(n)) for n in lens]
        assert (g.off == 0).all() and (g.ln == lens).all()
    elif case.prog in ("adjust_tail:1", "adjust_tail:200"):
        assert (g.out == einval).all() and (g.off == 0).all() and (g.ln == lens).all()
    elif case.prog == "adjust_head:14":
        assert (g.out == 0).all() and (g.off == 14).all() and (g.ln == lens - 14).all()
    elif case.prog == "adjust_tail:-4":
        assert (g.out == 0).all() and (g.off == 0).all() and (g.ln == lens - 4).all()
    else:
        assert (g.out == 0).all() and (g.off == 0).all() and (g.ln == lens).all()


@pytest.mark.parametrize("name", ["place-xdp_counter-h256-n65", "fam-helper_mix-n65", "fam-helper_mix-n257"])
def test_unused_fields_are_unused(fresh_oracle, fresh_runtime, name):
    """head, fixed_len and lens are not used in descriptor mode
    (include/ebpf-vm.h): a batch with head = 32, fixed_len = 7 and a lens
    array of 0xFFFFFFFF gives the results of the batch without them, bit for
    bit, and leaves lens alone.  (Before this test the device added head to
    every frame's address: shifted packets.)"""
    po, dev = fresh_oracle, fresh_runtime
    _, plain, _ = run(po, dev, name)
    po.reset()
    dev.reset_runtime()
    dev.set_ncpu(64)
    vm, g, _ = run(po, dev, name, unused=True)
    _staged(vm, U.CASES[name])
    np.testing.assert_array_equal(g.umem, plain.umem)
    np.testing.assert_array_equal(g.out, plain.out)
    if plain.off is not None:
        np.testing.assert_array_equal(g.off, plain.off)
        np.testing.assert_array_equal(g.ln, plain.ln)
    assert g.failed == plain.failed and g.maps == plain.maps
