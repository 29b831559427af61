"""What test_gpu_umem_matrix.py takes for granted about its cases
(tests/_umem.py), checked without a GPU: the frames are disjoint and inside
their chunks and the umem, each case fails the descriptors it declares, the
waves it declares as falling back from staging follow from the descriptors,
hash maps stay at most half full, and the reference is deterministic and
blind to the options word."""
import numpy as np
import pytest

from bpftime_amd import isa

import _umem as U

ALL = list(U.CASES)


@pytest.mark.parametrize("name", ALL)
def test_frames_disjoint_and_in_their_chunks(name):
    case = U.CASES[name]
    umem, descs, guard = U.build(case)
    place = case.chunk or U.CHUNK
    assert umem.size % place == 0 and umem.size == (case.n + 5) * place and guard.size == U.GUARD_BYTES
    fr = U.frames(descs, umem.size)
    assert sum(not ok for _, _, ok in fr) == case.nfail
    legal = sorted((a, ln) for a, ln, ok in fr if ok)
    assert len({a for a, _ in legal}) == len(legal)                         # no descriptor twice
    for (a, ln), (b, _) in zip(legal, legal[1:]):
        assert a + ln <= b, (a, ln, b)                                       # no overlap
    for a, ln in legal:
        assert a % place + ln <= place and a + ln <= umem.size               # inside one chunk, inside the umem
    assert any(a // place == 0 for a, _ in legal)                            # where a failed lane would land
    # an address a kernel may dereference stays inside umem + guard even when a
    # staged window (<= 64 B) or the stride-0 pad is added to it
    assert all(a + max(64, ln + U.PAD0) <= umem.size + U.GUARD_BYTES for a, ln in legal)
    assert (descs[:, 1] >> np.uint64(32) == np.uint64(case.options)).all()
    if case.edge in U.FAILING_EDGES:
        assert case.nfail == len(case.edge_units) and all(not fr[u][2] for u in case.edge_units)
    elif case.edge:
        assert all(fr[u][2] for u in case.edge_units)


@pytest.mark.parametrize("name", [k for k in ALL if U.CASES[k].prog in U.STAGE])
def test_declared_staging_follows_from_the_descriptors(name):
    case = U.CASES[name]
    umem, descs, _ = U.build(case)
    got = U.unstaged_waves(descs, umem.size, U.STAGE[case.prog])
    waves = (case.n + 63) // 64
    if case.unstaged == "all":
        assert got == tuple(range(waves))
    elif case.unstaged is not None:
        assert got == tuple(case.unstaged)
    assert set(got) <= set(range(waves))


def _reference(po, case):
    po.reset()
    po.set_ncpu(case.ncpu or 1)
    po.set_cpu(0)
    umem, descs, _ = U.build(case)
    s = U.setup(case.prog, po)
    r = U.reference(po, s.code, umem, descs, case.chunk, kind=s.kind, ncpu=case.ncpu, first_unit=case.first_unit,
                    ordered=case.ordered, load_bytes=s.load_bytes)
    return r, [U.map_state(o, False) for o, _ in s.maps], s


@pytest.mark.parametrize("name", ALL)
def test_reference_is_deterministic_and_ignores_options(fresh_oracle, name):
    case = U.CASES[name]
    (u1, v1, o1, l1, f1), m1, s = _reference(fresh_oracle, case)
    for o, _ in s.maps:
        if o.type == isa.BPF_MAP_TYPE_HASH:
            assert 0 < o.count() <= o.max_entries // 2
    assert f1 == case.nfail
    other = U.with_options(case, 0x80000001 if case.options == 0 else 0)
    for c in (case, other):
        (u2, v2, o2, l2, f2), m2, _ = _reference(fresh_oracle, c)
        np.testing.assert_array_equal(u2, u1)
        np.testing.assert_array_equal(v2, v1)
        np.testing.assert_array_equal(o2, o1)
        np.testing.assert_array_equal(l2, l1)
        assert f2 == f1 and m2 == m1
    # failed units leave verdict / ret 0, off 0, ln 0
    umem, descs, _ = U.build(case)
    for i, (_, _, ok) in enumerate(U.frames(descs, umem.size)):
        if not ok:
            assert v1[i] == 0 and o1[i] == 0 and l1[i] == 0
    # bytes outside what the legal units own are the builder's
    keep = ~U.owned(descs, umem.size, case.chunk, s.kind)
    np.testing.assert_array_equal(u1[keep], umem[keep])


def test_stride0_adjust_head_below_the_frame_moves_the_packet(fresh_oracle):
    """bpf_xdp_adjust_head(-1) on a slot of exactly len bytes does not fail:
    data < buffer_start takes the reference's memmove branch
    (bpf_helper.cpp:755-759), which writes the byte behind the frame."""
    case = U.CASES["stride0-adjust_head:-1-n65"]
    (after, v, off, ln, failed), _, _ = _reference(fresh_oracle, case)
    umem, descs, _ = U.build(case)
    assert failed == 0 and (v == 0).all() and (off == 0).all()
    a, length, _ = U.frames(descs, umem.size)[0]
    assert ln[0] == length
    np.testing.assert_array_equal(after[a + 1:a + length + 1], umem[a:a + length])
    # the growing adjust_tail does fail there, adjust_head(+14) and adjust_tail(-4) succeed
    for name, rc, d_off, d_len in (("stride0-adjust_tail:1-n65", 2 ** 32 - 22, 0, 0), ("stride0-adjust_tail:200-n65", 2 ** 32 - 22, 0, 0),
                                   ("stride0-adjust_head:14-n65", 0, 14, -14), ("stride0-adjust_tail:-4-n65", 0, 0, -4)):
        c = U.CASES[name]
        (_, v, off, ln, _), _, _ = _reference(fresh_oracle, c)
        _, d, _ = U.build(c)
        lens = (d[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (v == rc).all() and (off == d_off).all() and (ln == lens + d_len).all(), name


def test_ctx_reader_fold_is_what_the_oracle_reads(fresh_oracle):
    case = U.CASES["stride0-ctx_reader-n65"]
    (_, v, _, _, _), _, _ = _reference(fresh_oracle, case)
    _, d, _ = U.build(case)
    lens = (d[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert [int(x) for x in v] == [U.ctx_fold(0, int(n), int(n)) for n in lens]   # buffer = the frame
    case = U.CASES["fam-ctx_reader-n65"]
    (_, v, _, _, _), _, _ = _reference(fresh_oracle, case)
    _, d, _ = U.build(case)
    lens = (d[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert [int(x) for x in v] == [U.ctx_fold(int(a) % U.CHUNK, U.CHUNK, int(n)) for a, n in zip(d[:, 0], lens)]
