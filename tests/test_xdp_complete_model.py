"""The numpy model of bpftime_amd_xdp_complete (tests/_xdp_complete.py) against
cases worked out by hand from the rules in include/bpftime_amd.h: the expected
lists below are typed in, not computed, so the model is not its own judge."""
import numpy as np

import _xdp_complete as X
from _xdp_complete import ABORTED, DROP, PASS, REDIRECT, TX

CHUNK = 2048
UMEM = 16 * CHUNK


def _entries(lst):
    return [(int(e["addr"]), int(e["len"]), int(e["options"])) for e in lst]


def _eight():
    #        unit:  0     1     2     3     4      5      6      7
    addr = [256, 2304, 4098, 6400, 8448, 10496, 12544, 14592]
    length = [64, 64, 100, 64, 92, 64, 64, 64]
    opts = [0, 0, 7, 0, 0, 0, 0, 9]
    verdicts = [TX, DROP, PASS, ABORTED, REDIRECT, 5, 0xFFFFFFFF, TX]
    off = [0, 0, 14, 0, -14, 0, 0, 0]
    ln = [64, 64, 86, 64, 106, 64, 64, 64]
    return X.Case(verdicts, CHUNK, UMEM, descs=X.descs_of(addr, length, opts), off=off, ln=ln)


def test_eight_units_cover_all_five_classes():
    for exact in (True, False):
        r = X.model(_eight(), exact=exact)
        assert r.counts == [3, 1, 1, 2, 1]
        assert list(r.cls) == [3, 1, 2, 0, 4, 0, 0, 3]
        # ABORTED and the out-of-range verdicts 5 and 0xFFFFFFFF: class 0, chunk bases
        assert list(r.lists[ABORTED][1]) == [3, 5, 6]
        assert _entries(r.lists[ABORTED][0]) == [(6144, 0, 0), (10240, 0, 0), (12288, 0, 0)]
        # a FILL entry is the chunk base of a frame at chunk + 256
        assert list(r.lists[DROP][1]) == [1] and _entries(r.lists[DROP][0]) == [(2048, 0, 0)]
        # adjust_head(+14) on a NET_IP_ALIGN frame; options carried
        assert list(r.lists[PASS][1]) == [2] and _entries(r.lists[PASS][0]) == [(4112, 86, 7)]
        assert list(r.lists[TX][1]) == [0, 7] and _entries(r.lists[TX][0]) == [(256, 64, 0), (14592, 64, 9)]
        # a negative offset that stays in the chunk: kept, address lowered
        assert list(r.lists[REDIRECT][1]) == [4] and _entries(r.lists[REDIRECT][0]) == [(8434, 106, 0)]


def test_frame_against_its_chunk_end():
    # 256 + 1792 = 2048 ends exactly on the chunk end; one byte more crosses it
    c = X.Case([TX, TX], CHUNK, UMEM, descs=X.descs_of([256, 2304], [64, 64]), off=[0, 0], ln=[1792, 1793])
    for exact in (True, False):
        r = X.model(c, exact=exact)
        assert r.counts == [1, 0, 0, 1, 0]
        assert _entries(r.lists[TX][0]) == [(256, 1792, 0)] and list(r.lists[TX][1]) == [0]
        assert _entries(r.lists[ABORTED][0]) == [(2048, 0, 0)] and list(r.lists[ABORTED][1]) == [1]


def test_negative_offset_that_leaves_the_chunk():
    c = X.Case([PASS, PASS, PASS], CHUNK, UMEM, descs=X.descs_of([2304, 2304, 2], [64, 64, 64]),
               off=[-256, -257, -3], ln=[64, 64, 64])
    for exact in (True, False):
        r = X.model(c, exact=exact)
        assert list(r.cls) == [PASS, 0, 0]
        assert _entries(r.lists[PASS][0]) == [(2048, 64, 0)]
        # (unit 2: 2 - 3 is a negative sum, out of range)
        assert _entries(r.lists[ABORTED][0]) == [(2048, 0, 0), (0, 0, 0)]


def test_chunk_outside_the_umem_keeps_the_address():
    c = X.Case([TX, TX, DROP], CHUNK, UMEM, descs=X.descs_of([UMEM - CHUNK + 256, UMEM + 256, 40000], [64, 64, 64]))
    for exact in (True, False):
        r = X.model(c, exact=exact)
        assert list(r.cls) == [TX, 0, 0]
        assert _entries(r.lists[TX][0]) == [(UMEM - CHUNK + 256, 64, 0)]
        assert _entries(r.lists[ABORTED][0]) == [(UMEM + 256, 0, 0), (40000, 0, 0)]


def test_addresses_at_the_top_of_64_bits():
    top = (1 << 64) - 1
    c = X.Case([TX, TX], CHUNK, UMEM, descs=X.descs_of([top, top - 5], [64, 1]), off=[2, 2], ln=[8, 1])
    r = X.model(c)
    assert list(r.cls) == [0, 0] and _entries(r.lists[ABORTED][0]) == [(top, 0, 0), (top - 5, 0, 0)]


def test_strided_mode_offsets_are_relative_to_the_slot():
    c = X.Case([TX, PASS, TX], 256, 3 * 256, off=[32, 46, 250], ln=[64, 50, 7])
    for exact in (True, False):
        r = X.model(c, exact=exact)
        assert list(r.cls) == [TX, PASS, 0]  # 250 + 7 crosses the slot end
        assert _entries(r.lists[TX][0]) == [(32, 64, 0)] and _entries(r.lists[PASS][0]) == [(256 + 46, 50, 0)]
        assert _entries(r.lists[ABORTED][0]) == [(512, 0, 0)]


def test_frame_mask_chooses_frame_or_chunk():
    c = _eight()
    c.frame_mask = 1 << DROP
    r = X.model(c)
    assert _entries(r.lists[DROP][0]) == [(2304, 64, 0)]
    assert _entries(r.lists[TX][0]) == [(0, 0, 0), (14336, 0, 0)]


def test_cap_smaller_than_the_count():
    r = X.model(_eight())
    img = X.list_image(r.lists[TX][0], 1, 3, X.DESC)
    assert _entries(img[:1]) == [(256, 64, 0)]
    assert (img[1:].view(np.uint8) == X.SENTINEL).all()
    idx = X.list_image(r.lists[ABORTED][1], 2, 4, np.uint32)
    assert list(idx) == [3, 5, 0xA5A5A5A5, 0xA5A5A5A5]
    assert r.counts[TX] == 2 and r.counts[ABORTED] == 3  # the totals stay full


def test_gather_is_one_list_in_unit_order_across_two_classes():
    c = _eight()
    c.gather_mask, c.gather_stride, c.gather_cap = (1 << TX) | (1 << PASS), 128, 8
    c.umem = (np.arange(UMEM) % 251).astype(np.uint8)
    for exact in (True, False):
        r = X.model(c, exact=exact)
        assert list(r.g_index) == [0, 2, 7] and (r.g_count, r.g_skipped) == (3, 0)
        assert _entries(r.g_descs) == [(0, 64, 0), (128, 86, 7), (256, 64, 9)]
        assert [int(s) for s in r.g_src] == [256, 4112, 14592]
    img = X.gather_image(c, r, 4)
    assert (img[:64] == c.umem[256:320]).all() and (img[64:128] == X.SENTINEL).all()
    assert (img[128:128 + 86] == c.umem[4112:4112 + 86]).all() and (img[128 + 86:256] == X.SENTINEL).all()
    assert (img[384:] == X.SENTINEL).all()
    # a frame longer than the stride is skipped, not gathered, and takes no slot
    c.gather_stride = 64
    r = X.model(c)
    assert list(r.g_index) == [0, 7] and (r.g_count, r.g_skipped) == (2, 1)
    assert _entries(r.g_descs) == [(0, 64, 0), (64, 64, 9)]


def test_exact_and_vectorised_forms_agree():
    rng = np.random.default_rng(5)
    n = 700
    ub, d = X.shuffled_ring(n, rng)
    d["addr"][::97] += 5 * ub  # some outside the umem
    off = rng.integers(-300, 2100, n).astype(np.int32)
    ln = rng.integers(0, 2100, n).astype(np.uint32)
    c = X.Case(X.pattern("uniform7", n, rng), CHUNK, ub, descs=d, off=off, ln=ln, gather_mask=0xC, gather_stride=1500)
    a, b = X.model(c, exact=True), X.model(c, exact=False)
    assert a.counts == b.counts and min(a.counts) > 0
    for (ea, ia), (eb, ib) in zip(a.lists, b.lists):
        assert X.same(ea, eb) and X.same(ia, ib)
    assert X.same(a.g_index, b.g_index) and X.same(a.g_descs, b.g_descs) and X.same(a.g_src, b.g_src)
    assert (a.g_count, a.g_skipped) == (b.g_count, b.g_skipped) and a.g_skipped > 0
