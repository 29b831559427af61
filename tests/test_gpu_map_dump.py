"""bpftime_amd_map_dump on the device (csrc/map_dump.hip, map_dump.cpp) and the
bpf(2) *_BATCH commands over it.

The expected values never come from the dump itself: where a map is filled by
the same host updates on the oracle and the device they are the oracle's
get_next_key + lookup walk; where the table is written as an image
(Map.restore) they are that image's live rows decoded in numpy
(_map_dump.image_entries).  Against the oracle's HASH walk the order is
compared exactly (the same hash, probe and bucket count on both sides).  The
oracle keeps a PERCPU_HASH and an LRU_HASH map as lists (insertion order;
oracle/maps.c: the reference's unordered_map order is not its contract), so
there the contents are compared with the oracle's walk as a dict, and the order
with the snapshot's bucket order decoded in numpy and the device's own
next_key walk (_agrees)."""
import ctypes as C
import errno
import struct

import numpy as np
import pytest

import _map_dump as md
from _helpers import make_maps
from bpftime_amd import gen, isa, programs
from bpftime_amd.isa import Asm

pytestmark = pytest.mark.gpu

HASH, PERCPU_HASH, LRU = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_PERCPU_HASH, isa.BPF_MAP_TYPE_LRU_HASH
ARRAY, PERCPU_ARRAY = isa.BPF_MAP_TYPE_ARRAY, isa.BPF_MAP_TYPE_PERCPU_ARRAY
I32 = lambda v: struct.pack("<I", v)  # noqa: E731
I64 = lambda v: struct.pack("<Q", v)  # noqa: E731


def _fill(maps, keys, value):
    for k in keys:
        for m in maps:
            assert m.update(I32(k), value(k)) == 0


def _dump_error(m, **kw):
    with pytest.raises(Exception) as e:
        m.dump(**kw)
    return e.value.errno, str(e.value)


def _agrees(dm, got, om, exact_order):
    """`got` (pairs in dump order) against the oracle's walk -- exactly, or as
    a dict where the oracle's order is its own -- and, always, against the
    bucket order of the device table decoded in numpy."""
    want = md.walk(om)
    if exact_order:
        assert got == want
    else:
        assert len(got) == len(want) == len(dict(got)) and dict(got) == dict(want)
    _, wk, wv = md.image_entries(dm.snapshot(), dm.geometry(), dm.key_size, dm.user_value_size)
    assert got == md.as_pairs(wk, wv)
    return want


def _small(po, dev, keys=(11, 5000, 77, 123456, 9, 31, 4242)):
    (om,), (dm,) = make_maps([(HASH, 4, 8, 10)], po, dev)
    _fill((om, dm), keys, lambda k: I64(k * 1000 + 1))
    return om, dm


# ---- 1. less than a wave ---------------------------------------------------
def test_small_map_equals_oracle_walk(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    (oe,), (de,) = make_maps([(HASH, 4, 8, 10)], po, dev)
    k, v, nxt, end = de.dump()
    assert (len(k), len(v), nxt, end) == (0, 0, 11, 11) and k.shape == (0, 4) and v.shape == (0, 8)
    om, dm = _small(po, dev)
    assert dm.geometry()[0] == 11
    before, count = dm.snapshot(), dm.count()
    k, v, nxt, end = dm.dump()
    want = md.walk(om)
    assert len(want) == 7
    assert md.as_pairs(k, v) == want
    assert nxt == end == 11
    np.testing.assert_array_equal(dm.snapshot(), before)
    assert dm.count() == count == 7
    # the outputs may be device memory
    dk, dv = dev.DeviceBuffer(7 * 4), dev.DeviceBuffer(7 * 8)
    a = dev.MapDumpArgs(fd=dm.fd, cap=7, keys=dk.ptr, values=dv.ptr)
    assert dev.lib().bpftime_amd_map_dump(C.byref(a)) == 0 and (a.count, a.next, a.end) == (7, 11, 11)
    assert md.as_pairs(dk.download().reshape(7, 4), dv.download().reshape(7, 8)) == want


def test_full_table_returns_every_bucket(fresh_runtime):
    """11 entries in 11 buckets (an image: host updates stop at max_entries)."""
    dev = fresh_runtime
    m = dev.Map(HASH, 4, 8, 10)
    geo = m.geometry()
    raw = md.make_image(geo, range(11), seed=3)
    m.restore(raw)
    idx, wk, wv = md.image_entries(raw, geo, 4, 8)
    assert list(idx) == list(range(11))
    k, v, nxt, end = m.dump(cap=64)
    np.testing.assert_array_equal(k, wk)
    np.testing.assert_array_equal(v, wv)
    assert nxt == end == 11 and m.count() == 11


# ---- 2. cursor chain -------------------------------------------------------
def test_cursor_chain(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    om, dm = _small(po, dev)
    geo = dm.geometry()
    idx, _, _ = md.image_entries(dm.snapshot(), geo, 4, 8)
    want = md.walk(om)
    for cap in (1, 3, 7, 64):
        pairs, chain = md.dump_all(dm, cap)
        assert pairs == want, cap
        assert chain == md.chunks(idx, cap, 11), cap
    # a start in the middle of a run of live buckets: only entries at or after it
    run = next(int(i) for n, i in enumerate(idx[1:], 1) if idx[n - 1] == i - 1)
    pairs, chain = md.dump_all(dm, 64, start=run)
    first = list(idx).index(run)
    assert first > 0 and pairs == want[first:] and chain == [(7 - first, 11)]
    k, v, nxt, end = dm.dump(start=11)
    assert (len(k), nxt, end) == (0, 11, 11)
    err, text = _dump_error(dm, start=12)
    assert err == errno.EINVAL and "start" in text
    k, v, nxt, end = dm.dump(cap=0, start=int(idx[2]))
    assert (len(k), nxt, end) == (0, int(idx[2]), 11)
    # NULL keys or NULL values still counts (and fills the other)
    k, v, nxt, end = dm.dump(cap=3, keys=False)
    assert (len(k), nxt) == (3, int(idx[3])) and [bytes(x) for x in v] == [w[1] for w in want[:3]]
    k, v, nxt, end = dm.dump(cap=3, values=False)
    assert (len(v), nxt) == (3, int(idx[3])) and [bytes(x) for x in k] == [w[0] for w in want[:3]]
    rc, e, count, nxt, end, _, _ = md.dump_raw(dm, 64, keys=False, values=False)
    assert (rc, count, nxt) == (0, 7, 11)


# ---- 3. tile, wave and pass edges ------------------------------------------
def _edge_live(nb, T, seed):
    """Buckets 0, 63, 64, T-1, T and nb-1; where the table has the tiles for
    it, one tile all live and one all empty; a seeded random rest."""
    rng = np.random.default_rng(seed)
    live = rng.random(nb) < 0.4
    tiles = (nb + T - 1) // T
    if tiles == 3:
        live[0:T] = True                      # tile 0 all live
    if tiles >= 5:
        live[2 * T:3 * T] = True              # tile 2 all live
        live[3 * T:4 * T] = False             # tile 3 all empty
    for b in (0, 63, 64, T - 1, T, nb - 1):
        if b < nb:
            live[b] = True
    return np.flatnonzero(live)


@pytest.mark.parametrize("where", ["below_T", "above_T", "above_2T", "above_4T"])
def test_tile_and_wave_edges(fresh_runtime, where):
    dev = fresh_runtime
    T = dev.lib().bpftime_amd_map_dump_tile()
    max_entries = {"below_T": T - 10, "above_T": T + 1, "above_2T": 2 * T + 1, "above_4T": 4 * T + 1}[where]
    m = dev.Map(HASH, 4, 8, max_entries)
    geo = m.geometry()
    nb = geo[0]
    assert {"below_T": T - 10 <= nb < T, "above_T": T < nb < 2 * T, "above_2T": 2 * T < nb < 3 * T,
            "above_4T": 4 * T < nb < 5 * T}[where]
    raw = md.make_image(geo, _edge_live(nb, T, seed=nb), seed=nb + 1)
    m.restore(raw)
    idx, wk, wv = md.image_entries(raw, geo, 4, 8)
    live = len(idx)
    first_tile = int((idx < T).sum())
    assert m.count() == live
    for cap in (nb, live - 1, first_tile - 1, first_tile, first_tile + 1):
        rc, e, count, nxt, end, kb, vb = md.dump_raw(m, cap, room=nb)
        n = min(cap, live)
        assert (rc, count, end) == (0, n, nb), cap
        assert nxt == (int(idx[n]) if n < live else nb), cap
        np.testing.assert_array_equal(kb[:n * 4].reshape(n, 4), wk[:n])
        np.testing.assert_array_equal(vb[:n * 8].reshape(n, 8), wv[:n])
        assert (kb[n * 4:] == md.GUARD).all() and (vb[n * 8:] == md.GUARD).all(), cap
    # chained from the middle of the all-live / last tile
    pairs, chain = md.dump_all(m, 100, start=int(idx[live // 2]))
    assert pairs == md.as_pairs(wk[live // 2:], wv[live // 2:])
    assert chain == md.chunks(idx, 100, nb, start=int(idx[live // 2]))
    np.testing.assert_array_equal(m.snapshot(), raw)


def test_scan_pass_boundary(fresh_runtime):
    """More tiles than one pass of the scan takes (the smallest slots a hash
    map has, 32 B; one restore; numpy expected), a run of live buckets across
    the pass boundary."""
    dev = fresh_runtime
    T, S = dev.lib().bpftime_amd_map_dump_tile(), dev.lib().bpftime_amd_map_dump_scan_tiles()
    if S == 0:
        return  # (the scan has no passes: nothing to straddle)
    m = dev.Map(HASH, 4, 8, S * T + 2 * T + 5)
    geo = m.geometry()
    nb = geo[0]
    assert nb > S * T + 2 * T and geo[1] == 32
    rng = np.random.default_rng(17)
    live = rng.random(nb) < 0.03
    live[S * T - 150:S * T + 150] = True
    live[nb - 1] = True
    raw = md.make_image(geo, np.flatnonzero(live), seed=18)
    m.restore(raw)
    idx, wk, wv = md.image_entries(raw, geo, 4, 8)
    k, v, nxt, end = m.dump()
    assert len(k) == len(idx) and nxt == end == nb
    np.testing.assert_array_equal(k, wk)
    np.testing.assert_array_equal(v, wv)
    # a cap that cuts inside the run, then the rest from there
    cut = int(np.searchsorted(idx, S * T)) + 7
    k, v, nxt, end = m.dump(cap=cut)
    assert len(k) == cut and nxt == int(idx[cut]) and nxt > S * T
    np.testing.assert_array_equal(k, wk[:cut])
    k, v, nxt2, end = m.dump(start=nxt)
    assert nxt2 == nb
    np.testing.assert_array_equal(k, wk[cut:])
    np.testing.assert_array_equal(v, wv[cut:])


# ---- 4. size matrix ----------------------------------------------------------
@pytest.mark.parametrize("ks", [1, 4, 5, 16, 20])
def test_size_matrix(fresh_runtime, ks):
    dev = fresh_runtime
    for vs in (1, 8, 12, 120, 200):
        m = dev.Map(HASH, ks, vs, 199)
        geo = m.geometry()
        nb, ss = geo[0], geo[1]
        assert nb == 199
        if vs == 200:
            assert ss % 128 == 0 and ss > 128  # whole 128-B lines
        rng = np.random.default_rng(ks * 1000 + vs)
        live = np.flatnonzero(rng.random(nb) < 0.6)
        raw = md.make_image(geo, live, seed=ks * 1000 + vs + 1)
        m.restore(raw)
        idx, wk, wv = md.image_entries(raw, geo, ks, vs)
        n = len(idx)
        for cap, room in ((nb, nb), (n - 3, n)):
            rc, e, count, nxt, end, kb, vb = md.dump_raw(m, cap, room=room)
            c = min(cap, n)
            assert (rc, count, end) == (0, c, nb), (vs, cap)
            assert nxt == (int(idx[c]) if c < n else nb)
            np.testing.assert_array_equal(kb[:c * ks].reshape(c, ks), wk[:c], err_msg=f"keys vs={vs}")
            np.testing.assert_array_equal(vb[:c * vs].reshape(c, vs), wv[:c], err_msg=f"values vs={vs}")
            assert (kb[c * ks:] == md.GUARD).all() and (vb[c * vs:] == md.GUARD).all(), (vs, cap)
        np.testing.assert_array_equal(m.snapshot(), raw)
        m.close()


# ---- 5. per-CPU maps and arrays ----------------------------------------------
@pytest.mark.parametrize("ncpu,vs", [(64, 8), (3, 4)])
def test_percpu_hash(fresh_oracle, fresh_runtime, ncpu, vs):
    po, dev = fresh_oracle, fresh_runtime
    po.set_ncpu(ncpu)
    dev.set_ncpu(ncpu)
    (om,), (dm,) = make_maps([(PERCPU_HASH, 4, vs, 50)], po, dev)
    assert dm.user_value_size == ncpu * vs
    rng = np.random.default_rng(ncpu)
    for k in rng.choice(1 << 20, 37, replace=False):
        val = rng.integers(0, 256, ncpu * vs, dtype=np.uint8).tobytes()
        assert om.update(I32(int(k)), val) == 0 and dm.update(I32(int(k)), val) == 0
    before = dm.snapshot()
    k, v, nxt, end = dm.dump()
    assert v.shape == (37, ncpu * vs) and nxt == end == dm.geometry()[0]
    got = md.as_pairs(k, v)
    assert len(_agrees(dm, got, om, exact_order=False)) == 37
    assert [g[0] for g in got] == _next_key_walk(dm)
    pairs, _ = md.dump_all(dm, 5)
    assert pairs == got
    np.testing.assert_array_equal(dm.snapshot(), before)


@pytest.mark.parametrize("type_,vs,ncpu", [(PERCPU_ARRAY, 8, 3), (ARRAY, 12, 64)])
def test_arrays(fresh_oracle, fresh_runtime, type_, vs, ncpu):
    po, dev = fresh_oracle, fresh_runtime
    po.set_ncpu(ncpu)
    dev.set_ncpu(ncpu)
    (om,), (dm,) = make_maps([(type_, 4, vs, 5)], po, dev)
    uvs = dm.user_value_size
    assert uvs == (vs * ncpu if type_ == PERCPU_ARRAY else vs)
    rng = np.random.default_rng(vs)
    for i in (0, 2, 3, 4):
        val = rng.integers(0, 256, uvs, dtype=np.uint8).tobytes()
        assert om.update(I32(i), val) == 0 and dm.update(I32(i), val) == 0
    want = md.walk(om)
    assert [w[0] for w in want] == [I32(i) for i in range(5)]
    before = dm.snapshot()
    k, v, nxt, end = dm.dump()
    assert md.as_pairs(k, v) == want and nxt == end == 5
    pairs, chain = md.dump_all(dm, 2)
    assert pairs == want and chain == [(2, 2), (2, 4), (1, 5)]
    k, v, nxt, end = dm.dump(cap=64, start=3)
    assert md.as_pairs(k, v) == want[3:] and nxt == 5
    assert dm.dump(start=5)[2:] == (5, 5) and _dump_error(dm, start=6)[0] == errno.EINVAL
    assert dm.dump(cap=0, start=1)[2:] == (1, 5)
    k, v, nxt, end = dm.dump(cap=2, keys=False)
    assert [bytes(x) for x in v] == [w[1] for w in want[:2]] and nxt == 2
    err, text = _dump_error(dm, delete=True)
    assert err == errno.EINVAL
    np.testing.assert_array_equal(dm.snapshot(), before)


# ---- 6. after a parallel batch -----------------------------------------------
def test_after_parallel_batch(fresh_oracle, fresh_runtime):
    """flow-hash in a parallel launch without BATCH_SYNC's host wait being
    relied on: the dump's own wait covers the batch and its deferred counter
    adds."""
    po, dev = fresh_oracle, fresh_runtime
    (om,), (dm,) = make_maps([(HASH, 16, 16, 512)], po, dev)
    code = programs.flow_hash(dm.fd)
    n = 4096
    slots, lens = gen.flow_packets(n, nflows=300, stride=2048)
    ovm = po.OracleVM()
    ovm.load(code)
    ovm.run_xdp(slots.copy(), lens=lens)
    vm = dev.VM()
    vm.load(code)
    d, dl = dev.DeviceBuffer.from_array(slots), dev.DeviceBuffer.from_array(lens)
    dv = dev.DeviceBuffer(4 * n)
    s = dev.lib().bpftime_amd_stream_create()
    try:
        assert vm.exec_batch(dev.CTX_XDP, d, n, 2048, lens=dl, verdicts=dv, flags=0, stream=s) == 0
        k, v, nxt, end = dm.dump()   # (no wait of the test's between the launch and the dump)
    finally:
        dev.lib().bpftime_amd_stream_destroy(s)
    got = md.as_pairs(k, v)
    assert nxt == end == dm.geometry()[0]
    assert got == md.walk(dm)            # the device's own walk, order included
    o_items = om.items()
    assert len(got) == len(o_items) > 100 and dict(got) == o_items
    tot = sum(struct.unpack("<QQ", val)[0] for _, val in got)
    ip = (slots[:, 12] == 0x08) & (slots[:, 13] == 0)
    assert tot == int(ip.sum())


# ---- 7. LRU_HASH -------------------------------------------------------------
def test_lru_hash(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    (om,), (dm,) = make_maps([(LRU, 4, 8, 16)], po, dev)
    for k in range(100, 127):            # 11 evictions: tombstones
        for m in (om, dm):
            assert m.update(I32(k), I64(k * 3)) == 0
    for k in (115, 120):
        for m in (om, dm):
            assert m.delete(I32(k)) == 0
    nb = dm.geometry()[0]
    snap = dm.snapshot()
    states = snap[:nb * dm.geometry()[1]].reshape(nb, -1)[:, :4].copy().view(np.uint32)[:, 0]
    assert (states == 3).sum() >= 1 and (states == 1).sum() == 14   # tombstones among the live buckets
    # the oracle's walk uses every key (in the oracle's order): the same uses on the device
    want = md.walk(om)
    for key, val in want:
        assert dm.lookup(key) == val
    assert len(want) == 14
    before = dm.snapshot()
    k, v, nxt, end = dm.dump()
    got = md.as_pairs(k, v)
    assert nxt == end == nb
    assert len(got) == 14 and dict(got) == dict(want)
    idx, wk, wv = md.image_entries(before, dm.geometry(), 4, 8)
    assert got == md.as_pairs(wk, wv)                      # bucket order
    assert [g[0] for g in got] == _next_key_walk(dm)       # the device's own walk order
    pairs, chain = md.dump_all(dm, 3)
    assert pairs == got and chain == md.chunks(idx, 3, nb)
    np.testing.assert_array_equal(dm.snapshot(), before)
    assert dm.count() == 14
    # the dump was no use: fill up, then the next insert evicts the same victim on both
    for k in (200, 201, 202):
        for m in (om, dm):
            assert m.update(I32(k), I64(k)) == 0
    assert dm.count() == om.count() == 16
    assert dm.hash_items() == dict(md.walk(om))
    err, text = _dump_error(dm, delete=True)
    assert err == errno.ENOTSUP and "LRU_HASH" in text


def _next_key_walk(m):
    out, k = [], m.next_key(None)
    while k is not None:
        out.append(bytes(k))
        k = m.next_key(k)
    return out


# ---- 8. drain ------------------------------------------------------------------
def _lookup_prog(fd, vbytes):
    """r0 = the first vbytes (4 / 8) of lookup(map, *(u32 *)unit), or 0xdead on a miss."""
    a = Asm().ldx(4, 2, 1, 0).stx(4, 10, -4, "r2").mov64(2, "r10").add64(2, -4).ld_map_fd(1, fd).call(1)
    a.jmp("jeq", 0, 0, "miss").ldx(vbytes, 0, 0, 0).exit()
    return a.label("miss").mov64(0, 0xDEAD).exit().assemble()


def _lookups_both(po, dev, code, keys, ncpu):
    units = np.zeros((len(keys), 16), np.uint8)
    units[:, :4] = np.array(keys, np.uint32).view(np.uint8).reshape(-1, 4)
    ovm = po.OracleVM()
    ovm.load(code)
    want = np.zeros(len(keys), np.uint64)
    for w0 in range(0, len(keys), 64):
        po.set_cpu((w0 // 64) % ncpu)
        want[w0:w0 + 64] = ovm.run_raw(units[w0:w0 + 64].copy(), 16)
    po.set_cpu(0)
    vm = dev.VM()
    vm.load(code)
    d = dev.DeviceBuffer.from_array(units)
    dr = dev.DeviceBuffer(8 * len(keys))
    assert vm.exec_batch(dev.CTX_RAW, d, len(keys), 16, fixed_len=16, rets=dr) == 0
    return dr.download(np.uint64), want


@pytest.mark.parametrize("type_", [HASH, PERCPU_HASH])
def test_drain(fresh_oracle, fresh_runtime, type_):
    po, dev = fresh_oracle, fresh_runtime
    ncpu = 4
    po.set_ncpu(ncpu)
    dev.set_ncpu(ncpu)
    (om,), (dm,) = make_maps([(type_, 4, 8, 64)], po, dev)
    uvs = dm.user_value_size
    rng = np.random.default_rng(type_)
    keys = [int(k) for k in rng.choice(1 << 16, 40, replace=False)]
    vals = {k: rng.integers(0, 256, uvs, dtype=np.uint8).tobytes() for k in keys}
    for k in keys:
        assert om.update(I32(k), vals[k]) == 0 and dm.update(I32(k), vals[k]) == 0
    code = _lookup_prog(dm.fd, 8)
    probe = (keys + [70000, 70001, 70002]) * 8
    got, want = _lookups_both(po, dev, code, probe, ncpu)   # builds the lookup index, fills the caches' launch
    np.testing.assert_array_equal(got, want)
    assert (got != 0xDEAD).sum() == 40 * 8
    exact = type_ == HASH
    walk0 = md.walk(dm)                   # the device's own walk, pinned to the oracle and the table
    assert len(_agrees(dm, walk0, om, exact)) == 40
    k, v, nxt, end = dm.dump(cap=15, delete=True)
    drained = md.as_pairs(k, v)
    assert drained == walk0[:15]
    # (last returned first: each delete then finds its key.  In bucket order the
    # reference's delete of an earlier bucket of a probe run can orphan a later
    # key of the run, whose own delete then finds nothing and leaves it counted)
    for key, _ in reversed(drained):
        assert om.lookup(key) is not None and om.delete(key) == 0
    for k in keys:
        assert dm.lookup(I32(k)) == om.lookup(I32(k)), k
    rest = md.walk(dm)
    assert len(_agrees(dm, rest, om, exact)) == 25 and rest == walk0[15:]
    assert dm.count() == om.count() == 25
    # state words 0, key and value bytes in place: exactly what delete_elem leaves
    nb, ss, ko, vo = dm.geometry()[:4]
    rows = dm.snapshot()[:nb * ss].reshape(nb, ss)
    st = rows[:, :4].copy().view(np.uint32)[:, 0]
    assert (st == 1).sum() == 25 and set(st) <= {0, 1}
    held = {bytes(r[ko:ko + 4]) for r in rows[st == 0] if r[ko:ko + 4].any() or r[vo:vo + 8].any()}
    assert {key for key, _ in drained} <= held
    # the lookup index and the lookup cache were invalidated: drained keys miss now
    got, want = _lookups_both(po, dev, code, probe, ncpu)
    np.testing.assert_array_equal(got, want)
    assert (got != 0xDEAD).sum() == 25 * 8
    # drain the rest in chunks; then the same keys go back in
    pairs, chain = md.dump_all(dm, 10, start=nxt, delete=True)
    assert pairs == rest and [c for c, _ in chain] == [10, 10, 5]
    assert dm.count() == 0 and md.walk(dm) == [] and len(dm.dump()[0]) == 0
    for key, _ in rest:
        assert om.delete(key) == 0
    for k in keys:
        assert om.update(I32(k), vals[k]) == 0 and dm.update(I32(k), vals[k]) == 0
    assert dm.count() == om.count() == 40
    _agrees(dm, md.as_pairs(*dm.dump()[:2]), om, exact)
    _agrees(dm, md.walk(dm), om, exact)
    got, want = _lookups_both(po, dev, code, probe, ncpu)
    np.testing.assert_array_equal(got, want)


# ---- 9. bpf(2) -----------------------------------------------------------------
def _buf(n):
    a = bytearray(n)
    return a, C.addressof((C.c_char * max(n, 1)).from_buffer(a))


def _batch(dev, cmd, fd, start, count, ks=4, vs=8, **kw):
    """One *_BATCH call: (ret, errno, count out, next token, pairs)."""
    tin, tin_p = _buf(4)
    tout, tout_p = _buf(4)
    kb, kp = _buf(ks * count)
    vb, vp = _buf(vs * count)
    if start is not None:
        struct.pack_into("<I", tin, 0, start)
    attr = dev.attr_map_batch(fd, tin_p if start is not None else 0, tout_p, kp, vp, count, **kw)
    r, e = dev.sys_bpf(cmd, attr)
    n = dev.batch_count(attr)
    pairs = [(bytes(kb[i * ks:(i + 1) * ks]), bytes(vb[i * vs:(i + 1) * vs])) for i in range(n)]
    return r, e, n, struct.unpack("<I", tout)[0], pairs


def test_bpf_batch_commands(fresh_oracle, fresh_runtime):
    po, dev = fresh_oracle, fresh_runtime
    om, dm = _small(po, dev)
    want = md.walk(om)
    LOOKUP, LOOKUP_DELETE = dev.BPF_MAP_LOOKUP_BATCH, dev.BPF_MAP_LOOKUP_AND_DELETE_BATCH
    got, start, calls = [], None, []
    while True:
        r, e, n, tok, pairs = _batch(dev, LOOKUP, dm.fd, start, 4)
        got += pairs
        calls.append((r, e if r else 0, n))
        if r != 0:
            break
        start = tok
        assert len(calls) < 10
    assert got == want
    assert calls == [(0, 0, 4), (-1, errno.ENOENT, 3)]   # the last call: ENOENT with a valid count
    assert tok == 11
    assert _batch(dev, LOOKUP, dm.fd, 11, 4)[:4] == (-1, errno.ENOENT, 0, 11)
    assert _batch(dev, LOOKUP, dm.fd, 12, 4)[:2] == (-1, errno.EINVAL)
    assert _batch(dev, LOOKUP, dm.fd, None, 4, elem_flags=4)[:2] == (-1, errno.EINVAL)   # BPF_F_LOCK
    assert _batch(dev, LOOKUP, dm.fd, None, 4, flags=1)[:2] == (-1, errno.EINVAL)
    assert dm.count() == 7 and md.walk(dm) == want
    q = dev.Map(isa.BPF_MAP_TYPE_QUEUE, 0, 8, 16)
    assert _batch(dev, LOOKUP, q.fd, None, 4)[:3] == (-1, errno.ENOTSUP, 0)
    lru = dev.Map(LRU, 4, 8, 16)
    assert lru.update(I32(1), I64(2)) == 0
    assert _batch(dev, LOOKUP_DELETE, lru.fd, None, 4)[:3] == (-1, errno.ENOTSUP, 0)
    r, e, n, tok, pairs = _batch(dev, LOOKUP, lru.fd, None, 4)
    assert (r, e, n, pairs) == (-1, errno.ENOENT, 1, [(I32(1), I64(2))])
    # the delete command empties the map
    r, e, n, tok, pairs = _batch(dev, LOOKUP_DELETE, dm.fd, None, 5)
    assert (r, n, pairs) == (0, 5, want[:5])
    # (what is left, read with a plain dump: draining the head of a probe run can
    # orphan a kept key, as the same delete_elem calls would, and a next_key walk
    # restarts at a key that lookups no longer find)
    assert dm.count() == 2 and md.as_pairs(*dm.dump()[:2]) == want[5:]
    r, e, n, tok2, pairs = _batch(dev, LOOKUP_DELETE, dm.fd, tok, 5)
    assert (r, e, n, tok2, pairs) == (-1, errno.ENOENT, 2, 11, want[5:])
    assert dm.count() == 0 and dm.next_key(None) is None


# ---- 10. refusals --------------------------------------------------------------
REFUSED = [("RINGBUF", isa.BPF_MAP_TYPE_RINGBUF, 0, 0, 4096), ("QUEUE", isa.BPF_MAP_TYPE_QUEUE, 0, 8, 16),
           ("PROG_ARRAY", isa.BPF_MAP_TYPE_PROG_ARRAY, 4, 4, 4), ("LPM_TRIE", isa.BPF_MAP_TYPE_LPM_TRIE, 8, 4, 16),
           ("BLOOM_FILTER", isa.BPF_MAP_TYPE_BLOOM_FILTER, 0, 8, 64),
           ("STACK_TRACE", isa.BPF_MAP_TYPE_STACK_TRACE, 4, 48, 64),
           ("ARRAY_OF_MAPS", isa.BPF_MAP_TYPE_ARRAY_OF_MAPS, 4, 4, 4),
           ("PERF_EVENT_ARRAY", isa.BPF_MAP_TYPE_PERF_EVENT_ARRAY, 4, 4, 4)]


@pytest.mark.parametrize("name,type_,ks,vs,mx", REFUSED, ids=[r[0] for r in REFUSED])
def test_other_map_types_refused(fresh_runtime, name, type_, ks, vs, mx):
    dev = fresh_runtime
    m = dev.Map(type_, ks, vs, mx)
    before = m.snapshot()
    for flags in (0, dev.DUMP_DELETE):
        a = dev.MapDumpArgs(fd=m.fd, flags=flags, cap=4)
        C.set_errno(0)
        assert dev.lib().bpftime_amd_map_dump(C.byref(a)) == -1
        assert C.get_errno() == errno.ENOTSUP
        assert name in dev.lib().bpftime_amd_last_error().decode()
        assert a.count == 0
    np.testing.assert_array_equal(m.snapshot(), before)
