"""The Bloom filter model (tests/_bloom.py) against published vectors and
hand-worked cases, and the host-side shard merge.  No GPU."""
import numpy as np
import pytest

from bpftime_amd import shard

import _bloom


def test_jenkins_vectors():
    """Bob Jenkins's lookup3.c driver5 vectors for hashlittle."""
    s = b"Four score and seven years ago"
    assert _bloom.jhash(s, 0) == 0x17770551
    assert _bloom.jhash(s, 1) == 0xCD628161
    assert _bloom.jhash(b"", 0) == 0xDEADBEEF


@pytest.mark.parametrize("max_entries,k,bits", [(1, 1, 64), (1000, 5, 8192), (4096, 3, 32768), (4096, 15, 131072)])
def test_sizing(max_entries, k, bits):
    assert _bloom.bits_for(max_entries, k) == bits
    b = _bloom.Bloom(4, max_entries, k, 0)
    assert b.bits == bits and b.mask == bits - 1 and b.bytes().nbytes == bits // 8


def test_sizing_cap():
    assert _bloom.bits_for(0xFFFFFFFF, 15) == 1 << 31


def test_single_bit_position():
    b = _bloom.Bloom(4, 1, 1, 5)
    v = bytes([0x0A, 0x00, 0x00, 0x01])
    assert b.positions(v) == [30]
    assert not b.peek(v)
    assert b.push(v) == 0 and b.peek(v)
    want = np.zeros(8, dtype=np.uint8)
    want[3] = 1 << 6  # bit 30: byte 3, bit 6
    assert (b.bytes() == want).all()
    assert b.push(v, flags=1) == -1


def test_members_and_false_positives():
    rng = np.random.default_rng(3)
    pushed = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
    probes = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
    b = _bloom.Bloom(4, 4096, 3, 0xC0FFEE)
    for v in pushed:
        b.push(int(v).to_bytes(4, "little"))
    assert all(b.peek(int(v).to_bytes(4, "little")) for v in pushed)
    members = set(int(v) for v in pushed)
    fp = sum(b.peek(int(v).to_bytes(4, "little")) for v in probes if int(v) not in members)
    print("false positives:", fp)  # 114 of 4096 with this model
    assert 1 <= fp <= 410          # both answers occur; at most 10 % of the probes


def test_merge_bloom():
    a = _bloom.Bloom(4, 1000, 5, 7)
    b = _bloom.Bloom(4, 1000, 5, 7)
    both = _bloom.Bloom(4, 1000, 5, 7)
    for i in range(300):
        v = (i * 2654435761 & 0xFFFFFFFF).to_bytes(4, "little")
        (a if i % 2 else b).push(v)
        both.push(v)
    sa, sb = a.bytes(), b.bytes()
    m = shard.merge_bloom([sa, sb])
    assert (m == (sa | sb)).all() and (m == both.bytes()).all()
    assert (sa == a.bytes()).all()  # the shards are left alone
    assert (shard.merge_bloom([sa]) == sa).all()
    with pytest.raises(ValueError):
        shard.merge_bloom([sa, sb[:-1]])
    with pytest.raises(ValueError):
        shard.merge_bloom([])
