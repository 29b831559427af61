"""bench.py --dump-outputs: the sample of units it writes is a function of the
batch size alone (two builds run with the same arguments dump the same
units), stays inside the batch and under the size the dump may have."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_blocks_small_batch_is_whole():
    assert bench.dump_blocks(1000, 64) == [0]
    assert bench.dump_blocks(64 * bench.DUMP_BLOCK, 64) == [b * bench.DUMP_BLOCK for b in range(64)]
    assert bench.dump_blocks(2 * bench.DUMP_BLOCK + 1, 64) == [0, bench.DUMP_BLOCK, 2 * bench.DUMP_BLOCK]


def test_dump_blocks_sample_is_fixed_and_in_bounds():
    n = 1 << 24
    for nblocks in (bench.DUMP_PACKET_BLOCKS, bench.DUMP_VERDICT_BLOCKS):
        a, b = bench.dump_blocks(n, nblocks), bench.dump_blocks(n, nblocks)
        assert a == b and len(a) == nblocks and a == sorted(set(a))
        assert all(u % bench.DUMP_BLOCK == 0 and 0 <= u <= n - bench.DUMP_BLOCK for u in a)
    # a batch that is no multiple of the block: the last block may be short, never past the end
    assert max(bench.dump_blocks((1 << 20) + 5, 2000)) < (1 << 20) + 5


def test_dump_stays_under_64_mb():
    per_unit = 4 * (bench.DUMP_VERDICT_BLOCKS + bench.PKT * bench.DUMP_PACKET_BLOCKS) * bench.DUMP_BLOCK
    assert per_unit + 8 * 512 < 64 * 1000 * 1000
