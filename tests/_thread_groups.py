"""Key sets and the numpy reference for the tests of the thread grouping
(csrc/group.hip bpftime_amd_group_threads; tests/test_gpu_thread_groups.py on
the device, tests/test_syscall_many_threads_model.py for the reference alone).

The reference is np.argsort(keys, kind="stable") over the uint64 keys: perm is
that argsort, a segment starts wherever the sorted keys change."""
import numpy as np

# include/bpftime_amd.h: the caller's u64 pid_tgid lies at +88 of a 96- / 128-B
# replay record, and at +24 of a struct-of-arrays exit record (32 B: the 24-B
# trace_event_raw_sys_exit, then the pid_tgid)
AOS_TIMED = (128, 88)
SOA_EXIT = (32, 24)

NS = [1, 2, 255, 256, 257, 1031, (1 << 16) + 3, (1 << 20) + 1]
BIG = [n for n in NS if n > 1 << 16]
K0 = np.uint64((1003 << 32) | 2014)                      # an ordinary pid_tgid
TOP = np.uint64(1 << 63)


def pid_tgid(t):
    """gen.syscall_records_timed's scheme: thread t is tgid 1000 + t // 4, tid 2000 + t."""
    t = np.asarray(t, dtype=np.uint64)
    return ((np.uint64(1000) + t // np.uint64(4)) << np.uint64(32)) | (np.uint64(2000) + t)


def ragged_owner(n, threads, rng, heavy=3):
    """n records over exactly `threads` threads: every thread one record, the
    first `heavy` threads a tenth of the records each, the rest spread at
    random over the upper half of the threads -- so the lower half (but the
    heavy ones) own exactly one record each.  In random record order."""
    assert n >= threads + heavy * (n // 10)
    owner = [np.arange(threads), np.repeat(np.arange(heavy), n // 10 - 1)]
    rest = n - threads - heavy * (n // 10 - 1)
    owner.append(rng.integers(threads // 2, threads, rest))
    owner = rng.permutation(np.concatenate(owner))
    assert len(owner) == n
    return owner


def _few(n, rng):
    """Thread ids for sorted / reverse / contiguous key sets: up to 300 threads, ragged."""
    threads = min(n, 300)
    return np.concatenate([np.arange(threads), rng.integers(0, threads, n - threads) ** 2 // max(threads, 1)])


def one_thread(n, rng):
    return np.full(n, K0, dtype=np.uint64)


def distinct(n, rng):
    # multiplying by an odd constant is a bijection of u64: n distinct keys over all 64 bits
    return rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)


def bit63(n, rng):
    return K0 | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))


def bit0(n, rng):
    return K0 ^ rng.integers(0, 2, n).astype(np.uint64)


def high_word(n, rng):
    """Equal tids, 37 tgids up to bit 31 of the high word."""
    tg = rng.integers(0, 1 << 32, 37).astype(np.uint64)
    return (tg[rng.integers(0, 37, n)] << np.uint64(32)) | np.uint64(2014)


def low_word(n, rng):
    """One tgid, 53 tids up to bit 31 of the low word."""
    td = rng.integers(0, 1 << 32, 53).astype(np.uint64)
    return (np.uint64(1003) << np.uint64(32)) | td[rng.integers(0, 53, n)]


def unsigned_mix(n, rng):
    """Keys at or above 2^63 among small ones: a signed order would put them first."""
    edge = np.array([0, 1, 2, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1, (1 << 64) - 2, 1 << 32,
                     (1 << 32) - 1], dtype=np.uint64)
    pool = np.concatenate([edge, rng.integers(0, 1 << 20, 20).astype(np.uint64),
                           TOP | rng.integers(0, 1 << 62, 20).astype(np.uint64)])
    return pool[rng.integers(0, len(pool), n)]


def presorted(n, rng):
    return np.sort(pid_tgid(_few(n, rng)))


def reverse_sorted(n, rng):
    return np.sort(pid_tgid(_few(n, rng)))[::-1].copy()


def contiguous(n, rng):
    """Each thread's records side by side, the threads in random order."""
    t = _few(n, rng)
    order = rng.permutation(int(t.max()) + 1)
    return pid_tgid(order[np.sort(t)])


def ragged(threads):
    def f(n, rng):
        return pid_tgid(ragged_owner(n, threads, rng))
    f.__name__ = f"ragged{threads}"
    return f


# (builder, the n it runs at, the distinct keys it has at n or None: whatever numpy counts)
SETS = [(one_thread, NS, lambda n: 1),
        (distinct, NS, lambda n: n),
        (ragged(4096), BIG, lambda n: 4096),
        (ragged(16385), BIG, lambda n: 16385),
        (ragged(65537), BIG[1:], lambda n: 65537),
        (bit63, NS[1:], None),
        (bit0, NS[1:], None),
        (high_word, NS[1:], None),
        (low_word, NS[1:], None),
        (unsigned_mix, NS[1:], None),
        (presorted, NS[1:], lambda n: min(n, 300)),
        (reverse_sorted, NS[1:], lambda n: min(n, 300)),
        (contiguous, NS[1:], lambda n: min(n, 300))]
CASES = [(f, n, want) for f, ns, want in SETS for n in ns]
IDS = [f"{f.__name__}-{n}" for f, n, _ in CASES]


def keys_of(f, n):
    keys = f(n, np.random.default_rng(1000003 * n + len(f.__name__)))
    assert keys.dtype == np.uint64 and keys.shape == (n,)
    return keys


def reference(keys):
    """(perm, seg): the stable argsort, and the run heads of the sorted keys with n appended."""
    perm = np.argsort(keys, kind="stable")
    heads = np.flatnonzero(np.diff(keys[perm])) + 1
    return perm.astype(np.uint32), np.concatenate([[0], heads, [len(keys)]]).astype(np.uint32)


def _around(keys, perm, at):
    lo, hi = max(at - 2, 0), min(at + 3, len(perm))
    return ", ".join(f"[{j}] rec {int(perm[j])} key {int(keys[perm[j]]):#018x}" for j in range(lo, hi))


def check(keys, perm, seg, nseg):
    """Holds a grouping against the reference: every assertion names the first
    differing position and the keys around it."""
    n = len(keys)
    want_perm, want_seg = reference(keys)
    assert perm.shape == (n,), f"perm has {perm.shape} entries for {n} records"
    bad = np.flatnonzero(perm != want_perm)
    assert not len(bad), (f"perm differs from the stable argsort first at {int(bad[0])} ({len(bad)} places): got "
                          f"{_around(keys, np.minimum(perm, n - 1), int(bad[0]))}; want "
                          f"{_around(keys, want_perm, int(bad[0]))}")
    distinct_keys = len(np.unique(keys))
    assert nseg == distinct_keys, f"nseg {nseg}, {distinct_keys} distinct keys"
    assert seg.shape == (nseg + 1,)
    assert seg[0] == 0 and seg[nseg] == n, f"seg[0] = {int(seg[0])}, seg[nseg] = {int(seg[nseg])}, n = {n}"
    flat = np.flatnonzero(np.diff(seg.astype(np.int64)) <= 0)
    assert not len(flat), (f"seg is not strictly increasing at {int(flat[0])}: "
                           f"{[int(x) for x in seg[max(int(flat[0]) - 1, 0):int(flat[0]) + 3]]}")
    bad = np.flatnonzero(seg != want_seg)
    assert not len(bad), (f"seg differs from the run heads first at {int(bad[0])}: got {int(seg[bad[0]])}, want "
                          f"{int(want_seg[bad[0]])}; sorted keys there: "
                          f"{_around(keys, want_perm, int(want_seg[bad[0]]) if want_seg[bad[0]] < n else n - 1)}")


def strided(keys, stride, offset, rng):
    """The keys inside records of `stride` bytes at `offset`, noise everywhere else."""
    n = len(keys)
    raw = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    raw[:, offset:offset + 8] = keys.view(np.uint8).reshape(n, 8)
    return raw
