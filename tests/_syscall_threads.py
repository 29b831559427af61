"""Shared pieces of the thread-ordered syscall dispatch tests
(tests/test_gpu_syscall_threads.py, tests/test_gpu_syscall_many_threads.py and,
on the oracle alone, tests/test_syscall_many_threads_model.py): attaching one
program to the device and the oracle, syscount's latency pair and its maps,
and replay records with an explicit ragged owner assignment.

``dev`` may be None everywhere: the oracle alone, as the CPU-side
preconditions of the many-thread cases run it."""
import numpy as np

from bpftime_amd import gen, isa, programs

from _helpers import make_maps

TRACEPOINT = 5  # BPF_PROG_TYPE_TRACEPOINT
HASH, ARRAY = isa.BPF_MAP_TYPE_HASH, isa.BPF_MAP_TYPE_ARRAY
# common.hpp kSeqAsmThreads: up to this many recorded threads a dispatch that
# no environment variable steers runs its callbacks in the asm tier
SEQ_ASM_THREADS = 16384
PER_THREAD = 8                                           # records per thread, on average
HEAVY, HEAVY_RECORDS = (1, 66, 129), 300                 # three threads of the first waves, among one-record ones


def auto_tier(threads):
    return 1 if threads <= SEQ_ASM_THREADS else 0


def attach(dev, o, code, nr, enter):
    if dev is not None:
        dev.syscall_attach(dev.prog_create(code, "p", TRACEPOINT), nr, enter)
    o.attach(code, nr, enter)


def fds(omaps, dmaps):
    """The maps whose fds the programs name: the device's (the oracle's carry
    the same fds), or the oracle's own without a device."""
    return dmaps if dmaps[0] is not None else omaps


def syscount_all(po, dev, entries=10240, beside=None, **opts):
    """syscount(): (oracle dispatch, the three oracle maps, the three device
    maps).  beside: the device maps of an earlier call, programs attached --
    only the oracle's side is built, fresh maps at the same fds."""
    if beside is None:
        om, dm = make_maps([(HASH, 4, 8, entries), (HASH, 4, 32, entries),
                            (ARRAY, 4, programs.SYSCOUNT_RODATA, 1)], po, dev)
    else:
        om = [po.OracleMap(d.type, d.key_size, d.value_size, d.max_entries, fd=d.fd) for d in beside]
        dm, dev = list(beside), None
    ro = programs.syscount_rodata(measure_latency=True, **opts)
    for m in (om[2], None if beside is not None else dm[2]):
        assert m is None or m.update(b"\0" * 4, ro) == 0
    start, data, rodata = fds(om, dm)
    o = po.OracleSyscallDispatch()
    attach(dev, o, programs.syscount_enter(start.fd, rodata.fd), -1, True)
    attach(dev, o, programs.syscount_exit(data.fd, rodata.fd, start.fd), -1, False)
    return o, om, dm


def syscount(po, dev, entries=10240, **opts):
    """syscount's sys_enter + sys_exit pair with measure_latency
    (example/tracing/syscount/syscount.bpf.c:33-87) on the device and the
    oracle: (oracle dispatch, (ostart, odata), (dstart, ddata))."""
    o, om, dm = syscount_all(po, dev, entries, **opts)
    return o, tuple(om[:2]), tuple(dm[:2])


def thread_of(w):
    """The thread index of each record of (n, 16) int64 / uint64 timed records."""
    return (w[:, 11].astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64) - 2000


def tgid_of(t):
    return 1000 + t // 4


def ragged_owner(threads, rng):
    """PER_THREAD * threads records over exactly `threads` threads, in random
    record order.  By thread index t:
      t % 4 == 0             exactly one record;
      t in HEAVY             HEAVY_RECORDS records: lanes of one wave with very
                             different walk lengths (their neighbours own one);
      t % 64 == 5            two records, both exit / exit_group (EXIT_ONLY);
      t % 64 == 9            two records, both with id -1 (MINUS_ONLY);
      every other thread     one record and a random share of the rest."""
    n = PER_THREAD * threads
    t = np.arange(threads)
    single, exit_only, minus_only = t % 4 == 0, t % 64 == 5, t % 64 == 9
    heavy = np.isin(t, HEAVY)
    plain = ~(single | exit_only | minus_only | heavy)
    counts = np.where(heavy, HEAVY_RECORDS, np.where(exit_only | minus_only, 2, 1))
    rest = n - int(counts.sum())
    assert rest > 0 and heavy.sum() == len(HEAVY) and plain.sum() > 0
    counts = counts + np.bincount(rng.choice(np.flatnonzero(plain), rest), minlength=threads)
    owner = rng.permutation(np.repeat(t, counts))
    assert len(owner) == n
    return owner, exit_only, minus_only


def ragged_records(threads, seed=gen.SEED_CFG5, edit=None):
    """gen.syscall_records_timed with the caller column overwritten by
    ragged_owner's assignment (thread t: tgid 1000 + t // 4, tid 2000 + t, as
    the generator has them; the clocks follow the record index, so they stay
    monotonic within a thread).  edit(w) may change the (n, 16) int64 words
    before the exit-only and id -1 threads get their ids."""
    owner, exit_only, minus_only = ragged_owner(threads, np.random.default_rng(seed % 9973 + threads))
    n = len(owner)
    recs = gen.syscall_records_timed(n, seed=seed)
    w = recs.view(np.int64).reshape(n, 16)
    if edit is not None:
        edit(w)
    w[:, 11] = ((1000 + owner // 4) << 32) | (2000 + owner)
    ex, mi = exit_only[owner], minus_only[owner]
    w[ex, 1] = w[ex, 9] = np.where(np.arange(n)[ex] % 2 == 0, 60, 231)
    w[mi, 1] = w[mi, 9] = -1
    return recs


def assert_shape(recs, threads):
    """What every many-thread case asserts of its records before it touches the
    device: exactly `threads` callers, and the ragged classes are present."""
    n = len(recs)
    w = recs.view(np.int64).reshape(n, 16)
    assert len(np.unique(w[:, 11])) == threads
    per = np.bincount(thread_of(w), minlength=threads)
    assert per.min() >= 1 and (per == 1).sum() >= threads // 4 and (per >= HEAVY_RECORDS).sum() == len(HEAVY)
    dead = np.isin(w[:, 1], [60, 231])
    only_exit = np.bincount(thread_of(w), weights=~dead, minlength=threads) == 0
    only_minus = np.bincount(thread_of(w), weights=w[:, 1] != -1, minlength=threads) == 0
    assert only_exit.sum() >= (threads + 58) // 64 and only_minus.sum() >= (threads + 54) // 64
    return w


def half_full(*omaps):
    """The condition the many-thread cases run under: after the oracle's run no
    hash map holds more than half its max_entries, so no insert races for a
    last free slot."""
    for m in omaps:
        assert 2 * m.count() <= m.max_entries, (m.count(), m.max_entries)


# ---- the many-thread cases (tests/test_gpu_syscall_many_threads.py) ----------

class Case:
    """One attachment set on the oracle and (dev not None) the device, its
    records, and its maps as (oracle map, device map) pairs."""

    def __init__(self, o, recs, pairs):
        self.o, self.recs, self.pairs = o, recs, pairs

    def hash_maps(self):
        return [om for om, _ in self.pairs if om.type == HASH]


def entries_for(threads):
    """Every hash map holds at least 2 x threads entries (data keyed by syscall
    id has up to 337 keys whatever the threads: at least 1024)."""
    return max(2 * threads, 1024)


def build_syscount(po, dev, threads, seed=gen.SEED_CFG5, **opts):
    o, om, dm = syscount(po, dev, entries=entries_for(threads), **opts)
    return Case(o, ragged_records(threads, seed), list(zip(om, dm)))


def build_plain(po, dev, threads, seed=gen.SEED_CFG5):
    """programs.tid_state_enter / tid_state_exit: start[tid] = args[0], read at
    exit and summed into an ARRAY slot."""
    om, dm = make_maps([(HASH, 4, 8, entries_for(threads)), (ARRAY, 4, 16, 1)], po, dev)
    start, total = fds(om, dm)
    o = po.OracleSyscallDispatch()
    attach(dev, o, programs.tid_state_enter(start.fd), -1, True)
    attach(dev, o, programs.tid_state_exit(start.fd, total.fd), -1, False)
    return Case(o, ragged_records(threads, seed), list(zip(om, dm)))


def build_overrides(po, dev, threads, seed=gen.SEED_CFG5):
    """The attachments of test_overrides_and_per_syscall_thread_ordered:
    bpf_override_return at sys_enter_write, bpf_set_retval at sys_exit, the
    tid_state pair and per-syscall counters."""
    from bpftime_amd.isa import Asm
    om, dm = make_maps([(HASH, 4, 8, entries_for(threads)), (ARRAY, 4, 16, 1), (ARRAY, 4, 64, 1)], po, dev)
    start, total, cnt = fds(om, dm)
    counter = lambda slot: (Asm().ld_map_value(2, cnt.fd, 8 * slot).ldx(8, 3, 2, 0).add64(3, 1)  # noqa: E731
                            .stx(8, 2, 0, "r3").mov64(0, 0).exit().assemble())
    o = po.OracleSyscallDispatch()
    for code, nr, enter in [(programs.inject_enter(3, -1), 1, True),        # sys_enter_write: override
                            (programs.tid_state_enter(start.fd), -1, True),
                            (counter(0), 0, True),
                            (programs.tid_state_exit(start.fd, total.fd), -1, False),
                            (programs.exit_clamp(0), -1, False),            # sys_exit: set_retval
                            (counter(1), 0, False),                         # sys_exit_read
                            (counter(2), -1, False)]:
        attach(dev, o, code, nr, enter)

    def edit(w):
        w[::7, 1] = w[::7, 9] = 1
        w[3::97, 1] = w[3::97, 9] = 700                  # past the callback arrays: globals only
    return Case(o, ragged_records(threads, seed, edit), list(zip(om, dm)))


BUILDERS = {"syscount": build_syscount, "plain": build_plain, "overrides": build_overrides}
EDGES = [257, 1025, 4096, SEQ_ASM_THREADS, SEQ_ASM_THREADS + 1]
TWO = [4096, SEQ_ASM_THREADS + 1]
FILTER_TGID = tgid_of(128)                               # threads 128 .. 131: one, HEAVY_RECORDS, and two plain
FILTERS = [(SEQ_ASM_THREADS + 1, {"filter_pid": FILTER_TGID}), (4096, {"filter_failed": True})]
REUSE = [(257, gen.SEED_CFG5), (SEQ_ASM_THREADS + 1, gen.SEED_CFG5), (257, gen.SEED_CFG5 + 1)]
# every (builder, threads, options) a GPU case runs: the CPU-side preconditions run each on the oracle alone
ALL = ([("syscount", t, {}) for t in EDGES] + [("syscount", t, {"count_by_process": True}) for t in TWO]
       + [("syscount", t, kw) for t, kw in FILTERS] + [("syscount", 257, {"seed": gen.SEED_CFG5 + 1})]
       + [("plain", SEQ_ASM_THREADS + 1, {}), ("overrides", 4096, {})])


def case_id(c):
    name, threads, kw = c
    return "-".join([name, str(threads)] + [f"{k}={v}" for k, v in kw.items()])
