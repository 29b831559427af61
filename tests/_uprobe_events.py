"""Builders for the event-list uprobe replay's tests
(bpftime_amd_uprobe_dispatch_events): recorded traces with nested and recursive
calls, the model that runs an event list, and the call-depth program pair.

An event is the word (record << 1) | phase.  EventModel.dispatch_events runs
um.Model.dispatch's loop body once per event, in list order: the serial
reference run (frida's on_enter / on_leave on the calling thread,
frida_internal_attach_entry.cpp:221-239).  The parallel device run equals it for
programs that write per-thread keys only and touch shared words only by atomic
adds, as every pair here and in tests/_uprobe_threads.py does (the `plain`
histogram variant is for ORDERED dispatches)."""
import numpy as np

from bpftime_amd import isa
from bpftime_amd.isa import Asm

import _uprobe as um
import _uprobe_threads as ut

M64 = um.M64
SLOTS = 32
F0, F1, F2 = um.FUNCS


def event(record, phase):
    return (record << 1) | (phase & 1)


def flat_events(n):
    """E(0,0), E(0,1), E(1,0), E(1,1), ...: every record one call, nothing nested."""
    return np.arange(2 * n, dtype=np.uint32)


class EventModel(um.Model):
    def dispatch_events(self, events, func, enter=None, leave=None, pid_tgid=None, clock=None, out_state=None,
                        out_rets=None, default_pid=0, default_clock=0):
        """Runs every event in list order; returns the failed callbacks.  The
        body is um.Model.dispatch's, per (record, phase) instead of per call."""
        failed = 0
        for w in events:
            i, phase = int(w) >> 1, int(w) & 1
            f = func[i]
            cbs = self.running(int(f))[phase]
            regs = (enter, leave)[phase]
            for a in cbs:
                ovr = a["kind"] in (um.OVERRIDE, um.UREPLACE)
                e = um.Env(np.array(regs[i], dtype=np.uint64), 0 if ovr else int(f), a["cookie"] or 0,
                           int(pid_tgid[i]) if pid_tgid is not None else default_pid,
                           int(clock[i][phase]) if clock is not None else default_clock, None, ovr)
                try:
                    r0 = a["prog"](e)
                except um.Failed:
                    failed += 1
                    continue
                if a["kind"] == um.UREPLACE:
                    e.overridden = r0 & M64
                if e.overridden is not None:
                    out_state[i] |= 1
                    out_rets[i] = np.uint64(e.overridden).astype(np.int64)
        return failed


# ---- the call-depth pair -----------------------------------------------------------
def depth_entry(depth_fd, by_fd, depth, bydepth):
    """d = depth[tid] (0 when absent); depth[tid] = d + 1; bydepth[min(d, 31)] += 1
    (a 32-bit atomic add): how deep inside probed calls each probed call began."""
    a = Asm()
    ut._tid_to_stack(a)
    a.mov64(2, "r10").add64(2, -4).ld_map_fd(1, depth_fd).call(isa.BPF_FUNC_map_lookup_elem)
    ut._seq_count(a)                                    # r7 = d
    a.mov64(1, "r7").add64(1, 1).stx(8, 10, -16, 1)
    a.mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, depth_fd).call(isa.BPF_FUNC_map_update_elem)
    a.jmp("jle", 7, SLOTS - 1, "fits").mov64(7, SLOTS - 1).label("fits")
    a.st(4, 10, -8, 0)
    a.mov64(2, "r10").add64(2, -8).ld_map_fd(1, by_fd).call(isa.BPF_FUNC_map_lookup_elem)
    a.jmp("jeq", 0, 0, "out")
    a.alu64("lsh", 7, 2).add64(0, "r7")
    a.mov64(1, 1).atomic(4, isa.ATOMIC_ADD, 0, 0, 1)
    a.label("out").mov64(0, 0)

    def py(e):
        tid = e.pid_tgid & 0xFFFFFFFF
        d = depth.get(tid, 0)
        depth[tid] = (d + 1) & M64
        bydepth[min(d, SLOTS - 1)] += 1
        return 0
    return a.exit().assemble(), py


def depth_return(depth_fd, depth):
    """depth[tid] -= 1 when present (a return whose entry was never seen on a
    thread without any entry changes nothing; below 0 the u64 wraps)."""
    a = Asm()
    ut._tid_to_stack(a)
    a.mov64(2, "r10").add64(2, -4).ld_map_fd(1, depth_fd).call(isa.BPF_FUNC_map_lookup_elem)
    a.jmp("jeq", 0, 0, "out")
    a.ldx(8, 1, 0, 0).add64(1, -1).stx(8, 10, -16, 1)
    a.mov64(2, "r10").add64(2, -4).mov64(3, "r10").add64(3, -16).mov64(4, isa.BPF_ANY)
    a.ld_map_fd(1, depth_fd).call(isa.BPF_FUNC_map_update_elem)
    a.label("out").mov64(0, 0)

    def py(e):
        tid = e.pid_tgid & 0xFFFFFFFF
        if tid in depth:
            depth[tid] = (depth[tid] - 1) & M64
        return 0
    return a.exit().assemble(), py


# ---- traces -------------------------------------------------------------------------
def _owners(n, threads, rng):
    """The thread of each of n calls, with ut.records' skew: thread 0 owns about
    half the calls, the upper half of the threads exactly one each, every
    thread at least one.  At most n // 2 threads: with a call per thread, as
    ut.records has it for n == threads, nothing could nest."""
    threads = max(1, min(threads, n // 2))
    lower = max(threads // 2, 1)
    upper = np.arange(lower, threads)
    spots = rng.permutation(n)
    owner = np.zeros(n, dtype=np.int64)
    owner[spots[:len(upper)]] = upper
    rest = spots[len(upper):]
    mine = np.where(rng.random(len(rest)) < 0.5, 0, rng.integers(0, lower, len(rest)))
    mine[:lower] = np.arange(lower)
    owner[rest] = mine
    return owner


def traces(n, threads, seed=91, max_depth=5):
    """ut.records' fields for n calls by min(threads, n // 2) recorded threads
    (_owners: ut.records' skew), plus `events`: a uint32 event list in recorded
    order.

    Per thread the calls nest properly, at most max_depth deep: a thread's
    records are entered in record order, and before each entry some of the
    calls open on the thread return.  A call inside another is the outer one's
    function again with probability 0.4 (direct recursion), else any of
    um.FUNCS + (um.NOBODY,).  With six or more calls, thread 0 begins F0 -> F0
    -> F0 -> F1: recursion three deep and F1 called inside F0.  The threads are
    interleaved at random, each keeping its own order, and the clocks increase
    strictly along the list (a step is 2^k + noise ns, k in 0..28: durations over many
    steps reach every histogram slot, the clamp included); the clock
    of an event that is not in the list is 0.

    Unpaired records (n >= 64; at most n // 16 in all, at least one of each
    kind), all on thread 0: its first record was entered before the recording
    began (return only; the forced chain runs inside it), and the calls still
    open at its end never return (entry only; calls return before the end
    until no more are open than the cap leaves).  `ret_only` / `ent_only` list
    them."""
    r = ut.records(n, threads, seed=seed)
    rng = np.random.default_rng(seed + 131 * n + threads)
    owner = _owners(n, threads, rng)
    r["owner"] = owner
    r["pid"] = np.array([(ut.tgid_of(t) << 32) | ut.tid_of(t) for t in owner], dtype=np.uint64)
    funcs = um.FUNCS + (um.NOBODY,)
    func = np.zeros(n, dtype=np.uint64)
    cap = n // 16 if n >= 64 else 0
    ret_only, ent_only, per_thread = [], [], []
    for t in sorted(set(int(x) for x in owner)):
        recs = [int(i) for i in np.flatnonzero(owner == t)]
        unpaired = t == 0 and cap >= 2
        forced, after = {}, None
        if t == 0 and len(recs) >= 6:
            first = 1 if unpaired else 0
            forced = {recs[first + j]: f for j, f in enumerate((F0, F0, F0, F1))}
            after = recs[first + 4]                     # the call after the chain: everything open returns first
        ev, stack = [], []
        for j, i in enumerate(recs):
            if i in forced:
                pops = 0
            elif forced and i == after:
                pops = len(stack)
            else:
                pops = int(rng.integers(0, len(stack) + 1))
                pops = max(pops, len(stack) - (max_depth - 1))
            for _ in range(pops):
                ev.append(event(stack.pop(), 1))
            if i in forced:
                func[i] = forced[i]
            elif stack and rng.random() < 0.4:
                func[i] = func[stack[-1]]
            else:
                func[i] = funcs[int(rng.integers(0, len(funcs)))]
            stack.append(i)
            if unpaired and j == 0:
                ret_only.append(i)                      # entered before the recording began
            else:
                ev.append(event(i, 0))
        keep = min(len(stack), cap - len(ret_only)) if unpaired else 0
        if unpaired and stack and stack[0] == recs[0]:
            keep = 0                                    # (the return-only call returns: it is in the list)
        while len(stack) > keep:
            ev.append(event(stack.pop(), 1))
        ent_only += stack                               # never returned
        per_thread.append(ev)
    # a random interleaving that keeps every thread's own order
    turn = np.repeat(np.arange(len(per_thread)), [len(ev) for ev in per_thread])
    rng.shuffle(turn)
    at = [0] * len(per_thread)
    events = np.zeros(len(turn), dtype=np.uint32)
    clock = np.zeros((n, 2), dtype=np.uint64)
    step = (np.uint64(1) << rng.integers(0, 29, len(turn)).astype(np.uint64)) + \
        rng.integers(0, 3, len(turn)).astype(np.uint64)
    now = 1000
    for k, t in enumerate(turn):
        w = per_thread[t][at[t]]
        at[t] += 1
        events[k] = w
        now += int(step[k])
        clock[w >> 1, w & 1] = now
    r["func"], r["clock"], r["events"] = func, clock, events
    r["ret_only"], r["ent_only"] = sorted(ret_only), sorted(ent_only)
    return r


def depth_profile(r):
    """Checks that every thread's events nest properly (a return closes the
    innermost open call; a return-only record closes nothing seen) and returns
    the deepest nesting any thread reaches."""
    open_, seen_entry, deepest = {}, set(), 0
    for w in r["events"]:
        i, phase = int(w) >> 1, int(w) & 1
        st = open_.setdefault(int(r["owner"][i]), [])
        if phase == 0:
            assert i not in seen_entry
            seen_entry.add(i)
            st.append(i)
            deepest = max(deepest, len(st))
        elif i in seen_entry:
            assert st and st[-1] == i, "a return that does not close the innermost open call"
            st.pop()
        else:
            assert not st, "a return-only record returns while a call recorded inside it is open"
    return deepest
