"""The planner case library (tests/_dispatch_cases.py) against the oracle
alone: each case runs through orc_sys_dispatch twice, over the records and
over the same records with every thread's calls reversed.

* a case labelled order-sensitive gives different maps or returns (compared
  call by call) -- so a device run in the wrong order CAN differ from the
  oracle, whatever a particular race happens to produce;
* a case labelled insensitive gives identical ones;
* no order-sensitive case is labelled program-major (the labels themselves
  are sound), and both sides of each arm of the rule are present.
"""
import struct

import numpy as np
import pytest

import _dispatch_cases as dc


def _run(po, case, recs):
    po.reset()
    maps = {name: po.OracleMap(t, k, v, mx) for name, t, k, v, mx in dc.MAPS}
    for name in case.prefill:
        for tid in dc.tids(recs):
            assert maps[name].update(struct.pack("<I", tid), struct.pack("<Q", dc.prefill_value(name, int(tid)))) == 0
    o = po.OracleSyscallDispatch()
    for code, nr, enter in case.build({name: m.fd for name, m in maps.items()}):
        assert o.attach(code, nr, enter) > 0
    rets = o.dispatch(recs)
    assert o.failed() == 0
    return rets, {name: m.items() for name, m in maps.items()}


@pytest.fixture(scope="module")
def recs8():
    recs = dc.records(8)
    return recs, dc.reverse_threads(recs)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.id)
def test_order_sensitivity_label(fresh_oracle, recs8, case):
    recs, (rev, src) = recs8
    rets, maps = _run(fresh_oracle, case, recs)
    rets_rev, maps_rev = _run(fresh_oracle, case, rev)
    by_call = np.empty_like(rets_rev)
    by_call[src] = rets_rev  # the reversed run's returns, per original call
    same = maps == maps_rev and (rets == by_call).all()
    assert same != case.sensitive
    # the case does something: a map entry or a return other than the recorded one
    recorded = recs.view(np.int64).reshape(len(recs), 16)[:, 10]
    assert any(maps.values()) or (rets != recorded).any()


def test_reverse_threads_reverses_each_thread():
    recs = dc.records(8)
    rev, src = dc.reverse_threads(recs)
    pid = recs.view(np.uint64).reshape(len(recs), 16)[:, 11]
    assert (rev.view(np.uint64).reshape(len(recs), 16)[:, 11] == pid).all()  # every position keeps its thread
    for p in np.unique(pid):
        at = np.flatnonzero(pid == p)
        assert (src[at] == at[::-1]).all()
    assert sorted(src) == list(range(len(recs)))


def test_labels_are_sound_and_cover_the_rule():
    for c in dc.CASES:
        assert not (c.sensitive and c.plan == 0), c.id
    plans = {c.id: c.plan for c in dc.CASES}
    # the self rule's write arm: a NOEXIST insert on one side, every other write on the other
    # (nor is a NOEXIST insert free of it whose flags or value are constants on one path only)
    assert plans["S-init-add"] == 0 and all(plans[i] == 1 for i in (
        "S-update", "S-update-exist", "S-update-varflags", "S-update-joinflags", "S-init-value", "S-init-joinvalue",
        "S-store", "S-fetch", "S-toggle"))
    # its add-and-load arm: adds alone and loads alone on one side
    assert plans["S-add"] == 0 and plans["S-read"] == 0 and plans["S-load-add"] == 1
    # the pair rule, apart from the self rule
    assert plans["P-read-add-same"] == 1 and plans["P-read-add-disjoint"] == 0
    assert plans["P-add-add-same"] == 0 and plans["P-read-read-same"] == 0
    assert plans["P-init-read-same"] == 1 and plans["P-init-read-disjoint"] == 0
