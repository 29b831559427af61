"""The stack-trace model (tests/_stacktrace.py) against the reference's rules as
the issue restates them: hash_combine's known answers, fill_stack_trace, the
skip field's edges and bpf_get_stack's byte-count copy.  No GPU."""
import pytest

import _stacktrace as sm

U = sm.USER_STACK


@pytest.mark.parametrize("stack,want", [
    ([], 0xe6546b64),
    ([0], 0xa21166ee20272944),
    ([1, 2, 3], 0x90c7028508862eb4),
    ([0x7f0000001000 + 16 * i for i in range(127)], 0x5a0107a6254843e0),
])
def test_hash_known_answers(stack, want):
    assert sm.hash_stack_trace(stack) == want


def test_create_rules():
    for ks, vs, mx in ((3, 64, 4), (4, 12, 4), (4, 64, 0)):
        with pytest.raises(ValueError):
            sm.StackMap(ks, vs, mx)
    sm.StackMap(4, 0, 1)


def test_fill_rules():
    m = sm.StackMap(4, 64, 1)                           # one slot: every stack collides
    a, b, c = [1, 2, 3], [7, 8, 9], [4, 5]
    assert m.fill(a, False, False) == 0 and m.data[0] == a          # empty: stored
    assert m.fill(b, True, False) == 0 and m.data[0] == a           # same length, other content: "equal", kept
    assert m.fill(c, False, False) == 0 and m.data[0] == a          # other length, no REUSE: kept
    assert m.fill(c, True, True) == 0 and m.data[0] == a            # FAST_CMP: kept even with REUSE
    assert m.fill(c, True, False) == 0 and m.data[0] == c           # other length, REUSE: replaced
    assert m.fill([], True, False) == 0 and m.data[0] == []         # an empty stack is a stack


def test_ids_are_hash_mod_entries():
    m = sm.StackMap(4, 64, 16)
    for stk in ([], [0], [1, 2, 3], [5] * 8):
        assert m.fill(stk, False, False) == sm.hash_stack_trace(stk) % 16


@pytest.mark.parametrize("skip", [0, 3, 4, 255])
def test_skip_edges(skip):
    stack = [10, 11, 12, 13]                            # depth 4: skip 0, depth - 1, depth, 255
    m = sm.StackMap(4, 64, 64)
    want = stack[skip:]
    r = sm.get_stackid(m, stack, U | skip)
    assert r == sm.hash_stack_trace(want) % 64 and m.data[r] == want
    assert sm.get_stack(stack, 64, U | skip) == (0, b"".join(x.to_bytes(8, "little") for x in want)[:len(want)])


def test_error_order():
    m = sm.StackMap(4, 64, 4)
    assert sm.get_stackid(m, None, 0) == sm.ENOTSUP and sm.get_stackid(m, [], 0) == sm.ENOTSUP
    assert sm.get_stackid(m, None, U) == sm.ENOTSUP and sm.get_stackid(m, [], U) == sm.ENOENT
    assert sm.get_stackid(None, [1], U) == sm.EINVAL and not m.data
    assert sm.get_stack([1], 8, U | sm.BUILD_ID)[0] == sm.ENOTSUP and sm.get_stack([], 8, U)[0] == sm.ENOENT
    assert sm.get_stack(None, 8, U)[0] == sm.ENOTSUP and sm.get_stack([1], 8, 0)[0] == sm.ENOTSUP


@pytest.mark.parametrize("size,want", [(0, 0), (5, 5), (8, 6), (64, 6)])
def test_get_stack_copies_min_of_frames_and_size_bytes(size, want):
    stack = [0x1122334455667788 + i for i in range(6)]
    r, out = sm.get_stack(stack, size, U)
    assert r == 0 and len(out) == want and out == (b"".join(x.to_bytes(8, "little") for x in stack))[:want]
    assert sm.get_stack(stack, size, U, range_ok=False) == ((sm.EFAULT, b"") if want else (0, b""))


def test_host_ops():
    m = sm.StackMap(4, 16, 4)
    i = m.fill([9], False, False)
    k = i.to_bytes(4, "little")
    assert m.lookup(k) == (9).to_bytes(8, "little") + bytes(8) and m.lookup(None) is None
    assert m.update(k, b"") == -95 and m.next_key(None) is None
    assert m.delete(k) == 0 and m.delete(k) == -1 and m.lookup(k) is None
