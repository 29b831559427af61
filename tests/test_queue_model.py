"""The QUEUE / STACK model (tests/_queue.py) against hand-written sequences
taken from the maps' rules: FIFO / LIFO order, E2BIG on a full map, BPF_EXIST
dropping the oldest element, ENOENT on an empty one, the flags each entry
point accepts."""
import errno
import importlib.util
import pathlib

import pytest

# (by path: the interpreter has a built-in module named _queue)
_spec = importlib.util.spec_from_file_location("_queue_model", pathlib.Path(__file__).with_name("_queue.py"))
_queue = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_queue)
BPF_EXIST, Ring = _queue.BPF_EXIST, _queue.Ring

V = [bytes([i]) * 4 for i in range(10)]


def test_queue_is_fifo():
    q = Ring(4, 3, lifo=False)
    assert q.pop() == (-1, None) and q.err == errno.ENOENT
    assert q.peek() == (-1, None) and q.delete() == -1
    assert [q.push(V[i]) for i in range(3)] == [0, 0, 0]
    assert q.push(V[3]) == -1 and q.err == errno.E2BIG and q.count() == 3
    assert q.peek() == (0, V[0]) and q.count() == 3
    assert q.pop() == (0, V[0]) and q.pop() == (0, V[1])
    assert q.push(V[4]) == 0  # wraps
    assert q.items == [V[2], V[4]]
    assert q.delete() == 0 and q.lookup() == (0, V[4])
    assert q.pop() == (0, V[4]) and q.pop() == (-1, None)
    assert (q.head, q.tail) == (4, 4)
    img = q.image()
    assert img.size == 128 + 3 * 4 and bytes(img[:16]) == (4).to_bytes(8, "little") * 2 and not img[16:128].any()
    assert bytes(img[128:]) == V[4] + V[1] + V[2]  # ticket 3 wrapped into slot 0


def test_stack_is_lifo():
    s = Ring(4, 3, lifo=True)
    assert [s.push(V[i]) for i in range(3)] == [0, 0, 0]
    assert s.push(V[3]) == -1 and s.err == errno.E2BIG
    assert s.peek() == (0, V[2])
    assert s.pop() == (0, V[2])
    assert s.push(V[5]) == 0 and s.items == [V[0], V[1], V[5]]
    assert [s.pop()[1] for _ in range(3)] == [V[5], V[1], V[0]]
    assert s.pop() == (-1, None) and s.err == errno.ENOENT


@pytest.mark.parametrize("lifo", [False, True])
def test_exist_drops_the_oldest(lifo):
    r = Ring(4, 2, lifo)
    assert r.push(V[0], BPF_EXIST) == 0  # not full: a plain push
    assert r.push(V[1]) == 0
    assert r.push(V[2], BPF_EXIST) == 0
    assert r.items == [V[1], V[2]]  # the queue's head / the stack's bottom went
    assert (r.head, r.tail) == (1, 3)
    assert r.peek() == (0, V[2] if lifo else V[1])


@pytest.mark.parametrize("lifo", [False, True])
def test_flags(lifo):
    r = Ring(4, 1, lifo)
    assert r.push(V[0], 1) == -1 and r.err == errno.EINVAL  # BPF_NOEXIST
    assert r.push(V[0], 7) == -1 and r.err == errno.EINVAL
    assert r.push(None) == -1 and r.err == errno.EINVAL
    assert r.update(None) == -1 and r.err == errno.EINVAL
    assert r.update(V[0], 1) == 0  # update does not validate the flags ...
    assert r.update(V[1], 1) == -1 and r.err == errno.E2BIG  # ... only BPF_EXIST on a full map differs
    assert r.update(V[1], BPF_EXIST) == 0 and r.items == [V[1]]
    assert r.next_key() == -1 and r.err == errno.EINVAL
