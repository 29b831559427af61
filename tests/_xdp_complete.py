"""A numpy model of bpftime_amd_xdp_complete (include/bpftime_amd.h, DESIGN.md
§6 "XDP completion"), input builders, and the harness that runs the device
call over sentinel-filled buffers and compares every byte with the model.

The model works from the written rules with plain integer arithmetic: per
unit in Python ints (`exact=True`: any 64-bit value), or vectorised in int64
for inputs below 2^61, where nothing can wrap.  The two are checked against
each other in test_xdp_complete_model.py."""
import numpy as np

DESC = np.dtype([("addr", "<u8"), ("len", "<u4"), ("options", "<u4")])
NCLS = 5
ABORTED, DROP, PASS, TX, REDIRECT = range(5)
FRAME_MASK_DEFAULT = (1 << PASS) | (1 << TX) | (1 << REDIRECT)
SENTINEL = 0xA5
_SAFE = 1 << 61


def descs_of(addr, length, options=0):
    d = np.zeros(len(addr), DESC)
    d["addr"], d["len"], d["options"] = addr, length, options
    return d


class Case:
    """The inputs of one call.  descs None: strided mode."""

    def __init__(self, verdicts, stride, umem_bytes, descs=None, off=None, ln=None, frame_mask=FRAME_MASK_DEFAULT,
                 cap=None, gather_mask=0, gather_stride=0, gather_cap=0, umem=None):
        self.verdicts = np.asarray(verdicts, np.uint32)
        self.n = len(self.verdicts)
        self.stride, self.umem_bytes = int(stride), int(umem_bytes)
        self.descs = None if descs is None else np.asarray(descs, DESC)
        self.off = None if off is None else np.asarray(off, np.int32)
        self.ln = None if ln is None else np.asarray(ln, np.uint32)
        self.frame_mask, self.gather_mask = frame_mask, gather_mask
        self.cap = [self.n] * NCLS if cap is None else list(cap)
        self.gather_stride, self.gather_cap = int(gather_stride), int(gather_cap)
        self.umem = umem  # uint8 array: the frames' bytes (gather only)


class Result:
    pass


def _units_exact(c):
    """Per unit, in Python ints: class, confined, list entry, frame start."""
    n = c.n
    cls, confined = np.zeros(n, np.uint32), np.zeros(n, bool)
    entry, start, length = np.zeros(n, DESC), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    for i in range(n):
        a = int(c.descs["addr"][i]) if c.descs is not None else i * c.stride
        o = int(c.off[i]) if c.off is not None else 0
        ln = int(c.ln[i]) if c.ln is not None else int(c.descs["len"][i])
        opt = int(c.descs["options"][i]) if c.descs is not None else 0
        b = a - a % c.stride
        s = a + o
        chunk_in = b + c.stride <= c.umem_bytes
        frame_in = b <= s and s + ln <= b + c.stride
        confined[i] = not (chunk_in and frame_in)
        v = int(c.verdicts[i])
        cls[i] = 0 if confined[i] or v > 4 else v
        length[i] = ln
        if not confined[i]:
            start[i] = s
        if not confined[i] and (c.frame_mask >> int(cls[i])) & 1:
            entry[i] = (s, ln, opt)
        else:
            entry[i] = (b if chunk_in else a, 0, 0)
    return cls, confined, entry, start, length


def _units_fast(c):
    """The same in int64 arrays, for inputs below 2^61 (nothing can wrap)."""
    n = c.n
    addr = c.descs["addr"].astype(np.int64) if c.descs is not None else np.arange(n, dtype=np.int64) * c.stride
    off = c.off.astype(np.int64) if c.off is not None else np.zeros(n, np.int64)
    length = (c.ln if c.ln is not None else c.descs["len"]).astype(np.int64)
    opt = c.descs["options"].astype(np.int64) if c.descs is not None else np.zeros(n, np.int64)
    base = addr - addr % c.stride
    start = addr + off
    chunk_in = base + c.stride <= c.umem_bytes
    frame_in = (base <= start) & (start + length <= base + c.stride)
    confined = ~(chunk_in & frame_in)
    cls = np.where(confined | (c.verdicts > 4), 0, c.verdicts).astype(np.uint32)
    framed = ~confined & (((c.frame_mask >> cls) & 1) == 1)
    entry = np.zeros(n, DESC)
    entry["addr"] = np.where(framed, start, np.where(chunk_in, base, addr)).astype(np.uint64)
    entry["len"] = np.where(framed, length, 0)
    entry["options"] = np.where(framed, opt, 0)
    return cls, confined, entry, np.where(confined, 0, start).astype(np.uint64), length.astype(np.uint32)


def model(c, exact=None):
    """What the call must produce for Case c: .cls, .counts, .lists[k] = (DESC
    entries, u32 unit indices) in full (not clamped), and with a gather
    .g_index, .g_descs, .g_src (umem offsets), .g_count, .g_skipped."""
    if exact is None:
        big = max([c.stride, c.umem_bytes] + ([int(c.descs["addr"].max())] if c.descs is not None and c.n else []))
        exact = big >= _SAFE or c.n * c.stride >= _SAFE
    cls, confined, entry, start, length = (_units_exact if exact else _units_fast)(c)
    r = Result()
    r.cls = cls
    r.counts = [int((cls == k).sum()) for k in range(NCLS)]
    r.lists = []
    for k in range(NCLS):
        idx = np.flatnonzero(cls == k)
        r.lists.append((entry[idx], idx.astype(np.uint32)))
    if c.gather_stride:
        wanted = ~confined & (((c.gather_mask >> cls) & 1) == 1)
    else:
        wanted = np.zeros(c.n, bool)
    fits = length.astype(np.int64) <= c.gather_stride
    g = np.flatnonzero(wanted & fits)
    r.g_index = g.astype(np.uint32)
    r.g_count, r.g_skipped = len(g), int((wanted & ~fits).sum())
    r.g_descs = np.zeros(len(g), DESC)
    r.g_descs["addr"] = np.arange(len(g), dtype=np.uint64) * np.uint64(max(c.gather_stride, 0))
    r.g_descs["len"] = length[g]
    r.g_descs["options"] = c.descs["options"][g] if c.descs is not None else 0
    r.g_src = start[g]
    return r


def list_image(entries, cap, slots, dtype):
    """A buffer of `slots` elements, sentinel-filled, holding the first `cap`
    of `entries`: what the device buffer must look like afterwards."""
    img = np.full(slots * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype)
    k = min(len(entries), cap)
    img[:k] = entries[:k]
    return img


def gather_image(c, r, slots):
    img = np.full(slots * c.gather_stride, SENTINEL, np.uint8)
    for k in range(min(r.g_count, c.gather_cap)):
        ln = int(r.g_descs["len"][k])
        src = int(r.g_src[k])
        img[k * c.gather_stride:k * c.gather_stride + ln] = c.umem[src:src + ln]
    return img


# ---------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------
def pattern(name, n, rng):
    """Seeded verdict patterns (u32[n])."""
    if name.startswith("all"):
        return np.full(n, int(name[3:]), np.uint32)
    if name == "alternate":
        return np.where(np.arange(n) % 2 == 0, TX, DROP).astype(np.uint32)
    if name == "tx16":
        return np.where(rng.integers(0, 16, n) == 0, TX, DROP).astype(np.uint32)
    if name == "uniform7":
        return rng.integers(0, 7, n).astype(np.uint32)
    if name == "no_pass":
        return rng.choice(np.array([ABORTED, DROP, TX, REDIRECT], np.uint32), n)
    raise ValueError(name)


def shuffled_ring(n, rng, chunk=2048, length=64):
    """Descriptors in non-address order over a umem of n + 8 chunks: frames at
    chunk + 256 (XDP_PACKET_HEADROOM), every fifth at chunk + 2 (NET_IP_ALIGN),
    options = a tag of the unit."""
    chunks = rng.permutation(n + 8)[:n].astype(np.uint64)
    head = np.where(np.arange(n) % 5 == 3, 2, 256).astype(np.uint64)
    lens = np.full(n, length, np.uint32) if np.isscalar(length) else np.asarray(length, np.uint32)
    return (n + 8) * chunk, descs_of(chunks * np.uint64(chunk) + head, lens, (np.arange(n) * 7 + 1) & 0xFFFF)


# ---------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------
PAD = 3  # sentinel entries kept behind every output buffer


def launch(dev, c, out_null=(), index_null=(), stream=0, sync=True, gather_host=None, bufs=None):
    """Queues the call for Case c with sentinel-filled outputs; collect() reads
    what it left.  `bufs`: device inputs to use instead of uploading c's."""
    D = dev.DeviceBuffer
    sent = lambda nbytes: D.from_array(np.full(max(nbytes, 1), SENTINEL, np.uint8))  # noqa: E731
    if bufs is None:
        bufs = upload_inputs(dev, c)
    h = Result()
    h.dev, h.c, h.stream, h.sync, h.gather_host, h.bufs = dev, c, stream, sync, gather_host, bufs
    h.outs = [None if k in out_null else sent((c.cap[k] + PAD) * 16) for k in range(NCLS)]
    h.idxs = [None if k in index_null else sent((c.cap[k] + PAD) * 4) for k in range(NCLS)]
    h.counts = sent(4 * (NCLS + PAD))
    h.g = {}
    gslots = c.gather_cap + PAD
    if c.gather_stride:
        h.g["gather"] = gather_host if gather_host is not None else sent(gslots * c.gather_stride)
        h.g["gather_descs"], h.g["gather_index"] = sent(gslots * 16), sent(gslots * 4)
        h.g["gather_count"], h.g["gather_skipped"] = sent(4 * (1 + PAD)), sent(4 * (1 + PAD))
    h.ret = dev.xdp_complete(c.n, bufs["verdicts"], c.stride, c.umem_bytes, descs=bufs["descs"],
                             data_off_out=bufs["off"], len_out=bufs["ln"], umem=bufs["umem"], out=h.outs,
                             index_out=h.idxs, cap=c.cap, frame_mask=c.frame_mask, counts=h.counts,
                             gather_stride=c.gather_stride, gather_cap=c.gather_cap, gather_mask=c.gather_mask,
                             stream=stream, sync=sync, **h.g)
    return h


def collect(h):
    """What the device left: dict(ret=(host totals or None), dev_counts,
    out[k], index[k], gather, g_descs, g_index, g_count, g_skipped) as numpy
    arrays (None where the pointer was NULL)."""
    if not h.sync:
        assert h.dev.lib().bpftime_amd_stream_sync(h.stream or None) == 0
    got = {"ret": h.ret, "dev_counts": h.counts.download(np.uint32),
           "out": [None if b is None else b.download().view(DESC) for b in h.outs],
           "index": [None if b is None else b.download(np.uint32) for b in h.idxs]}
    if h.c.gather_stride:
        got["gather"] = None if h.gather_host is not None else h.g["gather"].download()
        got["g_descs"] = h.g["gather_descs"].download().view(DESC)
        got["g_index"] = h.g["gather_index"].download(np.uint32)
        got["g_count"] = h.g["gather_count"].download(np.uint32)
        got["g_skipped"] = h.g["gather_skipped"].download(np.uint32)
    return got


def run_device(dev, c, **kw):
    return collect(launch(dev, c, **kw))


def upload_inputs(dev, c):
    D = dev.DeviceBuffer
    up = lambda a: None if a is None else D.from_array(a)  # noqa: E731
    return {"verdicts": up(c.verdicts) if c.n else D(4), "descs": up(c.descs), "off": up(c.off), "ln": up(c.ln),
            "umem": up(c.umem)}


def same(a, b):
    """Bit for bit, structured arrays included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(c, got, r=None, out_null=(), index_null=()):
    """Every byte of every output buffer against the model."""
    r = r or model(c)
    sent32 = np.full(PAD, SENTINEL * 0x01010101, np.uint32)
    if got["ret"] is not None:
        totals = got["ret"][0] if c.gather_stride else got["ret"]
        assert totals == r.counts, (totals, r.counts)
        if c.gather_stride:
            assert got["ret"][1:] == (r.g_count, r.g_skipped), (got["ret"], r.g_count, r.g_skipped)
    assert same(got["dev_counts"], np.concatenate([np.array(r.counts, np.uint32), sent32])), got["dev_counts"]
    for k in range(NCLS):
        entries, idx = r.lists[k]
        assert (np.diff(idx.astype(np.int64)) > 0).all() and same(idx, np.flatnonzero(r.cls == k).astype(np.uint32))
        if k in out_null:
            assert got["out"][k] is None
        else:
            want = list_image(entries, c.cap[k], c.cap[k] + PAD, DESC)
            assert same(got["out"][k], want), (k, _first_diff(got["out"][k], want))
        if k in index_null:
            assert got["index"][k] is None
        else:
            want = list_image(idx, c.cap[k], c.cap[k] + PAD, np.uint32)
            assert same(got["index"][k], want), (k, _first_diff(got["index"][k], want))
    if c.gather_stride:
        slots = c.gather_cap + PAD
        assert same(got["g_count"], np.concatenate([np.array([r.g_count], np.uint32), sent32])), got["g_count"]
        assert same(got["g_skipped"], np.concatenate([np.array([r.g_skipped], np.uint32), sent32])), got["g_skipped"]
        want = list_image(r.g_descs, c.gather_cap, slots, DESC)
        assert same(got["g_descs"], want), _first_diff(got["g_descs"], want)
        want = list_image(r.g_index, c.gather_cap, slots, np.uint32)
        assert same(got["g_index"], want), _first_diff(got["g_index"], want)
        if got["gather"] is not None:
            want = gather_image(c, r, slots)
            assert same(got["gather"], want), _first_diff(got["gather"], want)
    return r


def _first_diff(a, b):
    a, b = a.view(np.uint8), b.view(np.uint8)
    d = np.flatnonzero(a != b)
    return f"{len(d)} bytes differ, first at byte {int(d[0])}: got {int(a[d[0]])}, want {int(b[d[0]])}" if len(d) else ""
