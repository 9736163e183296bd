"""Inputs, file format and references shared by tests/test_device_units.py and tests/test_sum_carries.py.

The device-unit driver (tests/device_units.hip, built as reconcile-rs_amd/examples/device_units) runs
the library's device functions and launchers on the cases written here; its host-only companion
(tests/round_decide_host.cpp) runs the host tier's decide_segment on the round cases of the same
file.  The formats are tests/device_units_io.hpp's.

Every expected value is computed here with Python integers mod 2^256 (sums, prefixes) or with numpy's
IEEE float32 square root and oracle/rbsr.py's policies (round decisions); nothing is taken from the
code under test.
"""
from __future__ import annotations

import itertools
import os
import struct

import numpy as np

import rbsr as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "reconcile-rs_amd", "examples", "device_units")
HOST_SRC = os.path.join(ROOT, "tests", "round_decide_host.cpp")
M256 = 1 << 256
ONES = M256 - 1
F32 = 0xFFFFFFFF

(OP_ROUND, OP_ROUND_SPANS, OP_FP_ADDSUB, OP_ACC_SEQ, OP_ACC_WAVE, OP_ACC_BLOCK, OP_BLOCK_SUM, OP_REDUCE, OP_TOTAL,
 OP_RANGE, OP_PREFIX, OP_BLOCK_PREFIX) = range(1, 13)


# ---- 256-bit values as rows of 32 little-endian bytes ----------------------------------------------
def rows_of(ints) -> np.ndarray:
    """Python integers (mod 2^256) -> (k, 32) uint8."""
    ints = list(ints)
    return np.frombuffer(b"".join((v % M256).to_bytes(32, "little") for v in ints), np.uint8).reshape(len(ints), 32)


def ints_of(rows) -> list:
    """(k, 32) uint8 (or raw bytes) -> Python integers."""
    b = rows.tobytes() if isinstance(rows, np.ndarray) else bytes(rows)
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def limbs(*ls) -> int:
    return sum((x & F32) << (32 * i) for i, x in enumerate(ls))


def agg_ints(out) -> list:
    """(r, 5) u64 aggregates {u64 fp[4]; u64 size} -> [(fingerprint, size)]."""
    a = np.asarray(out).reshape(-1, 5).view(np.uint64)
    return [(sum(int(x) << (64 * i) for i, x in enumerate(r[:4])), int(r[4])) for r in a]


FIVE = (0, 1, 0x7FFFFFFF, 0x80000000, F32)


def adversarial_values(seed: int = 11, mixed: int = 40) -> list:
    """zero, one, all-ones, 2^255, each single limb all-ones, limbs 0..j all-ones, alternating
    all-ones / zero limbs (both phases), and `mixed` values with limbs from FIVE."""
    v = [0, 1, ONES, 1 << 255]
    v += [F32 << (32 * j) for j in range(8)]
    v += [(1 << (32 * (j + 1))) - 1 for j in range(8)]
    v += [limbs(*[F32 if (i + p) % 2 == 0 else 0 for i in range(8)]) for p in (0, 1)]
    rng = np.random.default_rng(seed)
    v += [limbs(*[FIVE[int(k)] for k in rng.integers(0, 5, 8)]) for _ in range(mixed)]
    return v


def pattern(name: str, n: int) -> np.ndarray:
    """(n, 32) uint8 rows; every pattern at n is a prefix of itself at a larger n.
    P1 all-ones rows; P2 all-ones and one alternating (each pair cancels through a full-length carry);
    P3 row i has limb i mod 8 all-ones; P4 limbs drawn from FIVE; P5 random bytes."""
    if name == "P1":
        return np.full((n, 32), 0xFF, np.uint8)
    if name == "P2":
        a = np.zeros((n, 32), np.uint8)
        a[0::2] = 0xFF
        a[1::2, 0] = 1
        return a
    if name == "P3":
        a = np.zeros((n, 8), np.uint32)
        a[np.arange(n), np.arange(n) % 8] = F32
        return a.view(np.uint8).reshape(n, 32)
    if name == "P4":
        rng = np.random.default_rng(4)
        return np.array(FIVE, np.uint32)[rng.integers(0, 5, (n, 8))].view(np.uint8).reshape(n, 32)
    if name == "P5":
        return np.random.default_rng(5).integers(0, 256, (n, 32), dtype=np.uint8)
    raise KeyError(name)


PATTERNS = ("P1", "P2", "P3", "P4", "P5")


def prefix_ints(vals) -> list:
    """[Σ vals[0..i) mod 2^256 for i in 0..len]."""
    return [0] + [x % M256 for x in itertools.accumulate(vals)]


def block_sums(vals, width: int = 256) -> list:
    return [sum(vals[i:i + width]) % M256 for i in range(0, len(vals), width)]


def with_stride40(rows: np.ndarray, order=None, nrec=None) -> np.ndarray:
    """Records of 40 bytes: the 32-byte value first, then 8 bytes no sum may read (0xEE).  order[i]:
    the record slot of row i among nrec >= n slots (unused slots hold 0xEE throughout)."""
    n = rows.shape[0]
    nrec = n if nrec is None else nrec
    rec = np.full((nrec, 40), 0xEE, np.uint8)
    rec[np.arange(n) if order is None else order, :32] = rows
    return rec


# ---- the rank bounds of the range queries --------------------------------------------------------
RANGE_N = 131_372


def range_bounds(n: int = RANGE_N):
    """All 144 (lo, hi) pairs; the first 28 cover super-block 1 whole with ragged block and row edges
    on both sides (lo <= 65,536 and hi >= 131,072), so a prefix of any length >= 28 holds them."""
    vals = [0, 1, 255, 256, 257, 65_535, 65_536, 65_537, 131_072, n - 1, n, n + 50]
    pairs = [(lo, hi) for lo in vals for hi in vals]
    first = [p for p in pairs if p[0] <= 65_536 and p[1] >= 131_072]
    rest = [p for p in pairs if p not in first]
    pairs = first + rest
    assert len(pairs) == 144 and len(first) == 28
    return pairs


def range_expected(pre: list, n: int, pairs) -> list:
    out = []
    for lo, hi in pairs:
        hi = min(hi, n)
        lo = min(lo, hi)
        out.append(((pre[hi] - pre[lo]) % M256, hi - lo))
    return out


# ---- round decisions ----------------------------------------------------------------------------
def f32_sqrt_trunc(spans) -> np.ndarray:
    """(span as f32).sqrt() as usize, IEEE: numpy converts u64 -> f32 round-to-nearest-even and its
    float32 sqrt is correctly rounded."""
    return np.sqrt(np.asarray(spans, np.uint64).astype(np.float32)).astype(np.uint64)


def sqrt_sweep_spans() -> np.ndarray:
    """Every span in [2, 2^20]; and for every k in [1, 46,340], k^2 and the 16 representable float32
    values on either side of it, each as the lowest and the highest u64 that converts to it (so the
    u64 -> f32 conversion's ties are exercised); kept within [2, 2^31].  A 1-ULP error in the root
    cannot change the truncated stride farther than that from a square."""
    k = np.arange(1, 46_341, dtype=np.uint64)
    sq = (k * k).astype(np.float32)  # exact below 2^24, else the float32 nearest k^2
    vals = [sq]
    up = down = sq
    for _ in range(16):
        up = np.nextafter(up, np.float32(np.inf))
        down = np.nextafter(down, np.float32(0))
        vals += [up, down]
    v = np.unique(np.concatenate(vals))
    v = v[(v == np.floor(v)) & (v >= 1) & (v <= 2.0 ** 31)]  # only integers are some span's image
    v64 = v.astype(np.float64)  # exact, and so are the half-gaps to the neighbours below
    below = v64 - np.nextafter(v, np.float32(0)).astype(np.float64)
    above = np.nextafter(v, np.float32(np.inf)).astype(np.float64) - v64
    lo = np.ceil(v64 - below / 2).astype(np.uint64)   # the tie itself belongs to v or to its neighbour
    lo = np.where(lo.astype(np.float32) == v, lo, lo + 1)
    hi = np.floor(v64 + above / 2).astype(np.uint64)
    hi = np.where(hi.astype(np.float32) == v, hi, hi - 1)
    assert (lo.astype(np.float32) == v).all() and (hi.astype(np.float32) == v).all()
    assert ((lo - 1).astype(np.float32) != v)[lo > 1].all() and ((hi + 1).astype(np.float32) != v).all()
    exact = (k * k)  # k^2 itself and k^2 - 1 as spans, whatever they round to
    s = np.unique(np.concatenate([np.arange(2, (1 << 20) + 1, dtype=np.uint64), lo, hi, exact, exact - 1,
                                  np.array([(1 << 24) - 1, 1 << 31], np.uint64)]))
    return s[(s >= 2) & (s <= (1 << 31))]


def sweep_expected(spans: np.ndarray, sqrt_policy: int, b: int):
    """(stride, children, kind) of one segment [0, span) of a span-row store, remote size 1."""
    spans = np.asarray(spans, np.uint64)
    st = f32_sqrt_trunc(spans) if sqrt_policy else (spans + np.uint64(b - 1)) // np.uint64(b)
    st = np.maximum(st, 1)
    assert (spans >= 2).all()
    kind = np.where(st >= spans, 1, 2).astype(np.uint8)  # a SPLIT that would not progress is enumerated
    children = np.where(kind == 2, (spans - 1) // st + 1, 1).astype(np.uint64)
    return st.astype(np.uint64), children, kind


def decide_expected(l, h, L, R, n, sqrt_policy, b, clamp=True):
    """One segment as oracle/rbsr.py's protocol_round treats it: (kind, stride, si, ei, children,
    enums), kind 0 skip / 1 IDLIST / 2 SPLIT / 3 dropped.  clamp=False: the ranks are taken as
    given (the host tier's decide_segment is handed ranks already within the view)."""
    if h < l:
        return (3, 0, 0, 0, 0, 0)
    si, ei = (min(l, n), min(h, n)) if clamp else (l, h)
    local, remote = (tuple(L[:4]), L[4]), (tuple(R[:4]), R[4])
    span = local[1]
    d = (OR.sqrt_fan_out if sqrt_policy else OR.fixed_fan_out(b))(local, remote, 0)
    if d[0] == "split" and span > 1 and d[1] >= span:
        d = ("enumerate",)
    if d[0] == "skip":
        return (0, 0, si, ei, 0, 0)
    if d[0] == "enumerate":
        return (1, 0, si, ei, 1 if remote[1] != 0 else 0, 1)
    stride = int(d[1])
    children = ((ei - si - 1) // stride if ei > si else 0) + 1
    if children <= 4096:  # protocol_round's own loop, literally
        c, cur = 0, si
        while True:
            c += 1
            if not cur + stride < ei:
                break
            cur += stride
        assert c == children
    return (2, stride, si, ei, children, 0)


def round_cases():
    """(l, h, L[5], R[5], n, sqrt_policy, b) records: fixed fan-out b in {2, 16, 2^31} and the sqrt
    policy over spans {0, 1, 2, b-1, b, b+1, 2^31}; the (span, rem) corners; equal fingerprints with
    unequal sizes; h < l; l, h beyond n."""
    fa, fb = (7, 0, 0, 1 << 63), (7, 0, 0, (1 << 63) + 1)
    recs = []
    for sqrt_policy, b in ((0, 2), (0, 16), (0, 1 << 31), (1, 16)):
        spans = sorted({0, 1, 2, b - 1, b, b + 1, 1 << 31, 3, 4, 15, 16, 17, (1 << 24) - 1, 1 << 24})
        for span in spans:
            for rem in sorted({0, 1, 2, span, span + 1}):
                for fr in (fa, fb):  # equal fingerprints (SKIP only with equal sizes), unequal ones
                    for l, h, n in ((0, span, span), (5, 5 + span, span + 10), (span + 3, span + 7, span),
                                    (2, span + 9, span + 4), (10, 3, span + 20), (span, span, span)):
                        recs.append((l, h, fa + (span,), fr + (rem,), n, sqrt_policy, b))
    for span, rem in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2)):  # the cutoffs' corners, both policies
        for sqrt_policy in (0, 1):
            for fr in (fa, fb):
                recs.append((0, span, fa + (span,), fr + (rem,), span, sqrt_policy, 16))
    return recs


def round_records(recs) -> np.ndarray:
    return np.array([[l, h, *L, *R, n, sp, b] for l, h, L, R, n, sp, b in recs], np.uint64)


# ---- operand pairs for fp_add / fp_sub ----------------------------------------------------------------
def fp_pairs():
    adv = adversarial_values()
    pairs = [(a, b) for a in adv for b in adv]
    rng = np.random.default_rng(21)
    rnd = ints_of(rng.integers(0, 256, (64, 32), dtype=np.uint8))
    for a in adv + rnd[:16]:
        pairs += [(a, a), (a, (a + 1) % M256), (a, (a - 1) % M256), ((a + 1) % M256, a), ((a - 1) % M256, a)]
    pairs.append((0, 1))
    # equal from limb j upward, the lower limbs of a below b's: a borrow enters a limb where a[i] == b[i]
    # (and, for the sum, a carry enters limbs where a[i] + b[i] = 2^32 - 1)
    for j in range(1, 8):
        for top in (0, ONES, rnd[j], rnd[8 + j]):
            keep = (top >> (32 * j)) << (32 * j)
            lo_a, lo_b = sorted((rnd[16 + j] % (1 << (32 * j)), rnd[24 + j] % (1 << (32 * j))))
            pairs += [(keep | lo_a, keep | lo_b), (keep | lo_b, keep | lo_a), (keep, keep | 1),
                      (keep | lo_b, (~(keep | lo_a)) % M256)]
    pairs += list(zip(rnd[32:48], rnd[48:64]))  # the control
    return pairs


# ---- the cases file / results file ---------------------------------------------------------------
class CaseFile:
    def __init__(self):
        self.bufs, self.cases = [], []

    def buf(self, arr) -> int:
        b = arr if isinstance(arr, (bytes, bytearray)) else np.ascontiguousarray(arr).tobytes()
        self.bufs.append(b)
        return len(self.bufs) - 1

    def case(self, name: str, op: int, args=(), bufs=()):
        assert len(name) < 40 and len(args) <= 4 and len(bufs) <= 6
        a = list(args) + [0] * (4 - len(args))
        b = list(bufs) + [-1] * (6 - len(bufs))
        self.cases.append(struct.pack("<40sII4Q6q", name.encode(), op, 0, *a, *b))

    def write(self, path: str):
        with open(path, "wb") as f:
            f.write(b"RHDUC001" + struct.pack("<Q", len(self.bufs)))
            for b in self.bufs:
                f.write(struct.pack("<Q", len(b)))
                f.write(b)
                f.write(bytes(-len(b) % 8))
            f.write(struct.pack("<Q", len(self.cases)))
            for c in self.cases:
                f.write(c)


def read_results(path: str) -> dict:
    """{"case/what": bytes (a memoryview slice of the file)}"""
    data = np.fromfile(path, np.uint8)
    assert data[:8].tobytes() == b"RHDUR001"
    out, p = {}, 8
    while p < data.size:
        name = data[p:p + 64].tobytes().split(b"\0", 1)[0].decode()
        n = int(data[p + 64:p + 72].view(np.uint64)[0])
        assert name not in out
        out[name] = data[p + 72:p + 72 + n]
        p += 72 + n + (-n % 8)
    return out


def add_round_cases(cf: CaseFile):
    """The round cases (shared by the device driver and the host program)."""
    recs = round_cases()
    cf.case("round", OP_ROUND, (len(recs),), (cf.buf(round_records(recs)),))
    spans = sqrt_sweep_spans()
    sb = cf.buf(spans)
    cf.case("sweep-sqrt", OP_ROUND_SPANS, (spans.size, 1, 16), (sb,))
    edge = np.array(sorted({2, 3, 15, 16, 17, (1 << 31) - 1, 1 << 31, (1 << 31) - 2}), np.uint64)
    eb = cf.buf(edge)
    for b in (2, 16, 1 << 31):
        cf.case("sweep-fixed-%d" % b, OP_ROUND_SPANS, (edge.size, 0, b), (eb,))
    return recs, spans, edge
