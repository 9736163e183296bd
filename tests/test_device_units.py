"""Device units: the library's device functions and launchers on inputs the public API never gives them.

Almost every fingerprint the suite feeds a summing kernel is a BLAKE3 output, and every span it
feeds a fan-out policy comes from a few thousand rows.  The device-unit driver
(tests/device_units.hip -> reconcile-rs_amd/examples/device_units) calls round_decide, fp_add /
fp_sub, the carry-save helpers and the reduce / total / range-query / prefix launchers directly, on
operands chosen so that carries and borrows ripple through saturated limbs, carry-save totals sit at
their maximum, k_prefix_top runs past its first chunk, k_range_query takes its super-block branch,
and the SqrtFanOut stride is asked at every span where a 1-ULP error in the root could change it.

The driver runs once per module (one process, every case once, no retries): a non-zero exit fails
the fixture and with it every GPU test here.  Each test then compares one section of the results
with Python integers mod 2^256, or with numpy's IEEE float32 root and oracle/rbsr.py's policies.

The CPU tests check the same operand pairs through rh_fp_add / rh_fp_sub, the sweep's candidate
set, and the host tier's decide_segment on the round cases (tests/round_decide_host.cpp, built with
the address and undefined-behaviour sanitizers as a stand-alone program).
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import device_units_common as U

NS = (0, 1, 255, 256, 257, 65_535, 65_536, 65_537, U.RANGE_N)
BIG_N = 153_601 * 256 - 7  # 601 super-blocks: k_prefix_top's second and third chunk
_DATA = {}


def pattern_data(p):
    """The pattern at RANGE_N rows: rows, their integers and the prefix Σ rows[0..i)."""
    if p not in _DATA:
        rows = U.pattern(p, U.RANGE_N)
        vals = U.ints_of(rows)
        _DATA[p] = {"rows": rows, "vals": vals, "pre": U.prefix_ints(vals)}
    return _DATA[p]


def level_sums(pre, n, width):
    """Σ over each `width`-row group of the first n rows, from the prefix."""
    return [(pre[min(i + width, n)] - pre[i]) % U.M256 for i in range(0, n, width)]


def test_driver_is_built():
    assert os.access(U.DRIVER, os.X_OK), "make -C reconcile-rs_amd builds examples/device_units"
    r = subprocess.run([U.DRIVER, "--constants"], capture_output=True, text=True, timeout=60)  # no device call
    assert r.returncode == 0, r.stderr
    c = json.loads(r.stdout)
    assert c["DB_WG"] % 64 == 0 and c["DP_WG"] % 64 == 0 and c["guard"] >= 32


def test_host_fp_add_sub_on_the_device_pairs(rsos_hip_lib):
    L = rsos_hip_lib.lib()
    for a, b in U.fp_pairs():
        x = np.frombuffer(a.to_bytes(32, "little"), np.uint64).copy()
        y = np.frombuffer(b.to_bytes(32, "little"), np.uint64).copy()
        s, d = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        L.rh_fp_add(x.ctypes.data_as(C.POINTER(C.c_uint64)), y.ctypes.data_as(C.POINTER(C.c_uint64)),
                    s.ctypes.data_as(C.POINTER(C.c_uint64)))
        L.rh_fp_sub(x.ctypes.data_as(C.POINTER(C.c_uint64)), y.ctypes.data_as(C.POINTER(C.c_uint64)),
                    d.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert int.from_bytes(s.tobytes(), "little") == (a + b) % U.M256, (hex(a), hex(b))
        assert int.from_bytes(d.tobytes(), "little") == (a - b) % U.M256, (hex(a), hex(b))


def test_sweep_candidate_set():
    s = U.sqrt_sweep_spans()
    assert s.dtype == np.uint64 and (np.diff(s.astype(np.int64)) > 0).all() and s[0] == 2 and s[-1] == 1 << 31
    have = set(s.tolist())
    assert (1 << 24) - 1 in have
    assert int(U.f32_sqrt_trunc([(1 << 24) - 1])[0]) == 4095  # the true root sits a hair below the tie with 4096
    k = np.arange(2, 46_341, dtype=np.uint64)
    assert np.isin(k * k, s).all() and np.isin(k * k - 1, s).all()
    assert np.isin(np.arange(2, (1 << 20) + 1, dtype=np.uint64), s).all()
    # the reference truncates the exact root wherever the span is a float32: k^2 -> k below 2^24
    small = k[k < 4096]
    assert (U.f32_sqrt_trunc(small * small) == small).all()
    assert (U.f32_sqrt_trunc(small * small - 1) == small - 1).all()
    # both ends of a float32's preimage are there (by brute force around a few squares): the lowest
    # and the highest u64 that convert to the float32 nearest k^2, ties included
    for kk in (4097, 5793, 11_586, 23_171, 46_340):
        x = np.arange(kk * kk - 300, kk * kk + 300, dtype=np.uint64)
        same = x[x.astype(np.float32) == np.float32(kk * kk)]
        assert 1 <= same.size < 300 and int(same[0]) in have and int(same[-1]) in have, kk


# ---- the host tier's decision on the same cases ------------------------------------------------------
@pytest.fixture(scope="module")
def host_round(tmp_path_factory):
    d = tmp_path_factory.mktemp("rdh")
    exe = str(d / "round_decide_host")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", U.HOST_SRC, "-o", exe], check=True)
    cf = U.CaseFile()
    recs, spans, edge = U.add_round_cases(cf)
    cf.write(str(d / "cases"))
    # no leak check at exit: it needs ptrace, which a sandboxed user may not have
    r = subprocess.run([exe, str(d / "cases"), str(d / "results")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-4000:]
    return recs, spans, edge, U.read_results(str(d / "results"))


def test_host_decide_segment_general(host_round):
    recs, _, _, res = host_round
    got = res["round/out"].view(np.uint64).reshape(-1, 4)
    assert got.shape[0] == len(recs)
    for rec, g in zip(recs, got.tolist()):
        kind, stride, _, _, children, enums = U.decide_expected(*rec, clamp=False)
        assert (g[0], g[2], g[3]) == (kind, children, enums), rec
        if kind == 2:
            assert g[1] == stride, rec


def _check_sweep(res, name, spans, sqrt_policy, b):
    st, ch, kd = U.sweep_expected(spans, sqrt_policy, b)
    got_st = res[name + "/stride"].view(np.uint64)
    bad = np.flatnonzero(got_st != st)
    assert bad.size == 0, "%d spans differ, e.g. span %d: stride %d, reference %d" % (
        bad.size, spans[bad[0]], got_st[bad[0]], st[bad[0]])
    assert np.array_equal(res[name + "/children"].view(np.uint64), ch)
    assert np.array_equal(res[name + "/kind"], kd)


def test_host_decide_segment_sweep(host_round):
    _, spans, edge, res = host_round
    _check_sweep(res, "sweep-sqrt", spans, 1, 16)
    for b in (2, 16, 1 << 31):
        _check_sweep(res, "sweep-fixed-%d" % b, edge, 0, b)


# ---- the device run ------------------------------------------------------------------------------
def _acc_sequences():
    seqs = [U.ints_of(U.pattern(p, k)) for k in (1, 2, 255, 256, 700) for p in U.PATTERNS]
    seqs.append(U.adversarial_values())
    seqs.append([])
    return seqs


def _tiles():
    tiles = [U.pattern(p, 256) for p in U.PATTERNS]
    mixed = U.rows_of([U.adversarial_values()[-1]])[0]
    for lane in (0, 31, 32, 63, 64, 255):  # one non-zero lane
        for v in (np.full(32, 0xFF, np.uint8), mixed):
            t = np.zeros((256, 32), np.uint8)
            t[lane] = v
            tiles.append(t)
    return tiles


def _range_inputs(p):
    d = pattern_data(p)
    n = U.RANGE_N
    order = np.random.default_rng(40).permutation(n + 1000)[:n].astype(np.uint32)
    return {"fps32": d["rows"], "rec40": U.with_stride40(d["rows"]), "heap40": U.with_stride40(d["rows"], order, n + 1000),
            "slots": order, "bs": U.rows_of(level_sums(d["pre"], n, 256)), "ss": U.rows_of(level_sums(d["pre"], n, 65_536))}


def build_device_cases(cf, consts):
    """Every case of the device run into cf; returns what the tests need to form the expected values."""
    ctx = {"consts": consts}
    ctx["recs"], ctx["spans"], ctx["edge"] = U.add_round_cases(cf)
    pairs = ctx["pairs"] = U.fp_pairs()
    cf.case("fp", U.OP_FP_ADDSUB, (len(pairs),), (cf.buf(U.rows_of(a for a, _ in pairs)), cf.buf(U.rows_of(b for _, b in pairs))))
    seqs = ctx["seqs"] = _acc_sequences()
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    cf.case("acc-seq", U.OP_ACC_SEQ, (len(seqs),), (cf.buf(off), cf.buf(U.rows_of(v for s in seqs for v in s))))
    m = 3
    cf.case("acc-wave", U.OP_ACC_WAVE, (len(U.PATTERNS), m), (cf.buf(np.concatenate([U.pattern(p, 64 * m) for p in U.PATTERNS])),))
    for sel, nt in enumerate((256, consts["DB_WG"], consts["DP_WG"])):
        cf.case("acc-block-%d" % sel, U.OP_ACC_BLOCK, (len(U.PATTERNS), m, sel),
                (cf.buf(np.concatenate([U.pattern(p, nt * m) for p in U.PATTERNS])),))
    tiles = ctx["tiles"] = _tiles()
    cf.case("block-sum", U.OP_BLOCK_SUM, (len(tiles),), (cf.buf(np.concatenate(tiles)),))
    for p in U.PATTERNS:
        rows = pattern_data(p)["rows"]
        for n in (1, 255, 256, 257, 65_537):
            cf.case("reduce-%s-%d-32" % (p, n), U.OP_REDUCE, (n, 32), (cf.buf(rows[:n]),))
            cf.case("reduce-%s-%d-40" % (p, n), U.OP_REDUCE, (n, 40), (cf.buf(U.with_stride40(rows[:n])),))
        for n in (0, 1, 255, 256, 257, 601):
            cf.case("total-%s-%d" % (p, n), U.OP_TOTAL, (n,), (cf.buf(rows[:n]),))
    # range queries: every shape of (block sums, super-block sums), r on both sides of the two kernels'
    # threshold with both levels present, 40-byte records in order and behind a slots permutation
    pairs144 = ctx["bounds"] = U.range_bounds()
    lo, hi = (cf.buf(np.array([q[k] for q in pairs144], np.uint64)) for k in (0, 1))
    lo63, hi63 = (cf.buf(np.array([q[k] for q in pairs144[:63]], np.uint64)) for k in (0, 1))
    lo64, hi64 = (cf.buf(np.array([q[k] for q in pairs144[:64]], np.uint64)) for k in (0, 1))
    n = U.RANGE_N
    for p in U.PATTERNS:
        x = _range_inputs(p)
        b = {k: cf.buf(v) for k, v in x.items()}
        for name, stride, r, recs_, f, sl, bs, ss, ql, qh in (
                ("both", 32, 144, n, b["fps32"], -1, b["bs"], b["ss"], lo, hi),      # k_range_query_wave
                ("blocks", 32, 144, n, b["fps32"], -1, b["bs"], -1, lo, hi),         # k_range_query, block branch
                ("rows", 32, 144, n, b["fps32"], -1, -1, -1, lo, hi),                # k_range_query, rows only
                ("supers-only", 32, 144, n, b["fps32"], -1, -1, b["ss"], lo, hi),    # no block sums: rows only
                ("both-r63", 32, 63, n, b["fps32"], -1, b["bs"], b["ss"], lo63, hi63),  # k_range_query, super-block branch
                ("both-r64", 32, 64, n, b["fps32"], -1, b["bs"], b["ss"], lo64, hi64),  # k_range_query_wave
                ("s40", 40, 144, n, b["rec40"], -1, b["bs"], b["ss"], lo, hi),       # the 8-byte-word loads, wave kernel
                ("s40-slots", 40, 144, n + 1000, b["heap40"], b["slots"], b["bs"], b["ss"], lo, hi),
                ("s40-slots-r63", 40, 63, n + 1000, b["heap40"], b["slots"], b["bs"], b["ss"], lo63, hi63)):
            cf.case("range-%s-%s" % (p, name), U.OP_RANGE, (n, stride, r, recs_), (f, sl, bs, ss, ql, qh))
    # prefixes: every n, max_wgs 0 / 1 / 3 (the grid-stride loop with fewer workgroups than chunks)
    ctx["prefix"] = []
    for p in U.PATTERNS:
        d_ = pattern_data(p)
        for n_ in NS:
            f, bs, ss = cf.buf(d_["rows"][:n_]), cf.buf(U.rows_of(level_sums(d_["pre"], n_, 256))), \
                cf.buf(U.rows_of(level_sums(d_["pre"], n_, 65_536)))
            for mw in (0, 1, 3):
                if mw and n_ >= 65_535 and p not in ("P1", "P4"):
                    continue  # the large outputs under a capped grid: the saturated and the mixed pattern
                name = "prefix-%s-%d-%d" % (p, n_, mw)
                cf.case(name, U.OP_PREFIX, (n_, mw, 1 if mw == 0 else 0), (f, bs, ss))
                ctx["prefix"].append((name, p, n_, mw))
    ctx["big"] = {}
    for p in U.PATTERNS:
        bsv = U.ints_of(U.pattern(p, 153_601))
        ssv = U.block_sums(bsv)
        assert len(ssv) == 601
        ctx["big"][p] = (bsv, ssv)
        cf.case("block-prefix-%s" % p, U.OP_BLOCK_PREFIX, (BIG_N,), (cf.buf(U.rows_of(bsv)), cf.buf(U.rows_of(ssv))))
    return ctx


@pytest.fixture(scope="module")
def units(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("du")
    consts = json.loads(subprocess.run([U.DRIVER, "--constants"], capture_output=True, text=True, check=True).stdout)
    cf = U.CaseFile()
    ctx = build_device_cases(cf, consts)
    cf.write(str(d / "cases"))
    r = subprocess.run([U.DRIVER, str(d / "cases"), str(d / "results")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "device_units exit %d: %s" % (r.returncode, r.stderr[-2000:])
    ctx["res"] = U.read_results(str(d / "results"))
    return ctx


def _rows(res, name):
    return U.ints_of(res[name])


@pytest.mark.gpu
def test_round_decide_general(units):
    got = units["res"]["round/out"].view(np.uint64).reshape(-1, 6)
    assert got.shape[0] == len(units["recs"])
    for rec, g in zip(units["recs"], got.tolist()):
        want = U.decide_expected(*rec)
        assert (g[0],) + tuple(g[2:]) == (want[0],) + want[2:], rec
        if want[0] == 2:  # the stride of a segment that is not split is not used
            assert g[1] == want[1], rec


@pytest.mark.gpu
def test_sqrt_stride_sweep(units):
    """Every span where a 1-ULP error of the device's square root could change the truncated stride:
    the device's SqrtFanOut stride equals (span as f32).sqrt() as usize, IEEE."""
    _check_sweep(units["res"], "sweep-sqrt", units["spans"], 1, 16)


@pytest.mark.gpu
def test_fixed_stride_edges(units):
    for b in (2, 16, 1 << 31):
        _check_sweep(units["res"], "sweep-fixed-%d" % b, units["edge"], 0, b)


@pytest.mark.gpu
def test_fp_add_sub(units):
    add, sub = _rows(units["res"], "fp/add"), _rows(units["res"], "fp/sub")
    assert len(add) == len(sub) == len(units["pairs"])
    for (a, b), s, d in zip(units["pairs"], add, sub):
        assert s == (a + b) % U.M256, ("add", hex(a), hex(b))
        assert d == (a - b) % U.M256, ("sub", hex(a), hex(b))


@pytest.mark.gpu
def test_acc_add_and_normalise(units):
    got = _rows(units["res"], "acc-seq/out")
    assert got == [sum(s) % U.M256 for s in units["seqs"]]


@pytest.mark.gpu
def test_acc_wave_reduce(units):
    got = _rows(units["res"], "acc-wave/out")
    want = [sum(U.ints_of(U.pattern(p, 64 * 3))) % U.M256 for p in U.PATTERNS]
    assert got == [w for w in want for _ in range(64)]  # every lane ends with the wave's total


@pytest.mark.gpu
def test_acc_block_reduce(units):
    c = units["consts"]
    for sel, nt in enumerate((256, c["DB_WG"], c["DP_WG"])):
        got = _rows(units["res"], "acc-block-%d/out" % sel)
        assert got == [sum(U.ints_of(U.pattern(p, nt * 3))) % U.M256 for p in U.PATTERNS], nt


@pytest.mark.gpu
def test_block_sum_fps256(units):
    got = _rows(units["res"], "block-sum/out")
    assert got == [sum(U.ints_of(t)) % U.M256 for t in units["tiles"]]


@pytest.mark.gpu
@pytest.mark.parametrize("p", U.PATTERNS)
def test_launch_reduce_and_total(units, p):
    d = pattern_data(p)
    for n in (1, 255, 256, 257, 65_537):
        want = level_sums(d["pre"], n, 256)
        for stride in (32, 40):
            assert _rows(units["res"], "reduce-%s-%d-%d/out" % (p, n, stride)) == want, (n, stride)
    for n in (0, 1, 255, 256, 257, 601):
        assert _rows(units["res"], "total-%s-%d/out" % (p, n)) == [d["pre"][n]], n


@pytest.mark.gpu
@pytest.mark.parametrize("p", U.PATTERNS)
def test_launch_range_query(units, p):
    pre, n, bounds = pattern_data(p)["pre"], U.RANGE_N, units["bounds"]
    want = U.range_expected(pre, n, bounds)
    if p == "P1":  # Σ over [lo, hi) of all-ones rows = -(hi - lo) mod 2^256
        assert all(fp == -size % U.M256 for fp, size in want)
    for name, r in (("both", 144), ("blocks", 144), ("rows", 144), ("supers-only", 144), ("both-r63", 63),
                    ("both-r64", 64), ("s40", 144), ("s40-slots", 144), ("s40-slots-r63", 63)):
        got = U.agg_ints(units["res"]["range-%s-%s/out" % (p, name)].view(np.uint64))
        bad = [(bounds[i], name) for i in range(r) if got[i] != want[i]]
        assert len(got) == r and not bad, bad[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("p", U.PATTERNS)
def test_launch_prefix_and_row_prefix(units, p):
    pre = pattern_data(p)["pre"]
    want_rows = U.rows_of(pre)
    seen = 0
    for name, q, n, mw in units["prefix"]:
        if q != p:
            continue
        seen += 1
        res = units["res"]
        nbk = (n + 255) // 256
        ns = (nbk + 255) // 256
        assert _rows(res, name + "/spre") == [pre[min(65_536 * s, n)] for s in range(ns + 1)], name
        assert _rows(res, name + "/bpre") == [pre[min(256 * k, n)] for k in range(nbk + 1)], name
        for what in ("out", "row") if mw == 0 else ("out",):
            got = res["%s/%s" % (name, what)].reshape(-1, 32)
            bad = np.flatnonzero((got != want_rows[:n + 1]).any(axis=1)) if got.shape[0] == n + 1 else [-1]
            assert len(bad) == 0, "%s/%s: %d entries differ, the first at %d" % (name, what, len(bad), bad[0])
    assert seen >= len(NS) * 2


@pytest.mark.gpu
@pytest.mark.parametrize("p", U.PATTERNS)
def test_block_prefix_past_256_super_blocks(units, p):
    """601 super-block sums: k_prefix_top carries its running total into a second and a third chunk."""
    bsv, ssv = units["big"][p]
    res = units["res"]
    assert _rows(res, "block-prefix-%s/spre" % p) == U.prefix_ints(ssv)
    got = res["block-prefix-%s/bpre" % p].reshape(-1, 32)
    want = U.rows_of(U.prefix_ints(bsv))
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d entries differ, the first at %d" % (bad.size, bad[0])
