"""EnumerateBelowThreshold (rbsr/src/policy/enumerate_below_threshold.rs) on the CPU: the Python policy,
the host tier's decide_segment and HostTier::round with a threshold, and whole reconciliations on the
two-call path -- each against oracle/rbsr.py's literal round with the policy restated locally
(threshold_common.below_threshold).  Every comparison is exact."""
import os
import subprocess
import types

import numpy as np
import pytest

import rbsr as OR  # oracle/rbsr.py
from recon_common import DictView, _norm, _outcome, reconcile
from threshold_common import TwoCall, below_threshold, covered, expected_decision, to_product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0, 1, 2, 31, 32, 33, 1 << 31)
FAN_OUTS = (0, 2, 16)
FP_A, FP_B = (5, 0, 0, 1 << 63), (6, 0, 0, 1 << 63)


def _sweep():
    """(t, b, local, remote) over the spans, remote sizes and fingerprints of every (t, b)"""
    out = []
    for t in THRESHOLDS:
        for b in FAN_OUTS:
            tn, bn = max(t, 1), max(b, 2)
            spans = sorted({0, 1, 2, max(tn - 1, 0), tn, tn + 1, tn * bn, tn * bn + 1, 1 << 31})
            for span in spans:
                for rsize in sorted({0, 1, span, span + 1}):
                    for rfp in (FP_A, FP_B):  # equal and unequal fingerprints; equal with another size must not skip
                        out.append((t, b, (FP_A, span), (rfp, rsize)))
    return out


SWEEP = _sweep()


def test_python_policy_matches_the_restatement(rsos_hip_lib):
    from rsos_hip import Aggregate, Fingerprint
    from rsos_hip import rbsr as R
    skips = 0
    for t, b, local, remote in SWEEP:
        policy = R.EnumerateBelowThreshold(t, b)
        assert (policy.threshold, policy.fan_out) == (max(t, 1), max(b, 2))
        d = policy.decide(R.Comparison(Aggregate(local[1], Fingerprint(local[0])), Aggregate(remote[1], Fingerprint(remote[0]))))
        want = below_threshold(t, b)(local, remote, 0)
        got = ("skip",) if d == R.SKIP else ("enumerate",) if d == R.ENUMERATE else ("split", d.stride)
        assert got == want, (t, b, local, remote)
        assert (got == ("skip",)) == (local == remote)
        skips += got == ("skip",)
    assert skips > 0
    paper = R.EnumerateBelowThreshold()
    assert (paper.threshold, paper.fan_out) == (32, 16)
    with pytest.raises(TypeError, match="FixedFanOut / SqrtFanOut / EnumerateBelowThreshold"):
        R.protocol_round_segments(None, object(), None)


def _build(tmp, name, compiler, extra):
    exe = str(tmp / name)
    subprocess.run(compiler + ["-O2", "-g", "-std=c++17", "-Wall"] + extra + [os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, src, dst):
    # no leak check at exit: it needs ptrace, which a sandboxed user may not have
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])


def test_decide_segment_with_a_threshold(tmp_path):
    """csrc/round_decide.hpp on the sweep's records (raw ranks [7, 7 + span)), and threshold 0 on a
    handful: the seven-argument call gives the six-argument one's decision (checked by the program) and
    the shared cutoffs' (checked here against oracle/rbsr.py's FixedFanOut and SqrtFanOut)."""
    exe = _build(tmp_path, "threshold_decide_host", [os.environ.get("CXX", "c++")],
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    recs = [(7, 7 + l[1], l, r, 0, max(b, 2), max(t, 1), below_threshold(t, b)) for t, b, l, r in SWEEP]
    recs.append((9, 3, (FP_A, 0), (FP_B, 4), 0, 16, 32, below_threshold(32, 16)))  # inverted: dropped
    for span, rsize, rfp in ((0, 5, FP_B), (1, 5, FP_B), (1, 1, FP_B), (40, 0, FP_B), (40, 40, FP_A), (40, 41, FP_A),
                             (2, 9, FP_B), (1000, 3, FP_B)):
        recs.append((7, 7 + span, (FP_A, span), (rfp, rsize), 0, 16, 0, OR.fixed_fan_out(16)))
        recs.append((7, 7 + span, (FP_A, span), (rfp, rsize), 1, 2, 0, OR.sqrt_fan_out))
    src, dst = str(tmp_path / "records"), str(tmp_path / "results")
    with open(src, "w") as f:
        for lo, hi, l, r, sq, b, t, _ in recs:
            f.write(" ".join(str(x) for x in (lo, hi, *l[0], l[1], *r[0], r[1], sq, b, t)) + "\n")
    _run(exe, src, dst)
    got = [tuple(int(x) for x in line.split()) for line in open(dst)]
    assert len(got) == len(recs)
    kinds = set()
    for (lo, hi, l, r, sq, b, t, decide), (kind, stride, children, enums) in zip(recs, got):
        wk, ws, wc, we = expected_decision(decide, lo, hi, l, r)
        assert (kind, children, enums) == (wk, wc, we) and (wk != 2 or stride == ws), (lo, hi, l, r, sq, b, t)
        kinds.add((kind, t != 0))
    assert kinds >= {(0, True), (1, True), (2, True), (3, True), (0, False), (1, False), (2, False)}


def _map(rng, n):
    keys = np.unique(rng.integers(0, 256, (n + 32, 16), dtype=np.uint8), axis=0)
    rng.shuffle(keys)
    return {k.tobytes(): rng.bytes(32) for k in keys[:n]}


def _view(rows):
    return DictView(types.SimpleNamespace(rows={k: (None, fp) for k, fp in rows.items()}))


def _limbs(fp):
    return " ".join(str(int.from_bytes(fp[8 * i:8 * i + 8], "little")) for i in range(4))


def _parse_rounds(path):
    rounds = []
    key = lambda kind, h: bytes.fromhex(h) if kind == "1" else None  # noqa: E731
    for line in open(path):
        w = line.split()
        if w[0] == "R":
            rounds.append(([], [], tuple(int(x) for x in w[1:])))
        elif w[0] == "C":
            rounds[-1][0].append((key(w[1], w[2]), key(w[3], w[4]), (tuple(int(x) for x in w[5:9]), int(w[9]))))
        else:
            rounds[-1][1].append((key(w[1], w[2]), key(w[3], w[4])))
    return rounds


def test_host_tier_round_with_a_threshold(tmp_path):
    """HostTier::round(.., threshold) over a 3,000-key base with a 200-entry delta folded into its tree
    (inserts, overwrites, deletes), round by round against oracle/rbsr.py: every round the tier's side
    answers in two drives against a peer that differs in 37 keys, each started from either side."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = _build(tmp_path, "threshold_tier_host", [hipcc, "-x", "c++"], ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"])
    rng = np.random.default_rng(11)
    base = _map(rng, 3000)
    bk = sorted(base)
    cur = dict(base)
    delta = {}
    for k in bk[5:1500:25]:  # 60 deletes
        delta[k] = None
    for k in bk[7:2100:30]:  # 70 overwrites
        delta[k] = rng.bytes(32)
    for k in _map(rng, 70):  # 70 inserts
        if k not in base:
            delta[k] = rng.bytes(32)
    assert len(delta) == 200
    for k, fp in delta.items():
        if fp is None:
            cur.pop(k)
        else:
            cur[k] = fp
    peer = dict(cur)
    ck = sorted(cur)
    for k in ck[3::90][:20]:
        peer.pop(k)
    for k in ck[40::170][:10]:
        peer[k] = rng.bytes(32)
    for k in list(_map(rng, 7)):
        peer[k] = rng.bytes(32)
    va, vb = _view(cur), _view(peer)
    lines = ["K 16"] + [f"B {k.hex()} {_limbs(base[k])}" for k in bk]
    lines += [f"D {k.hex()} {int(delta[k] is not None)} {_limbs(delta[k] or bytes(32))}" for k in sorted(delta)]
    want = []
    for t, b in ((32, 16), (1, 2), (5, 3)):
        decide = below_threshold(t, b)
        fn = lambda v, act, ch, en: OR.protocol_round(v, decide, act, ch, en)  # noqa: E731
        for first, second in ((vb, va), (va, vb)):  # the tier's side (va) answers the even, then the odd rounds
            log = reconcile(first, second, fn, OR.initial_ranges)[0]
            active = OR.initial_ranges(first)
            for k, (children, enums, outcome) in enumerate(log):
                if (second if k % 2 == 0 else first) is va:
                    lines.append(f"R {t} {b} {len(active)}")
                    for s, e, (fp, size) in active:
                        lines.append(f"S {int(s is not None)} {(s or bytes(16)).hex()} {int(e is not None)} "
                                     f"{(e or bytes(16)).hex()} {' '.join(str(x) for x in fp)} {size}")
                    want.append((children, enums, outcome))
                active = children
    assert len(want) >= 12 and max(len(w[0]) for w in want) > 16
    src, dst = str(tmp_path / "input"), str(tmp_path / "results")
    with open(src, "w") as f:
        f.write("\n".join(lines) + "\n")
    _run(exe, src, dst)
    got = _parse_rounds(dst)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[2] == w[2] and g[1] == w[1] and g[0] == w[0]


@pytest.mark.parametrize("mixed", [False, True], ids=["threshold_both", "threshold_vs_fixed"])
def test_two_call_drives_through_a_dict_view(rsos_hip_lib, mixed):
    """Whole reconciliations on the two-call path (protocol_round_with_policy, native=False) over
    DictViews: EnumerateBelowThreshold on both sides, and against FixedFanOut(16) -- the policy is never
    a wire contract, so mixed policies converge.  Round by round against oracle/rbsr.py with the same
    policy per side; the enumerations cover every differing key on the side (or sides) that hold it."""
    from rsos_hip import rbsr as R
    rng = np.random.default_rng(5)
    a = _map(rng, 2000)
    b = dict(a)
    ak = sorted(a)
    only_a, changed = ak[11::60][:25], ak[30::130][:12]
    for k in only_a:
        b.pop(k)
    for k in changed:
        b[k] = rng.bytes(32)
    only_b = [k for k in _map(rng, 9) if k not in a]
    for k in only_b:
        b[k] = rng.bytes(32)
    va, vb = _view(a), _view(b)
    pa, pb = TwoCall(va), TwoCall(vb)
    pol = {id(va): (R.EnumerateBelowThreshold(32, 16), below_threshold(32, 16)),
           id(vb): (R.FixedFanOut(16), OR.fixed_fan_out(16)) if mixed else (R.EnumerateBelowThreshold(32, 16), below_threshold(32, 16))}
    pol[id(pa)], pol[id(pb)] = pol[id(va)], pol[id(vb)]
    want = reconcile(va, vb, lambda v, act, ch, en: OR.protocol_round(v, pol[id(v)][1], act, ch, en), OR.initial_ranges)

    def prod(v, act, ch, en):
        act = to_product(act) if act and isinstance(act[0], tuple) else act
        return _outcome(R.protocol_round_with_policy(v, pol[id(v)][0], act, ch, en, native=False))
    got = reconcile(pa, pb, prod, R.initial_ranges)
    assert len(got[0]) == len(want[0])
    for (gc, ge, go), (wc, we, wo) in zip(got[0], want[0]):
        assert go == wo and ge == we and _norm(gc) == wc
    ea, eb = got[1], got[2]
    for k in only_a:
        assert covered(k, ea)
    for k in only_b:
        assert covered(k, eb)
    for k in changed:
        assert covered(k, ea) or covered(k, eb)
    if not mixed:  # one descent level fewer than FixedFanOut(16) at the least never costs a round
        fixed = reconcile(va, vb, lambda v, act, ch, en: OR.protocol_round(v, OR.fixed_fan_out(16), act, ch, en),
                          OR.initial_ranges)
        assert len(got[0]) <= len(fixed[0])
