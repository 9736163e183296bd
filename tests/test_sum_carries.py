"""Carry chains of the Σ mod 2^256 kernels through the public API: reduce_blocks (k_reduce),
range_aggregates (k_range_query, k_range_query_wave) and combine_aggregates (k_combine) on arrays
whose limbs are saturated, cancel through full-length carries, or mix the five edge values --
tests/device_units_common.py's P1-P5 -- where BLAKE3 outputs meet such a limb with probability
2^-32.  Every expected value is a Python integer sum mod 2^256."""
import numpy as np
import pytest
import torch

import device_units_common as U

N = U.RANGE_N
_CACHE = {}


def _data(p):
    if p not in _CACHE:
        rows = U.pattern(p, N)
        _CACHE[p] = (rows, U.prefix_ints(U.ints_of(rows)))
    return _CACHE[p]


def _sums(pre, n, width):
    return [(pre[min(i + width, n)] - pre[i]) % U.M256 for i in range(0, n, width)]


@pytest.mark.gpu
@pytest.mark.parametrize("p", U.PATTERNS)
def test_reduce_blocks_saturated_limbs(gpu, rsos_hip_lib, p):
    rows, pre = _data(p)
    for n in (1, 255, 256, 257, 65_537):
        got = rsos_hip_lib.reduce_blocks(torch.from_numpy(rows[:n].copy()).to(gpu)).cpu().numpy()
        assert U.ints_of(got) == _sums(pre, n, 256), n


@pytest.mark.gpu
@pytest.mark.parametrize("p", U.PATTERNS)
def test_range_aggregates_saturated_limbs(gpu, rsos_hip_lib, p):
    rows, pre = _data(p)
    fps = torch.from_numpy(rows).to(gpu)
    bs = rsos_hip_lib.reduce_blocks(fps)
    ss = rsos_hip_lib.reduce_blocks(bs)
    want_bs = _sums(pre, N, 256)
    assert U.ints_of(bs.cpu().numpy()) == want_bs
    assert U.ints_of(ss.cpu().numpy()) == U.block_sums(want_bs)
    bounds = U.range_bounds()
    want = U.range_expected(pre, N, bounds)
    lo = torch.tensor([q[0] for q in bounds], dtype=torch.int64, device=gpu)
    hi = torch.tensor([q[1] for q in bounds], dtype=torch.int64, device=gpu)
    for name, b, s in (("both", bs, ss), ("blocks", bs, None), ("rows", None, None)):
        got = U.agg_ints(rsos_hip_lib.range_aggregates(fps, b, s, lo, hi).cpu().numpy())
        bad = [(bounds[i], name) for i in range(len(bounds)) if got[i] != want[i]]
        assert not bad, bad[:5]
    # fewer than 64 ranges with both levels: one workgroup per range, whole super-blocks from ssums
    # (the first 28 bounds cover super-block 1 with ragged block and row edges on both sides)
    got = U.agg_ints(rsos_hip_lib.range_aggregates(fps, bs, ss, lo[:40].contiguous(), hi[:40].contiguous()).cpu().numpy())
    bad = [bounds[i] for i in range(40) if got[i] != want[i]]
    assert not bad, bad[:5]


def _parts(columns):
    """columns[j] = [(fingerprint, size) per part] -> (P, r, 5) int64"""
    r, parts = len(columns), len(columns[0])
    a = np.zeros((parts, r, 5), np.uint64)
    for j, col in enumerate(columns):
        for q, (fp, size) in enumerate(col):
            a[q, j, :4] = np.frombuffer((fp % U.M256).to_bytes(32, "little"), np.uint64)
            a[q, j, 4] = size
    return a.view(np.int64)


@pytest.mark.gpu
def test_combine_aggregates_carry_chains(gpu, rsos_hip_lib):
    ones192 = (1 << 192) - 1  # u64 limbs 0..2 saturated: a carry out of limb 0 must pass limbs 1 and 2
    adv = U.adversarial_values()
    columns = [
        [(U.ONES, 1 << 40)] * 8,                                   # 8 parts, all all-ones
        [(U.ONES, 3), (1, 5)] * 4,                                 # parts that cancel pairwise
        [(ones192, 1), (1, 2)] + [(0, 0)] * 6,                     # ... + 1 = 2^192
        [(1, 2), (ones192, 1)] + [(0, 0)] * 6,
        [(ones192, 1), (0, 0), (1, 2)] + [(0, 0)] * 5,
        [((1 << 128) - 1, 1), (1, 1), ((1 << 192) - (1 << 128), 1), (1 << 128, 1)] + [(0, 0)] * 4,
        [((1 << 64) - 1, 0), (U.ONES - ((1 << 64) - 1), 0), (1, 0)] + [(0, 0)] * 5,  # a late carry over 3 limbs
    ]
    for i in range(0, len(adv) - 8, 8):  # the adversarial values, 8 at a time
        columns.append([(v, k) for k, v in enumerate(adv[i:i + 8])])
    parts = _parts(columns)
    got = U.agg_ints(rsos_hip_lib.combine_aggregates(torch.from_numpy(parts).to(gpu)).cpu().numpy())
    want = [(sum(fp for fp, _ in col) % U.M256, sum(s for _, s in col) % (1 << 64)) for col in columns]
    assert got == want
    assert want[0][0] == U.M256 - 8 and want[1] == (0, 32) and want[2][0] == 1 << 192
