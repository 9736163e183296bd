"""records_common.canonical -- the one statement of the reference's encoding that the lift and store
tests take their expected bytes from -- against bytes that do not come from it: the reference's
own vectors in tests/golden/vectors.json, the C oracle's encoder (oracle.Records.encode) on the
shapes it has, and oracle/pyref.py's typed model assembled by hand on the others."""
import numpy as np

import pyref as P  # oracle/pyref.py
from records_common import canonical, msg_len, prefix_len


def test_canonical_is_the_reference_encoding(golden, oracle_lib):
    O = oracle_lib
    vec = {v["name"]: v for v in golden["reference"]["vectors"]}
    le = lambda v, n: v.to_bytes(n, "little")  # noqa: E731
    # lift(&50u64, &"Hello") and the three parts of the combined vector: u64 key, var value, plain
    assert canonical("u64", "var", "plain", le(50, 8), b"Hello").hex() == vec["lift_50u64_Hello"]["encoded_hex"]
    parts = [canonical("u64", "var", "plain", le(k, 8), v) for k, v in ((25, b"World!"), (50, b"Hello"), (75, b"Everyone!"))]
    assert [p.hex() for p in parts] == vec["combined_25_50_75"]["encoded_hex_parts"]
    # a dated u32 / u32 entry, present, with the stamp of its record
    e = vec["entry_fingerprint_7u32"]
    r = e["record"]
    assert r["state"] == "present"
    stamp = (int(r["phys"], 16), int(r["logical"], 16), int(r["node"], 16))
    got = canonical("u32", "u32", "dated", le(r["key_u32"], 4), r["value_u32"], stamp)
    assert got.hex() == e["encoded_hex"] and len(got) == msg_len("u32", "u32", "dated")
    assert canonical("u32", "u32", "dated", r["key_u32"], le(r["value_u32"], 4), stamp) == got  # ints or row bytes

    # against the C oracle's encoder: a string key of 15 bytes is to the encoding what a [u8; 15]
    # key is (u64 length, then the bytes), a var value of 64 bytes what a [u8; 64] value is; row 1 is
    # a tombstone, whose value row is ignored
    rng = np.random.default_rng(1)
    keys, vals = rng.integers(0, 256, (2, 15), dtype=np.uint8), rng.integers(0, 256, (2, 64), dtype=np.uint8)
    phys, node = np.array([1_700_000_000_123, 5], np.uint64), np.array([(1 << 63) + 9, 7], np.uint64)
    logical, tags = np.array([3, (1 << 32) - 1], np.uint32), np.array([0, 1], np.uint8)
    for kind, rec_kind in (("dated", O.REC_DATED), ("projection", O.REC_PROJECTION)):
        recs = O.Records(O.Schema(O.KEY_BYTES, 15, O.VAL_BYTES, 64, rec_kind, 0), keys, vals, phys, logical, node, tags)
        for i in range(2):
            stamp = (int(phys[i]), int(logical[i]), int(node[i]))
            want = recs.encode(i)
            for key, value in (("str15", "var"), ("str31", "var"), ("bytes15", "bytes64"), ("str15", "bytes64")):
                assert canonical(key, value, kind, keys[i].tobytes(), vals[i].tobytes(), stamp, bool(tags[i])) == want, (kind, i, key)
            assert len(want) == msg_len("str15", "var", kind, 15, 64, tomb=bool(tags[i]))
    plain = O.Records(O.Schema(O.KEY_U64, 8, O.VAL_UNIT, 0, O.REC_PLAIN, 0), np.array([[9, 0, 0, 0, 0, 0, 0, 1]], np.uint8))
    assert canonical("u64", "unit", "plain", bytes([9, 0, 0, 0, 0, 0, 0, 1]), None) == plain.encode(0)

    # shapes the oracle's columns cannot hold, against pyref assembled by hand: a short string under
    # a wide row, an empty string, fixed values under string keys, a unit key
    ts = P.timestamp(11, 22, 33)
    assert canonical("str63", "var", "dated", b"pod/web-0", b"Running", (11, 22, 33)) == \
        P.encode(P.Str(b"pod/web-0")) + P.encode(P.entry(ts, P.present(P.Str(b"Running"))))
    assert canonical("str63", "var", "dated", b"pod/web-0", b"ignored", (11, 22, 33), True) == \
        P.encode(P.Str(b"pod/web-0")) + P.encode(P.entry(ts, P.TOMBSTONE))
    assert canonical("str15", "u64", "projection", b"", (1 << 64) - 1) == P.encode(P.Str(b"")) + P.encode(P.present(P.U64((1 << 64) - 1)))
    assert canonical("str31", "u32", "plain", b"k", 7) == P.encode(P.Str(b"k")) + P.encode(P.U32(7))
    assert canonical("str31", "unit", "projection", b"k", None, tomb=True) == P.encode(P.Str(b"k")) + P.encode(P.TOMBSTONE)
    assert canonical("unit", "var", "plain", b"", b"v") == P.encode(P.Unit()) + P.encode(P.Str(b"v"))
    assert len(canonical("str63", "var", "dated", b"pod/web-0", b"", (11, 22, 33))) == prefix_len("str63", "dated", 9) == 49
