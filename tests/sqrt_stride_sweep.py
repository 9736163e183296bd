"""Measures the device's SqrtFanOut stride against (span as f32).sqrt() as usize on the sweep of
tests/device_units_common.py (sqrt_sweep_spans) and writes the record kept as
profiles/sqrt_stride_sweep.json.  One run of the device-unit driver on the round cases alone; it
reports and does not assert (tests/test_device_units.py::test_sqrt_stride_sweep asserts).

    python tests/sqrt_stride_sweep.py <out.json>
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import device_units_common as U  # noqa: E402


def main(out_path: str) -> int:
    with tempfile.TemporaryDirectory() as d:
        cf = U.CaseFile()
        _, spans, _ = U.add_round_cases(cf)
        cases, results = os.path.join(d, "cases"), os.path.join(d, "results")
        cf.write(cases)
        r = subprocess.run([U.DRIVER, cases, results], capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            print("device_units exit %d: %s" % (r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = U.read_results(results)["sweep-sqrt/stride"].view(np.uint64).copy()
    want, _, _ = U.sweep_expected(spans, 1, 16)
    bad = np.flatnonzero(got != want)
    rec = {
        "what": "round_decide's SqrtFanOut stride on the device against numpy's IEEE "
                "trunc(sqrt(float32(span))), one launch of tests/device_units.hip",
        "spans_tried": int(spans.size), "span_min": int(spans[0]), "span_max": int(spans[-1]),
        "spans_that_differ": int(bad.size),
        "smallest_that_differs": int(spans[bad[0]]) if bad.size else None,
        "largest_that_differs": int(spans[bad[-1]]) if bad.size else None,
        "examples": [{"span": int(spans[i]), "device": int(got[i]), "reference": int(want[i])} for i in bad[:32]],
    }
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k != "examples"}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
