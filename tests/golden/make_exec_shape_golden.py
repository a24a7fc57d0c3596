"""Regenerate tests/golden/exec_shapes.json from the upstream reference.

For every case of tests/exec_shape_cases.py the same schedule goes through
the reference's siamese.h API (siamese_encoder_add, siamese_encode,
siamese_encoder_remove_before, through siamese_amd/binding.py): the length
and sha256 of each recovery packet are recorded with a hash of the schedule,
and the reference's own decoder must return exactly the lost packets with the
right bytes -- a case it does not fully decode is refused and nothing is
written.  The file holds lengths, loss sets, counts and hashes only.

Runs only where oracle/_ref/libsiamese_ref.so exists (make -C oracle).
Usage: python tests/golden/make_exec_shape_golden.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import exec_shape_cases as X  # noqa: E402
import scenario_lib as S  # noqa: E402
import size_cases as Z  # noqa: E402


def main():
    if not os.path.exists(S.REF_LIB):
        sys.exit("oracle/_ref/libsiamese_ref.so missing: run make -C oracle")
    cases = {}
    for name, case in X.CASES.items():
        t0 = time.time()
        data = Z.payloads(case)
        packets, recovered = X.reference_run(case, data)
        if recovered is None or sorted(recovered) != [(i, data[i]) for i in sorted(case.lost)]:
            sys.exit("%s: the reference does not decode this loss set (%s); pick another"
                     % (name, "NeedMoreData" if recovered is None else "%d packets" % len(recovered)))
        cases[name] = X.describe(packets, case)
        if not all(1 <= r["footer_bytes"] <= 8 for r in cases[name]["recovery"]):
            sys.exit("%s: a packet's payload is not as long as the longest symbol of its window" % name)
        print("%-13s originals=%-4d lost=%-4d recovery=%-4d %.2fs" % (
            name, len(case.lengths), len(case.lost), case.recovery, time.time() - t0), flush=True)
    out = {"generator": "tests/golden/make_exec_shape_golden.py (oracle/_ref/libsiamese_ref.so)", "cases": cases}
    with open(X.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
