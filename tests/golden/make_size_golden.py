"""Regenerate tests/golden/size_edges.json from the upstream reference.

For every case of tests/size_cases.py the same originals go through the
reference's siamese.h API: the length and sha256 of each recovery packet are
recorded, and the reference's own decoder must return exactly the lost
packets with the right bytes -- a case it does not fully decode is refused
and nothing is written.  The file holds lengths, loss sets, counts and hashes
only.

Runs only where oracle/_ref/libsiamese_ref.so exists (make -C oracle).
Usage: python tests/golden/make_size_golden.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import scenario_lib as S  # noqa: E402
import size_cases as Z  # noqa: E402


def main():
    if not os.path.exists(S.REF_LIB):
        sys.exit("oracle/_ref/libsiamese_ref.so missing: run make -C oracle")
    cases = {}
    for name, case in Z.CASES.items():
        t0 = time.time()
        data = Z.payloads(case)
        packets, recovered = Z.reference_run(case, data)
        if recovered is None or sorted(recovered) != [(i, data[i]) for i in sorted(case.lost)]:
            sys.exit("%s: the reference does not decode this loss set (%s); pick another"
                     % (name, "NeedMoreData" if recovered is None else "%d packets" % len(recovered)))
        cases[name] = Z.describe(packets, case)
        print("%-10s originals=%-4d lost=%-4d recovery=%-4d %.2fs" % (
            name, len(case.lengths), len(case.lost), case.recovery, time.time() - t0), flush=True)
    out = {"generator": "tests/golden/make_size_golden.py (oracle/_ref/libsiamese_ref.so)", "cases": cases}
    with open(Z.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
