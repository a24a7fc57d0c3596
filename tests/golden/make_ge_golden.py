"""Regenerate tests/golden/ge_edges.json from the upstream reference.

For every case of tests/ge_cases.py the same stream goes through the
reference's siamese.h API (through siamese_amd/binding.py): the length and
sha256 of each recovery packet, the result code and packet count of every
decode call, and the packet numbers it recovered are recorded with a hash of
the case's parts.  What the reference recovers must be the original's bytes;
a case whose decodes do not end as ge_cases.py says they must (everything
lost recovered, but for the case past the loss limit) is refused and nothing
is written.  The file holds lengths, loss sets, counts, codes and hashes only,
every distinct packet once (ge_cases.pack).

Runs only where oracle/_ref/libsiamese_ref.so exists (make -C oracle).
Usage: python tests/golden/make_ge_golden.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ge_cases as G  # noqa: E402
import scenario_lib as S  # noqa: E402
import size_cases as Z  # noqa: E402

UNDECODABLE = ("over_256x256",)   # past kMaxLossRecovery: NeedMoreData is the answer


def main():
    if not os.path.exists(S.REF_LIB):
        sys.exit("oracle/_ref/libsiamese_ref.so missing: run make -C oracle")
    cases = {}
    for name, case in G.CASES.items():
        t0 = time.time()
        data = Z.payloads(case)
        packets, decodes, recovered = G.reference_run(case, data)
        if any(recovered[i] != data[i] for i in recovered):
            sys.exit("%s: the reference recovered other bytes" % name)
        if name in UNDECODABLE:
            if recovered or decodes != [[[2, 0]]]:
                sys.exit("%s: the reference decoded past its loss limit: %r" % (name, decodes))
        elif sorted(recovered) != sorted(case.lost):
            sys.exit("%s: the reference does not recover this loss set: %r" % (name, decodes))
        if name.startswith("singular") and decodes[0] != [[2, 0]]:
            sys.exit("%s: the reference's first decode is not NeedMoreData: %r" % (name, decodes))
        cases[name] = G.describe(packets, decodes, recovered, case)
        if not all(1 <= r["footer_bytes"] <= 8 for r in cases[name]["recovery"]):
            sys.exit("%s: a packet's payload is not as long as the longest symbol of its window" % name)
        print("%-18s originals=%-4d lost=%-4d recovery=%-4d decodes=%r %.2fs" % (
            name, len(case.lengths), len(case.lost), case.recovery, decodes, time.time() - t0), flush=True)
    out = dict(G.pack(cases), generator="tests/golden/make_ge_golden.py (oracle/_ref/libsiamese_ref.so)")
    assert G.unpack(out) == cases
    with open(G.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
