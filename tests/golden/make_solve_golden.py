"""Regenerate tests/golden/solve_inconsistent.json from the upstream reference.

For every stream of every case of tests/solve_cases.py the same originals and
the same edit (one received original with a flipped byte, or handed over
short) go through the reference's siamese.h API: the length and sha256 of
each recovery packet, every decode call's result and packet count, and the
number, length and sha256 of every packet the first decode returned are
recorded.  The conditions that keep a case from passing vacuously
(solve_cases.conditions: the reference's answer is the one the case names, a
successful decode returns at least one wrong packet, the lost lengths lie on
both sides of a flip) are checked here too, and nothing is written if one
fails.  The Cauchy window's cuts of 1 to 59 bytes are walked: both outcomes
must exist, and cut_success and cut_disabled must name the smallest cut of
each.  The file holds lengths' hashes, loss sets, edits, counts and hashes
only.

Runs only where oracle/_ref/libsiamese_ref.so exists (make -C oracle).
Usage: python tests/golden/make_solve_golden.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import deliver_cases as D  # noqa: E402
import scenario_lib as S  # noqa: E402
import size_cases as Z  # noqa: E402
import solve_cases as V  # noqa: E402


def walk_cuts():
    """The first decode's result for every cut of the Cauchy window."""
    base = V.CASES["cut_success"].streams[0]
    data = Z.payloads(base)
    results = {}
    for n in range(1, 60):
        s = V.Stream(base.seed, base.lengths, base.lost, base.recovery, ("cut", V.C40_CUT, n))
        _, decodes, _ = V.dropin_run(S.REF_LIB, s, data)
        results[n] = decodes[0][0]
    ok = sorted(n for n, r in results.items() if r == D.SUCCESS)
    dis = sorted(n for n, r in results.items() if r == D.DISABLED)
    assert len(ok) + len(dis) == 59, "a cut with a third outcome: %r" % results
    assert ok and dis, "both outcomes must exist: Success %r, Disabled %r" % (ok, dis)
    for name, cuts in (("cut_success", ok), ("cut_disabled", dis)):
        named = V.CASES[name].streams[0].edit[2]
        assert named == cuts[0], "%s names cut %d, the smallest with that outcome is %d" % (name, named, cuts[0])
    print("cuts 1..59 of original %d: Success %d (first %d), Disabled %d (first %d)" % (
        V.C40_CUT, len(ok), ok[0], len(dis), dis[0]), flush=True)


def main():
    if not os.path.exists(S.REF_LIB):
        sys.exit("oracle/_ref/libsiamese_ref.so missing: run make -C oracle")
    walk_cuts()
    cases = {}
    for name, case in V.CASES.items():
        t0 = time.time()
        datas = [Z.payloads(s) for s in case.streams]
        wants = []
        for s, data in zip(case.streams, datas):
            packets, decodes, returned = V.dropin_run(S.REF_LIB, s, data)
            again = V.dropin_run(S.REF_LIB, s, data)
            assert again == (packets, decodes, returned), "%s: the reference's outcome is not deterministic" % name
            wants.append(V.describe(s, packets, decodes, returned))
        V.conditions(name, case, wants, datas)
        cases[name] = wants
        k = case.edited[0]
        wrong = sum(1 for num, length, sha in wants[k]["packets"]
                    if sha != V.hashlib.sha256(datas[k][num]).hexdigest())
        print("%-18s streams=%-2d m=%-3d %s, %d of %d packets wrong  %.2fs" % (
            name, len(case.streams), case.m, wants[k]["decodes"], wrong, len(wants[k]["packets"]),
            time.time() - t0), flush=True)
    out = {"generator": "tests/golden/make_solve_golden.py (oracle/_ref/libsiamese_ref.so)", "cases": cases}
    with open(V.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
