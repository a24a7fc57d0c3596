"""Regenerate tests/golden/wrap_edges.json from the upstream reference.

The reference's own encoder and decoder walk to the 22-bit packet-number wrap
on the schedule of tests/wrap_cases.py (one-byte originals, a remove_before,
one recovery packet and one acknowledgement per step, every original and
every recovery packet into the decoder); the sha256 over the walk's recovery
packets and acknowledgements is recorded.
The walk is made once.  Every case then runs in a forked child, which owns
the copy of the walked pair it inherited: the case's schedule through the
reference's siamese.h calls, the length and sha256 of each recovery packet,
each decode call's result with the numbers, lengths and sha256 of its packets,
and for the ARQ case the acknowledgement messages, their results and the
retransmission order.  A case whose loss set the reference does not decode is
refused and nothing is written.  The file holds numbers, lengths, results and
hashes only.

Runs only where oracle/_ref/libsiamese_ref.so exists (make -C oracle).
Usage: python tests/golden/make_wrap_golden.py [--out FILE]
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import scenario_lib as S  # noqa: E402
import wrap_cases as W  # noqa: E402


def in_child(fn, *args):
    """fn(*args) in a forked child (its own copy of the walked pair): the JSON it returns."""
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:
        status = 1
        try:
            os.close(r)
            with os.fdopen(w, "w") as f:
                json.dump(fn(*args), f)
            status = 0
        except SystemExit as e:
            sys.stderr.write("%s\n" % (e,))
        except BaseException:
            import traceback
            traceback.print_exc()
        finally:
            os._exit(status)
    os.close(w)
    with os.fdopen(r) as f:
        text = f.read()
    _, status = os.waitpid(pid, 0)
    if status != 0:
        sys.exit("%s%r failed" % (fn.__name__, args[1:]))
    return json.loads(text)


def main():
    if not os.path.exists(S.REF_LIB):
        sys.exit("oracle/_ref/libsiamese_ref.so missing: run make -C oracle")
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else W.GOLDEN
    t0 = time.time()
    ref = W.ApiPair()
    print("walk: %d recovery packets to %#x, %.2fs" % (ref.packets, W.PARK, time.time() - t0), flush=True)
    cases = {}
    for name in W.CASES:
        t0 = time.time()
        cases[name] = in_child(W.reference_case, ref, name)
        print("%-12s recovery=%-3d decodes=%d %.2fs" % (name, len(cases[name]["recovery"]), len(cases[name]["decodes"]),
                                                       time.time() - t0), flush=True)
    arq = in_child(W.reference_arq, ref)
    print("arq          acks=%d retransmits=%d" % (len(arq["acks"]), len(arq["retransmits"]) - 1), flush=True)
    out = {"generator": "tests/golden/make_wrap_golden.py (oracle/_ref/libsiamese_ref.so)",
           "walk": {"park": W.PARK, "step": W.STEP, "packets": ref.packets, "sha256": ref.sha256},
           "cases": cases, "arq": arq}
    with open(out_path, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
