"""Regenerate the fixtures of tests/walk_cases.py from the upstream reference.

Runs only where oracle/_ref/libsiamese_ref.so exists (make_golden.py).
Usage: python tests/golden/make_walk_golden.py
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import golden  # noqa: E402
import scenario_lib as S  # noqa: E402
import walk_cases as W  # noqa: E402


def main():
    if not os.path.exists(S.REF_LIB):
        sys.exit("oracle/_ref/libsiamese_ref.so missing: run make -C oracle")
    for name, cfg in W.CONFIGS.items():
        res, _, wall = S.run_capi(S.REF_LIB, cfg, threads=min(8, cfg.streams))
        golden.save(name, cfg, res, wall)
        print("%-16s %s" % (name, S.summary(res)), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = W.build_driver(os.path.join(tmp, "recovery_walks_test"))
        for name in W.SEQUENCES:
            out = W.run_driver(exe, S.REF_LIB, name)
            if out.returncode != 0:
                sys.exit("%s: the reference failed (%d)\n%s" % (name, out.returncode, out.stderr))
            with open(W.sequence_path(name), "w") as f:
                f.write(out.stdout)
            print("%-16s %d events" % (name, out.stdout.count("\n")), flush=True)


if __name__ == "__main__":
    main()
