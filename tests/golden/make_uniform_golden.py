"""Regenerate the fixtures of tests/uniform_cases.py from the upstream reference.

Runs only where oracle/_ref/libsiamese_ref.so exists (make_golden.py).
Usage: python tests/golden/make_uniform_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import golden  # noqa: E402
import scenario_lib as S  # noqa: E402
import uniform_cases as U  # noqa: E402


def main():
    if not os.path.exists(S.REF_LIB):
        sys.exit("oracle/_ref/libsiamese_ref.so missing: run make -C oracle")
    for name, cfg in U.CONFIGS.items():
        res, _, wall = S.run_capi(S.REF_LIB, cfg, threads=min(8, cfg.streams))
        golden.save(name, cfg, res, wall)
        with open(golden.path(name)) as f:   # (golden.save names make_golden.py)
            data = json.load(f)
        data["generator"] = "tests/golden/make_uniform_golden.py (oracle/_ref/libsiamese_ref.so)"
        with open(golden.path(name), "w") as f:
            json.dump(data, f, separators=(",", ":"))
        print("%-16s %s" % (name, S.summary(res)), flush=True)


if __name__ == "__main__":
    main()
