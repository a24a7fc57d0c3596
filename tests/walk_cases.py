"""Workloads around the decoder's recovery list and readiness walk
(test_recovery_walks_cpu.py, test_recovery_walks_gpu.py).

Harness configs, with reference digests under tests/golden/<name>.json, and
the scripted sequences of tests/recovery_walks_test.cpp, with the reference's
event logs under tests/golden/<name>.txt.  Both kinds of fixture are written
by tests/golden/make_walk_golden.py from oracle/_ref/libsiamese_ref.so.
"""
import os
import subprocess

import golden
import scenario_lib as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "recovery_walks_test.cpp")

CONFIGS = {
    # a block of 64 originals x 100 B, 30 % loss on originals and recovery
    # packets: every recovery packet of a stream has one key
    "walk_block64": S.make_config(block_mode=1, streams=8, originals=64, payload_bytes=100,
                                  loss_pct=30, recovery_loss_pct=30),
    # streaming with immediate acknowledgements, a recovery packet every 4
    # originals: keys never repeat
    "walk_ack4": S.make_config(streams=4, originals=400, payload_bytes=100, loss_pct=15,
                               recovery_loss_pct=15, recovery_interval=4, ack_policy=1),
}

SEQUENCES = ["block", "interleave", "reorder", "delete_run"]


def sequence_path(name):
    return os.path.join(golden.DIR, "walk_seq_%s.txt" % name)


def build_driver(out, extra=()):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + list(extra) +
                   [DRIVER_SRC, "-o", str(out), "-ldl"], check=True, timeout=300)
    return str(out)


def run_driver(exe, library, name, env=None):
    return subprocess.run([exe, library, name], capture_output=True, text=True, timeout=120, env=env)
