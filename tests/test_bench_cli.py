"""bench.py's command line on CPU (the test double of the backend): a plain
run does the timed steps only, `--full` adds the runs beside them, and
`--dump-outputs` writes the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np

import scenario_lib as S

ROOT = S.ROOT
ARGS = ["--library", S.SIM_LIB, "--gpus", "1", "--streams", "6", "--steps", "2", "--warmup", "1"]


def _bench(extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    lines = [_bench(["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 2 and line["warmup"] == 1
        assert line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
        # what takes runs of its own stays behind --full
        for key in ("cpu_baseline", "end_to_end", "legs", "decode_ab"):
            assert line[key] is None, key
        assert line["roofline"]["unique_frac"] is None
    for name, cols in (("stream_results", len(S.StreamResult._fields_) - 1), ("stream_digests", 4)):
        a = np.load(str(tmp_path / "a" / (name + ".npy")))
        b = np.load(str(tmp_path / "b" / (name + ".npy")))
        assert a.dtype == np.float64 and a.shape == (6, cols)
        assert np.array_equal(a, b), name
    # the dumped digests are those of the same streams with every byte hashed
    cfg = S.replace(S.CONFIGS["C4"], streams=6, add_ranges=1, hash_data=1)
    res, rep = S.run_batch(S.SIM_LIB, cfg, verify=True)
    assert rep.mismatches == 0
    got = np.load(str(tmp_path / "a" / "stream_digests.npy")).astype(np.uint64)
    assert [int(r[0]) << 48 | int(r[1]) << 32 | int(r[2]) << 16 | int(r[3]) for r in got] == S.digests(res)
    # every stream of the last timed step delivered all 256 originals, status 0
    results = np.load(str(tmp_path / "a" / "stream_results.npy"))
    assert (results[:, -1] == 0).all() and (results[:, -2] == 256).all()


def test_full_run_adds_the_side_measurements():
    line = _bench(["--full", "--no-cpu", "--no-legs"])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["decode_ab"] is not None and line["end_to_end"] is not None
    assert line["roofline"]["unique_bytes_per_launch"] is not None
