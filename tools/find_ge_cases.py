#!/usr/bin/env python3
"""Search for the pivoted and singular cases of tests/ge_cases.py.

A Siamese pivot is zero about once in 256, so a matrix that leaves the
no-pivot loop at a wanted column, or is singular, is a chance event.  This
tool walks seeds (and with them the lost sets, ge_cases.spread) for a wanted
shape on the CPU test double (tests/hostsim/libsiamese_hostsim.so), reads what
each device job did from the double's HOSTSIM_GE_TRACE line (rows, cols,
chained, the first zero pivot, where it stopped, the column counts raised, the
row kinds) and from the counters sgpu_engine_stats_ex [37] and [38], and
prints for each match the expression to commit in ge_cases.py, with the
counters it measured, and the trace as a comment.  (A singular case still
needs its further parts: ge_cases._singular, or mixed's `then`.)  It never touches a GPU, and no test runs it;
a case it finds is still checked against the reference by
tests/golden/make_ge_golden.py.

  find_ge_cases.py square N [--window W] [--recovery R] [--short]
  find_ge_cases.py mixed N [--first F]
  find_ge_cases.py single 1 --windows A B
      each with [--want plain|pivoted|singular] [--at first|middle|last|any]
                [--seeds A B] [--count K]

plain: the job eliminates without pivoting; pivoted: it eliminates, its first
zero pivot at column 0 (first), at the last column (last), or in the middle
third (middle); singular: it stops short, at a middle column with --at middle.
--recovery R offers R >= N packets (the region takes the newest N).
`mixed N` walks ge_cases.mixed(seed, ..., first=F) instead (N is ignored): two
windows, rows of two lengths, a square job that is not chained.
`single 1` walks every lost index of every window in [A, B) with one packet
(seeds are not used): the 1 x 1 jobs.
"""
import argparse
import ctypes as C
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deliver_cases as D  # noqa: E402
import exec_shape_cases as X  # noqa: E402
import ge_cases as G  # noqa: E402
import scenario_lib as S  # noqa: E402
import size_cases as Z  # noqa: E402

TRACE = re.compile(r"hostsim ge: rows (\d+) cols (\d+) chained (\d+) pickLen (\d+) first_zero (\d+) stop (\d+) grown (\d+) kinds (\d+) (\d+) (\d+)")


def probe(L, case):
    """The case with sgpu_decode_device on the test double: (the decode
    results per part, the trace of every job, the counters' growth)."""
    data = Z.payloads(case)
    os.environ["HOSTSIM_GE_TRACE"] = "1"
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            e0 = Z.engine(L)
            run = X.Run(L, case, data, schedule=())
            results, recovered = [], set()
            for k, part in enumerate(case.parts):
                run.play(part)
                assert L.sgpu_flush() == 0
                calls = []
                while len(calls) < G.MAX_DECODES and recovered != G.lost_so_far(case, k):
                    out, n = C.POINTER(D.Orig)(), C.c_uint(0)
                    r = L.sgpu_decode_device(run.dec, C.byref(out), C.byref(n))
                    if r == D.PENDING:
                        assert L.sgpu_flush() == 0
                        r = L.sgpu_decode_device(run.dec, C.byref(out), C.byref(n))
                    calls.append([r, n.value])
                    if r != D.SUCCESS:
                        break
                    recovered.update(out[i].PacketNum for i in range(n.value))
                results.append(calls)
            run.free()
            e1 = Z.engine(L)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    jobs = [dict(zip(("rows", "cols", "chained", "pickLen", "first_zero", "stop", "grown", "parity", "cauchy", "siamese"), map(int, m.groups())))
            for m in TRACE.finditer(text)]
    grew = {k: e1["ge_" + k] - e0["ge_" + k] for k in G.COUNTERS}
    return results, jobs, grew


def matches(job, want, at):
    cols, fz, stop = job["cols"], job["first_zero"], job["stop"]
    if want == "plain":
        return fz == cols
    if want == "pivoted" and stop != cols or want == "singular" and stop == cols:
        return False
    if fz == cols:
        return False
    where = stop if want == "singular" else fz
    if at == "first":
        return where == 0
    if at == "last":
        return where == cols - 1
    if at == "middle":
        return cols // 3 <= where < cols - cols // 3
    return True


def counters(grew):
    return "dev(%s)" % ", ".join("%s=%d" % (k, grew[k]) for k in G.COUNTERS)


def candidates(a):
    """(the case, the expression that makes it but for its counters) ..."""
    if a.shape == "single":
        for w in range(a.windows[0], a.windows[1]):
            for i in range(w):
                yield (G.Case(w, G.block(w, 1), (i,), G.dev()),
                       "Case(%d, block(%d, 1), (%d,), %%s, host=%%d)" % (w, w, i))
        return
    for seed in range(a.seeds[0], a.seeds[1]):
        if a.shape == "mixed":
            yield (G.mixed(seed, G.dev(), first=a.first),
                   "mixed(%d, %%s, host=%%d, first=%d)" % (seed, a.first))
        else:
            r = a.recovery or a.n
            yield (G.Case(seed, G.block(a.window, r), G.spread(a.n, a.window, seed), G.dev(), short=a.short),
                   "Case(%d, block(%d, %d), spread(%d, %d, %d), %%s, host=%%d%s)" % (
                       seed, a.window, r, a.n, a.window, seed, ", short=True" if a.short else ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shape", choices=["square", "mixed", "single"])
    ap.add_argument("n", type=int)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--windows", type=int, nargs=2, default=[296, 321])
    ap.add_argument("--first", type=int, default=60)
    ap.add_argument("--recovery", type=int, default=0)
    ap.add_argument("--want", choices=["plain", "pivoted", "singular"], default="pivoted")
    ap.add_argument("--at", choices=["first", "middle", "last", "any"], default="any")
    ap.add_argument("--seeds", type=int, nargs=2, default=[1, 4000])
    ap.add_argument("--count", type=int, default=1)
    ap.add_argument("--short", action="store_true")
    a = ap.parse_args()
    if not os.path.exists(S.SIM_LIB):
        sys.exit("tests/hostsim/libsiamese_hostsim.so missing: make -C siamese_amd hostsim")
    L = X.bind(D.load(S.SIM_LIB))
    found = 0
    for case, line in candidates(a):
        results, jobs, grew = probe(L, case)
        if not jobs or not matches(jobs[0], a.want, a.at):
            continue
        # (the host placement enters pivoted_ge once less per singular device job)
        print("%s  # results %r jobs %r" % (line % (counters(grew), grew["pivoted"] - grew["singular"]), results, jobs),
              flush=True)
        found += 1
        if found >= a.count:
            return
    sys.exit("no candidate gives a %s job (--at %s)" % (a.want, a.at))


if __name__ == "__main__":
    main()
