"""The uniform subwindows of both codecs on the device library: the workloads of
test_uniform_slots_cpu.py that bear on what the device is sent (the ingest
runs of the range adds, the window snapshots made from the descriptors),
against the same reference fixtures."""
import pytest

import golden
import scenario_lib as S
import uniform_cases as U

pytestmark = pytest.mark.gpu


def _check(name, **run):
    cfg = U.CONFIGS[name]
    res, rep = S.run_batch(S.AMD_LIB, cfg, verify=True, **run)
    want = golden.load(name)
    assert S.digests(res) == want["digests"]
    assert [int(r.status) for r in res] == want["status"]
    assert rep.mismatches == 0 and rep.checked > 0


def test_block_range_chained_decode():
    """8 streams x 130 x 100 B, block mode, 20 % loss, range calls, chained
    device decode, every byte hashed."""
    assert U.CONFIGS["uni_block130x8r"].hash_data == 1
    _check("uni_block130x8r", device_ge=True)


def test_streaming_with_acks():
    """4 streams of the streaming case: acknowledgements rotate uniform
    subwindows out of the window between range adds."""
    _check("uni_ack")
