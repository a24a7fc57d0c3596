"""The recovery list's shortcuts on the MI355X (see test_recovery_walks_cpu.py):
the change is in the host control plane, so this shows that the device path
gets the same rows in the same order -- 8 streams x 64 originals x 100 B in
block mode at 30 % loss, every recovery packet byte and recovered byte hashed,
against the reference's digests (tests/golden/walk_block64.json).
"""
import pytest

import golden
import scenario_lib as S
import walk_cases as W


@pytest.mark.gpu
@pytest.mark.parametrize("device_ge", [True, False], ids=["sgpu_decode_device", "sgpu_decode"])
def test_block64_every_byte_hashed(device_ge):
    import siamese_amd
    siamese_amd.require_gpu()
    cfg = W.CONFIGS["walk_block64"]
    assert cfg.hash_data == 1
    res, rep = S.run_batch(S.AMD_LIB, cfg, verify=True, device_ge=device_ge)
    want = golden.load("walk_block64")
    assert S.digests(res) == want["digests"]
    assert [int(r.status) for r in res] == want["status"]
    assert rep.mismatches == 0 and rep.checked > 0
    if device_ge:
        assert S.engine_dict(rep)["ge_jobs"] > 0
