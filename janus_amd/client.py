"""The client on the GPU: the reference client's prepare_report (client/src/lib.rs:339-383) for a batch of
measurements: vdaf.shard (HelperEngine.shard_batch), then the two hpke::seal calls over each report's
PlaintextInputShares with its InputShareAad (HelperEngine.seal_reports). Nothing here draws randomness on the
device: the shard randomness and the ephemeral X25519 keys come from os.urandom unless the caller supplies them.
"""
from __future__ import annotations

import os

import numpy as np

from .engine import SEAL_OK, SEAL_SKIPPED, HelperEngine
from .messages import HpkeCiphertext, Report, ReportMetadata


def prepare_reports(engine: HelperEngine, task_id: bytes, leader_sealer, helper_sealer, measurements, times,
                    rands=None, ephemeral=None, report_ids=None, leader_config_id: int = 0,
                    helper_config_id: int = 0) -> list[Report]:
    """One messages.Report per measurement, ready for aggregator.handle_upload. leader_sealer / helper_sealer:
    janus_amd.hpke.HpkeSealer contexts on the engine's device, made from the aggregators' HpkeConfigs with
    application_info(recipient=ROLE_LEADER / ROLE_HELPER); their config ids go into the HpkeCiphertexts. times: the
    reports' timestamps, already rounded to the task's time precision. rands: n x engine.client_rand_bytes() of shard
    randomness; ephemeral: n x 64 bytes, the leader seal's X25519 private key, then the helper seal's; report_ids: n x 16
    (the VDAF nonces). Each comes from os.urandom when None. A measurement out of range raises ValueError, as prio's
    encode_measurement fails the reference's shard."""
    times = [int(t) for t in times]
    n = len(times)
    ids = os.urandom(16 * n) if report_ids is None else bytes(report_ids)
    eph = os.urandom(64 * n) if ephemeral is None else bytes(ephemeral)
    if len(ids) != 16 * n or len(eph) != 64 * n:
        raise ValueError("report_ids: n x 16 bytes; ephemeral: n x 64 bytes")
    if n == 0:
        return []
    nonces = np.frombuffer(ids, np.uint8).reshape(n, 16)
    rows = engine.shard_batch(measurements, nonces, rands)
    sealed = engine.seal_reports(nonces, times, rows.public_shares, rows.leader_input_shares, rows.helper_input_shares,
                                 task_id, leader_sealer, helper_sealer, eph, shard_status=rows.status)
    bad = np.nonzero(sealed.status == SEAL_SKIPPED)[0]
    if len(bad):
        raise ValueError(f"measurements {bad[:8].tolist()} are out of range for {engine.vdaf.name()}")
    if (sealed.status != SEAL_OK).any():
        raise ValueError("an aggregator's HPKE public key is of low order: X25519 gave the all-zero output")
    return [Report(ReportMetadata(ids[16 * i:16 * i + 16], times[i]), rows.public_shares[i].tobytes(),
                   HpkeCiphertext(leader_config_id, sealed.leader_encs[i].tobytes(), sealed.leader_cts[i].tobytes()),
                   HpkeCiphertext(helper_config_id, sealed.helper_encs[i].tobytes(), sealed.helper_cts[i].tobytes()))
            for i in range(n)]
