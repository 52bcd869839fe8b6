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


def prepare_report_bodies(engine: HelperEngine, task_id: bytes, leader_sealer, helper_sealer, measurements, times,
                          rands=None, ephemeral=None, report_ids=None, leader_config_id: int = 0,
                          helper_config_id: int = 0):
    """prepare_reports without a Python object per report: shard, seal and the Report encoding all run on the engine's
    device (shard_device, seal_reports_device, encode_reports), and nothing but the seal's status bytes comes back
    before the bodies. Arguments as prepare_reports. Returns (bodies, offsets): a torch uint8 tensor on the device with
    the encoded Reports back to back, and numpy uint64[n + 1]; report i's upload body is
    bodies[offsets[i]:offsets[i + 1]], byte for byte prepare_reports(...)[i].encode() under the same randomness. The
    pair is what aggregator.handle_upload_wire takes. Raises ValueError as prepare_reports does."""
    import torch

    times = [int(t) for t in times]
    n = len(times)
    ids = os.urandom(16 * n) if report_ids is None else bytes(report_ids)
    eph = os.urandom(64 * n) if ephemeral is None else bytes(ephemeral)
    if len(ids) != 16 * n or len(eph) != 64 * n:
        raise ValueError("report_ids: n x 16 bytes; ephemeral: n x 64 bytes")
    dev = torch.device("cuda", engine.device)
    if n == 0:
        return torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros(1, np.uint64)
    rb = engine.client_rand_bytes()
    rd = os.urandom(n * rb) if rands is None else np.ascontiguousarray(np.asarray(rands, dtype=np.uint8)).tobytes()
    if len(rd) != n * rb:
        raise ValueError(f"rands: n x {rb} bytes")
    meas = engine._measurements(measurements, n)
    PS, LIS, HIS = engine.public_share_len, engine.leader_input_share_len, engine.helper_input_share_len
    stride = (LIS + 15) // 16 * 16
    lct, hct = engine.client_seal_sizes()
    with torch.cuda.device(dev):
        up = lambda b, dt=np.uint8: torch.from_numpy(np.frombuffer(b, dt).copy()).to(dev)  # noqa: E731
        d_meas, d_ids, d_rd, d_eph = torch.from_numpy(meas.view(np.int64).copy()).to(dev), up(ids), up(rd), up(eph)
        z = lambda k: torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)  # noqa: E731
        d_ps, d_lis, d_his, d_st = z(n * PS), z(n * stride), z(n * HIS), z(n)
        d_le, d_lc, d_he, d_hc, d_seal = z(n * 32), z(n * lct), z(n * 32), z(n * hct), z(n)
        engine.shard_device(n, d_meas.data_ptr(), d_ids.data_ptr(), d_rd.data_ptr(), d_ps.data_ptr() if PS else None,
                            d_lis.data_ptr(), d_his.data_ptr(), d_st.data_ptr(), lis_stride=stride)
        engine.seal_reports_device(n, d_ids.data_ptr(), times, d_ps.data_ptr() if PS else None, d_lis.data_ptr(),
                                   d_his.data_ptr(), task_id, leader_sealer, helper_sealer, d_eph.data_ptr(), d_le.data_ptr(),
                                   d_lc.data_ptr(), d_he.data_ptr(), d_hc.data_ptr(), d_seal.data_ptr(),
                                   d_shard_status=d_st.data_ptr(), lis_stride=stride)
        status = d_seal.cpu().numpy()[:n]
        bad = np.nonzero(status == SEAL_SKIPPED)[0]
        if len(bad):
            raise ValueError(f"measurements {bad[:8].tolist()} are out of range for {engine.vdaf.name()}")
        if (status != SEAL_OK).any():
            raise ValueError("an aggregator's HPKE public key is of low order: X25519 gave the all-zero output")
        return engine.encode_reports(n, d_ids.data_ptr(), times, d_ps.data_ptr() if PS else None, d_le.data_ptr(),
                                     d_lc.data_ptr(), d_he.data_ptr(), d_hc.data_ptr(), leader_config_id, helper_config_id,
                                     d_seal_status=d_seal.data_ptr())
