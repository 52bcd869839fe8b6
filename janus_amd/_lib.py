"""Loader for the in-tree HIP engine library (libjanus_prio3.so, C ABI in include/jx_prio3.h).

There is no CPU fallback: if the library is missing or no HIP device is present,
every engine entry point raises. Build with ``python -m janus_amd.build``.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libjanus_prio3.so")

# Every symbol include/jx_prio3.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = (
    "jx_engine_create", "jx_engine_create_ex", "jx_engine_destroy", "jx_engine_sizes", "jx_engine_set_capacity",
    "jx_helper_prep_batch", "jx_engine_batch_id", "jx_engine_batches", "jx_batch_release",
    "jx_batch_aggregate_records", "jx_batch_aggregate_records_device", "jx_engine_leader_sizes", "jx_leader_prep_init_batch",
    "jx_leader_prep_finish_batch", "jx_leader_prep_init_device", "jx_leader_prep_finish_device",
    "jx_accumulate", "jx_accumulate_device", "jx_helper_prep_aggregate", "jx_helper_prep_aggregate_device",
    "jx_aggregate_read", "jx_aggregate_checksum", "jx_aggregate_reset", "jx_aggregate_export_device",
    "jx_aggregate_combine_device", "jx_shard_record_bytes", "jx_shard_record_export_device",
    "jx_shard_record_combine_device", "jx_engine_sync", "jx_engine_stream", "jx_engine_timing",
    "jx_engine_timing_read", "jx_engine_debug", "jx_status_str", "jx_last_error",
    "jx_engine_wait_stream", "jx_engine_join_stream", "jx_engine_wait_event", "jx_engine_record_event",
    "jx_engine_memory", "jx_engine_coalesce", "jx_leader_prep_init_device_ex", "jx_helper_prep_encrypted_batch",
    "jx_helper_prep_encrypted_batch2", "jx_leader_upload_open_batch", "jx_leader_upload_open_device",
    "jx_helper_prep_aggregate_encrypted", "jx_helper_prep_aggregate_encrypted_device",
    "jx_client_shard_batch", "jx_client_shard_device", "jx_client_rand_bytes",
    "jx_client_seal_sizes", "jx_client_seal_batch", "jx_client_seal_device",
    "jx_init_req_decode", "jx_init_req_decode_device", "jx_init_req_info", "jx_init_req_arrays", "jx_init_req_exclude",
    "jx_init_req_route", "jx_init_req_route_arrays",
    "jx_init_resp_encode_device", "jx_init_resp_encode", "jx_init_req_release",
    "jx_init_req_encode_bound", "jx_init_req_encode_device", "jx_init_req_encode", "jx_leader_req_info",
    "jx_leader_req_sent", "jx_init_resp_decode", "jx_leader_req_release",
    "jx_report_encode_bound", "jx_report_encode_device", "jx_report_encode", "jx_upload_decode_device", "jx_upload_decode",
    "jx_upload_req_info", "jx_upload_req_arrays", "jx_upload_req_release",
    "jx_collect_seal", "jx_collect_seal_device", "jx_collect_open", "jx_collect_open_device",
)

_lib = None


class JxParams(ctypes.Structure):
    _fields_ = [("algo_id", ctypes.c_uint32), ("bits", ctypes.c_uint32), ("length", ctypes.c_uint32),
                ("chunk_length", ctypes.c_uint32), ("num_proofs", ctypes.c_uint32)]


class JxMemoryStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "resident_batches", "batch_bytes", "arena_budget", "arena_allocated", "arena_in_use", "arena_peak",
        "arena_allocs", "arena_reuses", "arena_waits", "arena_engines", "last_pipelines", "coalesced_launches",
        "coalesced_jobs", "coalesced_reports", "coalesce_window_us", "coalesce_gather_us", "coalesce_copy_us",
        "coalesce_enqueue_us", "coalesce_device_us", "arena_cross_stream_waits", "coalesce_pinned_bytes",
        "coalesced_helper_launches", "coalesced_helper_jobs", "coalesced_leader_launches", "coalesced_leader_jobs",
        "coalesced_encrypted_jobs", "arena_frees")]


class JxWireRecord(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "off", "len", "public_share_off", "enc_off", "payload_off", "message_off", "prep_msg_off", "prep_share_off")]
    _fields_ += [(name, ctypes.c_uint32) for name in (
        "public_share_len", "enc_len", "payload_len", "message_len", "prep_msg_len", "prep_share_len")]
    _fields_ += [("config_id", ctypes.c_uint8), ("ping_pong_type", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 6)]


class JxInitReqInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_uint32), ("has_batch_id", ctypes.c_uint32)]
    _fields_ += [(name, ctypes.c_uint64) for name in (
        "error_offset", "duplicate_index", "n", "agg_param_off", "agg_param_len", "fallback_iterations",
        "odd_public_shares", "enc_bytes", "payload_bytes")]
    _fields_ += [("batch_id", ctypes.c_uint8 * 32)]


class JxInitReqArrays(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "d_report_ids", "d_times", "d_public_shares", "d_leader_prep_shares", "d_encs", "d_enc_offsets", "d_payloads",
        "d_payload_offsets", "d_key_index", "d_wire_status", "d_route", "d_records",
        "times", "enc_offsets", "payload_offsets", "records", "report_ids", "key_index", "wire_status")]


class JxLeaderReqInfo(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n", "n_sent", "body_len")]


class JxInitRespInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_uint32), ("pad_", ctypes.c_uint32)]
    _fields_ += [(name, ctypes.c_uint64) for name in ("error_offset", "mismatch_index", "n")]


class JxUploadChecks(ctypes.Structure):
    _fields_ = [("now", ctypes.c_uint64), ("tolerable_clock_skew", ctypes.c_uint64),
                ("has_task_expiration", ctypes.c_uint32), ("task_expiration", ctypes.c_uint64),
                ("has_report_expiry_age", ctypes.c_uint32), ("report_expiry_age", ctypes.c_uint64)]


class JxUploadReqInfo(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "n", "m", "leader_enc_bytes", "leader_payload_bytes", "helper_enc_bytes", "helper_payload_bytes")]
    _fields_ += [("status_count", ctypes.c_uint64 * 6)]


class JxUploadReqArrays(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "d_index", "d_report_ids", "d_times", "d_public_shares", "d_key_index", "d_leader_encs", "d_leader_enc_offsets",
        "d_leader_payloads", "d_leader_payload_offsets", "d_helper_config_ids", "d_helper_encs", "d_helper_enc_offsets",
        "d_helper_payloads", "d_helper_payload_offsets", "d_all_report_ids", "d_all_times", "d_upload_status", "d_row_of",
        "index", "times", "key_index", "leader_enc_offsets", "leader_payload_offsets", "helper_enc_offsets",
        "helper_payload_offsets", "helper_config_ids", "all_report_ids", "all_times", "upload_status", "row_of")]


class EngineError(RuntimeError):
    pass


def load():
    """Load the shared library and declare exact argument types (fails loudly)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"{LIB_PATH} is missing: build it with `python -m janus_amd.build` "
                          "(there is no CPU fallback)")
    # One HIP runtime per process: torch bundles libamdhip64.so (soname libamdhip64.so.7).
    # Loading torch first makes our NEEDED libamdhip64.so.7 resolve to that same runtime;
    # loading ours first would put two HSA runtimes in the process and break torch.cuda.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u8p = ctypes.c_void_p, ctypes.c_void_p
    i32, u32, u64 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
    P = ctypes.POINTER
    sig = {
        "jx_engine_create": (i32, [P(JxParams), u8p, i32, P(vp)]),
        "jx_engine_create_ex": (i32, [P(JxParams), u8p, u32, i32, P(vp)]),
        "jx_engine_destroy": (None, [vp]),
        "jx_engine_sizes": (i32, [vp, P(u32), P(u32), P(u32), P(u32), P(u32), P(u32)]),
        "jx_engine_set_capacity": (i32, [vp, u64]),
        "jx_helper_prep_batch": (i32, [vp, u64, u8p, u8p, u8p, u8p, u8p, u8p, u8p, P(u64)]),
        "jx_helper_prep_encrypted_batch": (i32, [vp, u64, u8p, P(u64), u8p, u8p, P(vp), u32, u8p, u8p, u8p, P(u64),
                                                  u32, u8p, u8p, u8p, u8p, P(u64)]),
        "jx_helper_prep_encrypted_batch2": (i32, [vp, u64, u8p, P(u64), u8p, u8p, P(vp), u32, u8p, u8p, P(u64), u8p,
                                                   P(u64), u32, u8p, u8p, u8p, u8p, P(u64)]),
        "jx_leader_upload_open_batch": (i32, [vp, u64, u8p, P(u64), u8p, u8p, P(vp), u32, u8p, u8p, P(u64), u8p,
                                               P(u64), u8p, u8p, P(u32), u8p]),
        "jx_leader_upload_open_device": (i32, [vp, u64, vp, P(u64), vp, u8p, P(vp), u32, u8p, vp, P(u64), vp, P(u64),
                                                vp, u64, vp, vp, vp]),
        "jx_engine_batch_id": (i32, [vp, P(u64)]),
        "jx_engine_batches": (i32, [vp, P(u64), P(u64)]),
        "jx_batch_release": (i32, [vp, u64]),
        "jx_batch_aggregate_records": (i32, [vp, u64, u64, u8p, u8p, u32, u8p]),
        "jx_batch_aggregate_records_device": (i32, [vp, u64, u64, vp, vp, u32, vp]),
        "jx_engine_leader_sizes": (i32, [vp, P(u32)]),
        "jx_leader_prep_init_batch": (i32, [vp, u64, u8p, u8p, u8p, u8p, u8p, P(u64)]),
        "jx_leader_prep_finish_batch": (i32, [vp, u64, u64, u8p, u8p, u8p]),
        "jx_leader_prep_init_device": (i32, [vp, u64, vp, vp, vp, vp, vp, P(u64)]),
        "jx_leader_prep_init_device_ex": (i32, [vp, u64, vp, vp, vp, u64, vp, vp, P(u64)]),
        "jx_engine_memory": (i32, [vp, P(JxMemoryStats)]),
        "jx_engine_coalesce": (i32, [vp, i32, u32]),
        "jx_leader_prep_finish_device": (i32, [vp, u64, u64, vp, vp, vp]),
        "jx_accumulate": (i32, [vp, u64, u64, u8p, u8p]),
        "jx_accumulate_device": (i32, [vp, u64, u64, vp, vp, P(u32), u32]),
        "jx_helper_prep_aggregate": (i32, [vp, u64, u8p, u8p, u8p, u8p, u32, u8p, u8p]),
        "jx_helper_prep_aggregate_device": (i32, [vp, u64, vp, vp, vp, vp, vp, P(u32), u32, vp, vp]),
        "jx_helper_prep_aggregate_encrypted": (i32, [vp, u64, u8p, P(u64), u8p, u8p, P(vp), u32, u8p, u8p, P(u64), u8p,
                                                      P(u64), u32, u8p, u32, u8p, u8p, u8p]),
        "jx_helper_prep_aggregate_encrypted_device": (i32, [vp, u64, vp, P(u64), vp, u8p, P(vp), u32, u8p, vp, P(u64),
                                                             vp, P(u64), u32, vp, vp, P(u32), u32, vp, vp, vp]),
        "jx_aggregate_read": (i32, [vp, u32, u8p, P(u64)]),
        "jx_aggregate_checksum": (i32, [vp, u32, u8p]),
        "jx_aggregate_reset": (i32, [vp]),
        "jx_aggregate_export_device": (i32, [vp, u32, vp]),
        "jx_aggregate_combine_device": (i32, [vp, vp, u32, vp]),
        "jx_shard_record_bytes": (i32, [vp, P(u32)]),
        "jx_shard_record_export_device": (i32, [vp, u32, vp]),
        "jx_shard_record_combine_device": (i32, [vp, vp, u32, vp]),
        "jx_client_shard_batch": (i32, [vp, u64, u8p, u8p, u8p, u8p, u8p, u8p, u8p]),
        "jx_client_shard_device": (i32, [vp, u64, vp, vp, vp, vp, vp, u64, vp, vp]),
        "jx_client_rand_bytes": (i32, [vp, P(u32)]),
        "jx_client_seal_sizes": (i32, [vp, P(u32), P(u32)]),
        "jx_client_seal_batch": (i32, [vp, u64, u8p, P(u64), u8p, u8p, u64, u8p, u8p, vp, vp, u8p, u8p, u8p, u8p, u8p,
                                        u8p, u8p]),
        "jx_client_seal_device": (i32, [vp, u64, vp, P(u64), vp, vp, u64, vp, u8p, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "jx_init_req_decode": (i32, [vp, u8p, u64, u32, u8p, u8p, P(u64), P(vp)]),
        "jx_init_req_decode_device": (i32, [vp, vp, u64, u32, u8p, u8p, P(u64), P(vp)]),
        "jx_init_req_info": (i32, [vp, P(JxInitReqInfo)]),
        "jx_init_req_arrays": (i32, [vp, P(JxInitReqArrays)]),
        "jx_init_req_exclude": (i32, [vp, u8p]),
        "jx_init_req_route": (i32, [vp, vp, u64, P(u64), u64, P(u32), P(u32), vp]),
        "jx_init_req_route_arrays": (i32, [vp, P(vp), P(vp)]),
        "jx_init_resp_encode_device": (i32, [vp, vp, vp, vp, vp, u64, u8p, u8p, vp, u64, P(u64), vp]),
        "jx_init_resp_encode": (i32, [vp, vp, vp, vp, vp, u64, u8p, u8p, u8p, u64, P(u64), u8p]),
        "jx_init_req_release": (None, [vp]),
        "jx_init_req_encode_bound": (i32, [vp, u64, P(u64), P(u64), u64, u32, P(u64)]),
        "jx_init_req_encode_device": (i32, [vp, u64, vp, P(u64), vp, u8p, vp, P(u64), vp, P(u64), vp, u64, vp, u8p, u8p,
                                            u64, u32, u8p, vp, u64, P(u64), P(vp)]),
        "jx_init_req_encode": (i32, [vp, u64, u8p, P(u64), u8p, u8p, u8p, P(u64), u8p, P(u64), u8p, u64, u8p, u8p, u8p,
                                     u64, u32, u8p, u8p, u64, P(u64), P(vp)]),
        "jx_leader_req_info": (i32, [vp, P(JxLeaderReqInfo)]),
        "jx_leader_req_sent": (i32, [vp, P(vp), P(vp)]),
        "jx_init_resp_decode": (i32, [vp, vp, u8p, u64, vp, u64, vp, u8p, u8p, P(JxInitRespInfo)]),
        "jx_leader_req_release": (None, [vp]),
        "jx_report_encode_bound": (i32, [vp, u64, u32, u32, P(u64)]),
        "jx_report_encode_device": (i32, [vp, u64, vp, P(u64), vp, vp, u32, vp, vp, u32, vp, ctypes.c_uint8, ctypes.c_uint8,
                                          vp, vp, u64, vp, P(u64), P(u64)]),
        "jx_report_encode": (i32, [vp, u64, u8p, P(u64), u8p, u8p, u32, u8p, u8p, u32, u8p, ctypes.c_uint8, ctypes.c_uint8,
                                   u8p, u8p, u64, P(u64), P(u64)]),
        "jx_upload_decode_device": (i32, [vp, vp, u64, u64, P(u64), P(JxUploadChecks), u8p, u8p, P(vp)]),
        "jx_upload_decode": (i32, [vp, u8p, u64, u64, P(u64), P(JxUploadChecks), u8p, u8p, P(vp)]),
        "jx_upload_req_info": (i32, [vp, P(JxUploadReqInfo)]),
        "jx_upload_req_arrays": (i32, [vp, P(JxUploadReqArrays)]),
        "jx_upload_req_release": (None, [vp]),
        "jx_collect_seal": (i32, [vp, u64, u8p, u64, P(u64), P(u32), P(u64), u8p, u64, u64, u8p, P(u64), u8p, vp,
                                  u8p, P(u64), u8p, u8p, u8p, u8p]),
        "jx_collect_seal_device": (i32, [vp, u64, vp, u64, P(u64), P(u32), P(u64), u8p, u64, u64, u8p, P(u64), vp, vp,
                                         vp, vp, vp, vp, vp, vp]),
        "jx_collect_open": (i32, [vp, vp, vp, u64, u8p, u8p, P(u64), u8p, u8p, P(u64), u8p, P(u64), u8p, u8p]),
        "jx_collect_open_device": (i32, [vp, vp, vp, u64, vp, vp, P(u64), vp, vp, P(u64), u8p, P(u64), vp, vp]),
        "jx_engine_sync": (i32, [vp]),
        "jx_engine_stream": (i32, [vp, P(vp)]),
        "jx_engine_wait_stream": (i32, [vp, vp]),
        "jx_engine_join_stream": (i32, [vp, vp]),
        "jx_engine_wait_event": (i32, [vp, vp]),
        "jx_engine_record_event": (i32, [vp, vp]),
        "jx_engine_timing": (i32, [vp, i32]),
        "jx_engine_timing_read": (i32, [vp, P(ctypes.c_float), P(u64)]),
        "jx_engine_debug": (i32, [vp, i32, ctypes.c_int64]),
        "jx_status_str": (ctypes.c_char_p, [i32]),
        "jx_last_error": (ctypes.c_char_p, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def check(status: int, engine_ptr=None, what: str = "") -> None:
    if status == 0:
        return
    L = load()
    msg = L.jx_status_str(status).decode()
    detail = L.jx_last_error(engine_ptr).decode() if engine_ptr else ""
    raise EngineError(f"{what}: {msg} ({status}) {detail}".strip())
